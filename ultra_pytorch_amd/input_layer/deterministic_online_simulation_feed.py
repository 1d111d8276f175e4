"""DeterministicOnlineSimulationFeed — online learning to rank on simulated users with the model's own ranking (reference
deterministic_online_simulation_feed.py:24-363): every list is sorted by the current scores, descending and stable (ties keep
index order), and the clicks are simulated on that order.  The random streams are the query pick and the click model's."""
from .stochastic_online_simulation_feed import OnlineSimulationFeed


class DeterministicOnlineSimulationFeed(OnlineSimulationFeed):
    NAME = "deterministic"

    def rerank(self, scores, list_len):
        """:129-135: sorted(range(n), key=score, reverse=True) - Python's sort is stable under reverse as well."""
        return sorted(range(len(scores)), key=lambda k: scores[k], reverse=True)
