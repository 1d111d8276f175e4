"""NSGD - Null Space Gradient Descent (Wang et al., SIGIR 2018): MGD whose candidate directions avoid the recent losing ones.
Drop-in for ultra.learning_algorithm.NSGD (reference nsgd.py)."""
import torch

from .. import engine
from .dbgd import DBGD


class NSGD(DBGD):
    """MGD's step (R = ranker_num candidates, team-draft multileave or per-ranker NDCG, the model steps toward the winners) with the
    candidates' noise drawn from the null space of a memory of losing directions.  The memory holds one row per ranker over the flat
    parameter vector (its Linear entries): after each step row r becomes ranker r's noise if that ranker lost, else zeros.  Each
    Linear tensor's noise is Philox normals projected onto the complement of its memory rows, then normalized over the whole tensor
    (csrc/ultr_nsgd.hip, engine.NsgdEngine).

    Defaults as nsgd.py, plus DBGD's `interleave_strategy` and `tau` (MGD's set).  The memory is a device tensor [R, P] owned by this
    object, so it survives changes of the list length; like the reference's it is not checkpointed.  Kept and changed quirks:
    DESIGN.md section 8.  Works with the DNN and Linear ranking models; SetRank and data parallelism are refused."""
    DEFAULT_HPARAMS = dict(DBGD.DEFAULT_HPARAMS, ranker_num=4)
    BANNER = "Build Null Space Gradient Descent (DBGD) algorithm."

    def __init__(self, data_set, exp_settings):
        super().__init__(data_set, exp_settings)
        self.memory = torch.zeros(self.n_rankers, self.model.shape.n_params, dtype=torch.float32, device=self.cuda)

    def _make_engine(self, *args, **kw):
        return engine.NsgdEngine(*args, memory=self.memory, **kw)

    def _report(self):
        self.global_step += 1  # nsgd.py: train prints no loss line
