"""StochasticOnlineSimulationFeed — online learning to rank on simulated users (reference
stochastic_online_simulation_feed.py:23-377).  Each batch is re-ranked by the model being trained - a Plackett-Luce draw from
its scores - and the clicks are simulated on the NEW order.

Random streams, as there: one `random.random()` per query pick; one `np.random.choice(replace=False, p=probs,
size=count_nonzero(probs))` per list for the ranking (documents whose probability underflowed to 0 follow the drawn ones, in
index order); then the click model's own draws on the top rank_list_size positions, redrawn up to MAX_SAMPLE_ROUND_NUM times
while check_validation finds no click.  Re-ranked positions past the cutoff get label 0."""
import json
import os
import random

import numpy as np

from ..utils import HParams
from ..utils import click_models as cm
from .base_input_feed import BaseInputFeed


def _load_click_model(path):
    if not os.path.exists(path):  # the reference's default is relative to its repo root; the same file ships here
        alt = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", os.path.basename(path))
        path = alt if os.path.exists(alt) else path
    with open(path) as fin:
        return cm.loadModelFromJson(json.load(fin))


class OnlineSimulationFeed(BaseInputFeed):
    """What the stochastic and the deterministic online feeds share; subclasses define rerank(scores, list_len)."""
    NAME = "online"

    def _default_hparams(self):
        return dict(click_model_json="./example/ClickModel/pbm_0.1_1.0_4_1.0.json", oracle_mode=False,
                    dynamic_bias_eta_change=0.0, dynamic_bias_step_interval=1000)

    def __init__(self, model, batch_size, hparam_str):
        self.hparams = HParams(**self._default_hparams())
        print("Create online %s simluation feed" % self.NAME)
        print(hparam_str)
        self.hparams.parse(hparam_str)
        self.click_model = _load_click_model(self.hparams.click_model_json)  # loaded in oracle_mode too, as there
        self.start_index, self.count = 0, 1
        self.rank_list_size = model.rank_list_size
        self.max_candidate_num = model.max_candidate_num
        self.feature_size = model.feature_size
        self.batch_size, self.model = batch_size, model
        self.global_batch_count = 0
        self.need_interleave = bool(getattr(model.hparams, "need_interleave", False))
        # result interleaving happens inside train() of the algorithms that declare it (DBGD, MGD: INTERLEAVES_IN_TRAIN); the
        # feed itself serves the same batches either way, as the reference's does
        if self.need_interleave and not getattr(model, "INTERLEAVES_IN_TRAIN", False):
            raise NotImplementedError("result interleaving (TeamDraftInterleaving) is done by DBGD / MGD inside train(); %s does "
                                      "not interleave" % type(model).__name__)

    def prepare_true_labels_with_index(self, data_set, index, docid_inputs, letor_features, labels, check_validation=False):
        """stochastic_online_simulation_feed.py:78-94: the relevance labels of all max_candidate_num positions; a list without
        a positive label is dropped (not redrawn) under check_validation."""
        row, M = data_set.initial_list[index], self.max_candidate_num
        label_list = [0 if row[x] < 0 else data_set.labels[index][x] for x in range(M)]
        if check_validation and sum(label_list) == 0:
            return
        base = len(letor_features)
        for x in range(M):
            if row[x] >= 0:
                letor_features.append(data_set.features[row[x]])
        docid_inputs.append([-1 if row[x] < 0 else base + x for x in range(M)])
        labels.append(label_list)

    def rerank(self, scores, list_len):
        raise NotImplementedError

    def simulate_clicks_online(self, input_feed, check_validation=False):
        """:96-176: score the batch with the model (its GPU forward), re-rank every list, simulate clicks on the new order."""
        m = self.model
        rank_scores = m.validation(input_feed, True)[1].cpu().numpy()
        n_docs = len(input_feed[m.letor_features_name])
        ids_name, lab_name = m.docid_inputs_name, m.labels_name
        B = len(input_feed[ids_name[0]])
        for i in range(B):
            list_len = self.max_candidate_num
            while list_len > 0 and not input_feed[ids_name[list_len - 1]][i] < n_docs:
                list_len -= 1
            rerank_list = self.rerank(rank_scores[i][:list_len], list_len)
            new_docids = np.zeros(list_len)
            new_labels = np.zeros(list_len)
            for j in range(list_len):
                new_docids[j] = input_feed[ids_name[rerank_list[j]]][i]
                new_labels[j] = input_feed[lab_name[rerank_list[j]]][i]
            if self.hparams.oracle_mode:
                click_list = new_labels[:self.rank_list_size]
            else:
                click_list = self.click_model.sampleClicksForOneList(new_labels[:self.rank_list_size])[0]
                n = 0
                while check_validation and sum(click_list) == 0 and n < self.MAX_SAMPLE_ROUND_NUM:
                    click_list = self.click_model.sampleClicksForOneList(new_labels[:self.rank_list_size])[0]
                    n += 1
            for j in range(list_len):
                input_feed[ids_name[j]][i] = new_docids[j]
                input_feed[lab_name[j]][i] = click_list[j] if j < self.rank_list_size else 0
        return input_feed

    def _assemble_online(self, docid_inputs, letor_features, labels):
        n_docs, M, B = len(letor_features), self.max_candidate_num, len(docid_inputs)
        ids = np.asarray(docid_inputs, dtype=np.float32).reshape(B, M)
        ids[ids < 0] = n_docs
        lab = np.asarray(labels, dtype=np.float32).reshape(B, M)
        m = self.model
        feed = {m.letor_features_name: np.array(letor_features)}
        for l in range(M):
            feed[m.docid_inputs_name[l]] = np.ascontiguousarray(ids[:, l])
            feed[m.labels_name[l]] = np.ascontiguousarray(lab[:, l])
        return feed

    def get_batch(self, data_set, check_validation=False, data_format="ULTRA"):
        self._check(data_set)
        length = len(data_set.initial_list)
        docid_inputs, letor_features, labels, rank_list_idxs = [], [], [], []
        for _ in range(self.batch_size):
            i = int(random.random() * length)
            rank_list_idxs.append(i)
            self.prepare_true_labels_with_index(data_set, i, docid_inputs, letor_features, labels, check_validation)
        input_feed = self.simulate_clicks_online(self._assemble_online(docid_inputs, letor_features, labels), check_validation)
        info_map = {"rank_list_idxs": rank_list_idxs, "input_list": docid_inputs, "click_list": labels,
                    "letor_features": letor_features}
        self.global_batch_count += 1
        if self.hparams.dynamic_bias_eta_change != 0:
            if self.global_batch_count % self.hparams.dynamic_bias_step_interval == 0:
                self.click_model.eta += self.hparams.dynamic_bias_eta_change
                self.click_model.setExamProb(self.click_model.eta)
                print("Dynamically change bias severity eta to %.3f" % self.click_model.eta)
        return input_feed, info_map

    def get_next_batch(self, index, data_set, check_validation=False, data_format="ULTRA"):
        """:228-313.  The reference's stochastic feed reads `self.model.letor_features.name` here and crashes; this one works."""
        self._check(data_set)
        docid_inputs, letor_features, labels = [], [], []
        for offset in range(min(self.batch_size, len(data_set.initial_list) - index)):
            self.prepare_true_labels_with_index(data_set, index + offset, docid_inputs, letor_features, labels, check_validation)
        input_feed = self.simulate_clicks_online(self._assemble_online(docid_inputs, letor_features, labels), check_validation)
        return input_feed, {"input_list": docid_inputs, "click_list": labels}

    def get_data_by_index(self, data_set, index, check_validation=False):
        """:315-377 (the same crash fixed)."""
        self._check(data_set)
        docid_inputs, letor_features, labels = [], [], []
        self.prepare_true_labels_with_index(data_set, index, docid_inputs, letor_features, labels, check_validation)
        input_feed = self.simulate_clicks_online(self._assemble_online(docid_inputs, letor_features, labels), check_validation)
        return input_feed, {"input_list": docid_inputs, "click_list": labels}


class StochasticOnlineSimulationFeed(OnlineSimulationFeed):
    NAME = "stochastic"

    def _default_hparams(self):
        d = super()._default_hparams()
        d["tau"] = 1
        return d

    def rerank(self, scores, list_len):
        """Plackett-Luce sampling (:129-148) on the fp32 scores."""
        s = scores - np.max(scores)
        exp_scores = np.exp(self.hparams.tau * s)
        probs = exp_scores / np.sum(exp_scores)
        re_list = np.random.choice(np.arange(list_len), replace=False, p=probs, size=np.count_nonzero(probs))
        used = set(re_list)
        unused = [k for k in range(list_len) if k not in used]
        return np.append(re_list, unused).astype(int)
