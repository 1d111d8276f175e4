"""DeviceOnlineSimulationFeed — the online simulation feeds with the dataset resident in HBM and the batch drawn on the device.

The host feeds ({Stochastic,Deterministic}OnlineSimulationFeed, reference stochastic_online_simulation_feed.py:96-226) score the
batch on the GPU, copy the scores back and re-rank and click list by list in Python: ~15.5 ms of a 15.7 ms online batch at config 2.
Here `get_batch` queues three things on the current stream and returns without waiting for any of them:
  1. ultr_online_pick_args: B queries drawn uniformly (under check_validation among the queries whose candidate labels do not sum to
     0, an index built once per dataset) and their first max_candidate_num candidates;
  2. the algorithm's validation forward of those candidates with its CURRENT parameters (stream order puts it behind the update
     of the step before): every ranking model the algorithm accepts scores through its own engine;
  3. ultr_online_rerank_args: the re-ranking (a Plackett-Luce draw at temperature tau, or the stable descending sort) and the
     clicks on the new order, redrawn on the same order while check_validation finds none (MAX_SAMPLE_ROUND_NUM times at most).
The result is the `device_feed` dict the plugin algorithms take (docids / labels [max_candidate_num, B] on the device, labels 0
past selection_bias_cutoff).  Same per-list distribution as the host feeds, not the same random stream: a batch is a pure function
of (seed, batch counter, parameters) - Philox-4x32-10 on the device."""
import ctypes

import torch

from .. import _lib
from .. import hip_ops
from ..utils import HParams
from ..utils import click_models
from .device_click_feed import ResidentDataset


class DeviceOnlineSimulationFeed(object):
    MAX_SAMPLE_ROUND_NUM = 100
    MAX_CANDIDATES = 256  # ultr_online_rerank_args: one wavefront per list, PDGD's list limit
    MODES = {"deterministic": _lib.ONLINE_DETERMINISTIC, "stochastic": _lib.ONLINE_STOCHASTIC}

    def __init__(self, model, batch_size, hparam_str, seed=0, mode="stochastic"):
        if mode not in self.MODES:
            raise ValueError("mode must be one of %s (got %r)" % (sorted(self.MODES), mode))
        self.mode = mode
        defaults = dict(click_model_json="./example/ClickModel/pbm_0.1_1.0_4_1.0.json", oracle_mode=False,
                        dynamic_bias_eta_change=0.0, dynamic_bias_step_interval=1000)
        if mode == "stochastic":
            defaults["tau"] = 1
        self.hparams = HParams(**defaults)
        self.hparams.parse(hparam_str)
        self.need_interleave = bool(getattr(model.hparams, "need_interleave", False))
        # result interleaving happens inside train() of the algorithms that declare it (DBGD, MGD: INTERLEAVES_IN_TRAIN); the
        # feed itself serves the same batches either way, as the reference's does
        if self.need_interleave and not getattr(model, "INTERLEAVES_IN_TRAIN", False):
            raise NotImplementedError("result interleaving (TeamDraftInterleaving) is done by DBGD / MGD inside train(); %s does "
                                      "not interleave" % type(model).__name__)
        # click_model is the host twin: it owns eta and the examination table
        _, self.click_model, self.model_id = click_models.load_for_device(self.hparams.click_model_json, "DeviceOnlineSimulationFeed")
        self.model, self.batch_size = model, int(batch_size)
        self.rank_list_size = int(model.rank_list_size)
        self.max_candidate_num = int(model.max_candidate_num)
        if not 0 < self.max_candidate_num <= self.MAX_CANDIDATES:
            raise ValueError("DeviceOnlineSimulationFeed supports max_candidate_num up to %d (got %d)"
                             % (self.MAX_CANDIDATES, self.max_candidate_num))
        self.device = model.cuda
        self.exam, self.n_exam, self.cprob = click_models.device_tables(self.click_model, self.model_id, self.device)
        self.seed, self.step, self.global_batch_count = int(seed), 0, 0
        self.lib = _lib.load()
        self._resident = {}
        M, B, dev = self.max_candidate_num, self.batch_size, self.device
        # two buffer sets, used in turn: a batch (and its info_map) stays intact until the second get_batch after it
        self._bufs = [dict(cand_docids=torch.empty(M, B, dtype=torch.int32, device=dev),
                           cand_labels=torch.empty(M, B, dtype=torch.float32, device=dev),
                           docids=torch.empty(M, B, dtype=torch.int32, device=dev),
                           labels=torch.empty(M, B, dtype=torch.float32, device=dev),
                           perm=torch.empty(M, B, dtype=torch.int32, device=dev),
                           qidx=torch.empty(B, dtype=torch.int32, device=dev)) for _ in range(2)]
        self._args = [_lib.OnlineArgs(), _lib.OnlineArgs()]
        self._aptr = [ctypes.c_void_p(ctypes.addressof(a)) for a in self._args]
        self._cur = 1
        self._scores = [None, None]  # the scores each argument block points at (kept alive until the buffer comes round again)

    @staticmethod
    def preprocess_data(data_set, hparam_str, exp_settings):
        return

    def resident(self, data_set):
        """The dataset in HBM and the index of its queries whose first max_candidate_num labels do not sum to 0 (the reference's
        check_validation filter, stochastic_online_simulation_feed.py:84-85) - built once, at the upload."""
        key = id(data_set)
        if key not in self._resident:
            rd = ResidentDataset(data_set, self.device)
            M = self.max_candidate_num
            lab = torch.where(rd.lists[:, :M] >= 0, rd.labels[:, :M], torch.zeros((), device=self.device))
            eligible = torch.nonzero(lab.double().sum(1) != 0).flatten().to(torch.int32).contiguous()
            self._resident[key] = (data_set, rd, eligible, int(eligible.numel()))
        return self._resident[key]

    def _fill(self, k, rd, eligible, n_eligible, check_validation):
        a, buf = self._args[k], self._bufs[k]
        a.lists, a.labels, a.n_queries, a.n_docs, a.lmax = rd.lists.data_ptr(), rd.labels.data_ptr(), rd.n_queries, rd.n_docs, rd.lmax
        a.eligible, a.n_eligible = (eligible.data_ptr(), n_eligible) if check_validation else (None, 0)
        a.exam_prob, a.n_exam, a.click_prob, a.n_rel = self.exam.data_ptr(), self.n_exam, self.cprob.data_ptr(), int(self.cprob.numel())
        a.click_model, a.seed, a.step = self.model_id, self.seed, self.step
        a.batch, a.max_candidates, a.rank_list_size = self.batch_size, self.max_candidate_num, self.rank_list_size
        a.max_redraws = self.MAX_SAMPLE_ROUND_NUM if check_validation else 0
        a.mode, a.oracle_mode = self.MODES[self.mode], 1 if self.hparams.oracle_mode else 0
        a.tau = float(getattr(self.hparams, "tau", 1))
        a.cand_docids, a.cand_labels = buf["cand_docids"].data_ptr(), buf["cand_labels"].data_ptr()
        a.docids, a.out_labels, a.perm, a.query_idx = (buf["docids"].data_ptr(), buf["labels"].data_ptr(), buf["perm"].data_ptr(),
                                                       buf["qidx"].data_ptr())
        return a

    def get_batch(self, data_set, check_validation=False, data_format="ULTRA"):
        if len(data_set.initial_list[0]) < self.rank_list_size:  # BaseInputFeed._check, as the host feeds
            raise ValueError("Input ranklist length must be no less than the required list size, %d != %d."
                             % (len(data_set.initial_list[0]), self.rank_list_size))
        _, rd, eligible, n_eligible = self.resident(data_set)
        if check_validation and n_eligible == 0:
            raise ValueError("check_validation: no query of this dataset has a label > 0 among its first %d candidates"
                             % self.max_candidate_num)
        k = 1 - self._cur
        a, buf = self._fill(k, rd, eligible, n_eligible, check_validation), self._bufs[k]
        stream = hip_ops.raw_stream()
        _lib.check(self.lib.ultr_online_pick_args(self._aptr[k], stream), "ultr_online_pick_args")
        cand = {"device_feed": True, "features": rd.features, "n_docs": rd.n_docs, "docids": buf["cand_docids"],
                "labels": buf["cand_labels"], "batch_size": self.batch_size, "feed_obj": None}
        scores = self.model.validation(cand, True)[1]  # [B, max_candidate_num], the current parameters, queued on the stream
        if scores.shape != (self.batch_size, self.max_candidate_num) or not scores.is_contiguous():
            raise RuntimeError("the ranking model returned scores of shape %s" % (tuple(scores.shape),))
        self._scores[k] = scores
        a.scores = scores.data_ptr()
        _lib.check(self.lib.ultr_online_rerank_args(self._aptr[k], stream), "ultr_online_rerank_args")
        self._cur = k
        self.step += 1
        self.global_batch_count += 1
        # drifting bias severity (stochastic_online_simulation_feed.py:219-224), as DeviceClickFeed does it
        if self.hparams.dynamic_bias_eta_change != 0 and self.global_batch_count % self.hparams.dynamic_bias_step_interval == 0:
            self.click_model.eta += self.hparams.dynamic_bias_eta_change
            self.click_model.setExamProb(self.click_model.eta)
            self.exam, self.n_exam = click_models.device_tables(self.click_model, self.model_id, self.device)[:2]
        feed = {"device_feed": True, "features": rd.features, "n_docs": rd.n_docs, "docids": buf["docids"], "labels": buf["labels"],
                "batch_size": self.batch_size, "feed_obj": None}
        # device tensors: query index [B], the candidates before the re-ranking [M, B] and the candidate index at each rank [M, B]
        info_map = {"rank_list_idxs": buf["qidx"], "input_list": buf["cand_docids"], "click_list": buf["cand_labels"],
                    "permutation": buf["perm"]}
        return feed, info_map

    def get_next_batch(self, index, data_set, check_validation=False, data_format="ULTRA"):
        raise NotImplementedError("DeviceOnlineSimulationFeed draws random batches only; use StochasticOnlineSimulationFeed / "
                                  "DeterministicOnlineSimulationFeed for get_next_batch")

    def get_data_by_index(self, data_set, index, check_validation=False):
        raise NotImplementedError("DeviceOnlineSimulationFeed draws random batches only; use StochasticOnlineSimulationFeed / "
                                  "DeterministicOnlineSimulationFeed for get_data_by_index")


class DeviceStochasticOnlineSimulationFeed(DeviceOnlineSimulationFeed):
    """StochasticOnlineSimulationFeed's batches (Plackett-Luce re-ranking at temperature `tau`) drawn on the device."""

    def __init__(self, model, batch_size, hparam_str, seed=0):
        super().__init__(model, batch_size, hparam_str, seed=seed, mode="stochastic")


class DeviceDeterministicOnlineSimulationFeed(DeviceOnlineSimulationFeed):
    """DeterministicOnlineSimulationFeed's batches (the model's own stable descending order) drawn on the device."""

    def __init__(self, model, batch_size, hparam_str, seed=0):
        super().__init__(model, batch_size, hparam_str, seed=seed, mode="deterministic")
