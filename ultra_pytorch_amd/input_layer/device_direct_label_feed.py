"""DeviceDirectLabelFeed — DirectLabelFeed (reference direct_label_feed.py:22-284) with the dataset resident in HBM.

The host feed re-assembles every batch in Python: a loop per query that copies feature rows, then a staging copy to the GPU.  Here the
dataset is uploaded once (ResidentDataset) and a batch is one launch that writes global document ids and true labels [L, B]:
  get_next_batch / get_data_by_index   ultr_eval_pick: the queries index .. index + batch_size - 1 in order (the last batch short);
  get_batch                            ultr_online_pick_args: batch_size queries drawn uniformly, Philox keyed by (seed, batch counter).
The result is the `device_feed` dict the plugin algorithms take; `info_map["input_list"]` has one row per query, so the unchanged
driver loop (`it += len(info_map["input_list"])`) works, and BaseAlgorithm.validation_set recognises the feed and evaluates the
whole set without coming back to Python between batches.

Changed from the host feed: under check_validation, get_batch draws among the queries whose labels do not sum
to 0 (an index built once per dataset) and always returns batch_size lists - the host feed draws among all queries and drops the
all-zero ones, returning a short batch; the sequential calls do not filter (the driver never asks them to).
An interior -1 of a list is a PAD here (document id n_docs, label 0)."""
import ctypes

import torch

from .. import _lib
from .. import hip_ops
from ..utils import HParams
from .device_click_feed import ResidentDataset


class DeviceDirectLabelFeed(object):
    MAX_ONLINE_PICK = 256  # ultr_online_pick_args' candidate limit (get_batch only)

    def __init__(self, model, batch_size, hparam_str, seed=0):
        self.hparams = HParams(use_max_candidate_num=True)
        self.hparams.parse(hparam_str)
        self.rank_list_size = int(model.max_candidate_num if self.hparams.use_max_candidate_num else model.rank_list_size)
        self.feature_size, self.batch_size, self.model = model.feature_size, int(batch_size), model
        self.device = model.cuda
        self.seed, self.step = int(seed), 0
        self.lib = _lib.load()
        self._resident = {}
        L, B, dev = self.rank_list_size, self.batch_size, self.device
        # two buffer sets, used in turn: a batch (and its info_map) stays intact until the second call after it
        self._bufs = [(torch.empty(L * B, dtype=torch.int32, device=dev), torch.empty(L * B, dtype=torch.float32, device=dev),
                       torch.empty(B, dtype=torch.int32, device=dev)) for _ in range(2)]
        self._views = {}
        self._cur = 1
        self._args = _lib.OnlineArgs()
        self._aptr = ctypes.c_void_p(ctypes.addressof(self._args))
        print("Create device direct label feed with list size %d with feature size %d" % (self.rank_list_size, self.feature_size))

    @staticmethod
    def preprocess_data(data_set, hparam_str, exp_settings):
        return

    def _check(self, data_set):
        if len(data_set.initial_list[0]) < self.rank_list_size:
            raise ValueError("Input ranklist length must be no less than the required list size, %d != %d."
                             % (len(data_set.initial_list[0]), self.rank_list_size))

    def _entry(self, data_set):
        key = id(data_set)
        if key not in self._resident:
            self._resident[key] = [data_set, ResidentDataset(data_set, self.device), None]
        return self._resident[key]

    def resident(self, data_set):
        """The dataset in HBM (uploaded at the first use)."""
        return self._entry(data_set)[1]

    def eligible(self, data_set):
        """Index of the queries whose first rank_list_size labels do not sum to 0 (check_validation's filter) - built once."""
        e = self._entry(data_set)
        if e[2] is None:
            rd, L = e[1], self.rank_list_size
            lab = torch.where(rd.lists[:, :L] >= 0, rd.labels[:, :L], torch.zeros((), device=self.device))
            idx = torch.nonzero(lab.double().sum(1) != 0).flatten().to(torch.int32).contiguous()
            e[2] = (idx, int(idx.numel()))
        return e[2]

    def _buffers(self, b):
        """The next buffer set as [L, b] views (b <= batch_size lists)."""
        k = self._cur = 1 - self._cur
        v = self._views.get((k, b))
        if v is None:
            ids, lab, qidx = self._bufs[k]
            L = self.rank_list_size
            v = self._views[(k, b)] = (ids[:L * b].view(L, b), lab[:L * b].view(L, b), qidx[:b])
        return v

    def _feed(self, rd, ids, lab, qidx, b):
        feed = {"device_feed": True, "features": rd.features, "n_docs": rd.n_docs, "docids": ids, "labels": lab, "batch_size": b,
                "feed_obj": None}
        # device tensors, one row per query: the candidates [b, L] (global ids, PAD = n_docs) and their labels [b, L]
        return feed, {"rank_list_idxs": qidx, "input_list": ids.t(), "click_list": lab.t()}

    def _sequential(self, data_set, index, b, check_validation):
        if check_validation:
            raise NotImplementedError("DeviceDirectLabelFeed does not filter sequential batches (check_validation); the driver passes "
                                      "False - use DirectLabelFeed for the filtered walk")
        self._check(data_set)
        rd = self.resident(data_set)
        if not 0 <= index < rd.n_queries or b <= 0:
            raise IndexError("query index %d outside 0 .. %d" % (index, rd.n_queries - 1))
        ids, lab, qidx = self._buffers(b)
        _lib.check(self.lib.ultr_eval_pick(rd.lists.data_ptr(), rd.labels.data_ptr(), rd.n_queries, rd.lmax, rd.n_docs, int(index), b,
                                           self.rank_list_size, ids.data_ptr(), lab.data_ptr(), qidx.data_ptr(), hip_ops.raw_stream()),
                   "ultr_eval_pick")
        return self._feed(rd, ids, lab, qidx, b)

    def get_next_batch(self, index, data_set, check_validation=False, data_format="ULTRA"):
        return self._sequential(data_set, index, min(self.batch_size, len(data_set.initial_list) - index), check_validation)

    def get_data_by_index(self, data_set, index, check_validation=False):
        return self._sequential(data_set, index, 1, check_validation)

    def get_batch(self, data_set, check_validation=False, data_format="ULTRA"):
        self._check(data_set)
        L, B = self.rank_list_size, self.batch_size
        if L > self.MAX_ONLINE_PICK:
            raise NotImplementedError("DeviceDirectLabelFeed.get_batch draws lists of up to %d documents (got %d); the sequential "
                                      "calls take any size" % (self.MAX_ONLINE_PICK, L))
        rd = self.resident(data_set)
        elig, n_elig = self.eligible(data_set) if check_validation else (None, 0)
        if check_validation and n_elig == 0:
            raise ValueError("check_validation: no query of this dataset has a label > 0 among its first %d candidates" % L)
        ids, lab, qidx = self._buffers(B)
        a = self._args
        a.lists, a.labels, a.n_queries, a.n_docs, a.lmax = rd.lists.data_ptr(), rd.labels.data_ptr(), rd.n_queries, rd.n_docs, rd.lmax
        a.eligible, a.n_eligible = (elig.data_ptr(), n_elig) if check_validation else (None, 0)
        a.seed, a.step, a.batch, a.max_candidates = self.seed, self.step, B, L
        a.cand_docids, a.cand_labels, a.query_idx = ids.data_ptr(), lab.data_ptr(), qidx.data_ptr()
        _lib.check(self.lib.ultr_online_pick_args(self._aptr, hip_ops.raw_stream()), "ultr_online_pick_args")
        self.step += 1
        return self._feed(rd, ids, lab, qidx, B)
