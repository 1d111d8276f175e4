"""IPWrank — inverse propensity weighting with a pre-estimated propensity table.
Drop-in for ultra.learning_algorithm.IPWrank (reference ipw_rank.py:31-211)."""
import collections.abc
import json
import os

import numpy as np
import torch

from .. import _lib, hip_ops
from ..utils import HParams
from .base_algorithm import BaseAlgorithm


def resolve_estimator_json(path):
    """The reference resolves its default relative to the repo root; the same files ship in ultra_pytorch_amd/data."""
    if not os.path.exists(path):
        alt = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", os.path.basename(path))
        path = alt if os.path.exists(alt) else path
    return path


def load_ipw_list(path):
    """BasicPropensityEstimator.loadEstimatorFromFile: the JSON's "IPW_list" (propensity_estimator.py:44-56)."""
    with open(resolve_estimator_json(path)) as fin:
        return [float(x) for x in json.load(fin)["IPW_list"]]


TABLE_ESTIMATORS = ("RandomizedPropensityEstimator", "BasicPropensityEstimator")
ORACLE_ESTIMATOR = "OraclePropensityEstimator"


class PropensitySource(object):
    """What IPWrank / PRSrank train with, chosen by the last component of `propensity_estimator_type` (the reference's
    find_class(type)(json), ipw_rank.py:60-62; `ultra.` and `ultra_pytorch_amd.` module paths name the same classes):

      Randomized / BasicPropensityEstimator   the JSON's IPW_list as the loss kernels' position table (ipw_table)
      OraclePropensityEstimator, position-biased or cascade click model
                                              weight_table's [L] table through the same argument: no other launch
      OraclePropensityEstimator, user-browsing click model
                                              weight_table's [L, L] table, uploaded once per list size; every step queues
                                              hip_ops.history_pw on the step's stream, which fills ONE [B, L] buffer per engine (the same
                                              tensor object every step: train_step's pointer cache holds) handed to the step as pw

    all_positions: PRSrank's use_non_clicked_data=True."""

    def __init__(self, estimator_type, json_path, device, all_positions):
        from ..utils import propensity_estimator as PE
        name = str(estimator_type).rsplit(".", 1)[-1]
        self.device, self.all_positions = device, bool(all_positions)
        self.oracle = name == ORACLE_ESTIMATOR
        self._tables = {}
        if name in TABLE_ESTIMATORS:
            self.IPW_list = load_ipw_list(json_path)
            self.estimator = getattr(PE, name)()
            self.estimator.IPW_list = self.IPW_list
            self._ipw_table = torch.tensor(self.IPW_list, dtype=torch.float32, device=device)
        elif self.oracle:
            self.estimator = PE.OraclePropensityEstimator(resolve_estimator_json(json_path))
            self.IPW_list = None
        else:
            raise NotImplementedError("propensity_estimator_type %r: IPWrank and PRSrank train with %s"
                                      % (estimator_type, ", ".join(TABLE_ESTIMATORS + (ORACLE_ESTIMATOR,))))

    def _oracle_table(self, L):
        t = self._tables.get(L)
        if t is None:
            kind, w = self.estimator.weight_table(L)
            t = self._tables[L] = (kind, torch.from_numpy(w).to(self.device), _lib.HistoryPwArgs())
        return t

    def step_weights(self, eng, labels_LB, L):
        """(ipw_table, pw) for eng.train_step on this batch; the history case queues its weight launch on the current stream."""
        if not self.oracle:
            return self._ipw_table, None
        kind, table, args = self._oracle_table(L)
        if kind == "position":
            return table, None
        buf = getattr(eng, "oracle_pw", None)
        if buf is None:
            buf = eng.oracle_pw = torch.zeros(eng.B, eng.L, dtype=torch.float32, device=self.device)
        hip_ops.history_pw(labels_LB, table, buf, self.all_positions, args=args)
        return None, buf

    def host_weights(self, clicks_LB):
        """[L, B] float64, the estimator's own getPropensityForOneList per list of the host copy of the clicks."""
        L, B = clicks_LB.shape
        out = np.empty((L, B), np.float64)
        for b in range(B):
            out[:, b] = self.estimator.getPropensityForOneList(clicks_LB[:, b].tolist(), self.all_positions)
        return out


class _LazyColumn(collections.abc.Sequence):
    """`propensity_weights{l}` as the reference leaves it in the feed (a Python list of B floats, ipw_rank.py:118-128),
    materialised on first use: nothing in main.py reads these entries, and ten `.tolist()` calls per step were a third of the
    Python time of `train` at config 2."""
    __slots__ = ("_owner", "_l", "_list")

    def __init__(self, owner, l):
        self._owner, self._l, self._list = owner, l, None

    def tolist(self):
        if self._list is None:
            self._list = self._owner.matrix()[self._l].tolist()
        return self._list

    def __getitem__(self, i):
        return self.tolist()[i]

    def __len__(self):
        return self._owner.batch

    def __eq__(self, other):
        return self.tolist() == (other.tolist() if isinstance(other, _LazyColumn) else other)

    def __repr__(self):
        return repr(self.tolist())


class _LazyWeights(object):
    """pw[l, b] = click[l, b] > 0 ? IPW_list[min(l, len - 1)] : 0 (propensity_estimator.py:22-42), computed when first read."""
    __slots__ = ("clicks", "table", "batch", "_pw")

    def __init__(self, clicks, table):
        self.clicks, self.table, self.batch, self._pw = clicks, table, int(clicks.shape[1]), None

    def matrix(self):  # [L, B]
        if self._pw is None:
            self._pw = np.where(self.clicks > 0, self.table[:, None], 0.0)
        return self._pw


class _LazyEstimatorWeights(object):
    """The same for an estimator that reads the whole click list (the Oracle): PropensitySource.host_weights when first read."""
    __slots__ = ("clicks", "source", "batch", "_pw")

    def __init__(self, clicks, source):
        self.clicks, self.source, self.batch, self._pw = clicks, source, int(clicks.shape[1]), None

    def matrix(self):  # [L, B]
        if self._pw is None:
            self._pw = self.source.host_weights(self.clicks)
        return self._pw


class IPWrank(BaseAlgorithm):
    ENGINE_ALGO = "softmax"

    def __init__(self, data_set, exp_settings):
        self.hparams = HParams(
            propensity_estimator_type="ultra.utils.propensity_estimator.RandomizedPropensityEstimator",
            propensity_estimator_json="./example/PropensityEstimator/randomized_pbm_0.1_1.0_4_1.0.json",
            learning_rate=0.05, max_gradient_norm=5.0, loss_func="softmax_loss", l2_loss=0.0, grad_strategy="ada")
        print(exp_settings["learning_algorithm_hparams"])
        self.hparams.parse(exp_settings["learning_algorithm_hparams"])
        self._check_hparams()
        self._setup(data_set, exp_settings)
        self.propensity = PropensitySource(self.hparams.propensity_estimator_type, self.hparams.propensity_estimator_json, self.cuda,
                                           all_positions=False)
        self.propensity_estimator = self.propensity.estimator
        self.IPW_list = self.propensity.IPW_list  # None for the Oracle: it has no table
        self.ipw_table = None if self.propensity.oracle else self.propensity._ipw_table
        self._pw_table, self._lazy_pw = None, None
        self._pw_names = ["propensity_weights{0}".format(l) for l in range(self.max_candidate_num)]

    @property
    def propensity_weights(self):
        """[B, L], what the reference keeps as a list of per-list weight lists (ipw_rank.py:130)."""
        return None if self._lazy_pw is None else self._lazy_pw.matrix().T

    def train(self, input_feed):
        """ipw_rank.py:102-182.  The per-list Python loop over getPropensityForOneList is folded into the loss
        kernel (pw = click > 0 ? IPW_list[min(l, len-1)] : 0); the feed still gets the `propensity_weights{l}`
        entries the reference adds (ipw_rank.py:118-128)."""
        self.global_step += 1
        if not self.model.training:  # (nn.Module.train() walks every submodule: ~10 us a 47 us step does not have)
            self.model.train()
        L = self.rank_list_size
        clicks = self.create_input_feed(input_feed, L)  # [L, B] host (None for a device feed)
        if clicks is not None:
            if self.propensity.oracle:
                self._lazy_pw = lazy = _LazyEstimatorWeights(clicks.copy(), self.propensity)
            else:
                if self._pw_table is None or self._pw_table.shape[0] != L:
                    self._pw_table = np.asarray([self.IPW_list[min(l, len(self.IPW_list) - 1)] for l in range(L)])
                self._lazy_pw = lazy = _LazyWeights(clicks.copy(), self._pw_table)  # own copy: `clicks` is a view of the staging buffer
            for l in range(L):
                input_feed[self._pw_names[l]] = _LazyColumn(lazy, l)
        eng = self._train_engine(self.batch_size, L)
        ipw_table, pw = self.ipw_table, None
        if self.propensity.oracle:
            ipw_table, pw = self.propensity.step_weights(eng, self.labels_LB, L)
        sc = eng.train_step(self.model.flat_params, self.state_sum, self.letor_features, self.n_docs, self.docid_inputs,
                            self.labels_LB, ipw_table=ipw_table, pw=pw)
        self.loss = eng.read_loss()
        print(" Loss %f at Global Step %d: " % (self.loss, self.global_step))
        return self.loss, None, self.train_summary
