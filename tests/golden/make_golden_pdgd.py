#!/usr/bin/env python3
"""Golden vectors of the reference's PDGD (ultra.learning_algorithm.PDGD) and of its two online simulation feeds, recorded by
RUNNING them.

Same procedure and shims as make_golden.py (whose helpers this imports), plus one more: PDGD.train hands torch.as_tensor a list
of np.float32 docids with dtype=int64, which torch 2.10 refuses; the shim turns such a list into an array first.

  pdgd_*        teacher-forced PDGD steps on StochasticOnlineSimulationFeed batches of seeded synthetic data: inputs, pre/post
                parameters and Adagrad state, list scores, loss, pre-clip gradient and norm, the pair list and pair weights
  pdgd_feeds    batches of both online feeds against a stub model whose validation() returns recorded scores (ties, underflowed
                probabilities, PADs), with PBM and cascade clicks, oracle mode and click redraws
  pdgd_online   20 steps of PDGD + StochasticOnlineSimulationFeed on the toy ULTRA data: per-step loss, re-ranked docids, labels,
                final parameters
  pdgd_ipw_online   one IPWrank step on a StochasticOnlineSimulationFeed batch

A batch without a single pair cannot be recorded: the reference's pair scoring fails on empty docid lists (pdgd.py:193-198).

Usage:  python tests/golden/make_golden_pdgd.py [--only NAME]
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import (Recorder, adagrad_state, feed_arrays, flat_params, import_reference, make_dataset,  # noqa: E402
                         quiet)

CLICK = {"pbm": "./example/ClickModel/pbm_0.1_1.0_4_1.0.json", "cascade": "./example/ClickModel/cascade_0.1_1.0_4_1.0.json"}


def install_pdgd_shim():
    _as = torch.as_tensor

    def as_tensor(data, dtype=None, device=None):
        if isinstance(data, (list, tuple)) and data and isinstance(data[0], np.generic):
            data = np.asarray(data)
        return _as(data, dtype=dtype, device=device)

    torch.as_tensor = as_tensor


def pdgd_exp(M, cutoff, hidden, algo_hparams, model_cls="ultra.ranking_model.DNN"):
    return {
        "learning_algorithm": "ultra.learning_algorithm.PDGD",
        "learning_algorithm_hparams": algo_hparams,
        "ranking_model": model_cls,
        "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(hidden) if hidden is not None else "",
        "max_candidate_num": M,
        "selection_bias_cutoff": cutoff,
        "metrics": ["ndcg"],
        "metrics_topn": [1, 3, 5],
    }


def run_pdgd_case(ultra, name, F, M, cutoff, B, hidden, seed, n_steps=2, list_lens=None, n_queries=48, algo_hparams="",
                  feed_hparams="", model_cls="ultra.ranking_model.DNN"):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)
    ds = make_dataset(ultra, seed, n_queries, list_lens or M, F)
    exp = pdgd_exp(M, cutoff, hidden, algo_hparams, model_cls)
    ds.pad(M)
    algo = quiet(ultra.utils.find_class(exp["learning_algorithm"]), ds, exp)
    feed = quiet(ultra.utils.find_class("ultra.input_layer.StochasticOnlineSimulationFeed"), algo, B, feed_hparams)
    rec = Recorder(algo)
    hp = algo.hparams
    out = {"meta": json.dumps({
        "name": name, "algo": "pdgd", "F": F, "M": M, "cutoff": cutoff, "B": B, "hidden": hidden, "n_steps": n_steps,
        "seed": seed, "model": model_cls.rsplit(".", 1)[1], "algo_hparams": algo_hparams, "feed_hparams": feed_hparams,
        "param_keys": list(algo.model.state_dict().keys()),
        "param_shapes": [list(v.shape) for v in algo.model.state_dict().values()],
        "lr": float(algo.learning_rate), "max_gradient_norm": float(hp.max_gradient_norm), "tau": float(hp.tau),
        "l2_loss": float(hp.l2_loss), "grad_strategy": hp.grad_strategy,
    })}
    for t in range(n_steps):
        rec.reset()
        input_feed, _ = quiet(feed.get_batch, ds, check_validation=True)
        feats, docids, labels = feed_arrays(algo, input_feed, M)
        pre = {"params": flat_params(algo.model), "adagrad": adagrad_state(algo.optimizer_func, algo.model)}
        loss, _, _ = quiet(algo.train, input_feed)
        p = "s%d_" % t
        out[p + "features"] = feats
        out[p + "docids"] = docids
        out[p + "labels"] = labels
        for k, v in pre.items():
            out[p + "pre_" + k] = v
        out[p + "scores"] = rec.scores.astype(np.float32)
        out[p + "loss"] = np.float64(loss)
        out[p + "post_params"] = flat_params(algo.model)
        (g, n_), = rec.clips
        out[p + "grads"] = g
        out[p + "norm"] = np.float32(n_)
        out[p + "post_adagrad"] = adagrad_state(algo.optimizer_func, algo.model)
        out[p + "pair_pos"] = algo.positive_docid_inputs.numpy().astype(np.int32)
        out[p + "pair_neg"] = algo.negative_docid_inputs.numpy().astype(np.int32)
        out[p + "pair_weights"] = algo.pair_weights.cpu().numpy()
    rec.close()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, [float(out["s%d_loss" % t]) for t in range(n_steps)],
          [int(out["s%d_pair_weights" % t].size) for t in range(n_steps)])


class StubModel:
    """What the online feeds read from a learning algorithm; validation() returns seeded scores and records them."""

    def __init__(self, feature_size, rank_list_size, max_candidate_num, seed):
        self.feature_size, self.rank_list_size, self.max_candidate_num = feature_size, rank_list_size, max_candidate_num
        self.letor_features_name = "letor_features"
        self.docid_inputs_name = ["docid_input%d" % i for i in range(max_candidate_num)]
        self.labels_name = ["label%d" % i for i in range(max_candidate_num)]
        self.hparams = type("H", (), {})()
        self.is_cuda_avail = False
        self.rng = np.random.RandomState(seed)
        self.calls = []

    def validation(self, input_feed, is_online_simulation=False):
        B = len(input_feed[self.docid_inputs_name[0]])
        s = (self.rng.standard_normal((B, self.max_candidate_num)) * 2.0).astype(np.float32)
        s[self.rng.uniform(size=s.shape) < 0.3] = np.float32(0.5)  # ties
        s[self.rng.uniform(size=s.shape) < 0.15] = np.float32(-300.0)  # underflows to probability 0
        self.calls.append(s.copy())
        return None, torch.from_numpy(s), {}


FEED_CASES = [  # (key, feed class, hparams, check_validation, n_batches, batch size)
    ("sto_pbm", "StochasticOnlineSimulationFeed", "click_model_json=%s" % CLICK["pbm"], True, 3, 6),
    ("sto_cascade", "StochasticOnlineSimulationFeed", "click_model_json=%s,tau=2" % CLICK["cascade"], True, 3, 6),
    ("sto_oracle", "StochasticOnlineSimulationFeed", "oracle_mode=True", False, 2, 5),
    ("sto_eta", "StochasticOnlineSimulationFeed", "dynamic_bias_eta_change=0.5,dynamic_bias_step_interval=2", False, 3, 4),
    ("det_pbm", "DeterministicOnlineSimulationFeed", "click_model_json=%s" % CLICK["pbm"], True, 3, 6),
    ("det_cascade", "DeterministicOnlineSimulationFeed", "click_model_json=%s" % CLICK["cascade"], False, 2, 6),
]


def run_feeds_case(ultra, name, seed=101):
    data_dir = os.path.join(HERE, "ultra_toy_data") + "/"
    ds = quiet(ultra.utils.read_data, data_dir, "train", None, None)
    M, cutoff = ds.rank_list_size, 5
    ds.pad(M)
    out = {}
    for ci, (key, cls, hparams, check, n_batches, B) in enumerate(FEED_CASES):
        model = StubModel(ds.feature_size, cutoff, M, seed + ci)
        random.seed(seed + ci)
        np.random.seed(seed + ci)
        feed = quiet(ultra.utils.find_class("ultra.input_layer." + cls), model, B, hparams)
        for t in range(n_batches):
            f, info = quiet(feed.get_batch, ds, check_validation=check)
            fe, ids, lab = feed_arrays(model, f, M)
            p = "%s_b%d_" % (key, t)
            out[p + "docids"], out[p + "labels"], out[p + "n_features"] = ids, lab, np.int32(fe.shape[0])
            out[p + "idxs"] = np.asarray(info["rank_list_idxs"], dtype=np.int32)
            out[p + "scores"] = model.calls[-1]
        out[key + "_eta"] = np.float64(getattr(feed.click_model, "eta", 0.0))
        # get_next_batch / get_data_by_index: the deterministic feed's work in the reference (the stochastic one's crash there)
        if cls.startswith("Deterministic"):
            f, _ = quiet(feed.get_next_batch, 3, ds, check_validation=False)
            out[key + "_next_docids"], out[key + "_next_labels"] = feed_arrays(model, f, M)[1:]
            out[key + "_next_scores"] = model.calls[-1]
            f, _ = quiet(feed.get_data_by_index, ds, 7, check_validation=False)
            out[key + "_byidx_docids"], out[key + "_byidx_labels"] = feed_arrays(model, f, M)[1:]
            out[key + "_byidx_scores"] = model.calls[-1]
    out["meta"] = json.dumps({"name": name, "seed": seed, "M": int(M), "cutoff": cutoff, "F": int(ds.feature_size),
                              "cases": FEED_CASES})
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name)


def run_online_case(ultra, name, seed=111, n_steps=20, B=4, hidden=(16, 8)):
    """PDGD + StochasticOnlineSimulationFeed end to end on the toy ULTRA data."""
    data_dir = os.path.join(HERE, "ultra_toy_data") + "/"
    ds = quiet(ultra.utils.read_data, data_dir, "train", None, None)
    M, cutoff = ds.rank_list_size, 5
    ds.pad(M)
    torch.manual_seed(seed)
    exp = pdgd_exp(M, cutoff, list(hidden), "")
    algo = quiet(ultra.utils.find_class(exp["learning_algorithm"]), ds, exp)
    random.seed(seed)
    np.random.seed(seed)
    feed = quiet(ultra.utils.find_class("ultra.input_layer.StochasticOnlineSimulationFeed"), algo, B, "")
    out = {"init_params": flat_params(algo.model)}
    losses = []
    for t in range(n_steps):
        f, info = quiet(feed.get_batch, ds, check_validation=True)
        _, ids, lab = feed_arrays(algo, f, M)
        out["s%d_docids" % t], out["s%d_labels" % t] = ids, lab
        out["s%d_idxs" % t] = np.asarray(info["rank_list_idxs"], dtype=np.int32)
        loss, _, _ = quiet(algo.train, f)
        losses.append(loss)
    out["losses"] = np.asarray(losses, dtype=np.float64)
    out["final_params"] = flat_params(algo.model)
    out["final_adagrad"] = adagrad_state(algo.optimizer_func, algo.model)
    out["meta"] = json.dumps({"name": name, "seed": seed, "M": int(M), "cutoff": cutoff, "B": B, "hidden": list(hidden),
                              "n_steps": n_steps, "F": int(ds.feature_size), "lr": float(algo.learning_rate),
                              "param_keys": list(algo.model.state_dict().keys()),
                              "param_shapes": [list(v.shape) for v in algo.model.state_dict().values()]})
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, losses)


def run_ipw_online_case(ultra, name, seed=121, B=6, hidden=(16, 8)):
    data_dir = os.path.join(HERE, "ultra_toy_data") + "/"
    ds = quiet(ultra.utils.read_data, data_dir, "train", None, None)
    M, cutoff = ds.rank_list_size, 5
    ds.pad(M)
    torch.manual_seed(seed)
    exp = pdgd_exp(M, cutoff, list(hidden), "")
    exp["learning_algorithm"] = "ultra.learning_algorithm.IPWrank"
    algo = quiet(ultra.utils.find_class(exp["learning_algorithm"]), ds, exp)
    random.seed(seed)
    np.random.seed(seed)
    feed = quiet(ultra.utils.find_class("ultra.input_layer.StochasticOnlineSimulationFeed"), algo, B, "")
    f, _ = quiet(feed.get_batch, ds, check_validation=True)
    fe, ids, lab = feed_arrays(algo, f, M)
    rec = Recorder(algo)
    out = {"features": fe, "docids": ids, "labels": lab, "pre_params": flat_params(algo.model)}
    loss, _, _ = quiet(algo.train, f)
    rec.close()
    out["scores"] = rec.scores.astype(np.float32)
    out["loss"] = np.float64(loss)
    out["post_params"] = flat_params(algo.model)
    out["post_adagrad"] = adagrad_state(algo.optimizer_func, algo.model)
    out["meta"] = json.dumps({"name": name, "seed": seed, "M": int(M), "cutoff": cutoff, "B": B, "hidden": list(hidden),
                              "F": int(ds.feature_size), "lr": float(algo.learning_rate),
                              "max_gradient_norm": float(algo.hparams.max_gradient_norm)})
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, loss)


CASES = {
    "pdgd_tiny": lambda u: run_pdgd_case(u, "pdgd_tiny", 24, 10, 10, 8, [32, 16], 91),
    "pdgd_sgd_tau2": lambda u: run_pdgd_case(u, "pdgd_sgd_tau2", 24, 10, 10, 8, [16, 8], 92,
                                             algo_hparams="grad_strategy=sgd,l2_loss=0,tau=2"),
    "pdgd_linear": lambda u: run_pdgd_case(u, "pdgd_linear", 24, 10, 10, 8, None, 93, algo_hparams="l2_loss=0",
                                           model_cls="ultra.ranking_model.Linear"),
    # cutoff 6 < max_candidate_num 12, lists of 3 .. 12 documents: PADs inside and past the cutoff; graded labels
    "pdgd_cutoff": lambda u: run_pdgd_case(u, "pdgd_cutoff", 16, 12, 6, 8, [16, 8], 94, n_steps=3, list_lens=(3, 12),
                                           algo_hparams="tau=2", feed_hparams="oracle_mode=True"),
    "pdgd_feeds": lambda u: run_feeds_case(u, "pdgd_feeds"),
    "pdgd_online": lambda u: run_online_case(u, "pdgd_online"),
    "pdgd_ipw_online": lambda u: run_ipw_online_case(u, "pdgd_ipw_online"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.set_num_threads(1)  # bit-stable fixtures
    ultra = import_reference()
    install_pdgd_shim()
    for name, fn in CASES.items():
        if args.only and args.only != name:
            continue
        fn(ultra)


if __name__ == "__main__":
    main()
