#!/usr/bin/env python3
"""Golden vectors of the reference's PRSrank (ultra.learning_algorithm.PRSrank), recorded by RUNNING it.

Same procedure and shims as make_golden.py (whose helpers this imports): seeded synthetic data, ClickSimulationFeed
batches, two teacher-forced steps per case with inputs, pre/post parameters, Adagrad state, scores, loss, the clipped
gradient and its norm, plus the estimator's IPW_list.  The reference prints three debug tensors per step; `quiet`
swallows them.

Usage:  python tests/golden/make_golden_prs.py [--only NAME]
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


def run_prs_case(ultra, name, F, L, B, hidden, seed, n_steps=2, n_queries=64, model_cls="ultra.ranking_model.DNN",
                 algo_hparams="", model_extra=""):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)
    ds = make_dataset(ultra, seed, n_queries, L, F)
    exp = {
        "learning_algorithm": "ultra.learning_algorithm.PRSrank",
        "learning_algorithm_hparams": algo_hparams,
        "ranking_model": model_cls,
        "ranking_model_hparams": ("hidden_layer_sizes=%s" % json.dumps(hidden) if hidden is not None else "") + model_extra,
        "max_candidate_num": L,
        "selection_bias_cutoff": L,
        "metrics": ["ndcg"],
        "metrics_topn": [1, 3, 5, 10],
    }
    ds.pad(L)
    algo = quiet(ultra.utils.find_class(exp["learning_algorithm"]), ds, exp)
    feed = quiet(ultra.utils.find_class("ultra.input_layer.ClickSimulationFeed"), algo, B, "")
    rec = Recorder(algo)
    out = {"meta": json.dumps({
        "name": name, "algo": "prs", "F": F, "L": L, "B": B, "hidden": hidden, "n_steps": n_steps, "seed": seed,
        "model": model_cls.rsplit(".", 1)[1], "model_hparams": exp["ranking_model_hparams"], "algo_hparams": algo_hparams,
        "param_keys": list(algo.model.state_dict().keys()),
        "param_shapes": [list(v.shape) for v in algo.model.state_dict().values()],
        "lr": float(algo.learning_rate), "max_gradient_norm": float(algo.hparams.max_gradient_norm),
        "sigma": float(algo.hparams.sigma), "grad_strategy": algo.hparams.grad_strategy,
    })}
    out["ipw_list"] = np.asarray(algo.propensity_estimator.IPW_list, dtype=np.float64)
    for t in range(n_steps):
        rec.reset()
        input_feed, _ = feed.get_batch(ds, check_validation=True)
        feats, docids, labels = feed_arrays(algo, input_feed, L)
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
    rec.close()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, [float(out["s%d_loss" % t]) for t in range(n_steps)])


CASES = {
    "prs_tiny": lambda u: run_prs_case(u, "prs_tiny", 136, 10, 8, [32, 16], 81),
    "prs_odd": lambda u: run_prs_case(u, "prs_odd", 13, 7, 9, [19, 6, 3], 82, n_queries=32),
    "prs_sgd": lambda u: run_prs_case(u, "prs_sgd", 24, 10, 8, [16, 8], 83, algo_hparams="grad_strategy=sgd"),
    "prs_setrank_tiny": lambda u: run_prs_case(u, "prs_setrank_tiny", 24, 10, 8, None, 84,
                                               model_cls="ultra.ranking_model.SetRank.SetRank",
                                               model_extra="d_model=32,num_heads=4,num_layers=2,diff=16"),
    # L 50 against the shipped 40-entry IPW_list: positions 40..49 take its last entry
    "prs_l50": lambda u: run_prs_case(u, "prs_l50", 24, 50, 8, [16, 8], 85, n_queries=32),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.set_num_threads(1)  # bit-stable fixtures
    ultra = import_reference()
    for name, fn in CASES.items():
        if args.only and args.only != name:
            continue
        fn(ultra)


if __name__ == "__main__":
    main()
