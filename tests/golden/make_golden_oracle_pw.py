#!/usr/bin/env python3
"""Golden vectors of the reference's IPWrank / PRSrank trained with its OraclePropensityEstimator, recorded by RUNNING them.

Same procedure and shims as make_golden_prs.py (whose helpers come from make_golden.py): seeded synthetic data, two teacher-forced
steps per case with inputs, pre/post parameters, Adagrad state, scores, loss, the clipped gradient and its norm - plus the [B, L]
weights the reference formed from each list's clicks.

The reference cannot build this configuration from a settings file (find_class(type)(json_path) hands the Oracle the file NAME as
its click model), so the learner is built normally and its estimator replaced by OraclePropensityEstimator(click model), behind a
wrapper that casts the click list to ints (`use_non_clicked_data | click_list[r] > 0` raises on float clicks) and keeps the weights.
The batches come from ClickSimulationFeed on the shipped user-browsing-model JSON, so that lists carry several clicks; the Oracle's
own click model is the case's (`oracle_model`).

Usage:  python tests/golden/make_golden_oracle_pw.py [--only NAME]      (writes tests/golden/oracle_pw/<case>.npz)
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "oracle_pw")  # a directory of its own: tests/test_loss_ref_cpu.py takes every tests/golden/ipw_*.npz for a TABLE step
sys.path.insert(0, HERE)
from make_golden import (REF, Recorder, adagrad_state, feed_arrays, flat_params, import_reference, make_dataset,  # noqa: E402
                         quiet)

UBM, PBM = "ubm_0.1_1_4_1.0.json", "pbm_0.1_1.0_4_1.0.json"
ALGOS = {"ipw": "ultra.learning_algorithm.IPWrank", "prs": "ultra.learning_algorithm.PRSrank"}


class IntClicks(object):
    """The Oracle behind an int cast of the click list; keeps every list's weights of the current step."""

    def __init__(self, inner):
        self.inner, self.rows = inner, []

    def getPropensityForOneList(self, click_list, use_non_clicked_data=False):
        w = self.inner.getPropensityForOneList([int(c) for c in click_list], use_non_clicked_data)
        self.rows.append(list(w))
        return w


def run_case(ultra, name, algo_key, oracle_model, F, L, B, hidden, seed, n_steps=2, n_queries=64, model_cls="ultra.ranking_model.DNN",
             model_extra=""):
    from ultra.utils import click_models as RCM
    from ultra.utils.propensity_estimator import OraclePropensityEstimator
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)
    ds = make_dataset(ultra, seed, n_queries, L, F)
    exp = {
        "learning_algorithm": ALGOS[algo_key],
        "learning_algorithm_hparams": "",
        "ranking_model": model_cls,
        "ranking_model_hparams": ("hidden_layer_sizes=%s" % json.dumps(hidden) if hidden is not None else "") + model_extra,
        "max_candidate_num": L,
        "selection_bias_cutoff": L,
        "metrics": ["ndcg"],
        "metrics_topn": [1, 3, 5, 10],
    }
    ds.pad(L)
    algo = quiet(ultra.utils.find_class(exp["learning_algorithm"]), ds, exp)
    with open(os.path.join(REF, "example", "ClickModel", oracle_model)) as fin:
        click_model = RCM.loadModelFromJson(json.load(fin))
    est = algo.propensity_estimator = IntClicks(OraclePropensityEstimator(click_model))
    feed = quiet(ultra.utils.find_class("ultra.input_layer.ClickSimulationFeed"), algo, B,
                 "click_model_json=./example/ClickModel/" + UBM)
    rec = Recorder(algo)
    meta = {
        "name": name, "algo": algo_key, "F": F, "L": L, "B": B, "hidden": hidden, "n_steps": n_steps, "seed": seed,
        "model": model_cls.rsplit(".", 1)[1], "model_hparams": exp["ranking_model_hparams"], "algo_hparams": "",
        "param_keys": list(algo.model.state_dict().keys()),
        "param_shapes": [list(v.shape) for v in algo.model.state_dict().values()],
        "lr": float(algo.learning_rate), "max_gradient_norm": float(algo.hparams.max_gradient_norm),
        "grad_strategy": algo.hparams.grad_strategy, "oracle_model": oracle_model, "feed_model": UBM,
        "oracle_model_json": click_model.getModelJson(),
    }
    if algo_key == "prs":
        meta["sigma"] = float(algo.hparams.sigma)
    out = {"meta": json.dumps(meta)}
    for t in range(n_steps):
        rec.reset()
        est.rows = []
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
        # the weights as the step used them: torch.as_tensor(list of Python floats) is float32 (ipw_rank.py:138, prs_rank.py:116)
        out[p + "pw"] = torch.as_tensor(est.rows).numpy().astype(np.float32)  # [B, L]
        assert out[p + "pw"].shape == (B, L)
    rec.close()
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print("wrote", name, [float(out["s%d_loss" % t]) for t in range(n_steps)],
          "clicks per list %.2f" % float((out["s0_labels"] > 0).sum() / B))


SETRANK = dict(model_cls="ultra.ranking_model.SetRank.SetRank", model_extra="d_model=32,num_heads=4,num_layers=2,diff=16")
CASES = {
    "ipw_oracle_ubm_tiny": lambda u: run_case(u, "ipw_oracle_ubm_tiny", "ipw", UBM, 136, 10, 8, [32, 16], 91),
    "ipw_oracle_ubm_odd": lambda u: run_case(u, "ipw_oracle_ubm_odd", "ipw", UBM, 13, 7, 9, [19, 6, 3], 92, n_queries=32),
    "ipw_oracle_pbm_tiny": lambda u: run_case(u, "ipw_oracle_pbm_tiny", "ipw", PBM, 136, 10, 8, [32, 16], 93),
    "prs_oracle_ubm_tiny": lambda u: run_case(u, "prs_oracle_ubm_tiny", "prs", UBM, 136, 10, 8, [32, 16], 94),
    # L 50: ranks past the user-browsing model's 10 rows (click_models.py:174-185)
    "prs_oracle_ubm_l50": lambda u: run_case(u, "prs_oracle_ubm_l50", "prs", UBM, 24, 50, 8, [16, 8], 95, n_queries=32),
    "ipw_oracle_ubm_setrank_tiny": lambda u: run_case(u, "ipw_oracle_ubm_setrank_tiny", "ipw", UBM, 24, 10, 8, None, 96, **SETRANK),
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
