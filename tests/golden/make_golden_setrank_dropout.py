#!/usr/bin/env python3
"""Golden vectors of the reference's SetRank with dropout (ultra.ranking_model.SetRank.SetRank, rate > 0) under IPWrank,
recorded by RUNNING it.

torch's own dropout stream is not what this package draws, so the reference Encoder's nn.Dropout instances (`dropout`,
`encoder{i}.dropout1`, `encoder{i}.dropout2`) are replaced by modules that multiply by the restated mask of their site
(tests/setrank_dropout_ref.mask; the reference's [B, L, d] maps to the token t = l * B + b).  What the fixture pins is WHERE the
reference drops: on which tensors, before which residual, with which scale, in training mode only.  Everything else is
make_golden.py's procedure (whose helpers this imports): seeded synthetic data, ClickSimulationFeed batches, two teacher-forced
steps with inputs, pre / post parameters, Adagrad state, scores, loss, the pre-clip gradient and its norm.

Usage:  python tests/golden/make_golden_setrank_dropout.py
"""
import json
import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import (Recorder, adagrad_state, feed_arrays, flat_params, import_reference, make_dataset,  # noqa: E402
                         quiet)
from tests import setrank_dropout_ref as R  # noqa: E402


class Clock:
    """The count of training forwards: site 0 runs first in every forward and takes the next step."""

    def __init__(self, seed, rate):
        self.seed, self.rate, self.count, self.step = seed, rate, 0, None


class SiteMask(nn.Module):
    def __init__(self, clock, site):
        super().__init__()
        self.clock, self.site = clock, site

    def forward(self, x):
        if not self.training:
            return x
        c = self.clock
        if self.site == 0:
            c.step, c.count = c.count, c.count + 1
        B, L, d = x.shape
        return x * torch.from_numpy(R.mask(c.seed, c.step, 0, self.site, B, L, d, c.rate)).to(x.device)


def run_case(ultra, name, F, L, B, seed, rate, drop_seed, model_extra, n_steps=2, n_queries=64):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)
    ds = make_dataset(ultra, seed, n_queries, L, F)
    exp = {
        "learning_algorithm": "ultra.learning_algorithm.IPWrank",
        "learning_algorithm_hparams": "",
        "ranking_model": "ultra.ranking_model.SetRank.SetRank",
        "ranking_model_hparams": model_extra + ",rate=%g" % rate,
        "max_candidate_num": L,
        "selection_bias_cutoff": L,
        "metrics": ["ndcg", "mrr", "err"],
        "metrics_topn": [1, 3, 5, 10],
    }
    ds.pad(L)
    algo = quiet(ultra.utils.find_class(exp["learning_algorithm"]), ds, exp)
    enc = algo.model.Encoder_layer
    clock = Clock(drop_seed, rate)
    assert isinstance(enc.dropout, nn.Dropout) and enc.dropout.p == rate
    enc.dropout = SiteMask(clock, 0)
    n_layers = 0
    for i, layer in enumerate(enc.enc_layers):
        assert isinstance(layer.dropout1, nn.Dropout) and isinstance(layer.dropout2, nn.Dropout)
        layer.dropout1, layer.dropout2 = SiteMask(clock, 1 + 2 * i), SiteMask(clock, 2 + 2 * i)
        n_layers += 1
    assert not any(isinstance(m, nn.Dropout) for m in algo.model.modules())
    feed = quiet(ultra.utils.find_class("ultra.input_layer.ClickSimulationFeed"), algo, B, "")
    rec = Recorder(algo)
    out = {"meta": json.dumps({
        "name": name, "algo": "ipw", "F": F, "L": L, "B": B, "hidden": None, "n_steps": n_steps, "seed": seed,
        "model": "SetRank", "model_hparams": exp["ranking_model_hparams"], "algo_hparams": "",
        "param_keys": list(algo.model.state_dict().keys()),
        "param_shapes": [list(v.shape) for v in algo.model.state_dict().values()],
        "lr": float(algo.learning_rate), "max_gradient_norm": float(algo.hparams.max_gradient_norm),
    })}
    out["ipw_list"] = np.asarray(algo.propensity_estimator.IPW_list, dtype=np.float64)
    out["rate"] = np.float32(rate)
    out["seed"] = np.uint64(drop_seed)
    steps = []
    for t in range(n_steps):
        rec.reset()
        input_feed, _ = feed.get_batch(ds, check_validation=True)
        feats, docids, labels = feed_arrays(algo, input_feed, L)
        pre = {"params": flat_params(algo.model), "adagrad": adagrad_state(algo.optimizer_func, algo.model)}
        loss, _, _ = quiet(algo.train, input_feed)
        steps.append(clock.step)
        p = "s%d_" % t
        out[p + "features"] = feats
        out[p + "docids"] = docids
        out[p + "labels"] = labels
        for k, v in pre.items():
            out[p + "pre_" + k] = v
        out[p + "scores"] = rec.scores.astype(np.float32)
        out[p + "loss"] = np.float32(loss)
        out[p + "post_params"] = flat_params(algo.model)
        (g, n_), = rec.clips
        out[p + "grads"] = g
        out[p + "norm"] = np.float32(n_)
        out[p + "post_adagrad"] = adagrad_state(algo.optimizer_func, algo.model)
        out[p + "pw"] = np.asarray(algo.propensity_weights, dtype=np.float32)
    rec.close()
    assert steps == list(range(n_steps)), steps  # one training forward per step
    out["steps"] = np.asarray(steps, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, [float(out["s%d_loss" % t]) for t in range(n_steps)])


def main():
    torch.set_num_threads(1)  # bit-stable fixtures
    ultra = import_reference()
    run_case(ultra, "setrank_dropout_tiny", F=20, L=6, B=4, seed=97, rate=0.25, drop_seed=0x5EED0D20,
             model_extra="d_model=32,num_heads=4,num_layers=2,diff=16")


if __name__ == "__main__":
    main()
