#!/usr/bin/env python3
"""Golden vectors of the reference's NSGD (ultra.learning_algorithm.NSGD), recorded by RUNNING it on the CPU.

Same procedure and shims as make_golden_dbgd.py (the metric shim, the teacher-forced candidate theta + lr * u, the clip tap), plus:
  - only need_interleave=False runs: with interleaving the reference raises TypeError (click_simulation_winners is called without
    interleave_strategy);
  - the unit noise sample_from_null_space returns (per ranker and Linear tensor), the memory bad_noisy_params before and after the
    step, every ranker's NDCG@cutoff and the final_winners compute_gradient receives are recorded, in the flat DNN layout (0 on the
    LayerNorm entries);
  - the rest as make_golden_dbgd.py: scores, loss, gradient (parameter.grad before the clip), the clip's total norm, pre and post
    parameters and Adagrad state.

  nsgd_noint    DNN, SGD, R = 3: the seed is picked so that the steps hold both an all-losers step and a step with a winner
  nsgd_ada      DNN, Adagrad
  nsgd_linear   the Linear model

Usage:  python tests/golden/make_golden_nsgd.py [--only NAME]
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
from make_golden import adagrad_state, feed_arrays, flat_params, import_reference, make_dataset, quiet  # noqa: E402
from make_golden_dbgd import Tap, add_pads, dbgd_exp, install_metric_shim  # noqa: E402
from make_golden_pdgd import install_pdgd_shim  # noqa: E402


def flat_rows(algo, per_name, R):
    """{sequential parameter name: [R tensors]} -> [R, P] in the flat DNN layout, 0 elsewhere."""
    out = np.zeros((R, sum(p.numel() for p in algo.model.parameters())), np.float32)
    off = 0
    for name, p in algo.model.named_parameters():
        key = name.split(".", 1)[1]
        if key in per_name:
            for r in range(R):
                out[r, off:off + p.numel()] = per_name[key][r].detach().numpy().ravel()
        off += p.numel()
    return out


class NsgdTap(Tap):
    def __init__(self, ultra, algo, tau):
        super().__init__(ultra, algo, tau)
        self.samples, self.ndcgs, self.final_winners = [], [], None
        sample, grad = algo.sample_from_null_space, algo.compute_gradient

        def sample_from_null_space(*a, **k):
            u = sample(*a, **k)
            self.samples.append(u.detach().clone())
            return u

        def compute_gradient(final_winners, noisy_params):
            self.final_winners = np.asarray(torch.as_tensor(final_winners).detach().numpy(), np.float64)
            return grad(final_winners, noisy_params)

        algo.sample_from_null_space, algo.compute_gradient = sample_from_null_space, compute_gradient
        metric = ultra.utils.make_ranking_metric_fn

        def make_ranking_metric_fn(m, topn):
            fn = metric(m, topn)

            def rec(*a, **k):
                v = fn(*a, **k)
                self.ndcgs.append(float(v))
                return v
            return rec

        self._ultra, self._metric = ultra, metric
        ultra.utils.make_ranking_metric_fn = make_ranking_metric_fn

    def close(self):
        super().close()
        self._ultra.utils.make_ranking_metric_fn = self._metric
        del self.algo.sample_from_null_space, self.algo.compute_gradient


def run_nsgd_case(ultra, name, F, M, cutoff, B, hidden, seed, n_steps=4, list_lens=None, n_queries=48, algo_hparams="",
                  model_cls="ultra.ranking_model.DNN"):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)
    ds = make_dataset(ultra, seed, n_queries, list_lens or M, F)
    ds.pad(M)
    add_pads(ds, np.random.RandomState(seed + 1), M)
    exp = dbgd_exp(M, cutoff, hidden, algo_hparams, model_cls)
    exp["learning_algorithm"] = "ultra.learning_algorithm.NSGD"
    algo = quiet(ultra.utils.find_class(exp["learning_algorithm"]), ds, exp)
    feed = quiet(ultra.utils.find_class("ultra.input_layer.StochasticOnlineSimulationFeed"), algo, B, "")
    hp, R = algo.hparams, algo.ranker_num
    names = list(algo.model_params_to_update)
    out = {"meta": json.dumps({
        "name": name, "algo": "nsgd", "F": F, "M": M, "cutoff": cutoff, "B": B, "hidden": hidden, "n_steps": n_steps, "seed": seed,
        "model": model_cls.rsplit(".", 1)[1], "algo_hparams": algo_hparams, "lr": float(algo.learning_rate), "R": R,
        "max_gradient_norm": float(hp.max_gradient_norm), "grad_strategy": hp.grad_strategy,
        "need_interleave": bool(hp.need_interleave), "linear_names": names,
        "param_keys": list(algo.model.state_dict().keys()),
        "param_shapes": [list(v.shape) for v in algo.model.state_dict().values()],
    })}
    for t in range(n_steps):
        input_feed, _ = quiet(feed.get_batch, ds, check_validation=True)
        feats, docids, labels = feed_arrays(algo, input_feed, M)
        pre = {"params": flat_params(algo.model), "adagrad": adagrad_state(algo.optimizer_func, algo.model),
               "memory": flat_rows(algo, algo.bad_noisy_params, R)}
        tap = NsgdTap(ultra, algo, 1)
        try:
            loss, output, _ = quiet(algo.train, input_feed)
        finally:
            tap.close()
        p = "s%d_" % t
        out[p + "features"], out[p + "docids"], out[p + "labels"] = feats, docids, labels
        for k, v in pre.items():
            out[p + "pre_" + k] = v
        assert len(tap.samples) == R * len(names)
        per = {n_: [tap.samples[r * len(names) + i] for r in range(R)] for i, n_ in enumerate(names)}
        out[p + "unit_noise"] = flat_rows(algo, per, R)
        out[p + "post_memory"] = flat_rows(algo, algo.bad_noisy_params, R)
        out[p + "cand_scores"] = tap.new_output.numpy().astype(np.float32)  # the last candidate's
        out[p + "scores"] = algo.output.detach().numpy().astype(np.float32)
        out[p + "ndcg"] = np.asarray(tap.ndcgs[-(R + 1):], np.float64)  # every ranker's NDCG@cutoff, the current model first
        out[p + "final_winners"] = tap.final_winners
        out[p + "loss"] = np.float64(loss)
        g, tn = tap.clip
        out[p + "grads"], out[p + "norm"] = g, np.float32(tn)
        out[p + "clip_coef"] = np.float32(min(1.0, float(hp.max_gradient_norm) / (tn + 1e-6)))
        out[p + "post_params"] = flat_params(algo.model)
        out[p + "post_adagrad"] = adagrad_state(algo.optimizer_func, algo.model)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, [float(out["s%d_loss" % t]) for t in range(n_steps)],
          ["lost" if out["s%d_post_memory" % t].any() else "won" for t in range(n_steps)])


CASES = {
    "nsgd_noint": lambda u: run_nsgd_case(u, "nsgd_noint", 16, 10, 7, 8, [16, 8], 151, list_lens=(4, 10),
                                          algo_hparams="need_interleave=False,ranker_num=3"),
    "nsgd_ada": lambda u: run_nsgd_case(u, "nsgd_ada", 16, 10, 8, 8, [8], 152, list_lens=(2, 10), n_steps=3,
                                        algo_hparams="need_interleave=False,grad_strategy=ada,learning_rate=0.1"),
    "nsgd_linear": lambda u: run_nsgd_case(u, "nsgd_linear", 16, 10, 10, 8, None, 153, n_steps=3,
                                           algo_hparams="need_interleave=False", model_cls="ultra.ranking_model.Linear"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.set_num_threads(1)  # bit-stable fixtures
    ultra = import_reference()
    install_pdgd_shim()
    install_metric_shim(ultra)
    for name, fn in CASES.items():
        if args.only and args.only != name:
            continue
        fn(ultra)


if __name__ == "__main__":
    main()
