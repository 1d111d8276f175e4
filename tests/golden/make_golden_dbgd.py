#!/usr/bin/env python3
"""Golden vectors of the reference's DBGD (ultra.learning_algorithm.DBGD), its TeamDraftInterleaving with five rankings and MGD's
compute_gradient, recorded by RUNNING them on the CPU.

Same procedure and shims as make_golden.py / make_golden_pdgd.py, plus five more:
  - make_ranking_metric_fn(metric, topn) with an int topn (DBGD's loss, dbgd.py:129-131) fails inside the reference's metric
    (`min(n, list_size) for n in topn`); the shim passes [topn] and returns the one value;
  - `tau` is supplied (the reference's 'Stochastic' strategy reads self.hparams.tau, which DBGD never defines);
  - the candidate is teacher-forced to theta + lr * u: create_new_output_list perturbs a COPY of the current model instead of a
    freshly initialised one;
  - the torch.normal draws of create_noisy_param, the np.random.shuffle results inside TeamDraftInterleaving.interleave, the rankings
    it is given and the click lists infer_winner sees are recorded;
  - the rest is recorded too: scores, multileaved lists, teams, winners, loss, gradient (parameter.grad before the clip), the clip's
    total norm, pre and post parameters and Adagrad state.

  dbgd_det / dbgd_sto / dbgd_noint / dbgd_ada / dbgd_linear   DBGD steps on StochasticOnlineSimulationFeed batches of seeded synthetic
                data with PADs inside and at the tail and selection_bias_cutoff < max_candidate_num
  dbgd_mgd      MGD cannot be constructed in the reference: TeamDraftInterleaving.interleave on five rankings and MGD.compute_gradient
                on recorded inputs (winners, noise)

Usage:  python tests/golden/make_golden_dbgd.py [--only NAME]
"""
import argparse
import copy
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import adagrad_state, feed_arrays, flat_params, import_reference, make_dataset, quiet  # noqa: E402
from make_golden_pdgd import install_pdgd_shim  # noqa: E402


def install_metric_shim(ultra):
    orig = ultra.utils.make_ranking_metric_fn

    def make_ranking_metric_fn(metric, topn):
        if isinstance(topn, int):
            fn = orig(metric, [topn])
            return lambda *a, **k: fn(*a, **k)[0]
        return orig(metric, topn)

    ultra.utils.make_ranking_metric_fn = make_ranking_metric_fn


def dbgd_exp(M, cutoff, hidden, algo_hparams, model_cls="ultra.ranking_model.DNN"):
    return {
        "learning_algorithm": "ultra.learning_algorithm.DBGD",
        "learning_algorithm_hparams": algo_hparams,
        "ranking_model": model_cls,
        "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(hidden) if hidden is not None else "",
        "max_candidate_num": M,
        "selection_bias_cutoff": cutoff,
        "metrics": ["ndcg"],
        "metrics_topn": [1, 3, 5],
    }


class Tap:
    """The recording hooks on one DBGD object."""

    def __init__(self, ultra, algo, tau):
        self.algo = algo
        algo.hparams.tau = tau
        self.normals, self.shuffles, self.rankings, self.clicks, self.clip = [], [], [], [], None
        self.new_output = None
        torch_normal = torch.normal

        def normal(*a, **k):
            z = torch_normal(*a, **k)
            self.normals.append(z.detach().clone())
            return z

        self._torch_normal = torch_normal
        torch.normal = normal

        def create_new_output_list(noisy_params):  # teacher-forced: the candidate is the CURRENT model plus noise
            model_prime = copy.deepcopy(algo.model)
            ids = algo.docid_inputs if algo.hparams.need_interleave else algo.docid_inputs[:algo.rank_list_size]
            out = torch.cat(algo.get_ranking_scores(model_prime, ids, noisy_params=noisy_params, noise_rate=algo.hparams.learning_rate), 1)
            self.new_output = out.detach().clone()
            return out

        algo.create_new_output_list = create_new_output_list
        np_shuffle = np.random.shuffle

        def shuffle(x):
            np_shuffle(x)
            self.shuffles[-1].append(np.array(x, dtype=np.int32))

        self._np_shuffle = np_shuffle
        np.random.shuffle = shuffle
        if algo.interleaving is not None:
            inter, infer = algo.interleaving.interleave, algo.interleaving.infer_winner

            def interleave(rankings):
                self.shuffles.append([])
                self.rankings.append(np.asarray(rankings, dtype=np.int64).copy())
                ml = inter(rankings)
                self.multileaved.append(np.asarray(ml, dtype=np.int64).copy())
                self.teams.append(np.asarray(algo.interleaving.teams, dtype=np.int64).copy())
                return ml

            def infer_winner(clicks):
                self.clicks.append(np.asarray(clicks, dtype=np.float32).copy())
                return infer(clicks)

            algo.interleaving.interleave = interleave
            algo.interleaving.infer_winner = infer_winner
            self.teams = []
            self.multileaved = []

        orig_clip = torch.nn.utils.clip_grad_norm_

        def clip(parameters, max_norm, *a, **k):
            ps = list(parameters)
            g = np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().ravel()
                                for p in algo.model.parameters()]).astype(np.float32)
            tn = orig_clip(ps, max_norm, *a, **k)
            self.clip = (g, float(tn))
            return tn

        self._orig_clip = orig_clip
        torch.nn.utils.clip_grad_norm_ = clip

    def close(self):
        torch.normal = self._torch_normal
        np.random.shuffle = self._np_shuffle
        torch.nn.utils.clip_grad_norm_ = self._orig_clip


def flat_noise(algo, normals):
    """The recorded normals (one per Linear parameter, in named_parameters order) in the flat DNN layout, 0 on LayerNorm."""
    parts, it = [], iter(normals)
    for name, p in algo.model.named_parameters():
        parts.append(next(it).numpy().ravel() if "linear" in name else np.zeros(p.numel(), np.float32))
    return np.concatenate(parts).astype(np.float32)


def add_pads(ds, rng, M):
    """Interior PADs: a position of some lists becomes -1 (the online feed hands it on as a PAD inside the list)."""
    for q in range(len(ds.initial_list)):
        row = ds.initial_list[q]
        n = sum(1 for x in row[:M] if x >= 0)
        if n > 3 and rng.uniform() < 0.5:
            row[int(rng.randint(1, n - 1))] = -1


def run_dbgd_case(ultra, name, F, M, cutoff, B, hidden, seed, n_steps=2, list_lens=None, n_queries=48, algo_hparams="", tau=1,
                  model_cls="ultra.ranking_model.DNN"):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)
    ds = make_dataset(ultra, seed, n_queries, list_lens or M, F)
    ds.pad(M)
    add_pads(ds, np.random.RandomState(seed + 1), M)
    exp = dbgd_exp(M, cutoff, hidden, algo_hparams, model_cls)
    algo = quiet(ultra.utils.find_class(exp["learning_algorithm"]), ds, exp)
    feed = quiet(ultra.utils.find_class("ultra.input_layer.StochasticOnlineSimulationFeed"), algo, B, "")
    hp = algo.hparams
    out = {"meta": json.dumps({
        "name": name, "algo": "dbgd", "F": F, "M": M, "cutoff": cutoff, "B": B, "hidden": hidden, "n_steps": n_steps, "seed": seed,
        "model": model_cls.rsplit(".", 1)[1], "algo_hparams": algo_hparams, "lr": float(algo.learning_rate),
        "max_gradient_norm": float(hp.max_gradient_norm), "tau": float(tau), "grad_strategy": hp.grad_strategy,
        "need_interleave": bool(hp.need_interleave), "interleave_strategy": hp.interleave_strategy,
        "param_keys": list(algo.model.state_dict().keys()),
        "param_shapes": [list(v.shape) for v in algo.model.state_dict().values()],
    })}
    for t in range(n_steps):
        input_feed, _ = quiet(feed.get_batch, ds, check_validation=True)
        feats, docids, labels = feed_arrays(algo, input_feed, M)
        pre = {"params": flat_params(algo.model), "adagrad": adagrad_state(algo.optimizer_func, algo.model)}
        tap = Tap(ultra, algo, tau)
        try:
            loss, output, _ = quiet(algo.train, input_feed)
        finally:
            tap.close()
        p = "s%d_" % t
        out[p + "features"], out[p + "docids"], out[p + "labels"] = feats, docids, labels
        for k, v in pre.items():
            out[p + "pre_" + k] = v
        out[p + "noise"] = flat_noise(algo, tap.normals)[None, :]
        out[p + "cand_scores"] = tap.new_output.numpy().astype(np.float32)
        sc0 = output[0] if isinstance(output, tuple) else algo.output
        out[p + "scores"] = sc0.detach().numpy().astype(np.float32)
        out[p + "loss"] = np.float64(loss)
        g, tn = tap.clip
        out[p + "grads"], out[p + "norm"] = g, np.float32(tn)
        out[p + "clip_coef"] = np.float32(min(1.0, float(hp.max_gradient_norm) / (tn + 1e-6)))
        out[p + "post_params"] = flat_params(algo.model)
        out[p + "post_adagrad"] = adagrad_state(algo.optimizer_func, algo.model)
        if hp.need_interleave:
            Bn = docids.shape[1]
            NR = 2
            sh = np.full((Bn, M, NR), -1, np.int32)
            rk = np.full((Bn, NR, M), -1, np.int32)
            ck = np.zeros((M, Bn), np.float32)
            ml = np.full((M, Bn), -1, np.int64)
            tm = np.full((M, Bn), -2, np.int64)
            for b in range(Bn):
                for r_, s in enumerate(tap.shuffles[b]):
                    sh[b, r_] = s
                n = tap.rankings[b].shape[1]
                rk[b, :, :n] = tap.rankings[b]
                ck[:len(tap.clicks[b]), b] = tap.clicks[b]
                ml[:n, b], tm[:n, b] = tap.multileaved[b], tap.teams[b]
            out[p + "shuffles"], out[p + "rankings"], out[p + "clicks"] = sh, rk, ck
            out[p + "interleaved"], out[p + "teams"] = ml, tm
            out[p + "winners"] = np.asarray(algo.winners, np.float64)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, [float(out["s%d_loss" % t]) for t in range(n_steps)])


def run_mgd_case(ultra, name, seed=131, n_lists=12, NR=5, F=8, hidden=(6,)):
    """TeamDraftInterleaving with five rankings (rankings with an agreed prefix among them) and MGD.compute_gradient."""
    from ultra.utils.team_draft_interleave import TeamDraftInterleaving
    from ultra.learning_algorithm.mgd import MGD
    rng = np.random.RandomState(seed)
    np.random.seed(seed)
    out = {}
    inter = TeamDraftInterleaving()
    np_shuffle = np.random.shuffle
    for i in range(n_lists):
        n = int(rng.randint(1, 14))
        base = rng.permutation(n)
        rk = np.stack([base.copy() for _ in range(NR)])
        k = int(rng.randint(0, n))  # rankings agree on the first k positions
        for r in range(1, NR):
            tail = rk[r, k:].copy()
            rng.shuffle(tail)
            rk[r, k:] = tail
        shuffles = []

        def shuffle(x):
            np_shuffle(x)
            shuffles.append(np.array(x, dtype=np.int32))

        np.random.shuffle = shuffle
        try:
            ml = inter.interleave(rk)
        finally:
            np.random.shuffle = np_shuffle
        clicks = (rng.uniform(size=n) < 0.4).astype(np.int64).tolist()
        w = inter.infer_winner(clicks)
        out["l%d_rankings" % i], out["l%d_multileaved" % i], out["l%d_teams" % i] = rk, ml.astype(np.int64), inter.teams.astype(np.int64)
        out["l%d_shuffles" % i] = np.asarray(shuffles, np.int32).reshape(-1, NR)
        out["l%d_clicks" % i], out["l%d_winners" % i] = np.asarray(clicks, np.float32), np.asarray(w, np.float64)
    # MGD.compute_gradient on recorded inputs: a bare object with MGD's method, a DNN and random unit noise
    torch.manual_seed(seed)
    model = ultra.utils.find_class("ultra.ranking_model.DNN")("hidden_layer_sizes=%s" % json.dumps(list(hidden)), F)
    holder = type("H", (), {})()
    holder.model, holder.is_cuda_avail = model, False
    noisy = {}
    for name_, prm in model.sequential.named_parameters():
        if "linear" in name_:
            noisy[name_] = [torch.zeros_like(prm)] + [torch.nn.functional.normalize(torch.normal(0.0, 1.0, size=prm.shape), dim=0)
                                                      for _ in range(NR - 1)]
    B = 7
    winners = [rng.dirichlet(np.ones(NR)) * (rng.uniform() < 0.8) for _ in range(B)]
    MGD.compute_gradient(holder, winners, {k: list(v) for k, v in noisy.items()})
    g = np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().ravel()
                        for p in model.parameters()]).astype(np.float32)
    u = np.stack([np.concatenate([(noisy[n_][r].numpy().ravel() if "linear" in n_ else np.zeros(p.numel(), np.float32))
                                  for n_, p in model.sequential.named_parameters()]) for r in range(1, NR)]).astype(np.float32)
    out["mgd_winners"], out["mgd_noise"], out["mgd_grads"] = np.asarray(winners, np.float64), u, g
    out["meta"] = json.dumps({"name": name, "seed": seed, "n_lists": n_lists, "NR": NR, "F": F, "hidden": list(hidden), "B": B})
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name)


CASES = {
    # deterministic strategy, PADs inside and at the tail, cutoff 6 < max_candidate_num 12, a small lr so that rankings agree on prefixes
    "dbgd_det": lambda u: run_dbgd_case(u, "dbgd_det", 16, 12, 6, 8, [16, 8], 141, list_lens=(3, 12),
                                        algo_hparams="interleave_strategy=Deterministic,learning_rate=0.05"),
    "dbgd_sto": lambda u: run_dbgd_case(u, "dbgd_sto", 16, 10, 10, 8, [16, 8], 142, list_lens=(4, 10), tau=2),
    "dbgd_noint": lambda u: run_dbgd_case(u, "dbgd_noint", 16, 10, 7, 8, [16, 8], 143, list_lens=(4, 10),
                                          algo_hparams="need_interleave=False", n_steps=3),
    "dbgd_ada": lambda u: run_dbgd_case(u, "dbgd_ada", 16, 10, 8, 8, [8], 144, list_lens=(2, 10),
                                        algo_hparams="interleave_strategy=Deterministic,grad_strategy=ada,learning_rate=0.1"),
    "dbgd_linear": lambda u: run_dbgd_case(u, "dbgd_linear", 16, 10, 10, 8, None, 145,
                                           algo_hparams="interleave_strategy=Deterministic", model_cls="ultra.ranking_model.Linear"),
    "dbgd_mgd": lambda u: run_mgd_case(u, "dbgd_mgd"),
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
