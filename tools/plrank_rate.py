#!/usr/bin/env python3
"""Time one PLRank training step next to the IPWrank step at the same shape, and PLRank's loss launch next to the same law written in
stock torch ops in float32 on the same GPU (figures: profiles/plrank.md).

The model: a DNN of 136 features, hidden [256, 256], at batch 256 x 10 documents and batch 512 x 50, Adagrad, with 64 and 256 sampled
rankings per list.  Per (shape, sample count) one JSON line:

  ipw_ms      engine.StepEngine.train_step of IPWrank (algo softmax with the IPW table)
  plrank_ms   the same call for PLRank: ultr_dnn_forward -> ultr_plrank_loss -> ultr_dnn_backward -> ultr_apply_update
  loss_ms     the loss launch alone (hip_ops.plrank_loss on the scores of one forward), and loss_share = loss_ms / plrank_ms
  torch_loss_ms   the law of DESIGN.md section 4d in torch float32 on the device: uniform draw, race keys, argsort, gathers, the four scans
              as flipped / plain cumsum, scatter back (tests/plrank_ref.per_sample in torch; its own uniforms, not Philox)
  each        median / min / max over `--repeats` (>= 30) repetitions after `--warmup` calls; a repetition is `--iters` calls between two
              device synchronisations on a host clock, divided by `--iters`.

    python tools/plrank_rate.py [--repeats 30] [--iters 200] [--rounds 3] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL = (136, [256, 256])
SHAPES = ((256, 10), (512, 50))
SAMPLES = (64, 256)
TABLE = [1.0, 1.4, 1.9, 2.5, 3.2, 4.0, 4.9, 5.9, 7.0, 8.2]


def timed(fn, warmup, repeats, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / iters)
    return {"median": statistics.median(out), "min": min(out), "max": max(out), "repeats": repeats, "iters": iters}


def torch_plrank(scores, rho, valid, N, K):
    """dscores [B, L] and the per-list loss of the law, stock torch ops in the dtype of `scores`."""
    B, L = scores.shape
    s = scores.masked_fill(~valid, float("-inf"))
    m = s - s.max(dim=1, keepdim=True).values
    e = m.exp()
    u = torch.rand(B, N, L, device=scores.device, dtype=scores.dtype)
    keys = m[:, None, :] - torch.log(-torch.log1p(-u))
    order = keys.argsort(dim=2, descending=True)
    e_r = e[:, None, :].expand(B, N, L).gather(2, order)
    rho_r = rho[:, None, :].expand(B, N, L).gather(2, order)
    ranks = torch.arange(L, device=scores.device, dtype=scores.dtype)
    theta = 1.0 / torch.log2(ranks + 2.0)
    inside = (ranks < K).to(scores.dtype)
    Z = e_r.flip(2).cumsum(2).flip(2).clamp_min(1e-30)
    FR = (theta * rho_r * inside).flip(2).cumsum(2).flip(2)
    RI = (FR / Z * inside).cumsum(2)
    DR = (theta / Z * inside).cumsum(2)
    direct = torch.cat([FR[..., 1:], torch.zeros_like(FR[..., :1])], dim=2) * inside
    g = torch.zeros_like(e_r).scatter_(2, order, direct + e_r * (rho_r * DR - RI))
    return -g.mean(dim=1), -FR[..., 0].mean(dim=1)


def row(B, L, N, args):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    dev = torch.device("cuda")
    F, hidden = MODEL
    shape = hip_ops.DnnShape(F, hidden, "elu")
    feats, ids, clicks = synthetic.make_batch(np.random.RandomState(L), B, L, F, n_pad=2 if L > 10 else 0)
    f, i, y = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(clicks, device=dev)
    n_docs = feats.shape[0]
    table = torch.tensor(TABLE, device=dev)
    p0 = torch.tensor(O.init_params(F, hidden, seed=1), device=dev)
    w = (args.warmup, args.repeats, args.iters)
    out = {"batch": B, "list_size": L, "rows": B * L, "n_samples": N, "n_params": shape.n_params}
    runs = {}
    for name, algo, kw in (("ipw", "softmax", {}), ("plrank", "plrank", dict(num_samples=N, rng_seed=7))):
        eng = engine.StepEngine(shape, B, L, dev, algo=algo, **kw)
        runs[name] = (eng, p0.clone(), torch.zeros(max(engine.opt_state_floats(algo, "ada", L, shape.n_params), 1), device=dev))
    steps = [0]

    def plrank_step():
        eng, p, st = runs["plrank"]
        eng.set_draw_step(steps[0])
        steps[0] += 1
        eng.train_step(p, st, f, n_docs, i, y, ipw_table=table)

    eng, p, st = runs["ipw"]
    out["ipw_ms"] = timed(lambda: eng.train_step(p, st, f, n_docs, i, y, ipw_table=table), *w)
    assert np.isfinite(eng.read_scalars()[0])
    out["plrank_ms"] = timed(plrank_step, *w)
    eng, p, st = runs["plrank"]
    assert np.isfinite(eng.read_scalars()[0])
    eng.forward(p, f, n_docs, i, train=True)
    out["loss_ms"] = timed(lambda: eng.loss(y, ipw_table=table, docids=i, n_docs=n_docs), *w)
    out["loss_share"] = out["loss_ms"]["median"] / out["plrank_ms"]["median"]
    valid = (i.t() >= 0) & (i.t() < n_docs)
    wts = table[torch.arange(L, device=dev).clamp_max(len(TABLE) - 1)]
    rho = torch.where(valid, wts[None, :] * y.t(), torch.zeros((), device=dev)).contiguous()
    scores = eng.scores.clone()
    out["torch_loss_ms"] = timed(lambda: torch_plrank(scores, rho, valid, N, L), args.warmup, args.repeats, max(args.iters // 10, 5))
    out["torch_over_kernel"] = out["torch_loss_ms"]["median"] / out["loss_ms"]["median"]
    for eng, _, _ in runs.values():
        eng.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if args.repeats < 30:
        raise SystemExit("plrank_rate.py takes the median of at least 30 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("plrank_rate.py measures on the GPU: none found")
    rows = []
    for rnd in range(args.rounds):
        for B, L in SHAPES:
            for N in SAMPLES:
                r = row(B, L, N, args)
                r["round"] = rnd
                rows.append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
