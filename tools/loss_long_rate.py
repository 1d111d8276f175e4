#!/usr/bin/env python3
"""Time the long-list pair-walk losses (csrc/ultr_loss_long.hip) - PairDebias, LambdaRank, PRSrank - next to the same losses in stock
torch-ROCm ops and, at the short kernels' bounds, next to the short kernels (figures: profiles/loss_long.md).

Per algorithm JSON lines of three kinds:

  "loss"      batch 64 x 1251 documents (MSLR-WEB30K's longest list): loss_ms = the loss launch alone (hip_ops.*_loss_long on
              resident scores), step_ms = engine.StepEngine.train_step of a DNN [512, 256, 128] on 136 features (ONE ultr_train_step:
              forward, loss, backward, update), torch_loss_ms = the same loss and its gradient by autograd in stock torch ops on the
              same GPU (tools/torch_rocm_baseline.py's formulas; [B, L, L] tensors), pairs_per_s = B L^2 / loss time
  "handover"  batch 64 at the short kernel's longest list (585 / 531 / 952): short_ms and long_ms of the two kernels on the same
              inputs - what the hand-over at the short bound costs or saves
  each        median / min / max over `--repeats` (>= 30) repetitions after `--warmup` calls; a repetition is `--iters` calls between two
              device synchronisations on a host clock, divided by `--iters`

    python tools/loss_long_rate.py [--repeats 30] [--iters 20] [--no-baseline] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL_F, MODEL_HIDDEN = 136, [512, 256, 128]
BATCH, MSLR = 64, 1251
SHORT_MAX = {"pairdebias": 585, "lambdarank": 531, "prs": 952}


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


# ---- the same losses in stock torch ops (scores [B, L], labels [B, L]) -------------------------------------------------------------------
def torch_pairdebias(s, y, tp, tm):
    B = s.shape[0]
    mask = torch.clamp(y.unsqueeze(2) - y.unsqueeze(1), 0.0, 1.0)
    PL = float(B) * (mask * F.softplus(s.unsqueeze(1) - s.unsqueeze(2))).sum(0)
    return (PL / tp.unsqueeze(1) / tm.unsqueeze(0)).sum()


def _sorted_pairs(s, y):
    ps, inds = torch.sort(s, dim=1, descending=True)
    ls = torch.gather(y, 1, inds)
    L = s.shape[1]
    ideal = torch.sort(y, dim=1, descending=True)[0]
    idcg = ((torch.pow(2.0, ideal) - 1.0) / torch.log(torch.arange(1, L + 1, device=s.device, dtype=s.dtype) + 1.0)).sum()
    gains = (torch.pow(2.0, ls) - 1.0) / idcg
    disc = 1.0 / torch.log2(torch.arange(L, device=s.device, dtype=s.dtype) + 2.0)
    delta = (gains.unsqueeze(2) - gains.unsqueeze(1)).abs() * (disc.view(1, L, 1) - disc.view(1, 1, L)).abs()
    pbar = 0.5 * (1.0 + torch.clamp(ls.unsqueeze(2) - ls.unsqueeze(1), -1.0, 1.0))
    return ps, inds, delta, pbar


def torch_lambdarank(s, y, tp, tm, sigma=1.0):
    ps, _, delta, pbar = _sorted_pairs(s, y)
    p = 1.0 / (torch.exp(-sigma * (ps.unsqueeze(2) - ps.unsqueeze(1))) + 1.0)
    PL = F.binary_cross_entropy_with_logits(p, pbar, weight=delta, reduction="none").sum(0)
    return (PL / (tp.unsqueeze(1) * tm.unsqueeze(0))).sum()


def torch_prs(s, y, ipw, sigma=1.0):
    ps, inds, delta, pbar = _sorted_pairs(s, y)
    ipws = ipw[torch.clamp(inds, max=ipw.numel() - 1)]
    prs = torch.triu(ipws.unsqueeze(2) / ipws.unsqueeze(1), 1)
    x = 1.0 / (torch.exp(-sigma * (ps.unsqueeze(2) - ps.unsqueeze(1))) + 1.0)
    return (F.binary_cross_entropy(x, pbar, weight=delta, reduction="none") * prs).sum()


def inputs(algo, B, L, dev):
    rng = np.random.RandomState(L)
    s = torch.tensor(rng.normal(size=(B, L)).astype(np.float32), device=dev)
    if algo == "lambdarank":
        y = rng.randint(0, 5, size=(L, B)).astype(np.float32)
    else:
        y = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32)
        y[0, :] = 1.0
    t = torch.tensor(rng.uniform(0.8, 1.2, size=2 * L).astype(np.float32), device=dev)
    ipw = torch.tensor(np.linspace(1.0, 9.0, 40).astype(np.float32), device=dev)
    return s, torch.tensor(y, device=dev), t, ipw


def loss_call(algo, long, B, L, s, y, t, ipw, ds, ws):
    from ultra_pytorch_amd import hip_ops
    sfx = "_long" if long else ""
    if algo == "pairdebias":
        return lambda: getattr(hip_ops, "pairdebias_loss" + sfx)(s, y, t[:L], t[L:], B, L, B, ds, ws)
    if algo == "lambdarank":
        return lambda: getattr(hip_ops, "lambdarank_loss" + sfx)(s, y, t[:L], t[L:], 1.0, B, L, ds, ws)
    return lambda: getattr(hip_ops, "prs_loss" + sfx)(s, y, ipw, 1.0, B, L, ds, ws)


def buffers(B, L, dev):
    from ultra_pytorch_amd import hip_ops
    return torch.zeros(B, L, device=dev), torch.zeros(hip_ops.loss_workspace_bytes(B, L) // 4, device=dev)


def loss_row(algo, args):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    dev = torch.device("cuda")
    B, L = BATCH, MSLR
    w = (args.warmup, args.repeats, args.iters)
    s, y, t, ipw = inputs(algo, B, L, dev)
    ds, ws = buffers(B, L, dev)
    out = {"kind": "loss", "algo": algo, "batch": B, "list_size": L, "pairs": B * L * L}
    out["loss_ms"] = timed(loss_call(algo, True, B, L, s, y, t, ipw, ds, ws), *w)
    out["pairs_per_s"] = out["pairs"] / (1e-3 * out["loss_ms"]["median"])
    shape = hip_ops.DnnShape(MODEL_F, MODEL_HIDDEN, "elu")
    feats, ids, lab = synthetic.make_batch(np.random.RandomState(1), B, L, MODEL_F, clicks=(algo != "lambdarank"))
    f, i, yb = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(lab, device=dev)
    p = torch.tensor(O.init_params(MODEL_F, MODEL_HIDDEN, seed=0), device=dev)
    st, aux = torch.zeros_like(p), (None if algo == "prs" else torch.ones(2 * L, device=dev))
    eng = engine.StepEngine(shape, B, L, dev, algo=algo, learning_rate=0.005)
    out["step_ms"] = timed(lambda: eng.train_step(p, st, f, feats.shape[0], i, yb, aux=aux, ipw_table=ipw if algo == "prs" else None), *w)
    out["last_loss"] = float(eng.read_scalars()[0])  # (the timed steps train: finite, or the timing is of NaN arithmetic)
    eng.close()
    if not args.no_baseline:
        yt = y.t().contiguous()

        def torch_loss():
            sr = s.detach().requires_grad_(True)
            loss = (torch_pairdebias(sr, yt, t[:L], t[L:]) if algo == "pairdebias" else
                    torch_lambdarank(sr, yt, t[:L], t[L:]) if algo == "lambdarank" else torch_prs(sr, yt, ipw))
            return torch.autograd.grad(loss, sr)[0]

        out["torch_loss_ms"] = timed(torch_loss, args.warmup, args.repeats, max(1, args.iters // 10))
        out["torch_pairs_per_s"] = out["pairs"] / (1e-3 * out["torch_loss_ms"]["median"])
    return out


def handover_row(algo, args):
    dev = torch.device("cuda")
    B, L = BATCH, SHORT_MAX[algo]
    w = (args.warmup, args.repeats, args.iters)
    s, y, t, ipw = inputs(algo, B, L, dev)
    ds, ws = buffers(B, L, dev)
    out = {"kind": "handover", "algo": algo, "batch": B, "list_size": L, "pairs": B * L * L}
    out["short_ms"] = timed(loss_call(algo, False, B, L, s, y, t, ipw, ds, ws), *w)
    out["long_ms"] = timed(loss_call(algo, True, B, L, s, y, t, ipw, ds, ws), *w)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if args.repeats < 30:
        raise SystemExit("loss_long_rate.py takes the median of at least 30 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("loss_long_rate.py measures on the GPU: none found")
    rows = []
    for algo in ("pairdebias", "lambdarank", "prs"):
        for fn in (loss_row, handover_row):
            rows.append(fn(algo, args))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
