#!/usr/bin/env python3
"""Time one DLCM training step and one scoring call, next to the same model in stock torch-ROCm ops (figures: profiles/dlcm.md).

The model: 136 features, hidden 136, 3 heads (ranking_model.DLCM's defaults on MSLR-WEB30K) at batch 256 x 10 documents (the flagship
batch) and batch 512 x 50.  Per shape one JSON line:

  step_ms     engine.DlcmStepEngine.train_step (softmax loss, Adagrad): ultr_dlcm_forward -> ultr_softmax_ce -> ultr_dlcm_backward ->
              ultr_grad_sumsq -> ultr_apply_update
  score_ms    engine.DlcmEvalEngine.forward: the scoring form of ultr_dlcm_forward
  forward_ms / backward_ms   the two entries alone (the backward re-run on the record of one forward)
  torch_step_ms / torch_score_ms   nn.LayerNorm + nn.GRU + nn.Linear in fp32 on the same GPU: forward, the listwise softmax loss,
              autograd, clip_grad_norm_, torch.optim.Adagrad; the forward alone under no_grad
  each        median / min / max over `--repeats` (>= 30) repetitions after `--warmup` calls; a repetition is `--iters` calls between two
              device synchronisations on a host clock, divided by `--iters`
  max_score_diff   largest |score| difference between the two implementations on the timed inputs (same parameters)

    python tools/dlcm_rate.py [--repeats 30] [--iters 50] [--rounds 1] [--no-baseline] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL = (136, 136, 3)  # F, H, heads
SHAPES = ((256, 10), (512, 50))


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


class TorchDLCM(nn.Module):
    """The baseline: the same model in stock torch ops."""

    def __init__(self, F, H, heads):
        super().__init__()
        self.H, self.heads = H, heads
        self.layer_norm, self.gru = nn.LayerNorm(F), nn.GRU(F, H, batch_first=True)
        self.att_linear, self.att_v = nn.Linear(H, heads * H), nn.Linear(heads, 1, bias=False)

    def forward(self, x):  # [B, L, F]
        out, _ = self.gru(torch.flip(self.layer_norm(x), dims=[1]))
        o = torch.flip(out, dims=[1])
        M = torch.tanh(self.att_linear(o[:, 0])).view(-1, self.heads, self.H)
        return torch.einsum("blh,bh->bl", o, torch.einsum("j,bjh->bh", self.att_v.weight[0], M))


def row(B, L, args):
    from ultra_pytorch_amd import engine, synthetic
    from ultra_pytorch_amd.ranking_model import DLCM
    dev = torch.device("cuda")
    F, H, heads = MODEL
    torch.manual_seed(0)
    model = DLCM("hidden_size=%d,num_heads=%d" % (H, heads), F)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    feats, ids, clicks = synthetic.make_batch(np.random.RandomState(L), B, L, F, n_pad=2)
    f, i, y = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(clicks, device=dev)
    n_docs = feats.shape[0]
    p, st = model.flat_params.clone(), torch.zeros_like(model.flat_params)
    eng = engine.DlcmStepEngine(model.shape, B, L, dev, algo="softmax")
    ev = engine.DlcmEvalEngine(model.shape, B, L, dev)
    w = (args.warmup, args.repeats, args.iters)
    out = {"batch": B, "list_size": L, "tokens": B * L, "n_params": model.shape.n_params}
    out["score_ms"] = timed(lambda: ev.forward(model.flat_params, f, n_docs, i), *w)
    ours = ev.scores.clone()
    out["forward_ms"] = timed(lambda: eng.forward(p, f, n_docs, i, train=True), *w)
    eng.loss(y)
    out["backward_ms"] = timed(lambda: eng.backward(p, f, n_docs, i), *w)
    out["step_ms"] = timed(lambda: eng.train_step(p, st, f, n_docs, i, y), *w)
    assert np.isfinite(eng.read_scalars()[0])

    if args.no_baseline:  # (a profiler run: the library's kernels alone)
        eng.close()
        return out
    print(json.dumps(dict(out, partial="library figures; the torch baseline follows")), file=sys.stderr, flush=True)
    base = TorchDLCM(F, H, heads)
    base.load_state_dict(sd)
    base = base.to(dev)
    pad = torch.cat([f, torch.zeros(1, F, device=dev)], dim=0)
    x = pad[i.t().long()]          # [B, L, F], gathered once outside the timed window (the engine gathers inside its forward)
    yb = y.t().contiguous()
    opt = torch.optim.Adagrad(base.parameters(), lr=0.05)

    def torch_step():
        wl = yb + 1e-7
        loss = torch.sum(-torch.sum(wl / wl.sum(1, keepdim=True) * torch.log_softmax(base(x), dim=-1), dim=-1) * wl.sum(1)) / wl.sum()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(base.parameters(), 5.0)
        opt.step()

    def torch_score():
        with torch.no_grad():
            return base(x)

    out["max_score_diff"] = float((torch_score() - ours).abs().max())
    out["torch_score_ms"] = timed(torch_score, *w)
    out["torch_step_ms"] = timed(torch_step, *w)
    eng.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if args.repeats < 30:
        raise SystemExit("dlcm_rate.py takes the median of at least 30 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("dlcm_rate.py measures on the GPU: none found")
    rows = []
    for rnd in range(args.rounds):
        for B, L in SHAPES:
            r = row(B, L, args)
            r["round"] = rnd
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
