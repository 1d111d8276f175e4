#!/usr/bin/env python3
"""Time one GSF training step and one scoring call, next to the same model in stock torch-ROCm ops (figures: profiles/gsf.md).

The model: 136 features, group_size 2, hidden [512, 256, 128] (ranking_model.GSF's defaults on MSLR-WEB30K) at batch 256 x 10 documents
(the flagship batch) and batch 512 x 50.  Per shape one JSON line:

  step_ms     engine.GsfStepEngine.train_step in presented order (softmax loss, Adagrad): ultr_gsf_forward -> ultr_softmax_ce ->
              ultr_gsf_backward -> ultr_grad_sumsq -> ultr_apply_update
  step_shuffle_ms   the same step with the training shuffle (ultr_gsf_shuffle in front)
  score_ms    engine.GsfEvalEngine.forward: the scoring form of ultr_gsf_forward
  forward_ms / backward_ms   the two entries alone (the backward re-run on the record of one forward)
  torch_step_ms / torch_score_ms   the groups by torch.roll + torch.cat, nn.LayerNorm + nn.Linear + nn.ELU in fp32 on the same GPU:
              forward, the listwise softmax loss, autograd, clip_grad_norm_, torch.optim.Adagrad; the forward alone under no_grad
  dnn272_step_ms   engine.StepEngine.train_step of the DNN ranking model with 272 features and the same hidden layers at the same number
              of rows: the nearest yardstick of the same GEMM work; dnn272_route names the kernels that step took (ultr_dnn_route)
  each        median / min / max over `--repeats` (>= 30) repetitions after `--warmup` calls; a repetition is `--iters` calls between two
              device synchronisations on a host clock, divided by `--iters`
  max_score_diff   largest |score| difference between the two implementations on the timed inputs (same parameters)

    python tools/gsf_rate.py [--repeats 30] [--iters 50] [--rounds 1] [--shapes 256x10,512x50] [--no-baseline] [--out FILE.json]
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

MODEL = (136, 2, [512, 256, 128])  # F, group_size, hidden
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


class TorchGSF(nn.Module):
    """The baseline: the same model in stock torch ops, presented order."""

    def __init__(self, F, m, hidden):
        super().__init__()
        self.m, self.k = m, len(hidden)
        self.sequential = nn.Module()
        width = F * m
        for j, out in enumerate(list(hidden) + [m]):
            self.sequential.add_module("layer_norm%d" % j, nn.LayerNorm(width))
            self.sequential.add_module("linear%d" % j, nn.Linear(width, out))
            width = out
        self.act = nn.ELU()

    def forward(self, x):  # [B, L, F]
        h = torch.cat([torch.roll(x, -j, dims=1) for j in range(self.m)], dim=-1)
        for j in range(self.k + 1):
            h = getattr(self.sequential, "linear%d" % j)(getattr(self.sequential, "layer_norm%d" % j)(h))
            if j < self.k:
                h = self.act(h)
        s = h[:, :, 0]
        for j in range(1, self.m):
            s = s + torch.roll(h[:, :, j], j, dims=1)
        return s


def row(B, L, args):
    from ultra_pytorch_amd import engine, synthetic
    from ultra_pytorch_amd.ranking_model import DNN, GSF
    dev = torch.device("cuda")
    F, m, hidden = MODEL
    hp = "hidden_layer_sizes=[%s]" % ",".join(str(h) for h in hidden)
    torch.manual_seed(0)
    model = GSF(hp + ",group_size=%d" % m, F)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    feats, ids, clicks = synthetic.make_batch(np.random.RandomState(L), B, L, F, n_pad=2)
    f, i, y = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(clicks, device=dev)
    n_docs = feats.shape[0]
    p, st = model.flat_params.clone(), torch.zeros_like(model.flat_params)
    eng = engine.GsfStepEngine(model.shape, B, L, dev, algo="softmax")
    ev = engine.GsfEvalEngine(model.shape, B, L, dev)
    w = (args.warmup, args.repeats, args.iters)
    out = {"batch": B, "list_size": L, "rows": B * L, "n_params": model.shape.n_params}
    out["score_ms"] = timed(lambda: ev.forward(model.flat_params, f, n_docs, i), *w)
    ours = ev.scores.clone()
    model.shape.train_shuffle = False
    out["forward_ms"] = timed(lambda: eng.forward(p, f, n_docs, i, train=True), *w)
    eng.loss(y)
    out["backward_ms"] = timed(lambda: eng.backward(p, f, n_docs, i), *w)
    out["step_ms"] = timed(lambda: eng.train_step(p, st, f, n_docs, i, y), *w)
    model.shape.train_shuffle = True
    out["step_shuffle_ms"] = timed(lambda: eng.train_step(p, st, f, n_docs, i, y), *w)
    assert np.isfinite(eng.read_scalars()[0])
    eng.close()
    if args.no_baseline:  # (a profiler run: the library's kernels alone)
        return out
    print(json.dumps(dict(out, partial="library figures; the yardsticks follow")), file=sys.stderr, flush=True)

    # the DNN with 2 F features at the same rows
    torch.manual_seed(0)
    dnn = DNN(hp, m * F).to(dev)
    f2 = torch.tensor(np.concatenate([feats, feats], axis=1), device=dev)
    p2, st2 = dnn.flat_params.clone(), torch.zeros_like(dnn.flat_params)
    eng2 = engine.StepEngine(dnn.shape, B, L, dev, algo="softmax")
    out["dnn272_step_ms"] = timed(lambda: eng2.train_step(p2, st2, f2, n_docs, i, y), *w)
    out["dnn272_route"] = dnn.shape.route(B, L, n_docs)
    eng2.close()

    base = TorchGSF(F, m, hidden)
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
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--shapes", type=str, default=",".join("%dx%d" % s for s in SHAPES), help="batch x list_size, comma separated")
    args = ap.parse_args(argv)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.repeats < 30:
        raise SystemExit("gsf_rate.py takes the median of at least 30 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("gsf_rate.py measures on the GPU: none found")
    rows = []
    for rnd in range(args.rounds):
        for B, L in shapes:
            r = row(B, L, args)
            r["round"] = rnd
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
