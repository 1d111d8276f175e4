#!/usr/bin/env python3
"""Time SetRank's evaluation forward through engine.SetRankEvalEngine and print the engine's buffer size (figures:
profiles/setrank_score.md).

Config 5's model (136 features, d_model 256, 8 heads, 2 layers, dff 64) at two shapes: config 5's own (batch 1024 x 100
documents) and batch 64 x 1251 documents, MSLR-WEB30K's longest query.  Per shape one JSON line:

  forward_ms    median / min / max over `--repeats` (>= 30) repetitions after `--warmup` calls; a repetition is `--iters` calls of
                SetRankEvalEngine.forward between two device synchronisations on a host clock, divided by `--iters`
  buffer_bytes  the engine's forward buffer (the scoring buffer; `saved` in a tree from before ultr_setrank_score), and per token
  scores_crc    a checksum of the scores' bits: two trees that print the same value computed the same scores

The tool reads nothing but the engine's public surface, so the same file runs in a checkout of an earlier commit: copy it there, run
both, alternate them (`--rounds` repeats the pair of shapes so that a drift of the machine shows in both).

    python tools/setrank_score_rate.py [--repeats 30] [--iters 100] [--rounds 1] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL = (136, 256, 8, 2, 64)  # F, d_model, heads, layers, dff
SHAPES = ((1024, 100), (64, 1251))


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


def row(B, L, args):
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    dev = torch.device("cuda")
    F, d, H, nl, dff = MODEL
    shape = hip_ops.SetRankShape(F, d, H, nl, dff)
    feats, ids, _ = synthetic.make_batch(np.random.RandomState(L), B, L, F, clicks=False, n_pad=2)
    p = init_setrank_params(shape, seed=0).to(dev)
    f, i = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev)
    eng = engine.SetRankEvalEngine(shape, B, L, dev)
    buf = getattr(eng, "work", None)
    buf = buf if buf is not None else eng.saved
    nbytes = buf.numel() * buf.element_size()
    t = timed(lambda: eng.forward(p, f, feats.shape[0], i), args.warmup, args.repeats, args.iters)
    torch.cuda.synchronize()
    crc = zlib.crc32(eng.scores.cpu().numpy().tobytes())
    out = {"batch": B, "list_size": L, "tokens": B * L, "attn_path": hip_ops.setrank_attn_path(shape, L), "forward_ms": t,
           "buffer_bytes": nbytes, "buffer_bytes_per_token": nbytes / float(B * L), "scores_crc": "%08x" % crc}
    del eng, buf
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--label", type=str, default="")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if args.repeats < 30:
        raise SystemExit("setrank_score_rate.py takes the median of at least 30 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("setrank_score_rate.py measures on the GPU: none found")
    rows = []
    for rnd in range(args.rounds):
        for B, L in SHAPES:
            r = row(B, L, args)
            r["round"], r["label"] = rnd, args.label
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
