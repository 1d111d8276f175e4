#!/usr/bin/env python3
"""Time what the trust-bias click model and AffineRank add, each next to its peer on the same build (figures: profiles/trust_bias.md).

Per round one JSON line per measurement:

  loss        hip_ops.affine_loss next to hip_ops.softmax_ce (the peer kernel with the same traffic: scores, labels, a position
              table in; dscores and one tail partial per list out) at 256 x 10 and 512 x 50
  click       ultr_click_batch with the trust-bias model next to the position-biased model at 256 x 10 (1000 resident queries)
  step        engine.StepEngine.train_step of AffineRank next to IPWrank's (DNN of 136 features, hidden [256, 256], Adagrad) at
              256 x 10 and 512 x 50, under the default route and under ULTR_NO_FUSED_FB=1 (IPWrank without its fused small-batch kernel)

The two sides of a pair alternate repetition by repetition; each figure is the median / min / max over `--repeats` (>= 30)
repetitions after `--warmup` calls; a repetition is `--iters` calls between two device synchronisations on a host clock, divided by
`--iters`.

    python tools/affine_rate.py [--repeats 30] [--iters 200] [--rounds 3] [--out FILE.json]
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
IPW_TABLE = [1.0, 1.4, 1.9, 2.5, 3.2, 4.0, 4.9, 5.9, 7.0, 8.2]


def timed_pair(fa, fb, warmup, repeats, iters):
    """The two callables alternating repetition by repetition: (stats of fa, stats of fb), milliseconds per call."""
    for fn in (fa, fb):
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(repeats):
        for k, fn in enumerate((fa, fb)):
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append(1e3 * (time.perf_counter() - t0) / iters)
    return tuple({"median": statistics.median(o), "min": min(o), "max": max(o), "repeats": repeats, "iters": iters} for o in out)


def trust_tables(dev):
    from ultra_pytorch_amd.utils import click_models as CM
    trust, pbm = CM.TrustBiasModel(0.1, 1.0, 4, 1.0), CM.PositionBiasedModel(0.1, 1.0, 4, 1.0)
    return CM.device_tables(trust, 3, dev), CM.device_tables(pbm, 0, dev)


def loss_row(B, L, args):
    from ultra_pytorch_amd import hip_ops
    dev = torch.device("cuda")
    rng = np.random.RandomState(L)
    s = torch.tensor(rng.normal(size=(B, L)).astype(np.float32), device=dev)
    y = torch.tensor((rng.uniform(size=(L, B)) < 0.3).astype(np.float32), device=dev)
    (image, n, _), _ = trust_tables(dev)
    alpha, beta = image[0].contiguous(), image[1].contiguous()
    table = torch.tensor(IPW_TABLE, device=dev)
    ds = torch.empty(B, L, device=dev)
    ws = torch.zeros(hip_ops.loss_workspace_bytes(B, L) // 4, device=dev)
    a, b = timed_pair(lambda: hip_ops.affine_loss(s, y, alpha, beta, B, L, ds, ws),
                      lambda: hip_ops.softmax_ce(s, y, B, L, ds, ws, ipw_table=table), args.warmup, args.repeats, args.iters)
    return {"what": "loss", "batch": B, "list_size": L, "affine_ms": a, "softmax_ce_ms": b, "ratio": a["median"] / b["median"]}


def click_row(B, L, args):
    from ultra_pytorch_amd import _lib, hip_ops
    dev = torch.device("cuda")
    rng = np.random.RandomState(7)
    n_queries, n_docs = 1000, 10000
    lists = torch.tensor(rng.randint(0, n_docs, size=(n_queries, L)).astype(np.int32), device=dev)
    labels = torch.tensor(rng.randint(0, 5, size=(n_queries, L)).astype(np.float32), device=dev)
    ids = torch.empty(L, B, dtype=torch.int32, device=dev)
    ck = torch.empty(L, B, device=dev)
    q = torch.empty(B, dtype=torch.int32, device=dev)
    lib, step = _lib.load(), [0]

    def draw(tables, model):
        exam, n_exam, cprob = tables

        def fn():
            step[0] += 1
            _lib.check(lib.ultr_click_batch(lists.data_ptr(), labels.data_ptr(), n_queries, L, n_docs, exam.data_ptr(), n_exam, cprob.data_ptr(),
                                            int(cprob.numel()), model, 1, step[0], B, L, 100, ids.data_ptr(), ck.data_ptr(), q.data_ptr(),
                                            hip_ops.raw_stream()), "ultr_click_batch")
        return fn

    trust, pbm = trust_tables(dev)
    a, b = timed_pair(draw(trust, 3), draw(pbm, 0), args.warmup, args.repeats, args.iters)
    return {"what": "click", "batch": B, "list_size": L, "trust_ms": a, "pbm_ms": b, "ratio": a["median"] / b["median"]}


def step_row(B, L, no_fused, args):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    dev = torch.device("cuda")
    F, hidden = MODEL
    if no_fused:
        os.environ["ULTR_NO_FUSED_FB"] = "1"
    else:
        os.environ.pop("ULTR_NO_FUSED_FB", None)
    try:
        shape = hip_ops.DnnShape(F, hidden, "elu")
        feats, ids, clicks = synthetic.make_batch(np.random.RandomState(L), B, L, F, n_pad=2 if L > 10 else 0)
        f, i, y = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(clicks, device=dev)
        n_docs = feats.shape[0]
        (image, n, _), _ = trust_tables(dev)
        tables = {"softmax": torch.tensor(IPW_TABLE, device=dev), "affine": image.reshape(-1).contiguous()}
        p0 = torch.tensor(O.init_params(F, hidden, seed=1), device=dev)
        runs = {}
        for algo in ("affine", "softmax"):
            eng = engine.StepEngine(shape, B, L, dev, algo=algo)  # (the knobs are read here)
            runs[algo] = (eng, p0.clone(), torch.zeros(max(engine.opt_state_floats(algo, "ada", L, shape.n_params), 1), device=dev))

        def step_of(algo):
            eng, p, st = runs[algo]
            return lambda: eng.train_step(p, st, f, n_docs, i, y, ipw_table=tables[algo])

        a, b = timed_pair(step_of("affine"), step_of("softmax"), args.warmup, args.repeats, args.iters)
        for eng, _, _ in runs.values():
            assert np.isfinite(eng.read_scalars()[0])
            eng.close()
    finally:
        os.environ.pop("ULTR_NO_FUSED_FB", None)
    return {"what": "step", "batch": B, "list_size": L, "no_fused_fb": bool(no_fused), "affine_ms": a, "ipw_ms": b,
            "ratio": a["median"] / b["median"], "difference_us": 1e3 * (a["median"] - b["median"])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if args.repeats < 30:
        raise SystemExit("affine_rate.py takes the median of at least 30 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("affine_rate.py measures on the GPU: none found")
    rows = []
    for rnd in range(args.rounds):
        todo = [lambda s=s: loss_row(*s, args) for s in SHAPES] + [lambda: click_row(256, 10, args)]
        todo += [lambda s=s, nf=nf: step_row(*s, nf, args) for s in SHAPES for nf in (False, True)]
        for fn in todo:
            r = fn()
            r["round"] = rnd
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
