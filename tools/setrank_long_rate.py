#!/usr/bin/env python3
"""Time SetRank's validation forward at long lists on the GPU (figures: profiles/setrank_long.md).

Config-5 width (F = 220, d = 256, H = 8, 2 layers, dff = 64), list sizes 128 / 256 / 257 / 512 / 1251 with the batch chosen for about
100k tokens.  Per list size, one JSON line with

  forward_ms          engine.SetRankEvalEngine.forward - the library's forward, the attention kernel the dispatch picks
  torch_ms            the same forward in stock PyTorch-ROCm ops on the same GPU (tools/torch_rocm_baseline.SetRank, no_grad)
  attn_us_per_launch  the attention launches alone: device time of the kernels named *sr_attn* in a torch.profiler trace of five
                      forwards (a pass of its own, after the timed windows), mean / min / max over the launches;
                      attn_tflops = 4 B L^2 d / the mean, attn_peak_share = that over the fp32 matrix peak (157.3 TFLOP/s: exact-fp32
                      MFMA runs at the vector rate) from the mean, the slowest and the fastest launch; null where the trace shows no
                      such kernel: not measured

then the same with ULTR_SR_ATTN_LONG_MIN lowered (the streaming kernel at 128, and at 192 / 256 against the scalar kernel of
129 .. 256; default and lowered rows alternate, twice), and one BaseAlgorithm.validation_set pass over a resident set of 1251-document lists.  Every time is the median of
`--repeats` windows of `--iters` calls, a host clock around a window that ends in a device synchronisation, with the spread
(min .. max) beside it; the last line repeats everything as ONE JSON object.

    python tools/setrank_long_rate.py [--out FILE.json]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F, D, H, NL, DFF = 220, 256, 8, 2, 64
FP32_MATRIX_PEAK = 157.3e12


def windows(fn, warmup, repeats, iters):
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
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def kernel_name(name):
    m, t = re.search(r"sr_attn\w*", name), re.search(r"<(\d+)>", name)
    return m.group(0) + ("<%s>" % t.group(1) if t else "")


def attention_time_us(fn, n_calls=5):
    """Device time per attention launch over n_calls forwards: {"mean", "min", "max", "launches", "kernels"}; None when the trace holds
    no kernel named *sr_attn*."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(n_calls):
            fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if "sr_attn" in e.name]
    if not evs:
        return None
    t = [float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)) for e in evs]
    return {"mean": sum(t) / len(t), "min": min(t), "max": max(t), "launches": len(t), "kernels": sorted({kernel_name(e.name) for e in evs})}


def set_knob(value):
    from ultra_pytorch_amd import _lib
    if value is None:
        os.environ.pop("ULTR_SR_ATTN_LONG_MIN", None)
    else:
        os.environ["ULTR_SR_ATTN_LONG_MIN"] = str(value)
    _lib.load().ultr_config_reload()


def forward_row(L, tokens, args, long_min=None, with_torch=True):
    from tools import torch_rocm_baseline as T
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    dev = torch.device("cuda")
    B = max(1, int(round(tokens / float(L))))
    set_knob(long_min)
    try:
        shape = hip_ops.SetRankShape(F, D, H, NL, DFF)
        feats, ids, _ = synthetic.make_batch(np.random.RandomState(L), B, L, F, clicks=False, n_pad=2)
        p = init_setrank_params(shape, seed=0).to(dev)
        f, i = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev)
        eng = engine.SetRankEvalEngine(shape, B, L, dev)
        run = lambda: eng.forward(p, f, feats.shape[0], i)  # noqa: E731
        row = {"list_size": L, "batch": B, "tokens": B * L, "long_min": long_min, "attn_path": hip_ops.setrank_attn_path(shape, L),
               "forward_ms": windows(run, args.warmup, args.repeats, args.iters)}
        at = attention_time_us(run)
        flops = 4.0 * B * float(L) * L * D  # per launch: S = x x^T and P V over every (list, head)
        row["attn_us_per_launch"] = at
        row["attn_tflops"] = None if at is None else flops / (at["mean"] * 1e-6) / 1e12
        # from the mean, the slowest and the fastest launch: the spread a comparison of two shares has to exceed
        row["attn_peak_share"] = None if at is None else [flops / (at[k] * 1e-6) / FP32_MATRIX_PEAK for k in ("mean", "max", "min")]
        if with_torch:
            torch.manual_seed(0)
            model = T.SetRank(F, D, H, NL, DFF).to(dev)
            ft = torch.cat([f, torch.zeros(1, F, device=dev)])
            it = i.long()
            with torch.no_grad():
                row["torch_ms"] = windows(lambda: model.scores(ft, it), args.warmup, args.repeats, max(1, args.iters // 2))
            del model, ft, it
        del eng
        torch.cuda.empty_cache()
        return row
    finally:
        set_knob(None)


class SyntheticSet:
    """n_queries lists of exactly L documents drawn from a pool of n_docs feature rows (a padded Raw_data look-alike)."""

    def __init__(self, n_queries, L, n_docs, seed):
        rng = np.random.RandomState(seed)
        self.feature_size, self.rank_list_size = F, L
        self.features = np.concatenate([rng.uniform(-1, 1, size=(n_docs, F)).astype(np.float32), np.zeros((1, F), np.float32)])
        self.dids = ["d%d" % i for i in range(n_docs)]
        self.qids = ["q%d" % q for q in range(n_queries)]
        self.initial_list = rng.randint(0, n_docs, size=(n_queries, L)).tolist()
        self.labels = rng.randint(0, 5, size=(n_queries, L)).tolist()


def validation_set_row(L, args):
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import find_class, metrics
    metrics.RankingMetricKey.MAX_LABEL = 4.0
    ds = SyntheticSet(args.set_queries, L, 65536, seed=L)
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.SetRank.SetRank",
           "ranking_model_hparams": "d_model=%d,num_heads=%d,num_layers=%d,diff=%d" % (D, H, NL, DFF),
           "max_candidate_num": L, "selection_bias_cutoff": 10, "metrics": ["ndcg", "mrr", "err"], "metrics_topn": [1, 3, 5, 10]}
    algo = find_class(exp["learning_algorithm"])(ds, exp)
    feed = input_layer.DeviceDirectLabelFeed(algo, args.set_batch, "")
    t = windows(lambda: algo.validation_set(feed, ds)[0], 1, args.repeats, 1)
    return {"validation_set": True, "list_size": L, "queries": args.set_queries, "batch": args.set_batch, "pass_ms": t,
            "queries_per_s": args.set_queries / (1e-3 * t["median"])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=100000)
    ap.add_argument("--lists", type=int, nargs="+", default=[128, 256, 257, 512, 1251])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--set-queries", type=int, default=512)
    ap.add_argument("--set-batch", type=int, default=64)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("setrank_long_rate.py measures on the GPU: none found")
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    for L in args.lists:
        emit(forward_row(L, args.tokens, args))
    # the streaming kernel below the default hand-over point, against the one-pass matrix-core kernel at 128 and the scalar kernel at
    # 192 / 256: default and lowered knob alternate, twice, so that a drift of the machine shows in both
    for L, low in ((128, 17), (192, 129), (256, 129)):
        for _ in range(2):
            emit(forward_row(L, args.tokens, args, with_torch=False))
            emit(forward_row(L, args.tokens, args, long_min=low, with_torch=False))
    emit(validation_set_row(1251, args))
    print(json.dumps({"tool": "setrank_long_rate", "width": [F, D, H, NL, DFF], "rows": rows}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
