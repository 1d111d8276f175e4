#!/usr/bin/env python3
"""Time SetRank's training step at long lists on the GPU, for a model with attention_backward=streaming (figures:
profiles/setrank_long_train.md).

Width: 136 features, d_model 256, 8 heads of depth 32, 2 layers, dff 64.  List sizes 128 / 300 / 439 / 1251 with the batch chosen for
about `--tokens` tokens.  Per list size, one JSON line with

  step_ms             engine.SetRankStepEngine.train_step (forward, softmax loss, backward, update)
  attn_bwd_us         the attention backward launches alone: device time of the kernels named *sr_attn_bwd* in a torch.profiler trace of
                      five steps (a pass of its own, behind the timed windows), mean / min / max over the launches; attn_t_us the same for
                      the pre-pass sr_attn_t_kernel (null where none ran)
  attn_bwd_tflops     FLOP of the five products of a launch (2 B L^2 d each: S, dP^T, dP, dq + dk, dv - one S / dP^T / dP tile per
                      pair of an own and a partner block, in the streaming kernel as in the one-pass kernel) over the mean, and its share
                      of the fp32 matrix peak (157.3 TFLOP/s)

then the longest list at head depth 64 and 16 (4 and 16 heads), and, at 128 documents with ULTR_SR_ATTN_H3=0, the streaming kernels (ULTR_SR_ATTN_LONG_MIN=17) against the one-pass fp32 matrix-core
kernels of a model without the flag: the two alternate, twice, in this one process.  Every time is the median of `--repeats` windows of
`--iters` steps, a host clock around a window that ends in a device synchronisation, with (min .. max); the last line repeats everything
as ONE JSON object.

    python tools/setrank_long_train_rate.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.setrank_long_rate import FP32_MATRIX_PEAK, kernel_name, windows  # noqa: E402

F, D, H, NL, DFF = 136, 256, 8, 2, 64


def set_knobs(**kv):
    """Set (value) or clear (None) library knobs and have the library read them."""
    from ultra_pytorch_amd import _lib
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    _lib.load().ultr_config_reload()


def kernel_times_us(fn, pattern, n_calls=5):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(n_calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for key, pat in pattern.items():
        evs = [e for e in prof.events() if pat in e.name]
        t = [float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)) for e in evs]
        out[key] = None if not t else {"mean": sum(t) / len(t), "min": min(t), "max": max(t), "launches": len(t),
                                       "kernels": sorted({kernel_name(e.name) for e in evs})}
    return out


def step_row(L, tokens, args, streaming=True, knobs=None, heads=H):
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    dev = torch.device("cuda")
    B = max(1, int(round(tokens / float(L))))
    knobs = knobs or {}
    set_knobs(**knobs)
    try:
        shape = hip_ops.SetRankShape(F, D, heads, NL, DFF, attention_backward="streaming" if streaming else "one_pass")
        feats, ids, y = synthetic.make_batch(np.random.RandomState(L), B, L, F, n_pad=2)
        p = init_setrank_params(shape, seed=0).to(dev)
        st = torch.zeros_like(p)
        f, i, yy = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(y, dtype=torch.float32, device=dev)
        tab = torch.tensor(np.asarray(synthetic.load_ipw(), np.float32), device=dev)
        eng = engine.SetRankStepEngine(shape, B, L, dev, algo="softmax", learning_rate=0.05, max_gradient_norm=5.0)
        run = lambda: eng.train_step(p, st, f, feats.shape[0], i, yy, ipw_table=tab)  # noqa: E731
        row = {"list_size": L, "batch": B, "tokens": B * L, "head_depth": D // heads, "streaming": streaming, "knobs": knobs,
               "attn_path": [hip_ops.setrank_attn_path(shape, L), hip_ops.setrank_attn_path(shape, L, backward=True)],
               "step_ms": windows(run, args.warmup, args.repeats, args.iters)}
        kt = kernel_times_us(run, {"bwd": "sr_attn_bwd", "t": "sr_attn_t"})
        flops = 5.0 * 2.0 * B * float(L) * L * D
        row["attn_bwd_us"], row["attn_t_us"] = kt["bwd"], kt["t"]
        row["attn_bwd_tflops"] = None if kt["bwd"] is None else flops / (kt["bwd"]["mean"] * 1e-6) / 1e12
        row["attn_bwd_peak_share"] = None if kt["bwd"] is None else flops / (kt["bwd"]["mean"] * 1e-6) / FP32_MATRIX_PEAK
        eng.close()
        del eng
        torch.cuda.empty_cache()
        return row
    finally:
        set_knobs(**{k: None for k in knobs})


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=51200)
    ap.add_argument("--lists", type=int, nargs="+", default=[128, 300, 439, 1251])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("setrank_long_train_rate.py measures on the GPU: none found")
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    for L in args.lists:
        emit(step_row(L, args.tokens, args))
    # the other matrix-core head depths at the longest list (64: one workgroup per CU, see the kernel's comment)
    for heads in (4, 16):
        emit(step_row(max(args.lists), args.tokens, args, heads=heads))
    # 128 documents, fp32 matrix cores on both sides: one pass (no flag) and streaming (flag, hand-over lowered) alternate, twice
    for _ in range(2):
        emit(step_row(128, args.tokens, args, streaming=False, knobs={"ULTR_SR_ATTN_H3": 0}))
        emit(step_row(128, args.tokens, args, streaming=True, knobs={"ULTR_SR_ATTN_H3": 0, "ULTR_SR_ATTN_LONG_MIN": 17}))
    print(json.dumps({"tool": "setrank_long_train_rate", "width": [F, D, H, NL, DFF], "rows": rows}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
