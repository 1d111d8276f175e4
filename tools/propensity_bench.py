#!/usr/bin/env python3
"""Sessions per second of the GPU propensity estimator (ultr_propensity_count), on the GPU box:

    python tools/propensity_bench.py [--sessions 10000000] [--repeats 5] [--out profiles/propensity_bench.json]

Per case (click model, list length; 1000 synthetic label lists of that length, labels 0 .. 4): the device path alone - device events
around the count calls of one table, median over --repeats after a warm-up - and RandomizedPropensityEstimator.
estimateParametersFromModel end to end (upload, count, read-back, the table formula; host clock, ends in a synchronising copy).
The host comparison is the reference's own loop, timed by tests/golden/make_golden_propensity.py (propensity_ref.npz: seconds,
sessions).  For the kernel's rocprofv3 line run this under `rocprofv3 --kernel-trace --stats` with --repeats 1, in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DATA = os.path.join(ROOT, "ultra_pytorch_amd", "data")
CASES = [("pbm_0.1_1.0_4_1.0.json", 10), ("cascade_0.1_1.0_4_1.0.json", 10), ("ubm_0.1_1_4_1.0.json", 10), ("pbm_0.1_1.0_4_1.0.json", 120)]


class Lists(object):
    def __init__(self, n_lists, length, seed=0):
        rng = np.random.RandomState(seed)
        self.labels = [[int(v) for v in rng.randint(0, 5, size=length)] for _ in range(n_lists)]
        self.rank_list_size = length


def main():
    import torch
    from ultra_pytorch_amd import hip_ops
    from ultra_pytorch_amd.utils import click_models as CM
    from ultra_pytorch_amd.utils import propensity_estimator as PE
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "propensity_bench.py measures the GPU path: it needs a GPU"
    dev = torch.device("cuda")
    rows = []
    for name, length in CASES:
        with open(os.path.join(DATA, name)) as f:
            cm = CM.loadModelFromJson(json.load(f))
        data = Lists(1000, length)
        mid = PE.CLICK_MODEL_IDS[cm.model_name]
        ep = cm.exam_prob
        if mid == 2:
            ep = [[(row[c] if c < len(row) else 0.0) for c in range(len(ep))] for row in ep]
        labels = torch.tensor(data.labels, dtype=torch.float32, device=dev)
        lengths = torch.full((len(data.labels),), length, dtype=torch.int32, device=dev)
        exam = torch.tensor(ep, dtype=torch.float32, device=dev).contiguous()
        cprob = torch.tensor(cm.click_prob, dtype=torch.float32, device=dev)
        table = torch.zeros(length, length, dtype=torch.int64, device=dev)

        def count(n):
            for first in range(0, n, PE.SESSIONS_PER_CALL):
                hip_ops.propensity_count(labels, lengths, exam, len(cm.exam_prob), cprob, mid, 0, first, min(PE.SESSIONS_PER_CALL, n - first), table)

        count(min(args.sessions, 1 << 20))  # warm-up: the code object is loaded, the shape's kernel has run
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            table.zero_()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            count(args.sessions)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        clicks = int(table.sum())
        est = PE.RandomizedPropensityEstimator()
        w0 = time.perf_counter()
        est.estimateParametersFromModel(cm, data, session_num=args.sessions, seed=0)
        wall = time.perf_counter() - w0
        assert np.array_equal(est.click_count, table.cpu().numpy())  # same (seed, sessions): the same table, bit for bit
        med = float(np.median(ms))
        row = {"click_model": cm.model_name, "list_length": length, "n_lists": len(data.labels), "sessions": args.sessions,
               "clicks": clicks, "device_ms_median": med, "device_ms_min": float(min(ms)), "device_ms_max": float(max(ms)),
               "device_sessions_per_s": args.sessions / (med * 1e-3), "end_to_end_s": wall,
               "end_to_end_sessions_per_s": args.sessions / wall, "IPW_list_head": est.IPW_list[:10]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
