"""GPU box: the update launch alone, Adagrad against Adam, at config 2's parameter count (DNN [256, 256] on 136 features: the tiled
kernel that keeps the weight copies) and config 5's (SetRank d_model 256, 8 heads, 2 layers, dff 64 on 220 features: the flat
kernel).  Adam moves 6 P floats of parameters and state (p, m, v in and out) where Adagrad moves 4 P (p, s), each plus the P
gradient words.  Back-to-back launches on synthetic gradients, stream-timed; prints the launch table of profiles/adam.md and, with
--out FILE, appends it there.
   python tools/update_rate.py [--out out/update_rate.md] [--launches 2000]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ultra_pytorch_amd import _lib, engine, hip_ops  # noqa: E402


def time_update(shape, P, L, optimizer, launches, rows):
    """Microseconds per ultr_apply_update with `optimizer` ('ada' / 'adam'); shape = None: the flat kernel."""
    lib = _lib.load()
    dev = torch.device("cuda")
    rng = np.random.RandomState(1)
    tail = hip_ops.tail_floats(L)
    grads = torch.zeros(P + tail, device=dev)
    grads[:P] = torch.from_numpy((1e-6 * rng.standard_normal(P)).astype(np.float32)).to(dev)  # tiny: thousands of launches must not
    grads[P], grads[P + 1] = 1.0, 1.0                                                       # walk the weights out of the split-half range
    n_ws = (P + tail + 63) // 64 + P // 4096 + 16
    if shape is not None:
        n_ws = max(n_ws, shape.bwd_workspace_bytes(rows) // 4)
    ws, sc = torch.zeros(n_ws, device=dev), torch.zeros(16, device=dev)
    hip_ops.grad_sumsq(grads, P, L, ws)
    u = _lib.UpdateDesc()
    u.algo, u.optimizer, u.list_size, u.n_params = _lib.ALGO_SOFTMAX, engine.optimizer_id(optimizer), L, P
    # (Adam's step is scale-free: a rate of 1e-9 keeps thousands of equal-sign steps inside the weight copies' range)
    u.learning_rate, u.max_gradient_norm = (1e-9 if optimizer == "adam" else 0.05), 5.0
    u.adagrad_eps, u.adam_t = (_lib.ADAM_EPS if optimizer == "adam" else 1e-10), 1000
    if shape is not None:
        from ultra_pytorch_amd.ranking_model import init_flat_params
        p = init_flat_params(shape, seed=0).to(dev)
        wt = hip_ops.weight_copy(shape).get(p)
        desc, wtp = ctypes.byref(shape.desc), wt.data_ptr()
    else:
        p = torch.from_numpy(rng.uniform(-0.1, 0.1, size=P).astype(np.float32)).to(dev)
        desc, wtp = None, None
    st = torch.zeros(engine.opt_state_floats("softmax", optimizer, L, P), device=dev)
    args = (ctypes.byref(u), desc, p.data_ptr(), wtp, st.data_ptr(), grads.data_ptr(), None, ws.data_ptr(), sc.data_ptr(), hip_ops.raw_stream())
    for _ in range(50):
        _lib.check(lib.ultr_apply_update(*args), "ultr_apply_update")
    torch.cuda.synchronize()
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            lib.ultr_apply_update(*args)
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / launches
        best = us if best is None else min(best, us)
    assert bool(torch.isfinite(p).all())
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=2000)
    a = ap.parse_args()
    dnn = hip_ops.DnnShape(136, [256, 256], "elu")
    sr = hip_ops.SetRankShape(220, 256, 8, 2, 64)
    rows = ["| parameters | kernel | Adagrad us | Adam us | Adam / Adagrad |", "|---|---|---|---|---|"]
    for name, shape, P, L, n_rows in (("config 2 (DNN [256,256], F 136)", dnn, dnn.n_params, 10, 2560),
                                      ("config 5 (SetRank 256 x 8 x 2 x 64, F 220)", None, sr.n_params, 100, 0)):
        ada = time_update(shape, P, L, "ada", a.launches, n_rows)
        adam = time_update(shape, P, L, "adam", a.launches, n_rows)
        rows.append("| %s: %d | %s | %.2f | %.2f | %.2f |" % (name, P, "tiled (weight copies)" if shape is not None else "flat", ada, adam, adam / ada))
    text = "\n".join(rows) + "\n(best of 5 runs of %d back-to-back launches, stream-timed: launch rate, host overhead included)\n" % a.launches
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
