"""The cases of tests/test_gpu_dnn_operands.py and of the CPU checks on them (tests/test_dnn_ref_cpu.py): shapes, inputs, operand
variants and the float64 reference (tests/dnn_ref.py).  Plain numpy; nothing here touches the GPU.

Shapes (F, hidden, B, L): the smallest at which each decision of dnn_route (csrc/ultr_dnn.hip) still exists."""
import functools

import numpy as np

from tests import dnn_ref as R

SHAPES = [
    (24, [], 3, 5),               # one Linear layer
    (24, [32], 5, 7),             # 35 rows in three 16-row tiles, the last one ragged
    (136, [64, 32], 6, 9),        # the aligned route is the fused launch on 8 waves
    (24, [256], 5, 16),           # ... on 16 waves, with the split-half copies
    (13, [64], 8, 10),            # odd width (the scalar builds whatever the pointers) and misalignment together
    (40, [128, 64], 440, 10),     # 4400 rows: the aligned route is the wide-tile forward and backward
]
# (shape index, activation, PAD positions per list): elu throughout, one tanh case, one conditioned relu case
CASES = [(0, "elu", 0), (1, "elu", 2), (2, "elu", 0), (3, "elu", 1), (4, "elu", 3), (5, "elu", 0), (1, "tanh", 0), (2, "relu", 2)]
# a case whose fp32 oracle does not stay within a third of the GPU bars of the float64 reference gets another seed here
# (tests/test_dnn_ref_cpu.py); the bars stay
SEEDS = [0, 0, 0, 0, 0, 0, 0, 0]
IPW = np.linspace(1.0, 6.0, 12).astype(np.float32)

# operand variants: byte offsets of params / features / wt from a 16-byte boundary (wt None: no copy), whether a dscores buffer exists
VARIANTS = {
    "aligned": dict(),
    "params+4": dict(params=4),
    "params+8": dict(params=8),
    "params+12": dict(params=12),
    "features+4": dict(features=4),
    "params+4_features+4": dict(params=4, features=4),
    "wt_null": dict(wt=None),
    "wt+4": dict(wt=4),          # read paths only: the calls that write the copies refuse it
    "dscores_null": dict(dscores=False),
}


def operand_bits(variant):
    """The names of _lib.DNN_OPERANDS that hold for a call under the variant."""
    v = VARIANTS[variant]
    out = []
    if v.get("params", 0) == 0:
        out.append("params16")
    if v.get("features", 0) == 0:
        out.append("features16")
    if v.get("wt", 0) is not None:
        out.append("wt")
        if v.get("wt", 0) == 0:
            out.append("wt16")
    if v.get("dscores", True):
        out.append("dscores")
    return out


def case_id(c):
    F, hidden, B, L = SHAPES[c[0]]
    return "F%d_%s_B%dxL%d_%s" % (F, "x".join(map(str, hidden)) or "linear", B, L, c[1])


@functools.lru_cache(maxsize=None)
def inputs(k):
    """Case k: features [n_docs, F], docids [L, B], clicks [L, B], params [P] (fp32, LayerNorm affine parameters away from (1, 0))."""
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import synthetic
    si, act, n_pad = CASES[k]
    F, hidden, B, L = SHAPES[si]
    rng = np.random.RandomState(4000 + 10 * k + SEEDS[k])
    feats, ids, y = synthetic.make_batch(rng, B, L, F, clicks=True, n_pad=n_pad)
    params = O.init_params(F, hidden, seed=70 + k + SEEDS[k])
    for n, s, o in O.param_layout(F, hidden):
        if "layer_norm" in n:
            params[o:o + int(np.prod(s))] += rng.normal(scale=0.2, size=int(np.prod(s))).astype(np.float32)
    share = 0.0
    if act == "relu":
        feats, params, share = R.condition_relu(rng, params, F, hidden, feats, ids)
    return dict(F=F, hidden=hidden, B=B, L=L, act=act, feats=feats, ids=ids, y=y, params=params, redrawn=share)


@functools.lru_cache(maxsize=None)
def reference(k):
    """The float64 reference of case k's IPW step: scores [B, L], loss, D, dscores [B, L] (= d loss / d scores), grads and their
    per-entry sums of |terms| (of the loss: the library's grads are these times D)."""
    d = inputs(k)
    F, hidden, B, L, act = d["F"], d["hidden"], d["B"], d["L"], d["act"]
    x = R.gather(d["feats"], d["ids"])
    fw = R.forward(d["params"], F, hidden, x, act)
    scores = R.scores_BL(fw["scores"], B, L)
    pw = R.ipw_weights(d["y"], IPW)
    loss, dsc, D = R.softmax_loss(scores, d["y"].T, pw)
    # row n = l * B + b of the position-major batch takes dscores[b, l]
    grads, terms = R.backward(d["params"], F, hidden, x, dsc.T.reshape(-1), act, fwd=fw)
    return dict(scores=scores, loss=loss, D=D, dscores=dsc, grads=grads, terms=terms, pw=pw, x=x, fwd=fw)


# ---- the project's bars (tests/test_gpu_full_size.py, tests/test_gpu_planner_sweep.py), as error-to-bar ratios ---------------------
def score_ratio(got, ref):
    return float((np.abs(np.asarray(got, np.float64) - ref) / (1e-5 + 1e-5 * np.abs(ref))).max())


def loss_ratio(got, ref):
    return abs(float(got) - ref) / (1e-5 * max(1.0, abs(ref)))


def grad_ratio(got, ref, terms):
    return float((np.abs(np.asarray(got, np.float64) - ref) / (1e-5 * (np.abs(ref) + terms) + 1e-12)).max())
