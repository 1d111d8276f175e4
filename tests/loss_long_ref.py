"""Long-list cases for the pair-walk losses (csrc/ultr_loss_long.hip), shared by tests/test_loss_long_cpu.py and
tests/test_gpu_losses_long.py: the inputs of tests/loss_ref.make_case and the float64 restatements of tests/loss_ref.py and
tests/prs_ref.py, evaluated LIST BY LIST.

The restatements form [B, L, L] float64 arrays; at 6823 documents one such array is 372 MB per list.  Every word of the step tail is a
sum over the lists and a list's dscores depend on that list alone (the kernels emit them x D, the batch-global normaliser is applied
by the update), so the batch's reference is the per-list references added up - the same functions, a smaller working set."""
import numpy as np

from tests import loss_ref as R
from tests import prs_ref

SHORT_MAX = {"pairdebias": 585, "lambdarank": 531, "prs": 952}   # the longest lists the short kernels take (test_loss_layout_cpu.py)
MSLR = 1251                                                       # MSLR-WEB30K's longest candidate list


def floats(algo, L):
    """Floats of dynamic LDS of the long kernel of `algo`: PairDebiasLongLds, LambdaRankLongLds, PrsLongLds (csrc/ultr_listloss.h) -
    the tail, the O(L) arrays, one partial per wave (16) of a workgroup-wide sum."""
    tail = 4 + 2 * L
    return {"pairdebias": tail + 4 * L + 16, "lambdarank": tail + 5 * L + 6 * L + 16, "prs": tail + 5 * L + 4 * L + 16}[algo]


LIMIT = 160 * 1024
MAX_LIST = {a: max(L for L in range(1, 20000) if floats(a, L) * 4 <= LIMIT) for a in SHORT_MAX}


def make_case(name, algo, B, L, **kw):
    """loss_ref.make_case, unchanged (it builds any length)."""
    return R.make_case(name, algo, B, L, **kw)


_REF = {}


def reference(case, batch_total=None):
    """loss_ref.pairdebias / loss_ref.lambdarank on a case, one list at a time, computed once per process."""
    key = (case["name"], case["B"], batch_total)
    r = _REF.get(key)
    if r is None:
        a, s, y, L, B = case["algo"], case["scores"], case["labels"], case["L"], case["B"]
        tp, tm = case["aux"][:L], case["aux"][L:]
        parts = []
        for b in range(B):
            if a == "pairdebias":
                parts.append(R.pairdebias(s[b:b + 1], y[:, b:b + 1], tp, tm, batch_total=B if batch_total is None else batch_total))
            else:
                parts.append(R.lambdarank(s[b:b + 1], y[:, b:b + 1], tp, tm, float(np.float32(case["kw"].get("sigma", 1.0)))))
        r = dict(tail=sum(p["tail"] for p in parts), tail_abs=sum(p["tail_abs"] for p in parts),
                 ds=np.concatenate([p["ds"] for p in parts]), ds_abs=np.concatenate([p["ds_abs"] for p in parts]))
        _REF[key] = r
    return r


# ---- the whole-step cases: DNN [16, 8] on 12 features, B = 2, L = 1251 -----------------------------------------------------------------
STEP_F, STEP_HIDDEN, STEP_B = 12, [16, 8], 2
# The step tests hold the gradient to the float32 oracle at tests/test_gpu_parity.py's bar (gtol: 1e-5 |g| + 1e-6 max |g|).  At 2502
# rows an entry of the gradient can be a sum that cancels a thousandfold (seed 12, LambdaRank: the first output weight is -0.012 from
# terms that add up to 27 in absolute value), and the float32 ORACLE is then itself 0.79 of that bar away from its own float64
# evaluation - a reference that leaves the code a fifth of the bar.  The seeds below are the first ones from 11 on at which the oracle
# keeps to a quarter of the bar (oracle_share(), asserted by tests/test_loss_long_cpu.py; measured 0.16 and, after 0.37 at seed 11 and
# 0.79 at seed 12, 0.19): chosen by the reference's own error on the CPU, not by a GPU figure.  PRSrank's loss reference is float64
# already (tests/prs_ref.py): its seed is simply the next one.
STEP_SEED = {"pairdebias": 11, "lambdarank": 13, "prs": 14}
ORACLE_SHARE = 0.5  # what the CPU test asserts: chosen at a quarter, held at half - torch's float32 sums differ from CPU to CPU


def step_inputs(algo, L=MSLR):
    from tests.test_gpu_workspace_bounds import dnn_inputs
    return dnn_inputs(STEP_F, STEP_HIDDEN, STEP_B, L, algo, seed=STEP_SEED[algo], n_pad=0)


def oracle_share(algo):
    """The largest |g32 - g64| / (1e-5 |g64| + 1e-6 max(1, max |g64|)) over the gradient of the step case of `algo`: the float32
    oracle's step against the same composition evaluated in float64."""
    import torch
    from oracle import ultr_oracle as O
    d = step_inputs(algo)
    L, ids = d["L"], d["ids"].astype(np.int64)
    step = O.pairdebias_step if algo == "pairdebias" else O.lambdarank_step
    g32 = step(d["params"], d["state"], d["aux"][:L], d["aux"][L:], d["F"], d["hidden"], d["feats"], ids, d["y"], lr=0.05)["grads"]
    p = torch.as_tensor(d["params"], dtype=torch.float64).clone().requires_grad_(True)
    s = O.dnn_forward(p, d["F"], d["hidden"], O.gather_rows(d["feats"], ids).double(), "elu").view(L, STEP_B).t()
    tp, tm = torch.as_tensor(d["aux"][:L]).double(), torch.as_tensor(d["aux"][L:]).double()
    if algo == "pairdebias":
        loss = O.pairdebias_loss(s, torch.as_tensor(d["y"]).double(), tp, tm)[0]
    else:
        loss = O.lambdarank_loss(s, torch.from_numpy(np.ascontiguousarray(d["y"].T)).double(), tp, tm, 1.0)[0]
    g = torch.autograd.grad(loss, p)[0].numpy()
    return float((np.abs(g32 - g) / (1e-5 * np.abs(g) + 1e-6 * max(1.0, float(np.abs(g).max())))).max())


def prs_batch(B, L, seed, per_entry=False):
    """scores [B, L], clicks [L, B] (list 1 % B without a click, as tests/test_gpu_prs.py has one), the table - or, per_entry, a weight
    per list entry [B, L] with a zero among them (pw = 0 there)."""
    rng = np.random.RandomState(seed)
    s = rng.normal(scale=1.5, size=(B, L)).astype(np.float32)  # (the inputs of tests/test_gpu_prs.py: _batch)
    y = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32)
    if B > 1:
        y[:, 1] = 0.0
    y[0, 0] = 1.0
    ipw = np.linspace(1.0, 9.0, 40)
    ipw[4 % 40] = 0.0
    if per_entry:
        ipw = rng.uniform(1.0, 9.0, size=(B, L))
        ipw[0, min(4, L - 1)] = 0.0
    return s, y, ipw.astype(np.float32)


def prs_reference(s, y_LB, ipw, sigma=1.0):
    """(loss, d loss / d scores [B, L], D) of prs_ref.prs_score_grad, one list at a time: a list's loss and gradient times its own
    ideal DCG are what it adds to the kernel's sums, the batch's ideal DCG (D) is the lists' added up."""
    import torch
    B, L = s.shape
    loss_sum, D, g = 0.0, 0.0, np.zeros((B, L), np.float64)
    for b in range(B):
        lab = y_LB[:, b:b + 1].T
        idcg = float(prs_ref.batch_idcg(torch.as_tensor(lab)))
        if idcg == 0.0:
            continue  # no click: every delta-NDCG weight is 0, the list adds nothing
        tab = ipw[b] if np.ndim(ipw) == 2 else ipw
        lb, gb = prs_ref.prs_score_grad(s[b:b + 1].astype(np.float32), lab, tab, sigma)
        loss_sum += lb * idcg
        g[b] = gb[0] * idcg
        D += idcg
    return loss_sum / D, g / D, D
