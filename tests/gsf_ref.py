"""The yardstick for the GSF ranking model: a restatement in stock torch on the CPU (nn.LayerNorm / nn.Linear on explicitly built groups,
autograd for the gradients), evaluated in float64.  The reference holds no GSF code, so nothing is recorded from it; the model is the one
DESIGN.md section 3e fixes.  CPU only - GPU tests compute it once per case and share it.

Also here: the fixed inputs of the GPU tests (uniform features, one list with PADs from the middle to the end, one list all PADs, normal
dscores), the Python twin of the shuffle law (ultr_gsf_shuffle) on tests/philox_ref.py, and the parity bar
max|err| <= 1e-5 * max|ref| per tensor."""
import numpy as np
import torch
import torch.nn as nn

from tests import philox_ref as P

# (B, L, F, m, hidden): ragged tiles with widths off the 16 grid; one position (m > L); no hidden layer; lists longer than a wave; the
# real widths; K = m F = 1400; and the largest group (every slot of the kernels' unrolled loops, a document twice in a group)
SHAPES = [(5, 7, 12, 2, [20, 8]), (4, 1, 12, 2, [8]), (3, 5, 16, 3, []), (3, 70, 16, 4, [32]), (33, 10, 136, 2, [512, 256, 128]),
          (3, 3, 700, 2, [64]), (3, 6, 8, 8, [16])]
WIDE = 5  # the index of the K = 1400 shape
BAR = 1e-5
SHUFFLE_TAG = 0x47534653  # csrc/ultr_device.h: ULTR_GSF_SHUFFLE_TAG
ACT = {"elu": nn.ELU, "relu": nn.ReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid}

# The edge cases of tests/test_gpu_gsf_edges.py, (B, L, F, m, hidden, activation) (NOT part of SHAPES: other tests index that).  Each
# sits on a boundary of csrc/ultr_gsf_plan.h, csrc/ultr_gemm.h or csrc/ultr_sr_rows.hip; tests/test_model_edges_cpu.py proves that it does.
EDGES = {}
for _k in (0, 4):  # every activation id through both tile widths of the first product (N = 20 and N = 512) and the LayerNorm backward
    for _a in ("relu", "tanh", "sigmoid"):
        EDGES["act-%s-%d" % (_a, _k)] = SHAPES[_k] + (_a,)
EDGES.update({
    "act-tanh-no-hidden": (3, 5, 16, 3, [], "tanh"),   # no hidden layer: the activation changes nothing (the elu model's bits)
    "slots-5": (3, 9, 12, 5, [16], "elu"),              # the unrolled slot selects of AGroupLN::raw ...
    "slots-6": (3, 4, 12, 6, [16], "relu"),             # ... with m > L: a document twice in a group
    "slots-7": (3, 9, 12, 7, [20, 8], "tanh"),
    "wide-N-walk": (272, 64, 12, 2, [512], "relu"),     # T = 17408: 1088 chunks of the 64x128 tile; wgrad chunk 272
    "long": (2300, 33, 12, 3, [24, 8], "sigmoid"),      # T = 75900: 1186 chunks of the 64x64 tile, 297 column-sum chunks, wgrad chunk 1188
})
NO_HIDDEN_EDGE = "act-tanh-no-hidden"
EDGE_SEED = {"wide-N-walk": 429, "long": 423}  # a case's own seed where 400 + its index leaves e32 little room under the bar / the cap of
# tests/test_model_edges_cpu.py (wide-N-walk at 410: 1.6e-5 for layer_norm1.bias; long at 411: 7.7e-6 on one of two hosts)
PERMUTED_ONLY = ("wide-N-walk", "long")                 # the large cases run under a permutation only
GUARDED_DIRECT = ("wide-N-walk", "long")                # the direct C-ABI call on a guarded arena
GUARDED_STEPS = ("wide-N-walk",)                        # two guarded engine steps
EDGE_RUNS = [(n, pm) for n in EDGES for pm in (False, True) if pm or n not in PERMUTED_ONLY]


class Twin(nn.Module):
    """state_dict keys and order are the DNN's: sequential.layer_norm{j}.{weight,bias}, sequential.linear{j}.{weight,bias}."""

    def __init__(self, feature_size, hidden, group_size, activation="elu"):
        super().__init__()
        self.F, self.m, self.k = int(feature_size), int(group_size), len(hidden)
        self.sequential = nn.Module()
        width = self.F * self.m
        for j, out in enumerate(list(hidden) + [self.m]):
            self.sequential.add_module("layer_norm%d" % j, nn.LayerNorm(width, eps=1e-5))
            self.sequential.add_module("linear%d" % j, nn.Linear(width, out))
            width = out
        self.act = ACT[activation]()

    def network(self, u):
        """[..., m F] -> [..., m]: LayerNorm precedes every Linear, the activation follows every Linear but the last."""
        h = u
        for j in range(self.k + 1):
            h = getattr(self.sequential, "linear%d" % j)(getattr(self.sequential, "layer_norm%d" % j)(h))
            if j < self.k:
                h = self.act(h)
        return h

    def forward(self, x, perm=None):
        """x [B, L, F] in presented order (PAD rows are zero rows), perm [B, L] int64 or None -> scores [B, L] in presented order."""
        B, L, _ = x.shape
        if perm is None:
            perm = torch.arange(L).expand(B, L)
        at_place = torch.gather(x, 1, perm.unsqueeze(-1).expand(B, L, self.F))          # [b, p] = the document at place p
        groups = torch.cat([torch.roll(at_place, -j, dims=1) for j in range(self.m)], dim=-1)  # slot j of group g: place (g + j) mod L
        o = self.network(groups)                                                         # [B, L, m]
        by_place = torch.zeros(B, L, dtype=x.dtype)
        for j in range(self.m):                                                          # place p: sum_j o[(p - j) mod L][j], j ascending
            by_place = by_place + torch.roll(o[:, :, j], j, dims=1)
        return torch.zeros(B, L, dtype=x.dtype).scatter(1, perm, by_place)


def brute_force_scores(twin, x, perm=None):
    """The score law as a loop over groups: every output of every group is added to the document it names."""
    B, L, F = x.shape
    scores = torch.zeros(B, L, dtype=x.dtype)
    for b in range(B):
        pm = list(range(L)) if perm is None else [int(v) for v in perm[b]]
        for g in range(L):
            members = [pm[(g + j) % L] for j in range(twin.m)]
            o = twin.network(torch.cat([x[b, d] for d in members]))
            for j, d in enumerate(members):
                scores[b, d] = scores[b, d] + o[j]
    return scores


def twin_from(state_dict, feature_size, hidden, group_size, activation="elu", dtype=torch.float64):
    """The twin loaded BY NAME from a model's state_dict (any device), in `dtype`."""
    t = Twin(feature_size, hidden, group_size, activation)
    t.load_state_dict({k: v.detach().cpu() for k, v in state_dict.items()}, strict=True)
    return t.to(dtype)


def gather(features, docids_LB, dtype=torch.float64):
    """x [B, L, F] from the feature matrix [n_docs, F] and position-major ids [L, B] (PAD = n_docs -> the zero row)."""
    f = torch.as_tensor(features, dtype=dtype)
    ids = torch.as_tensor(np.asarray(docids_LB), dtype=torch.int64).t()
    padded = torch.cat([f, torch.zeros(1, f.shape[1], dtype=dtype)], dim=0)
    return padded[ids.clamp(max=f.shape[0])]


def make_inputs(B, L, F, seed=0):
    """features [n_docs, F] f32 uniform in [-1, 1), docids [L, B] i32, dscores [B, L] f32 normal: list B - 1 is all PADs, list B - 2 has
    PADs from the middle on."""
    g = torch.Generator().manual_seed(2000 + seed)
    ids = np.arange(B * L, dtype=np.int32).reshape(B, L)
    n_docs = B * L
    ids[B - 1, :] = n_docs
    if B >= 2:
        ids[B - 2, L // 2 + (0 if L > 1 else 1):] = n_docs
    features = (2.0 * torch.rand(n_docs, F, generator=g) - 1.0).float()
    dscores = torch.randn(B, L, generator=g).float()
    return features, np.ascontiguousarray(ids.T), dscores


def numpy_perm(B, L, seed):
    """A seeded permutation per list, [B, L] int32 (the GPU tests' `perm`; the model's own draw is `shuffle` below)."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.permutation(L) for _ in range(B)]).astype(np.int32)


def reference(state_dict, F, hidden, m, features, docids_LB, dscores, perm=None, activation="elu", dtype=torch.float64):
    """scores [B, L] and {name: gradient} of sum(scores * dscores), in `dtype`."""
    t = twin_from(state_dict, F, hidden, m, activation, dtype)
    pm = None if perm is None else torch.as_tensor(np.asarray(perm), dtype=torch.int64)
    scores = t(gather(features, docids_LB, dtype), pm)
    (scores * dscores.to(dtype)).sum().backward()
    return scores.detach(), {k: p.grad.detach() for k, p in t.named_parameters()}


def rel_err(got, ref):
    """max|got - ref| / max|ref| (the project's parity measure; an all-zero reference compares absolutely)."""
    ref = ref.double()
    scale = float(ref.abs().max())
    return float((got.detach().cpu().double() - ref).abs().max()) / (scale if scale > 0 else 1.0)


def shuffle(seed, step, B, L):
    """ultr_gsf_shuffle's law: list b starts from the identity; i = L - 1 .. 1: r = word i % 4 of Philox(b, 0, i / 4, SHUFFLE_TAG) under
    key(seed, step), j = (r * (i + 1)) >> 32, swap entries i and j.  [B, L] int32."""
    k = P.key(seed, step)
    perm = np.tile(np.arange(L, dtype=np.int32), (B, 1))
    blocks = np.arange((L + 3) // 4, dtype=np.uint64)
    for b in range(B):
        w = P.philox4x32(b, 0, blocks, SHUFFLE_TAG, *k)
        for i in range(L - 1, 0, -1):
            j = (int(w[i & 3][i >> 2]) * (i + 1)) >> 32
            perm[b, i], perm[b, j] = perm[b, j], perm[b, i]
    return perm


def float32_error(ref_scores, ref_grads, scores32, grads32):
    """e32 per tensor: the twin evaluated in float32 on the CPU against its float64 evaluation ({"scores": ..., name: ...})."""
    e = {"scores": rel_err(scores32, ref_scores)}
    e.update({k: rel_err(grads32[k], ref_grads[k]) for k in ref_grads})
    return e


def one_thread(fn, *args, **kw):
    """fn(*args) with torch on ONE CPU thread: a float32 sum over many rows depends on how torch splits it over threads (the long
    case's e32 moved between 1e-6 and 1e-5 with the thread count alone); one thread is the same chain whatever the host offers."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn(*args, **kw)
    finally:
        torch.set_num_threads(n)


def widened_bars(e32):
    """The K = 1400 shape's rule, per tensor: max(BAR, 4 e32) - wider than BAR only where e32 > BAR / 4 (the factor 4: another summation
    order over the same terms)."""
    return {k: max(BAR, 4.0 * e) for k, e in e32.items()}


def hparams(hidden, m, activation="elu"):
    return "hidden_layer_sizes=[%s],group_size=%d,activation_func=%s" % (",".join(str(h) for h in hidden), m, activation)


_EDGE_CACHE = {}


def edge_case(name, permuted, activation=None):
    """(model, feats, ids, dsc, perm, ref_scores, ref_grads, e32) of EDGES[name] in presented order or under a seeded permutation:
    parameters (LayerNorm off 1 / 0), inputs, the float64 reference and the twin's per-tensor float32 error - computed once, shared by
    the GPU tests and tests/test_model_edges_cpu.py, never modified.  `activation` replaces the case's own (the same parameters and
    inputs: the draws do not depend on it)."""
    key = (name, permuted, activation)
    if key not in _EDGE_CACHE:
        from ultra_pytorch_amd.ranking_model import GSF
        k = list(EDGES).index(name)
        B, L, F, m, hidden, act = EDGES[name]
        act = activation or act
        seed = EDGE_SEED.get(name, 400 + k)
        torch.manual_seed(seed)
        model = GSF(hparams(hidden, m, act), F)
        with torch.no_grad():
            for pname, p in model.state_dict().items():
                if "layer_norm" in pname:
                    p.add_(0.3 * torch.randn(p.shape))
        feats, ids, dsc = make_inputs(B, L, F, seed=seed)
        perm = numpy_perm(B, L, 100 + seed) if permuted else None
        sd = model.state_dict()
        ref_scores, ref_grads = reference(sd, F, hidden, m, feats, ids, dsc, perm, act)
        e32 = float32_error(ref_scores, ref_grads, *one_thread(reference, sd, F, hidden, m, feats, ids, dsc, perm, act, dtype=torch.float32))
        _EDGE_CACHE[key] = (model, feats, ids, dsc, perm, ref_scores, ref_grads, e32)
    return _EDGE_CACHE[key]
