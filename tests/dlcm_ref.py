"""The yardstick for the DLCM ranking model: a restatement in stock torch on the CPU (nn.LayerNorm, nn.GRU on the flipped list, the
local ranking function), evaluated in float64 with autograd.  The reference holds no DLCM code, so nothing is recorded from it; the
model is the one DESIGN.md section 3d fixes.  CPU only - GPU tests compute it once per shape and share it.

Also here: the fixed inputs of the GPU tests (features 3 * randn, one list with PADs from the middle to the end, one list all PADs,
random dscores) and the parity bar max|err| <= 1e-5 * max|ref| per tensor."""
import numpy as np
import torch
import torch.nn as nn

# (B, L, F, H, heads): ragged row tile with H off the 16 grid; a single position (s = o_0); a long recurrence; the real width with three
# row tiles and one list in the last
SHAPES = [(5, 7, 12, 20, 3), (4, 1, 12, 20, 3), (3, 64, 16, 32, 2), (33, 10, 136, 136, 3)]
# the widest dataset (Yahoo, 700 features) at hidden_size = feature_size: the backward carries dh in its workspace, not in LDS
WIDE = (3, 3, 12, 700, 2)
ALL_SHAPES = SHAPES + [WIDE]
BAR = 1e-5

# The edge cases of tests/test_gpu_dlcm_edges.py (NOT part of SHAPES / ALL_SHAPES: other tests index those).  Each sits on a boundary of
# csrc/ultr_dlcm_plan.h, csrc/ultr_gemm.h or csrc/ultr_sr_rows.hip; tests/test_model_edges_cpu.py proves that it does.
EDGES = {
    "tile-exact": (16, 9, 12, 20, 1),          # one full workgroup of lists; heads = 1
    "tile+1": (17, 5, 12, 20, 4),              # one list in the second workgroup
    "many-lists": (260, 33, 12, 20, 5),        # T = 8580: wgrad chunk 136 (no multiple of L), 64 splits; B > 256; heads = 5
    "lds-max-resident": (3, 2, 12, 624, 2),    # the largest backward with dh in LDS
    "dh-global-first": (40, 3, 12, 640, 2),    # the first Hp with dh in the workspace, three workgroups
    "dh-global-ragged": (19, 2, 12, 636, 1),   # Hp = 640 with H off the 16 grid, two workgroups
    "bwd-max": (2, 2, 12, 848, 2),             # the largest hidden size that trains
    "saturated": (5, 7, 12, 20, 3),            # every gru.* parameter x GRU_SCALE["saturated"]
    "long": (2300, 33, 12, 24, 3),             # T = 75900: 1186 ugemm chunks, 297 column-sum chunks, wgrad chunk 1188
}
FWD_ONLY = {"fwd-only-852": (2, 2, 12, 852, 2), "fwd-only-1264": (2, 2, 12, 1264, 2)}  # the forward runs, the backward is refused
GRU_SCALE = {"saturated": 8.0}
EDGE_SEED = {"long": 333}  # a case's own seed where 300 + its index leaves e32 little room under the cap of tests/test_model_edges_cpu.py
# (long at 308: 7.3e-6)
LONG_EDGES = ("long",)
GUARDED_DIRECT = ("many-lists", "dh-global-first", "bwd-max", "long")  # the direct C-ABI call on a guarded arena
GUARDED_STEPS = ("many-lists", "dh-global-first")                       # two guarded engine steps


class Twin(nn.Module):
    def __init__(self, feature_size, hidden_size=0, num_heads=3):
        super().__init__()
        H = int(hidden_size) if int(hidden_size) > 0 else int(feature_size)
        self.H, self.heads = H, int(num_heads)
        self.layer_norm = nn.LayerNorm(feature_size, eps=1e-5)
        self.gru = nn.GRU(feature_size, H, num_layers=1, batch_first=True)
        self.att_linear = nn.Linear(H, self.heads * H)
        self.att_v = nn.Linear(self.heads, 1, bias=False)

    def forward(self, x):
        """x [B, L, F] (PAD rows are zero rows) -> scores [B, L]."""
        xh = self.layer_norm(x)
        out, _ = self.gru(torch.flip(xh, dims=[1]))     # reads the list from the last position to the first, h0 = 0
        o = torch.flip(out, dims=[1])                   # o[:, l] = the state after reading position l
        s = o[:, 0]                                     # after the top document
        M = torch.tanh(self.att_linear(s)).view(-1, self.heads, self.H)
        m = torch.einsum("j,bjh->bh", self.att_v.weight[0], M)
        return torch.einsum("blh,bh->bl", o, m)


def twin_from(state_dict, feature_size, hidden_size, num_heads, dtype=torch.float64):
    """The twin loaded BY NAME from a model's state_dict (any device), in `dtype`."""
    t = Twin(feature_size, hidden_size, num_heads)
    t.load_state_dict({k: v.detach().cpu() for k, v in state_dict.items()}, strict=True)
    return t.to(dtype)


def gather(features, docids_LB, dtype=torch.float64):
    """x [B, L, F] from the feature matrix [n_docs, F] and position-major ids [L, B] (PAD = n_docs -> the zero row)."""
    f = torch.as_tensor(features, dtype=dtype)
    ids = torch.as_tensor(np.asarray(docids_LB), dtype=torch.int64).t()
    padded = torch.cat([f, torch.zeros(1, f.shape[1], dtype=dtype)], dim=0)
    return padded[ids.clamp(max=f.shape[0])]


def make_inputs(B, L, F, seed=0):
    """features [n_docs, F] f32, docids [L, B] i32, dscores [B, L] f32: list B - 1 is all PADs, list B - 2 has PADs from the middle on."""
    g = torch.Generator().manual_seed(1000 + seed)
    ids = np.arange(B * L, dtype=np.int32).reshape(B, L)
    n_docs = B * L
    ids[B - 1, :] = n_docs
    if B >= 2:
        ids[B - 2, L // 2 + (0 if L > 1 else 1):] = n_docs
    features = (3.0 * torch.randn(n_docs, F, generator=g)).float()
    dscores = torch.randn(B, L, generator=g).float()
    return features, np.ascontiguousarray(ids.T), dscores


def reference(state_dict, F, H, heads, features, docids_LB, dscores, dtype=torch.float64):
    """scores [B, L] and {name: gradient} of sum(scores * dscores), in `dtype`."""
    t = twin_from(state_dict, F, H, heads, dtype)
    scores = t(gather(features, docids_LB, dtype))
    (scores * dscores.to(dtype)).sum().backward()
    return scores.detach(), {k: p.grad.detach() for k, p in t.named_parameters()}


def rel_err(got, ref):
    """max|got - ref| / max|ref| (the project's parity measure; an all-zero reference compares absolutely)."""
    ref = ref.double()
    scale = float(ref.abs().max())
    return float((got.detach().cpu().double() - ref).abs().max()) / (scale if scale > 0 else 1.0)


def float32_error(ref_scores, ref_grads, scores32, grads32):
    """e32 per tensor: the twin evaluated in float32 on the CPU against its float64 evaluation ({"scores": ..., name: ...})."""
    e = {"scores": rel_err(scores32, ref_scores)}
    e.update({k: rel_err(grads32[k], ref_grads[k]) for k in ref_grads})
    return e


def one_thread(fn, *args, **kw):
    """fn(*args) with torch on ONE CPU thread: a float32 sum over many rows depends on how torch splits it over threads (the long
    case's e32 moved between 1e-6 and 7e-6 with the thread count alone); one thread is the same chain whatever the host offers."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn(*args, **kw)
    finally:
        torch.set_num_threads(n)


def widened_bars(e32):
    """The project's rule for sums over many terms, per tensor: max(BAR, 4 e32) - wider than BAR only where e32 > BAR / 4 (the factor 4:
    another summation order over the same terms)."""
    return {k: max(BAR, 4.0 * e) for k, e in e32.items()}


_EDGE_CACHE = {}


def edge_case(name):
    """(model, feats, ids, dsc, ref_scores, ref_grads, e32) of EDGES[name] / FWD_ONLY[name]: parameters (LayerNorm off 1 / 0, gru.* scaled
    by GRU_SCALE), inputs, the float64 reference and the twin's per-tensor float32 error - computed once, shared by the GPU tests and
    tests/test_model_edges_cpu.py, never modified."""
    if name not in _EDGE_CACHE:
        from ultra_pytorch_amd.ranking_model import DLCM
        names = list(EDGES) + list(FWD_ONLY)
        k = names.index(name)
        B, L, F, H, heads = {**EDGES, **FWD_ONLY}[name]
        seed = EDGE_SEED.get(name, 300 + k)
        torch.manual_seed(seed)
        model = DLCM("hidden_size=%d,num_heads=%d" % (H, heads), F)
        with torch.no_grad():
            model.layer_norm.weight.add_(0.3 * torch.randn(F))
            model.layer_norm.bias.add_(0.3 * torch.randn(F))
            for key, p in model.state_dict().items():
                if key.startswith("gru."):
                    p.mul_(GRU_SCALE.get(name, 1.0))
        feats, ids, dsc = make_inputs(B, L, F, seed=seed)
        sd = model.state_dict()
        ref_scores, ref_grads = reference(sd, F, H, heads, feats, ids, dsc)
        e32 = float32_error(ref_scores, ref_grads, *one_thread(reference, sd, F, H, heads, feats, ids, dsc, dtype=torch.float32))
        _EDGE_CACHE[name] = (model, feats, ids, dsc, ref_scores, ref_grads, e32)
    return _EDGE_CACHE[name]
