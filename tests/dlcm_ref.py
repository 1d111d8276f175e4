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


def gather(features, docids_LB):
    """x [B, L, F] float64 from the feature matrix [n_docs, F] and position-major ids [L, B] (PAD = n_docs -> the zero row)."""
    f = torch.as_tensor(features, dtype=torch.float64)
    ids = torch.as_tensor(np.asarray(docids_LB), dtype=torch.int64).t()
    padded = torch.cat([f, torch.zeros(1, f.shape[1], dtype=torch.float64)], dim=0)
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


def reference(state_dict, F, H, heads, features, docids_LB, dscores):
    """float64 scores [B, L] and {name: gradient} of sum(scores * dscores)."""
    t = twin_from(state_dict, F, H, heads)
    scores = t(gather(features, docids_LB))
    (scores * dscores.double()).sum().backward()
    return scores.detach(), {k: p.grad.detach() for k, p in t.named_parameters()}


def rel_err(got, ref):
    """max|got - ref| / max|ref| (the project's parity measure; an all-zero reference compares absolutely)."""
    ref = ref.double()
    scale = float(ref.abs().max())
    return float((got.detach().cpu().double() - ref).abs().max()) / (scale if scale > 0 else 1.0)
