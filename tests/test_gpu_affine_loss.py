"""affine_loss_kernel (csrc/ultr_affine.hip) against the float64 twin tests/trust_ref.loss_parts, per entry at the project's bar
TERMS_RTOL = 1e-5 of (|ref| + sum |terms|) (tests/loss_ref.py; excess() is tests/twotower_ref's: entries whose reference and terms lie
below float32's smallest normal number are asked to be below it themselves).

(B, L) in (1, 1), (5, 10), (3, 63), (3, 64), (3, 65), (2, 130), (37, 10); scores at unit scale and x 30; with and without docids (PAD
holes and tails, an all-PAD list); an all-unclicked list (W_b < 0), a list built so that W_b == 0; a table three entries shorter than
the list; a clipped alpha; fractional labels.  dscores and the workspace sit inside larger NaN-patterned buffers whose margins must
come back untouched; two runs agree bitwise; the longest list the layout takes, one document past it, bad arguments."""
import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests import trust_ref as T

pytestmark = pytest.mark.gpu

F0 = R.TAIL_FIXED
SHAPES = [(1, 1), (5, 10), (3, 63), (3, 64), (3, 65), (2, 130), (37, 10)]
MARGIN_WORDS = 64
PATTERN = 0x7FC0BEEF  # a quiet NaN with a payload: margins are compared as bits


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def guarded(n):
    """A float32 buffer of n words between two margins, all NaN-patterned: (whole buffer, the view of the n words)."""
    whole = torch.full((n + 2 * MARGIN_WORDS,), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole, whole[MARGIN_WORDS:MARGIN_WORDS + n]


def margins_untouched(whole, n):
    bits = whole.view(torch.int32).cpu().numpy()
    return (bits[:MARGIN_WORDS] == PATTERN).all() and (bits[MARGIN_WORDS + n:] == PATTERN).all()


def run_kernel(s, y, alpha, beta, ids=None, n_docs=0):
    """(dscores [B, L], the partial tails summed in float64 [4 + 2 L], the bits of both outputs) of one ultr_affine_loss."""
    from ultra_pytorch_amd import hip_ops
    B, L = s.shape
    tail = hip_ops.tail_floats(L)
    n_ws = hip_ops.loss_workspace_bytes(B, L) // 4
    ds_whole, ds = guarded(B * L)
    ws_whole, ws = guarded(n_ws)
    hip_ops.affine_loss(dev(s), dev(y), dev(alpha), dev(beta), B, L, ds.view(B, L), ws, docids=None if ids is None else dev(ids, torch.int32),
                        n_docs=n_docs)
    torch.cuda.synchronize()
    assert margins_untouched(ds_whole, B * L) and margins_untouched(ws_whole, n_ws)
    n_parts = hip_ops.loss_part_count(B)
    parts = ws[:n_parts * tail].view(-1, tail).cpu().numpy()
    out = ds.view(B, L).cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(parts).all()  # every word of dscores and of the partials was written
    return out, parts.astype(np.float64).sum(0), (out.view(np.uint32).copy(), parts.view(np.uint32).copy())


def hold_parts(tag, ds, tail, ref):
    e_ds = T.excess(ds, ref["ds"], ref["ds_abs"])
    e_tail = T.excess(tail[:1], ref["tail"][:1], ref["tail_abs"][:1])
    print("%s: dscores %.3e, loss sum %.3e of (|ref| + terms) (bar %.0e)" % (tag, e_ds, e_tail, R.TERMS_RTOL))
    assert e_ds <= R.TERMS_RTOL, (tag, "dscores", e_ds)
    assert e_tail <= R.TERMS_RTOL, (tag, "tail", e_tail)
    assert tail[1] == ref["tail"][1] and not tail[2:].any()  # D counts lists; nothing else in the tail


def table(n, seed=0):
    """alpha in [0.05, 0.6], beta in [0, 0.45]: the range of the shipped model, entries that differ by position."""
    rng = np.random.RandomState(1000 + n + seed)
    return rng.uniform(0.05, 0.6, size=n).astype(np.float32), rng.uniform(0.0, 0.45, size=n).astype(np.float32)


def make_case(B, L, scale, labels="binary", seed=0):
    rng = np.random.RandomState(100 * L + B + int(scale) + seed)
    s = (scale * rng.normal(size=(B, L))).astype(np.float32)
    if labels == "binary":
        y = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32)
    else:
        y = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0, -0.5], np.float32), size=(L, B))
    y[:, 0] = 0.0  # an all-unclicked list: every weight is -beta / alpha
    return s, y


@pytest.mark.parametrize("B,L", SHAPES)
def test_kernel_against_the_twin(B, L):
    alpha, beta = table(L)
    for scale in (1.0, 30.0):
        for labels in ("binary", "fractional"):
            s, y = make_case(B, L, scale, labels)
            ds, tail, bits = run_kernel(s, y, alpha, beta)
            ref = T.loss_parts(s, y, alpha, beta)
            hold_parts("B%d L%d x%g %s" % (B, L, scale, labels), ds, tail, ref)
            assert ref["W"][0] < 0 and (ref["w"][0] < 0).all()  # the all-unclicked list
            ds2, tail2, bits2 = run_kernel(s, y, alpha, beta)
            assert np.array_equal(bits[0], bits2[0]) and np.array_equal(bits[1], bits2[1])  # two runs, the same bits


def padded_ids(B, L):
    """docids [L, B]: list 0 full; the others with PAD holes and tails (ids n_docs, beyond n_docs, negative); the last all PAD (B > 1)."""
    n_docs = B * L
    ids = np.arange(B * L, dtype=np.int32).reshape(L, B)
    for b in range(1, B):
        ids[L - (b * 7) % (L + 1):, b] = n_docs
        ids[(3 * b) % L, b] = -1
        ids[(5 * b + 1) % L, b] = n_docs + 5
    if B > 1:
        ids[:, B - 1] = n_docs
    return ids, n_docs


@pytest.mark.parametrize("B,L", SHAPES)
def test_masked_padding(B, L):
    alpha, beta = table(L, seed=1)
    ids, n_docs = padded_ids(B, L)
    for scale in (1.0, 30.0):
        s, y = make_case(B, L, scale, "fractional", seed=2)
        y[:, 0] = 1.0  # (here list 0 is all clicked)
        ds, tail, _ = run_kernel(s, y, alpha, beta, ids, n_docs)
        ref = T.loss_parts(s, y, alpha, beta, ids, n_docs)
        hold_parts("masked B%d L%d x%g" % (B, L, scale), ds, tail, ref)
        live = ref["live"]
        assert (ref["w"][~live] == 0.0).all() and tail[1] == B
        if B > 1:
            assert not live[B - 1].any() and (ds[B - 1] == 0.0).all() and ref["W"][B - 1] == 0.0  # the all-PAD list: W = 0, nothing flows
        if scale == 1.0:  # a PAD keeps its place in the softmax: its dscores is softmax x W, not 0, wherever the list's W is not 0
            for b in range(B):
                if ref["W"][b] != 0.0:
                    assert (ds[b][~live[b]] != 0.0).all()
        # without docids every position counts
        ds_all, tail_all, _ = run_kernel(s, y, alpha, beta)
        hold_parts("unmasked B%d L%d x%g" % (B, L, scale), ds_all, tail_all, T.loss_parts(s, y, alpha, beta))


def test_weight_sum_of_exactly_zero():
    """alpha = 0.5, beta = 0.25 everywhere and labels 0.5 / 0 in equal number: w = +0.5 / -0.5, W_b == 0 exactly, dscores = -w."""
    for L in (2, 10, 64, 130):
        B = 3
        s, _ = make_case(B, L, 1.0)
        y = np.zeros((L, B), np.float32)
        y[::2] = 0.5
        alpha, beta = np.full(L, 0.5, np.float32), np.full(L, 0.25, np.float32)
        ds, tail, _ = run_kernel(s, y, alpha, beta)
        ref = T.loss_parts(s, y, alpha, beta)
        assert (ref["W"] == 0.0).all()
        hold_parts("W == 0, L%d" % L, ds, tail, ref)
        assert np.array_equal(ds, -ref["w"].astype(np.float32))


@pytest.mark.parametrize("B,L", [(5, 10), (3, 65), (2, 130)])
def test_short_table_and_clipped_alpha(B, L):
    """n_aff = L - 3: the last three positions read the table's last entry.  A clipped alpha: max(alpha, 0.3) on the host, as
    AffineRank's affine_clip makes it."""
    s, y = make_case(B, L, 1.0, seed=4)
    alpha, beta = table(L - 3, seed=2)
    ds, tail, _ = run_kernel(s, y, alpha, beta)
    hold_parts("n_aff %d of L %d" % (L - 3, L), ds, tail, T.loss_parts(s, y, alpha, beta))
    wide = np.concatenate([alpha, np.repeat(alpha[-1:], 3)]), np.concatenate([beta, np.repeat(beta[-1:], 3)])
    ds_w, _, _ = run_kernel(s, y, *wide)
    assert np.array_equal(ds_w, ds)
    clipped = np.maximum(alpha, np.float32(0.3))
    assert (clipped != alpha).any()
    ds_c, tail_c, _ = run_kernel(s, y, clipped, beta)
    hold_parts("clipped alpha", ds_c, tail_c, T.loss_parts(s, y, clipped, beta))
    assert not np.array_equal(ds_c, ds)


def test_longest_list_one_past_it_and_bad_arguments():
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    lo, hi = 1, 1 << 20  # the bound by asking: the largest L ultr_loss_lds_bytes accepts
    assert int(lib.ultr_loss_lds_bytes(_lib.ALGO_AFFINE, lo)) > 0 and int(lib.ultr_loss_lds_bytes(_lib.ALGO_AFFINE, hi)) == -2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if int(lib.ultr_loss_lds_bytes(_lib.ALGO_AFFINE, mid)) >= 0 else (lo, mid)
    longest = lo
    assert hip_ops.loss_route(_lib.ALGO_AFFINE, longest) == "short"
    with pytest.raises(_lib.UltrHipError):
        hip_ops.loss_route(_lib.ALGO_AFFINE, longest + 1)
    alpha, beta = table(10)
    s, y = make_case(2, longest, 1.0)
    ds, tail, _ = run_kernel(s, y, alpha, beta)
    hold_parts("L%d" % longest, ds, tail, T.loss_parts(s, y, alpha, beta))
    L = longest + 1
    z = torch.zeros(2, L, device="cuda")
    ab = dev(np.full(4, 0.5, np.float32))
    ds_whole, dsb = guarded(2 * L)
    ws_whole, ws = guarded(hip_ops.loss_workspace_bytes(2, L) // 4)
    ids = torch.zeros(L, 2, dtype=torch.int32, device="cuda")

    def call(scores=z, labels=z, alpha=ab, beta=ab, n_aff=4, docids=None, n_docs=0, B=2, L_=L - 1, out=dsb, w=ws):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return lib.ultr_affine_loss(p(scores), p(labels), p(alpha), p(beta), n_aff, p(docids), n_docs, B, L_, p(out), p(w), hip_ops.raw_stream())

    assert call(L_=L) == -2  # ULTR_E_UNSUPPORTED, on the host
    for bad in (dict(scores=None), dict(labels=None), dict(alpha=None), dict(beta=None), dict(out=None), dict(w=None), dict(B=0), dict(L_=0),
                dict(n_aff=0), dict(docids=ids, n_docs=-1)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    pat = lambda t: (t.view(torch.int32) == PATTERN).all()  # noqa: E731
    assert pat(ds_whole) and pat(ws_whole)  # outputs and workspace untouched
