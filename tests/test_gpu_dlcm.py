"""DLCM's kernels (csrc/ultr_dlcm.hip) against the float64 torch twin (tests/dlcm_ref.py) at the four shapes that reach every path of
the recurrent kernels: a ragged tile of lists with H off the 16-column grid, a single position, a long recurrence, the real width with
three tiles of lists - and the widest dataset's hidden size (700: the backward's carried dh in its workspace).  Scores and every
parameter gradient to the project's parity bar, max|err| <= 1e-5 * max|ref| per tensor; the scoring form's bits; run-to-run bits;
refusals that leave the outputs alone."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import dlcm_ref as R  # noqa: E402

POISON = 12345.0


@functools.lru_cache(maxsize=None)
def case(k):
    """Inputs, parameters and the float64 reference of shape k - computed once, shared by the tests, never modified."""
    from ultra_pytorch_amd.ranking_model import DLCM
    B, L, F, H, heads = R.ALL_SHAPES[k]
    torch.manual_seed(20 + k)
    model = DLCM("hidden_size=%d,num_heads=%d" % (H, heads), F)
    with torch.no_grad():  # LayerNorm off its 1 / 0 initialisation: gamma and beta matter
        model.layer_norm.weight.add_(0.3 * torch.randn(F))
        model.layer_norm.bias.add_(0.3 * torch.randn(F))
    feats, ids, dsc = R.make_inputs(B, L, F, seed=k)
    ref_scores, ref_grads = R.reference(model.state_dict(), F, H, heads, feats, ids, dsc)
    return model, feats, ids, dsc, ref_scores, ref_grads


def plain_alloc(n_floats, fill, name):
    return torch.full((n_floats,), fill, device="cuda")


def run_on(model, feats, ids, dsc, dims, scoring=False, backward=True, alloc=plain_alloc):
    """One forward (+ backward) through the C ABI on fresh buffers from `alloc` (n_floats, fill, name), each exactly as long as the
    size queries say: scores [B, L], grads [P] (None without a backward)."""
    from ultra_pytorch_amd import hip_ops
    B, L, F, H, heads = dims
    d = torch.device("cuda")
    shape = model.shape
    params, x = model.flat_params.to(d), feats.to(d)
    docids, dscores = torch.as_tensor(ids).to(d), dsc.to(d)
    scores = torch.full((B, L), POISON, device=d)
    if scoring:
        work = alloc(shape.score_bytes(B * L) // 4, float("nan"), "work")
        hip_ops.dlcm_forward(shape, params, x, B * L, docids, B, L, scores, work=work)
        return scores, None
    saved = alloc(shape.saved_bytes(B * L) // 4, float("nan"), "saved")
    hip_ops.dlcm_forward(shape, params, x, B * L, docids, B, L, scores, saved=saved)
    if not backward:
        return scores, None
    ws = alloc(shape.workspace_bytes(B, L) // 4, float("nan"), "workspace")
    grads = alloc(shape.n_params + hip_ops.tail_floats(L), POISON, "grads")
    hip_ops.dlcm_backward(shape, params, x, B * L, docids, B, L, saved, dscores, None, 0, ws, grads)
    torch.cuda.synchronize()
    assert bool((grads[shape.n_params:] == POISON).all())  # no loss partials given: the step tail is left alone
    return scores, grads[:shape.n_params]


def run(k, scoring=False, backward=True):
    """run_on at shape k."""
    model, feats, ids, dsc, _, _ = case(k)
    return run_on(model, feats, ids, dsc, R.ALL_SHAPES[k], scoring, backward)


@pytest.mark.parametrize("k", range(len(R.ALL_SHAPES)), ids=[str(s) for s in R.ALL_SHAPES])
def test_scores_and_gradients_against_the_float64_twin(k):
    model, _, _, _, ref_scores, ref_grads = case(k)
    scores, grads = run(k)
    errs = {"scores": R.rel_err(scores, ref_scores)}
    for name, shp, off in model.shape.layout():
        n = ref_grads[name].numel()
        errs[name] = R.rel_err(grads[off:off + n].view(*shp), ref_grads[name])
    print("DLCM %s: largest error %.3g; %s" % (R.ALL_SHAPES[k], max(errs.values()), ", ".join("%s %.2g" % kv for kv in errs.items())))
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(grads).all())
    for name, e in errs.items():
        assert e <= R.BAR, (name, e)


@pytest.mark.parametrize("k", range(len(R.ALL_SHAPES)), ids=[str(s) for s in R.ALL_SHAPES])
def test_scoring_form_and_rerun_give_the_same_bits(k):
    s1, g1 = run(k)
    s2, g2 = run(k)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    s3, _ = run(k, scoring=True)
    assert torch.equal(s1.view(torch.int32), s3.view(torch.int32))


def test_a_single_token_has_no_previous_state():
    """B = L = 1 with one real document (make_inputs would make the only list all PADs): dW_hh sums over T - 1 = 0 tokens, so the
    weight-gradient launch is not reached and the gradient is zeroed - exactly zero, everything else to the bar."""
    from ultra_pytorch_amd.ranking_model import DLCM
    dims = B, L, F, H, heads = (1, 1, 12, 20, 3)
    torch.manual_seed(77)
    model = DLCM("hidden_size=%d,num_heads=%d" % (H, heads), F)
    with torch.no_grad():
        model.layer_norm.weight.add_(0.3 * torch.randn(F))
        model.layer_norm.bias.add_(0.3 * torch.randn(F))
    feats, dsc = 3.0 * torch.randn(1, F), torch.randn(B, L)
    ids = torch.zeros(L, B, dtype=torch.int32)
    ref_scores, ref_grads = R.reference(model.state_dict(), F, H, heads, feats, ids, dsc)
    scores, grads = run_on(model, feats, ids, dsc, dims)
    assert R.rel_err(scores, ref_scores) <= R.BAR
    for name, shp, off in model.shape.layout():
        g = grads[off:off + ref_grads[name].numel()].view(*shp)
        if name == "gru.weight_hh_l0":
            assert bool((g == 0).all())
        e = R.rel_err(g, ref_grads[name])
        print("DLCM %s %s: %.3g" % (dims, name, e))
        assert e <= R.BAR, (name, e)


def test_pad_rows_come_out_as_beta_and_pad_lists_share_one_score_row():
    """A PAD is the zero row: LayerNorm gives beta whatever the position, so every all-PAD list scores like every other."""
    from ultra_pytorch_amd import hip_ops
    model = case(0)[0]
    B, L, F, H, heads = R.SHAPES[0]
    d = torch.device("cuda")
    ids = torch.full((L, B), 0, dtype=torch.int32, device=d)  # n_docs = 0: every document is a PAD, no feature matrix at all
    scores = torch.empty(B, L, device=d)
    work = torch.empty(model.shape.score_bytes(B * L) // 4, device=d)
    hip_ops.dlcm_forward(model.shape, model.flat_params.to(d), None, 0, ids, B, L, scores, work=work)
    ref = R.twin_from(model.state_dict(), F, H, heads)(torch.zeros(1, L, F, dtype=torch.float64))
    assert R.rel_err(scores[0:1], ref.detach()) <= R.BAR
    assert all(torch.equal(scores[0], scores[b]) for b in range(1, B))


@pytest.mark.parametrize("F,H", [(13, 20), (12, 18)])
def test_unsupported_shapes_are_refused_with_the_outputs_untouched(F, H):
    from ultra_pytorch_amd import _lib, hip_ops
    B, L = 3, 4
    d = torch.device("cuda")
    shape = hip_ops.DlcmShape(F, H, 3)
    params = torch.zeros(shape.n_params, device=d)
    x = torch.zeros(B * L, F, device=d)
    ids = torch.arange(B * L, dtype=torch.int32, device=d).view(L, B)
    scores = torch.full((B, L), POISON, device=d)
    buf = torch.full((1 << 16,), POISON, device=d)
    grads = torch.full((shape.n_params + hip_ops.tail_floats(L),), POISON, device=d)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.dlcm_forward(shape, params, x, B * L, ids, B, L, scores, saved=buf)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.dlcm_forward(shape, params, x, B * L, ids, B, L, scores, work=buf)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.dlcm_backward(shape, params, x, B * L, ids, B, L, buf, scores, None, 0, buf, grads)
    torch.cuda.synchronize()
    assert bool((scores == POISON).all()) and bool((buf == POISON).all()) and bool((grads == POISON).all())
