"""GSF's kernels (csrc/ultr_gsf.hip) against the float64 torch twin (tests/gsf_ref.py) at the seven shapes of gsf_ref.SHAPES - ragged tiles
with widths off the 16 grid, one position with m > L, no hidden layer, lists longer than a wave, the real widths, K = m F = 1400, and
m = 8 (every slot of the kernels' unrolled loops) - each in presented order (perm = NULL) and under a seeded permutation, LayerNorm
parameters off 1 / 0.  Scores and every parameter gradient to the
project's parity bar, max|err| <= 1e-5 * max|ref| per tensor; the K = 1400 shape alone may use max(1e-5, 4 x e32), e32 = the same twin in
float32 on the CPU against float64 at that shape (the factor 4: another summation order over 1400 terms).

Measured on an MI355X (largest error over scores and gradients, perm NULL / permuted): see profiles/gsf.md."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gsf_ref as R  # noqa: E402

POISON = 12345.0
CASES = [(k, pm) for k in range(len(R.SHAPES)) for pm in (False, True)]
IDS = ["%s-%s" % (R.SHAPES[k], "perm" if pm else "identity") for k, pm in CASES]


def hp(hidden, m, extra=""):
    return "hidden_layer_sizes=[%s],group_size=%d%s" % (",".join(str(h) for h in hidden), m, extra)


@functools.lru_cache(maxsize=None)
def case(k, permuted):
    """Inputs, parameters and the float64 reference of shape k - computed once, shared by the tests, never modified."""
    from ultra_pytorch_amd.ranking_model import GSF
    B, L, F, m, hidden = R.SHAPES[k]
    torch.manual_seed(40 + k)
    model = GSF(hp(hidden, m), F)
    with torch.no_grad():  # LayerNorm off its 1 / 0 initialisation: gamma and beta matter
        for name, p in model.state_dict().items():
            if "layer_norm" in name:
                p.add_(0.3 * torch.randn(p.shape))
    feats, ids, dsc = R.make_inputs(B, L, F, seed=k)
    perm = R.numpy_perm(B, L, 70 + k) if permuted else None
    ref_scores, ref_grads = R.reference(model.state_dict(), F, hidden, m, feats, ids, dsc, perm)
    return model, feats, ids, dsc, perm, ref_scores, ref_grads


def plain_alloc(n_floats, fill, name):
    return torch.full((n_floats,), fill, device="cuda")


def run_on(model, feats, ids, dsc, perm, dims, scoring=False, alloc=plain_alloc):
    """One forward (+ backward) through the C ABI on fresh buffers from `alloc` (n_floats, fill, name), each exactly as long as the
    size queries say: scores [B, L], grads [P] (None for the scoring form)."""
    from ultra_pytorch_amd import hip_ops
    B, L = dims[0], dims[1]
    d = torch.device("cuda")
    shape = model.shape
    params, x = model.flat_params.to(d), feats.to(d)
    docids, dscores = torch.as_tensor(ids).to(d), dsc.to(d)
    pm = None if perm is None else torch.as_tensor(perm).to(d)
    scores = torch.full((B, L), POISON, device=d)
    if scoring:
        work = alloc(shape.score_bytes(B * L) // 4, float("nan"), "work")
        hip_ops.gsf_forward(shape, params, x, B * L, docids, B, L, scores, perm=pm, work=work)
        return scores, None
    saved = alloc(shape.saved_bytes(B * L) // 4, float("nan"), "saved")
    hip_ops.gsf_forward(shape, params, x, B * L, docids, B, L, scores, perm=pm, saved=saved)
    ws = alloc(shape.workspace_bytes(B, L) // 4, float("nan"), "workspace")
    grads = alloc(shape.n_params + hip_ops.tail_floats(L), POISON, "grads")
    hip_ops.gsf_backward(shape, params, x, B * L, docids, B, L, saved, dscores, None, 0, ws, grads, perm=pm)
    torch.cuda.synchronize()
    assert bool((grads[shape.n_params:] == POISON).all())  # n_loss_parts = 0: the step tail is left alone
    return scores, grads[:shape.n_params]


def run(k, permuted, scoring=False, perm_override=None):
    """run_on at shape k."""
    model, feats, ids, dsc, perm, _, _ = case(k, permuted)
    return run_on(model, feats, ids, dsc, perm if perm_override is None else perm_override, R.SHAPES[k], scoring)


def twin_float32_error(k, permuted):
    """e32: the twin evaluated in float32 on the CPU against its float64 evaluation, largest over scores and gradients."""
    model, feats, ids, dsc, perm, ref_scores, ref_grads = case(k, permuted)
    B, L, F, m, hidden = R.SHAPES[k]
    s32, g32 = R.reference(model.state_dict(), F, hidden, m, feats, ids, dsc, perm, dtype=torch.float32)
    return max([R.rel_err(s32, ref_scores)] + [R.rel_err(g32[n], ref_grads[n]) for n in ref_grads])


@pytest.mark.parametrize("k,permuted", CASES, ids=IDS)
def test_scores_and_gradients_against_the_float64_twin(k, permuted):
    model, _, _, _, _, ref_scores, ref_grads = case(k, permuted)
    scores, grads = run(k, permuted)
    errs = {"scores": R.rel_err(scores, ref_scores)}
    for name, shp, off in model.shape.layout():
        n = ref_grads[name].numel()
        errs[name] = R.rel_err(grads[off:off + n].view(*shp), ref_grads[name])
    bar = R.BAR
    if k == R.WIDE:
        e32 = twin_float32_error(k, permuted)
        bar = max(R.BAR, 4.0 * e32)
        print("GSF %s: e32 (twin float32 vs float64) %.3g, bar %.3g" % (IDS[CASES.index((k, permuted))], e32, bar))
    print("GSF %s: largest error %.3g; %s" % (IDS[CASES.index((k, permuted))], max(errs.values()),
                                              ", ".join("%s %.2g" % kv for kv in errs.items())))
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(grads).all())
    for name, e in errs.items():
        assert e <= bar, (name, e)


@pytest.mark.parametrize("k,permuted", CASES, ids=IDS)
def test_scoring_form_training_form_and_rerun_give_the_same_bits(k, permuted):
    s1, g1 = run(k, permuted)
    s2, g2 = run(k, permuted)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    s3, _ = run(k, permuted, scoring=True)
    assert torch.equal(s1.view(torch.int32), s3.view(torch.int32))


@pytest.mark.parametrize("permuted", [False, True])
def test_group_size_1_is_the_dnn(permuted):
    from ultra_pytorch_amd import hip_ops
    from ultra_pytorch_amd.ranking_model import GSF
    B, L, F, hidden = 5, 7, 12, [20, 8]
    d = torch.device("cuda")
    torch.manual_seed(8)
    model = GSF(hp(hidden, 1), F)
    feats, ids, _ = R.make_inputs(B, L, F, seed=9)
    params, x, docids = model.flat_params.to(d), feats.to(d), torch.as_tensor(ids).to(d)
    want = torch.empty(B, L, device=d)
    hip_ops.dnn_forward(hip_ops.DnnShape(F, hidden), params, x, B * L, docids, B, L, want, None)
    pm = torch.as_tensor(R.numpy_perm(B, L, 3)).to(d) if permuted else None
    got = torch.empty(B, L, device=d)
    work = torch.empty(model.shape.score_bytes(B * L) // 4, device=d)
    hip_ops.gsf_forward(model.shape, params, x, B * L, docids, B, L, got, perm=pm, work=work)
    assert R.rel_err(got, want.cpu()) <= R.BAR


@pytest.mark.parametrize("k", [0, 3])
def test_a_cyclic_rotation_of_perm_leaves_the_scores_unchanged(k):
    """The groups are the circular windows of the order: rotating the order renames the groups and changes no score."""
    perm = case(k, True)[4]
    base, _ = run(k, True, scoring=True)
    for shift in (1, 3):
        rotated, _ = run(k, True, scoring=True, perm_override=np.ascontiguousarray(np.roll(perm, shift, axis=1)))
        assert R.rel_err(rotated, base.cpu()) <= R.BAR


@pytest.mark.parametrize("B,L", [(5, 7), (3, 1), (2, 300)])
def test_shuffle_is_the_python_twin(B, L):
    from ultra_pytorch_amd import hip_ops
    seed, step = 0xFEDCBA9876543210, 7
    perm = torch.full((B, L), -1, dtype=torch.int32, device="cuda")
    hip_ops.gsf_shuffle(seed, step, B, L, perm)
    assert (perm.cpu().numpy() == R.shuffle(seed, step, B, L)).all()


def test_no_documents_at_all_scores_every_list_alike():
    """n_docs = 0: every document is a PAD and there is no feature matrix; the zero rows normalise to beta whatever the order."""
    from ultra_pytorch_amd import hip_ops
    model = case(0, False)[0]
    B, L, F, m, hidden = R.SHAPES[0]
    d = torch.device("cuda")
    ids = torch.zeros((L, B), dtype=torch.int32, device=d)
    scores = torch.empty(B, L, device=d)
    work = torch.empty(model.shape.score_bytes(B * L) // 4, device=d)
    hip_ops.gsf_forward(model.shape, model.flat_params.to(d), None, 0, ids, B, L, scores, work=work)
    ref = R.twin_from(model.state_dict(), F, hidden, m)(torch.zeros(1, L, F, dtype=torch.float64))
    assert R.rel_err(scores[0:1], ref.detach()) <= R.BAR
    assert all(torch.equal(scores[0], scores[b]) for b in range(1, B))


@pytest.mark.parametrize("F,hidden,m", [(13, [20], 2), (12, [18], 2), (12, [20], 9)])
def test_unsupported_shapes_are_refused_with_the_outputs_untouched(F, hidden, m):
    from ultra_pytorch_amd import _lib, hip_ops
    B, L = 3, 4
    d = torch.device("cuda")
    shape = hip_ops.GsfShape(F, hidden, "elu", m)
    params = torch.zeros(shape.n_params, device=d)
    x = torch.zeros(B * L, F, device=d)
    ids = torch.arange(B * L, dtype=torch.int32, device=d).view(L, B)
    scores = torch.full((B, L), POISON, device=d)
    buf = torch.full((1 << 16,), POISON, device=d)
    grads = torch.full((shape.n_params + hip_ops.tail_floats(L),), POISON, device=d)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.gsf_forward(shape, params, x, B * L, ids, B, L, scores, saved=buf)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.gsf_forward(shape, params, x, B * L, ids, B, L, scores, work=buf)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.gsf_backward(shape, params, x, B * L, ids, B, L, buf, scores, None, 0, buf, grads)
    torch.cuda.synchronize()
    assert bool((scores == POISON).all()) and bool((buf == POISON).all()) and bool((grads == POISON).all())
