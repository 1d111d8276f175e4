"""DLCM's kernels (csrc/ultr_dlcm.hip) against the float64 torch twin at the boundaries of their plans - dlcm_ref.EDGES and FWD_ONLY; that
each case sits on the boundary it is named for is proved without a GPU in tests/test_model_edges_cpu.py:

    tile-exact, tile+1   16 and 17 lists (a full workgroup of the recurrent kernels; one list in a second), heads = 1 and 4
    many-lists           260 lists of 33: the weight gradients' token chunk off its floor (136, no multiple of L), 64 splits, two row chunks
                         of dM's column sums, the 16-column fold of dv's 260 partials, a second trip over the heads
    lds-max-resident, dh-global-first, dh-global-ragged, bwd-max
                         H = 624, 640, 636, 848: the largest backward with dh in LDS, the first with dh in the workspace (three
                         workgroups), the same with H off the 16 grid, the largest dynamic LDS a backward asks for
    fwd-only             H = 852 and 1264: the forward runs, the backward refuses and touches nothing
    saturated            gru.* x 8: gates that round to exactly 1 in float32, candidate states at +-1
    long                 2300 lists of 33: 1186 chunks of both persistent products (more than the GPU holds at once: the gathering
                         LayerNorm producer crosses chunk boundaries), 297 column-sum chunks (the 16-column fold), token chunk 1188

Scores and every parameter gradient per tensor to max(1e-5, 4 x e32) x max|ref|, e32 = the same twin in float32 on the CPU against float64
at the case's own inputs, on one CPU thread (the project's rule for sums over many terms: the factor 4 allows another summation order; it
widens a bar only where e32 > 2.5e-6 - here the long case's layer_norm.weight and layer_norm.bias, e32 about 4e-6: sums over 75 900
tokens; no short case needs it).  The scoring form, the training form and a rerun give the same bits; the direct calls keep to buffers
exactly as long as the size queries say (tests/guarded.py).

Measured on an MI355X (largest error over scores and gradients per case): see profiles/dlcm.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import dlcm_ref as R  # noqa: E402
from tests import guarded as G  # noqa: E402
from tests.test_gpu_dlcm import POISON, run_on  # noqa: E402
from tests.test_gpu_dlcm_bounds import two_guarded_steps_are_two_plain_steps  # noqa: E402

ALL = {**R.EDGES, **R.FWD_ONLY}


def run(name, **kw):
    model, feats, ids, dsc = R.edge_case(name)[:4]
    return run_on(model, feats, ids, dsc, ALL[name], **kw)


def errors(name, scores, grads):
    model, _, _, _, ref_scores, ref_grads, _ = R.edge_case(name)
    errs = {"scores": R.rel_err(scores, ref_scores)}
    if grads is not None:
        for pname, shp, off in model.shape.layout():
            n = ref_grads[pname].numel()
            errs[pname] = R.rel_err(grads[off:off + n].view(*shp), ref_grads[pname])
    return errs


def check_against_the_twin(name, scores, grads):
    e32 = R.edge_case(name)[6]
    errs, bars = errors(name, scores, grads), R.widened_bars(e32)
    for t in errs:
        if bars[t] > R.BAR:
            print("DLCM %s: %s e32 (twin float32 vs float64) %.3g, bar %.3g" % (name, t, e32[t], bars[t]))
    print("DLCM %s %s: largest error %.3g; %s" % (name, ALL[name], max(errs.values()), ", ".join("%s %.2g" % kv for kv in errs.items())))
    assert bool(torch.isfinite(scores).all()) and (grads is None or bool(torch.isfinite(grads).all()))
    for t, e in errs.items():
        assert e <= bars[t], (t, e, bars[t])


@pytest.mark.parametrize("name", list(R.EDGES))
def test_scores_and_gradients_against_the_float64_twin(name):
    check_against_the_twin(name, *run(name))


@pytest.mark.parametrize("name", list(R.EDGES))
def test_scoring_form_training_form_and_rerun_give_the_same_bits(name):
    s1, g1 = run(name)
    s2, g2 = run(name)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    s3, _ = run(name, scoring=True)
    assert torch.equal(s1.view(torch.int32), s3.view(torch.int32))


@pytest.mark.parametrize("name", list(R.FWD_ONLY))
def test_hidden_sizes_past_the_backward_score_and_refuse_to_train(name):
    """852 <= H <= 1264: both forms of the forward against the twin (the training form still fills `saved`); the backward raises
    "unsupported shape" and leaves `grads` and `workspace` as they were."""
    from ultra_pytorch_amd import _lib, hip_ops
    model, feats, ids, dsc = R.edge_case(name)[:4]
    B, L, F, H, heads = ALL[name]
    s1, _ = run(name, backward=False)
    check_against_the_twin(name, s1, None)
    s2, _ = run(name, scoring=True)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    d = torch.device("cuda")
    shape = model.shape
    saved = torch.full((shape.saved_bytes(B * L) // 4,), float("nan"), device=d)
    scores = torch.empty(B, L, device=d)
    params, x, docids = model.flat_params.to(d), feats.to(d), torch.as_tensor(ids).to(d)
    hip_ops.dlcm_forward(shape, params, x, B * L, docids, B, L, scores, saved=saved)
    ws = torch.full((shape.workspace_bytes(B, L) // 4,), POISON, device=d)
    grads = torch.full((shape.n_params + hip_ops.tail_floats(L),), POISON, device=d)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.dlcm_backward(shape, params, x, B * L, docids, B, L, saved, dsc.to(d), None, 0, ws, grads)
    torch.cuda.synchronize()
    assert bool((ws == POISON).all()) and bool((grads == POISON).all())
    assert torch.equal(scores.view(torch.int32), s1.view(torch.int32))


@pytest.mark.parametrize("name", R.GUARDED_DIRECT)
def test_direct_calls_keep_to_the_sizes_the_queries_return(name):
    """saved, work, workspace and grads carved from a guarded arena at exactly the queried sizes: no band is written, and the results
    are the plain run's bits (a read of a word no kernel wrote would change them)."""
    from ultra_pytorch_amd import hip_ops
    model = R.edge_case(name)[0]
    B, L, F, H, heads = ALL[name]
    sizes = [model.shape.saved_bytes(B * L), model.shape.score_bytes(B * L), model.shape.workspace_bytes(B, L),
             4 * (model.shape.n_params + hip_ops.tail_floats(L))]
    arena = G.Arena(torch.device("cuda"), G.bytes_for(sizes))

    def alloc(n_floats, fill, what):
        return arena.view(n_floats, name=what).fill_(fill)

    s1, g1 = run(name, alloc=alloc)
    s3, _ = run(name, scoring=True, alloc=alloc)
    arena.check()
    assert [v[0] for v in arena.views] == ["saved", "workspace", "grads", "work"]
    s0, g0 = run(name)
    assert torch.equal(s1.view(torch.int32), s0.view(torch.int32)) and torch.equal(g1.view(torch.int32), g0.view(torch.int32))
    assert torch.equal(s3.view(torch.int32), s0.view(torch.int32))


@pytest.mark.parametrize("name", R.GUARDED_STEPS)
def test_two_guarded_steps_are_two_plain_steps(name):
    two_guarded_steps_are_two_plain_steps(R.EDGES[name], 300 + list(R.EDGES).index(name), "softmax")
