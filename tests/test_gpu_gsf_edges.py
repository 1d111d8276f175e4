"""GSF's kernels (csrc/ultr_gsf.hip) against the float64 torch twin at the settings and sizes the first suite left out - gsf_ref.EDGES;
that each case sits on the boundary it is named for is proved without a GPU in tests/test_model_edges_cpu.py:

    act-*          relu, tanh and sigmoid at the ragged shape and at the real widths: every activation id through the epilogue of the
                   first product (both tile widths, N = 20 and N = 512) and through the LayerNorm backward; with no hidden layer the
                   activation changes nothing, to the bit
    slots-5/6/7    group sizes 5, 6 and 7: the unrolled slot selects of the gathering producer, m > L at m = 6
    wide-N-walk    272 lists of 64, one hidden layer of 512: 1088 chunks of the 64 x 128 tile, more than the GPU holds at once, so the
                   slot-table producer crosses chunk boundaries; weight-gradient row chunk 272
    long           2300 lists of 33: 1186 chunks of the 64 x 64 tile for both products, 297 column-sum chunks (the 16-column fold),
                   row chunk 1188

each in presented order and under a seeded permutation (the two large cases under the permutation only).  Scores and every parameter
gradient per tensor to max(1e-5, 4 x e32) x max|ref|, e32 = the same twin in float32 on the CPU against float64 at the case's own inputs,
on one CPU thread (the K = 1400 shape's rule, per tensor; it widens a bar only where e32 > 2.5e-6: the long case's LayerNorm gradients -
sums over 75 900 rows, e32 up to 6e-6 - and, the one short case, wide-N-walk's layer_norm1.weight and layer_norm1.bias, e32 up to
3.8e-6: sums over 17 408 rows of 512 columns, which float32 on the CPU adds in one chain per column).  The scoring form, the training
form and a rerun give the same bits; the direct calls keep to buffers exactly as long as the size queries say (tests/guarded.py).

Measured on an MI355X (largest error over scores and gradients per case): see profiles/gsf.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gsf_ref as R  # noqa: E402
from tests import guarded as G  # noqa: E402
from tests.test_gpu_gsf import run_on  # noqa: E402
from tests.test_gpu_gsf_bounds import two_guarded_steps_are_two_plain_steps  # noqa: E402

IDS = ["%s-%s" % (n, "perm" if pm else "identity") for n, pm in R.EDGE_RUNS]


def run(name, permuted, activation=None, **kw):
    model, feats, ids, dsc, perm = R.edge_case(name, permuted, activation)[:5]
    return run_on(model, feats, ids, dsc, perm, R.EDGES[name], **kw)


@pytest.mark.parametrize("name,permuted", R.EDGE_RUNS, ids=IDS)
def test_scores_and_gradients_against_the_float64_twin(name, permuted):
    model, _, _, _, _, ref_scores, ref_grads, e32 = R.edge_case(name, permuted)
    tag = "%s-%s" % (name, "perm" if permuted else "identity")
    scores, grads = run(name, permuted)
    errs = {"scores": R.rel_err(scores, ref_scores)}
    for pname, shp, off in model.shape.layout():
        n = ref_grads[pname].numel()
        errs[pname] = R.rel_err(grads[off:off + n].view(*shp), ref_grads[pname])
    bars = R.widened_bars(e32)
    for t in errs:
        if bars[t] > R.BAR:
            print("GSF %s: %s e32 (twin float32 vs float64) %.3g, bar %.3g" % (tag, t, e32[t], bars[t]))
    print("GSF %s %s: largest error %.3g; %s" % (tag, R.EDGES[name], max(errs.values()), ", ".join("%s %.2g" % kv for kv in errs.items())))
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(grads).all())
    for t, e in errs.items():
        assert e <= bars[t], (t, e, bars[t])


@pytest.mark.parametrize("name,permuted", R.EDGE_RUNS, ids=IDS)
def test_scoring_form_training_form_and_rerun_give_the_same_bits(name, permuted):
    s1, g1 = run(name, permuted)
    s2, g2 = run(name, permuted)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    s3, _ = run(name, permuted, scoring=True)
    assert torch.equal(s1.view(torch.int32), s3.view(torch.int32))


@pytest.mark.parametrize("permuted", [False, True])
def test_without_a_hidden_layer_the_activation_changes_nothing(permuted):
    """The one Linear is the head: the same parameters under elu give the same scores and gradients, bit for bit."""
    name = R.NO_HIDDEN_EDGE
    a, b = R.edge_case(name, permuted)[0], R.edge_case(name, permuted, "elu")[0]
    assert a.shape.activation != "elu" and b.shape.activation == "elu" and torch.equal(a.flat_params, b.flat_params)
    s1, g1 = run(name, permuted)
    s2, g2 = run(name, permuted, "elu")
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))


@pytest.mark.parametrize("name", R.GUARDED_DIRECT)
def test_direct_calls_keep_to_the_sizes_the_queries_return(name):
    """saved, work, workspace and grads carved from a guarded arena at exactly the queried sizes: no band is written, and the results
    are the plain run's bits (a read of a word no kernel wrote would change them)."""
    from ultra_pytorch_amd import hip_ops
    model = R.edge_case(name, True)[0]
    B, L = R.EDGES[name][:2]
    sizes = [model.shape.saved_bytes(B * L), model.shape.score_bytes(B * L), model.shape.workspace_bytes(B, L),
             4 * (model.shape.n_params + hip_ops.tail_floats(L))]
    arena = G.Arena(torch.device("cuda"), G.bytes_for(sizes))

    def alloc(n_floats, fill, what):
        return arena.view(n_floats, name=what).fill_(fill)

    s1, g1 = run(name, True, alloc=alloc)
    s3, _ = run(name, True, scoring=True, alloc=alloc)
    arena.check()
    assert [v[0] for v in arena.views] == ["saved", "workspace", "grads", "work"]
    s0, g0 = run(name, True)
    assert torch.equal(s1.view(torch.int32), s0.view(torch.int32)) and torch.equal(g1.view(torch.int32), g0.view(torch.int32))
    assert torch.equal(s3.view(torch.int32), s0.view(torch.int32))


@pytest.mark.parametrize("name", R.GUARDED_STEPS)
def test_two_guarded_steps_are_two_plain_steps(name):
    B, L, F, m, hidden, act = R.EDGES[name]
    two_guarded_steps_are_two_plain_steps((B, L, F, m, hidden), act, 400 + list(R.EDGES).index(name), "softmax")
