"""The workspace contract applied to the DLCM entries: every buffer of engine.DlcmStepEngine and
engine.DlcmEvalEngine re-seated on a guarded arena (tests/guarded.py: exact lengths as the library's own size queries declare them,
NaN-pattern bands in front and behind, torch.empty buffers poisoned) - two steps bit for bit against a plain engine, no band touched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import dlcm_ref as R  # noqa: E402
from tests import guarded as G  # noqa: E402

# (attribute, zeroed by the engine)
STEP_BUFFERS = [("saved", False), ("dl_ws", False), ("bwd_ws", False), ("scores", False), ("dscores", False), ("loss_ws", True),
                ("grads", True), ("scalars", True)]
EVAL_BUFFERS = [("work", False), ("scores", False), ("masked", False), ("order", False), ("ndcg", False), ("ndcg_ws", False)]
LEFT = {"_counter"}  # EvalEngine's 4-byte launch counter: zeroed once, reset by every launch, no size to declare


def guard(eng, plan):
    tensors = {n: v for n, v in vars(eng).items() if isinstance(v, torch.Tensor) and v.is_cuda}
    assert set(tensors) - LEFT == {n for n, _ in plan}, "a device tensor of the engine is neither guarded nor named in LEFT"
    arena = G.Arena(torch.device("cuda"), G.bytes_for([t.numel() * t.element_size() for t in tensors.values()]))
    for name, zero in plan:
        old = getattr(eng, name)
        assert old.is_contiguous() and old.element_size() == 4, name
        new = arena.view(old.numel(), zero=zero, name=name)
        setattr(eng, name, (new if old.dtype == torch.float32 else new.view(old.dtype)).view(old.shape))
    return arena


def bits(t):
    return t.detach().clone().view(torch.int32)


@pytest.mark.parametrize("k,algo", [(0, "softmax"), (3, "softmax"), (4, "softmax"), (0, "dla"), (2, "lambdarank")])
def test_two_guarded_steps_are_two_plain_steps(k, algo):
    two_guarded_steps_are_two_plain_steps(R.ALL_SHAPES[k], k, algo)


def two_guarded_steps_are_two_plain_steps(dims, k, algo):
    """dims = (B, L, F, H, heads); k seeds the inputs, the labels and the parameters."""
    from ultra_pytorch_amd import engine, hip_ops
    B, L, F, H, heads = dims
    d = torch.device("cuda")
    shape = hip_ops.DlcmShape(F, H, heads)
    feats, ids, _ = R.make_inputs(B, L, F, seed=k)
    g = torch.Generator().manual_seed(77 + k)
    labels = (torch.rand(L, B, generator=g) < 0.4).float().to(d)
    p0 = (0.2 * torch.randn(shape.n_params, generator=g)).to(d)
    aux0 = {"softmax": None, "dla": 0.1 * torch.randn(L + 1, generator=g), "lambdarank": torch.ones(2 * L)}[algo]
    x, docids = feats.to(d), torch.as_tensor(ids).to(d)
    runs = []
    for guarded in (False, True):
        eng = engine.DlcmStepEngine(shape, B, L, d, algo=algo)
        arena = guard(eng, STEP_BUFFERS) if guarded else None
        params, state = p0.clone(), torch.zeros_like(p0)
        aux = aux0.clone().to(d) if aux0 is not None else None
        out = []
        for step in range(2):
            eng.train_step(params, None if algo == "dla" else state, x, B * L, docids, labels, aux=aux)
            sc = eng.read_scalars()
            if arena is not None:
                arena.check()
            out += [bits(eng.scores), bits(eng.grads), bits(params), bits(state), torch.from_numpy(sc.copy()).view(torch.int32)]
            if aux is not None:
                out.append(bits(aux))
        runs.append(out)
        eng.close()
    assert len(runs[0]) == len(runs[1])
    for j, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a.cpu(), b.cpu()), "output %d of the guarded run differs from the plain run" % j
    assert bool(torch.isfinite(runs[1][2].view(torch.float32)).all())


@pytest.mark.parametrize("k", [0, 3])
def test_guarded_evaluation_is_the_plain_evaluation(k):
    from ultra_pytorch_amd import engine, hip_ops
    B, L, F, H, heads = R.ALL_SHAPES[k]
    d = torch.device("cuda")
    shape = hip_ops.DlcmShape(F, H, heads)
    feats, ids, _ = R.make_inputs(B, L, F, seed=k)
    g = torch.Generator().manual_seed(5 + k)
    labels = torch.randint(0, 5, (L, B), generator=g).float().to(d)
    params = (0.2 * torch.randn(shape.n_params, generator=g)).to(d)
    x, docids = feats.to(d), torch.as_tensor(ids).to(d)
    outs = []
    for guarded in (False, True):
        ev = engine.DlcmEvalEngine(shape, B, L, d, topn=(1, 3, 10))
        arena = guard(ev, EVAL_BUFFERS) if guarded else None
        for _ in range(2):
            scores, _ = ev.run(params, x, B * L, docids, labels)
            ndcg = ev.read_ndcg()
            if arena is not None:
                arena.check()
        outs.append((bits(scores).cpu(), ndcg.copy()))
    assert torch.equal(outs[0][0], outs[1][0]) and (outs[0][1] == outs[1][1]).all()
