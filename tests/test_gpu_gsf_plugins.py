"""ranking_model.GSF behind the plugin seams, driven the way main.py drives them, on the seeded 12-query synthetic set the DLCM plugin
tests use: three train() steps of each of the seven algorithms; NavieAlgorithm without the shuffle against the float64 twin
(tests/gsf_ref.py) trained with the reference's arithmetic restated here - softmax_loss (base_algorithm.py:309-330), clip_grad_norm_,
torch.optim.Adagrad; the shuffle's seed; validation() against build(); validation_set() on the device feed against the per-batch loop;
the checkpoint round trip; and the refusals (the online learners, a process group)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gsf_ref as R  # noqa: E402
from tests.test_gpu_dlcm_plugins import softmax_loss, synthetic_set  # noqa: E402
from tests.test_gpu_eval_set import DS, per_batch_loop  # noqa: E402
from tests.test_gpu_plugins import make_feed  # noqa: E402

F, HIDDEN, M, L, NQ = 12, [20, 8], 2, 8, 12
HP = "hidden_layer_sizes=[20,8],group_size=2"
TOPN = [1, 3, 5, 10]
METRICS = ["ndcg", "mrr", "err"]
LR, CLIP = 0.05, 5.0
TRAINERS = ["NavieAlgorithm", "IPWrank", "DLA", "PairDebias", "LambdaRank", "RegressionEM", "PRSrank"]


def algo_of(cls, seed=0, metrics=METRICS, hp=HP):
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + cls, "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.GSF", "ranking_model_hparams": hp, "max_candidate_num": L,
           "selection_bias_cutoff": L, "metrics": list(metrics), "metrics_topn": list(TOPN)}
    torch.manual_seed(seed)
    return find_class(exp["learning_algorithm"])(DS(1, L, F, 0), exp)


def held(got, ref, what):
    e = R.rel_err(got, ref)
    assert e <= R.BAR, (what, e)
    return e


@pytest.mark.parametrize("cls", TRAINERS)
def test_three_steps_of_every_algorithm_give_finite_changing_losses(cls):
    _, feats, ids, _, clicks = synthetic_set()
    algo = algo_of(cls, seed=7)
    assert type(algo.model).__name__ == "GSF"
    feed = make_feed(algo, feats, ids, clicks)
    p0 = algo.model.flat_params.clone()
    losses = [algo.train(feed)[0] for _ in range(3)]
    assert all(np.isfinite(v) for v in losses) and len(set(losses)) == 3, losses
    assert bool(torch.isfinite(algo.model.flat_params).all()) and not torch.equal(algo.model.flat_params, p0)
    assert algo.model.shape.shuffle_step == 3  # every training forward drew its own order


# The head's LayerNorm bias and Linear bias shift every o_g[j] of a list by the same amount, hence every score of the list: the softmax
# loss does not see them and their exact gradient is zero (sum_g d o_g[j] = the list's d scores summed = 0).  Adagrad divides a gradient
# by its own magnitude, so what these entries do in a step is the sign of rounding noise times the learning rate, in float32 and in the
# float64 twin alike (there against eps = 1e-10): the parameters cannot be compared.  Their GRADIENT is held to the same bar instead,
# against the largest gradient of the model (the reference is all zeros: an absolute comparison on the model's scale).
ZERO_GRADIENT = ("sequential.layer_norm2.bias", "sequential.linear2.bias")


def test_navie_softmax_three_steps_against_the_twin_without_the_shuffle():
    """Measured on an MI355X: see profiles/gsf.md."""
    _, feats, ids, _, clicks = synthetic_set()
    algo = algo_of("NavieAlgorithm", hp=HP + ",train_shuffle=false")
    spans = {name: (off, int(np.prod(shp))) for name, shp, off in algo.model.shape.layout()}
    twin = R.twin_from(algo.model.state_dict(), F, HIDDEN, M)
    x, y = R.gather(feats, ids), torch.from_numpy(clicks.T.copy()).double()
    opt = torch.optim.Adagrad(twin.parameters(), lr=LR)  # one optimizer for the run: the accumulator persists (navie_algorithm.py:60)
    feed = make_feed(algo, feats, ids, clicks)
    worst, noise = 0.0, 0.0
    for step in range(3):
        loss, out, _ = algo.train(feed)
        ref = softmax_loss(twin(x), y)
        opt.zero_grad()
        ref.backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), CLIP)
        opt.step()
        assert out is None and abs(loss - ref.item()) <= R.BAR * abs(ref.item()), (step, loss, ref.item())
        sd = algo.model.state_dict()
        grads = next(iter(algo._train_engines.values())).grads[:algo.model.shape.n_params]
        scale = float(grads.abs().max())
        for k, p in twin.named_parameters():
            if k in ZERO_GRADIENT:
                off, n = spans[k]
                noise = max(noise, float(grads[off:off + n].abs().max()) / scale)
                assert noise <= R.BAR, (step, k, noise)
            else:
                worst = max(worst, held(sd[k], p.detach(), (step, k)))
    print("NA + GSF, three steps: largest parameter error %.3g; zero-gradient entries at %.3g of the largest gradient" % (worst, noise))
    assert algo.global_step == 3 and algo.model.shape.shuffle_step == 0


def test_the_shuffle_is_keyed_by_the_models_seed():
    _, feats, ids, _, clicks = synthetic_set()

    def three_steps(seed, shuffle_seed=None):
        algo = algo_of("NavieAlgorithm", seed=seed)
        assert algo.model.shape.shuffle_seed == seed  # torch.initial_seed() at construction ...
        if shuffle_seed is not None:
            algo.model.shape.shuffle_seed = shuffle_seed  # ... and settable
        feed = make_feed(algo, feats, ids, clicks)
        p0 = algo.model.flat_params.clone()
        for _ in range(3):
            algo.train(feed)
        return p0, algo.model.flat_params.clone()

    a0, a = three_steps(11)
    b0, b = three_steps(11)
    assert torch.equal(a0, b0) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # another shuffle seed under the same initial parameters: the draws, and with them the steps, differ
    d0, d = three_steps(11, shuffle_seed=12)
    assert torch.equal(d0, a0) and not torch.equal(d, a)
    c0, c = three_steps(13)
    assert not torch.equal(c0, a0) and not torch.equal(c, a)


def test_validation_scores_are_builds_and_the_twins(monkeypatch):
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    _, feats, ids, labels, _ = synthetic_set()
    algo = algo_of("NavieAlgorithm", seed=2)
    _, scores, summary = algo.validation(make_feed(algo, feats, ids, labels))
    x = R.gather(feats, ids).float().cuda()
    built = torch.cat(algo.model.build([x[:, l].contiguous() for l in range(L)]), dim=1)
    assert torch.equal(built.view(torch.int32), scores.view(torch.int32))
    ref = R.twin_from(algo.model.state_dict(), F, HIDDEN, M)(R.gather(feats, ids)).detach()
    held(scores, ref, "scores")
    masked = torch.where(torch.from_numpy(ids.T == feats.shape[0]), torch.full((), float(algo.PADDING_SCORE), dtype=torch.float64), ref)
    lab = torch.from_numpy(labels.T.copy())
    for metric in METRICS:
        want = metrics.make_ranking_metric_fn(metric, TOPN)(lab, masked.float(), None)
        for n, v in zip(TOPN, want):
            assert abs(summary["%s_%d" % (metric, n)] - float(v)) <= 1e-6, (metric, n)
    assert algo.model.shape.shuffle_step == 0  # evaluation never shuffles


def test_validation_set_on_the_device_feed_is_the_per_batch_loop(monkeypatch):
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    ds = synthetic_set()[0]
    algo = algo_of("NavieAlgorithm", seed=3)
    dfeed = input_layer.DeviceDirectLabelFeed(algo, 5, "")
    want, want_scores, _, sizes = per_batch_loop(algo, dfeed, ds)
    assert sizes == [5, 5, 2]
    summary, scores, pq = algo.validation_set(dfeed, ds, want_scores=True, per_query=True)
    assert set(summary) == set(want)
    for k in summary:
        assert summary[k] == want[k], (k, summary[k], want[k])
    assert torch.equal(scores.view(torch.int32), want_scores.view(torch.int32))
    assert tuple(pq.shape) == (NQ, len(METRICS), len(TOPN))
    # the device feeds' batches train, too: labelled ones and simulated clicks
    loss, _, _ = algo.train(dfeed.get_batch(ds, check_validation=True)[0])
    assert np.isfinite(loss)
    cfeed = input_layer.DeviceClickFeed(algo, 6, "", seed=3)
    for _ in range(2):
        loss, _, _ = algo.train(cfeed.get_batch(ds, check_validation=True)[0])
        assert np.isfinite(loss)


def test_state_dict_round_trips_through_torch_save(tmp_path):
    from ultra_pytorch_amd.ranking_model import GSF
    _, feats, ids, _, _ = synthetic_set()
    torch.manual_seed(5)
    a = GSF(HP, F).cuda()
    path = str(tmp_path / "gsf.ckpt")
    torch.save(a.state_dict(), path)
    torch.manual_seed(6)
    b = GSF(HP, F).cuda()
    assert not torch.equal(a.flat_params, b.flat_params)
    b.load_state_dict(torch.load(path))
    assert list(b.state_dict()) == list(a.state_dict()) and torch.equal(a.flat_params, b.flat_params)
    x = R.gather(feats, ids).float().cuda()  # [B, L, F]
    outs = [m.build([x[:, l].contiguous() for l in range(L)]) for m in (a, b)]
    assert len(outs[0]) == L and tuple(outs[0][0].shape) == (NQ, 1)
    assert all(torch.equal(u, v) for u, v in zip(*outs))
    ref = R.twin_from(a.state_dict(), F, HIDDEN, M)(x.double().cpu()).detach()
    held(torch.cat(outs[0], dim=1), ref, "build")


def test_refusals():
    from ultra_pytorch_amd import engine
    for cls in ("DBGD", "MGD", "NSGD", "PDGD"):
        with pytest.raises(NotImplementedError):
            algo_of(cls)
    shape = algo_of("NavieAlgorithm").model.shape
    with pytest.raises(NotImplementedError):
        engine.GsfStepEngine(shape, 4, L, torch.device("cuda"), process_group=object())
