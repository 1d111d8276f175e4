"""ranking_model.DLCM behind the plugin seams, driven the way main.py drives them: NavieAlgorithm (softmax) and DLA train() against the
float64 twin (tests/dlcm_ref.py) trained with the reference's arithmetic restated here - softmax_loss (base_algorithm.py:309-330), DLA's
two losses (dla.py:194-237), clip_grad_norm_ and torch.optim.Adagrad - on a seeded 12-query synthetic set; validation() against
utils.metrics on the twin's scores; validation_set() on the device feed against the per-batch loop; the checkpoint round trip; and the
refusals (DBGD, PDGD, a process group)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

from tests import dlcm_ref as R  # noqa: E402
from tests.test_gpu_eval_set import DS, per_batch_loop  # noqa: E402
from tests.test_gpu_plugins import make_feed  # noqa: E402

F, H, HEADS, L, NQ = 12, 20, 3, 8, 12
HP = "hidden_size=%d,num_heads=%d" % (H, HEADS)
TOPN = [1, 3, 5, 10]
METRICS = ["ndcg", "mrr", "err"]
LR, CLIP = 0.05, 5.0


def algo_of(cls, seed=0, metrics=METRICS):
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + cls, "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DLCM", "ranking_model_hparams": HP, "max_candidate_num": L,
           "selection_bias_cutoff": L, "metrics": list(metrics), "metrics_topn": list(TOPN)}
    torch.manual_seed(seed)
    return find_class(exp["learning_algorithm"])(DS(1, L, F, 0), exp)


def synthetic_set(seed=4):
    """12 ragged queries: features [n_docs, F], docids [L, NQ] (PAD = n_docs), labels [L, NQ] 0 .. 4, clicks [L, NQ] = label >= 3."""
    ds = DS(NQ, L, F, seed=seed)
    feats = np.asarray(ds.features[:-1], np.float32)
    n_docs = feats.shape[0]
    ids = np.asarray([[d if d >= 0 else n_docs for d in row] for row in ds.initial_list], np.int32).T
    labels = np.zeros((L, NQ), np.float32)
    for q, lab in enumerate(ds.labels):
        labels[:len(lab), q] = lab
    return ds, feats, np.ascontiguousarray(ids), labels, (labels >= 3).astype(np.float32)


def softmax_loss(output, labels, propensity_weights=None):
    """base_algorithm.py:309-330, in the dtype of its arguments."""
    if propensity_weights is None:
        propensity_weights = torch.ones_like(labels)
    weighted_labels = (labels + 0.0000001) * propensity_weights
    label_dis = torch.nan_to_num(weighted_labels / torch.sum(weighted_labels, 1, keepdim=True))
    loss = -torch.sum(label_dis * Fn.log_softmax(output, dim=-1), dim=-1) * torch.sum(weighted_labels, 1)
    return torch.sum(loss) / torch.sum(weighted_labels)


def held(got, ref, what):
    e = R.rel_err(got, ref)
    assert e <= R.BAR, (what, e)
    return e


def test_navie_softmax_three_steps_against_the_twin():
    _, feats, ids, _, clicks = synthetic_set()
    algo = algo_of("NavieAlgorithm")
    twin = R.twin_from(algo.model.state_dict(), F, H, HEADS)
    x, y = R.gather(feats, ids), torch.from_numpy(clicks.T.copy()).double()
    opt = torch.optim.Adagrad(twin.parameters(), lr=LR)  # one optimizer for the run: the accumulator persists (navie_algorithm.py:60)
    feed = make_feed(algo, feats, ids, clicks)
    worst = 0.0
    for step in range(3):
        loss, out, _ = algo.train(feed)
        ref = softmax_loss(twin(x), y)
        opt.zero_grad()
        ref.backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), CLIP)
        opt.step()
        assert out is None and abs(loss - ref.item()) <= R.BAR * abs(ref.item()), (step, loss, ref.item())
        sd = algo.model.state_dict()
        for k, p in twin.named_parameters():
            worst = max(worst, held(sd[k], p.detach(), (step, k)))
    print("NA + DLCM, three steps: largest parameter error %.3g" % worst)
    assert algo.global_step == 3


def test_dla_three_steps_against_the_twin():
    _, feats, ids, _, clicks = synthetic_set()
    algo = algo_of("DLA", seed=1)
    twin = R.twin_from(algo.model.state_dict(), F, H, HEADS)
    prop = algo.propensity_model.flat_params.detach().cpu().double().clone().requires_grad_(True)  # DenoisingNet: W [L] | b [1]
    x, y = R.gather(feats, ids), torch.from_numpy(clicks.T.copy()).double()
    feed = make_feed(algo, feats, ids, clicks)

    def weights(logits):  # dla.py:287-306 on logits_to_prob = softmax
        p = torch.softmax(logits.detach(), dim=-1)
        return p[:, :1] / p

    worst = 0.0
    for step in range(3):
        loss, _, _ = algo.train(feed)
        out = twin(x)
        propensity = Fn.elu(prop[:L] + prop[L]).unsqueeze(0).expand(NQ, L)
        rank_loss = softmax_loss(out, y, weights(propensity))
        exam_loss = softmax_loss(propensity, y, weights(out))
        ref = exam_loss + 1.0 * rank_loss
        # dla.py:141-166: fresh optimizers every step (the accumulator never persists), one clip per model
        opts = [torch.optim.Adagrad([prop], lr=LR), torch.optim.Adagrad(twin.parameters(), lr=LR)]
        for o in opts:
            o.zero_grad()
        ref.backward()
        torch.nn.utils.clip_grad_norm_([prop], CLIP)
        torch.nn.utils.clip_grad_norm_(twin.parameters(), CLIP)
        for o in opts:
            o.step()
        assert abs(loss - ref.item()) <= R.BAR * abs(ref.item()), (step, loss, ref.item())
        sd = algo.model.state_dict()
        for k, p in twin.named_parameters():
            worst = max(worst, held(sd[k], p.detach(), (step, k)))
        worst = max(worst, held(algo.propensity_model.flat_params, prop.detach(), (step, "propensity")))
    print("DLA + DLCM, three steps: largest parameter error %.3g" % worst)


def test_validation_metrics_are_utils_metrics_on_the_twins_scores(monkeypatch):
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    _, feats, ids, labels, _ = synthetic_set()
    algo = algo_of("NavieAlgorithm", seed=2)
    twin = R.twin_from(algo.model.state_dict(), F, H, HEADS)
    _, scores, summary = algo.validation(make_feed(algo, feats, ids, labels))
    ref = twin(R.gather(feats, ids)).detach()
    held(scores, ref, "scores")
    masked = torch.where(torch.from_numpy(ids.T == feats.shape[0]), torch.full((), float(algo.PADDING_SCORE), dtype=torch.float64), ref)
    lab = torch.from_numpy(labels.T.copy())
    for metric in METRICS:
        want = metrics.make_ranking_metric_fn(metric, TOPN)(lab, masked.float(), None)
        for n, v in zip(TOPN, want):
            assert abs(summary["%s_%d" % (metric, n)] - float(v)) <= 1e-6, (metric, n)
    # ["ndcg"] alone takes the NDCG launch
    algo2 = algo_of("NavieAlgorithm", seed=2, metrics=["ndcg"])
    _, scores2, summary2 = algo2.validation(make_feed(algo2, feats, ids, labels))
    assert torch.equal(scores2, scores)
    for n in TOPN:
        assert abs(summary2["ndcg_%d" % n] - summary["ndcg_%d" % n]) <= 1e-6


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
    # the device feed's batches train, too
    loss, _, _ = algo.train(dfeed.get_batch(ds, check_validation=True)[0])
    assert np.isfinite(loss)


def test_state_dict_round_trips_through_torch_save(tmp_path):
    from ultra_pytorch_amd.ranking_model import DLCM
    _, feats, ids, _, _ = synthetic_set()
    torch.manual_seed(5)
    a = DLCM(HP, F).cuda()
    path = str(tmp_path / "dlcm.ckpt")
    torch.save(a.state_dict(), path)
    torch.manual_seed(6)
    b = DLCM(HP, F).cuda()
    assert not torch.equal(a.flat_params, b.flat_params)
    b.load_state_dict(torch.load(path))
    assert list(b.state_dict()) == list(a.state_dict()) and torch.equal(a.flat_params, b.flat_params)
    x = R.gather(feats, ids).float().cuda()  # [B, L, F]
    outs = [m.build([x[:, l].contiguous() for l in range(L)]) for m in (a, b)]
    assert len(outs[0]) == L and tuple(outs[0][0].shape) == (NQ, 1)
    assert all(torch.equal(u, v) for u, v in zip(*outs))
    ref = R.twin_from(a.state_dict(), F, H, HEADS)(x.double().cpu()).detach()
    held(torch.cat(outs[0], dim=1), ref, "build")


def test_refusals():
    from ultra_pytorch_amd import engine
    for cls in ("DBGD", "PDGD"):
        with pytest.raises(NotImplementedError):
            algo_of(cls)
    shape = algo_of("NavieAlgorithm").model.shape
    with pytest.raises(NotImplementedError):
        engine.DlcmStepEngine(shape, 4, L, torch.device("cuda"), process_group=object())
