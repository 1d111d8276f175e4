"""End-to-end plumbing on the GPU (BASELINE.json configs[0]: the toy offline pipeline): the driver
(ultra_pytorch_amd.main, counterpart of the reference's main.py) trains on the toy ULTRA dataset with the plugin
classes picked by class path from a settings JSON, validates, checkpoints, reloads and writes a TREC ranklist."""
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(GOLDEN, "ultra_toy_data") + "/"


def settings(algo, train_feed, tmp_path, hparams=""):
    s = {
        "train_input_feed": "ultra_pytorch_amd.input_layer." + train_feed, "train_input_hparams": "",
        "valid_input_feed": "ultra_pytorch_amd.input_layer.DirectLabelFeed", "valid_input_hparams": "",
        "test_input_feed": "ultra_pytorch_amd.input_layer.DirectLabelFeed", "test_input_hparams": "",
        "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[32,16]",
        "learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + algo, "learning_algorithm_hparams": hparams,
        "metrics": ["err", "ndcg"], "metrics_topn": [1, 3, 5, 10], "objective_metric": "ndcg_10",
    }
    path = os.path.join(str(tmp_path), "settings.json")
    json.dump(s, open(path, "w"))
    return path


@pytest.mark.parametrize("algo,feed", [("NavieAlgorithm", "DirectLabelFeed"), ("IPWrank", "ClickSimulationFeed"),
                                       ("DLA", "ClickSimulationFeed"), ("PairDebias", "ClickSimulationFeed"),
                                       ("LambdaRank", "ClickSimulationFeed")])
def test_toy_pipeline(algo, feed, tmp_path):
    from ultra_pytorch_amd import main as driver
    random.seed(0)
    torch.manual_seed(0)
    sf = settings(algo, feed, tmp_path)
    model_dir, out_dir = str(tmp_path) + "/model/", str(tmp_path) + "/out/"
    argv = ["--data_dir", DATA, "--setting_file", sf, "--model_dir", model_dir, "--output_dir", out_dir,
            "--batch_size", "64" if algo in ("PairDebias", "LambdaRank") else "8", "--max_train_iteration", "10",
            "--steps_per_checkpoint", "10"]
    # PairDebias / LambdaRank divide the EM sums by their position-0 entry (pairwise_debias.py:160-163): with a
    # handful of lists position 0 may be in no valid pair -> 0/0 = NaN, in the reference exactly as here;
    # a realistic batch avoids it
    model, history = driver.main(argv)
    # stop test only at checkpoint boundaries: 10 < 10 is false at step 10 -> runs until step 20 (Appendix A.12)
    assert [h[0] for h in history] == [10, 20]
    assert all(np.isfinite(h[1]) for h in history)
    assert set(history[-1][2].keys()) == {"%s_%d" % (m, n) for m in ("err", "ndcg") for n in (1, 3, 5, 10)}
    assert all(0.0 <= v <= 1.0 + 1e-6 for v in history[-1][2].values())
    ckpt = os.path.join(model_dir, "ultra_pytorch_amd.learning_algorithm.%s.ckpt" % algo)
    sd = torch.load(ckpt, map_location="cpu")
    assert list(sd.keys())[:4] == ["sequential.layer_norm0.weight", "sequential.layer_norm0.bias",
                                   "sequential.linear0.weight", "sequential.linear0.bias"]
    # --test_only: reload the checkpoint, score the test set, write the run file
    summary = driver.main(argv + ["--test_only", "True"])
    assert "ndcg_10" in summary
    lines = open(os.path.join(out_dir, "test.ranklist")).read().strip().split("\n")
    assert len(lines) > 10 and lines[0].split()[1] == "Q0" and lines[0].split()[3] == "1"
    float(lines[0].split()[4])  # plain float scores


def test_training_improves_ndcg(tmp_path):
    """A few hundred NA steps on true labels must lift validation NDCG@10 well above its starting value."""
    from ultra_pytorch_amd import main as driver
    random.seed(1)
    torch.manual_seed(1)
    sf = settings("NavieAlgorithm", "DirectLabelFeed", tmp_path)
    argv = ["--data_dir", DATA, "--setting_file", sf, "--model_dir", str(tmp_path) + "/m/", "--output_dir", str(tmp_path) + "/o/",
            "--batch_size", "16", "--max_train_iteration", "150", "--steps_per_checkpoint", "50"]
    model, history = driver.main(argv)
    assert history[-1][1] < history[0][1]  # training loss falls
    assert history[-1][2]["ndcg_10"] >= history[0][2]["ndcg_10"] - 0.02


def test_driver_matches_the_reference_run(tmp_path, monkeypatch):
    """The driver pinned to the reference's own main.py: tests/golden/driver_toy.npz holds a seeded run of the
    reference driver on this toy dataset - initial weights, the loss of every step, what it printed at each checkpoint and
    every state_dict it saved.  Same seed, same settings (class paths swapped to the plugin package), the reference's
    initial weights loaded through the driver's own checkpoint path: the first step is teacher-forced (loss to 1e-5), the
    step count, the checkpoint schedule and the stop rule are exact, later steps / metrics / saved tensors agree to the
    fp32 trajectory band."""
    from ultra_pytorch_amd import main as driver
    from ultra_pytorch_amd.learning_algorithm import NavieAlgorithm
    d = np.load(os.path.join(GOLDEN, "driver_toy.npz"))
    m = json.loads(str(d["meta"]))
    s = dict(m["settings"])
    for k in ("train_input_feed", "valid_input_feed", "test_input_feed", "ranking_model", "learning_algorithm"):
        s[k] = s[k].replace("ultra.", "ultra_pytorch_amd.", 1)
    sf = os.path.join(str(tmp_path), "settings.json")
    json.dump(s, open(sf, "w"))
    model_dir = str(tmp_path) + "/model/"
    os.makedirs(model_dir)
    init = {k: torch.from_numpy(d["init_" + k].copy()) for k in m["param_keys"]}
    ckpt = os.path.join(model_dir, "%s.ckpt" % s["learning_algorithm"])
    torch.save(init, ckpt)  # create_model loads it: the run starts from the reference's initial weights
    losses, saves = [], []
    orig_train, orig_save = NavieAlgorithm.train, torch.save

    def train(self, feed):
        out = orig_train(self, feed)
        losses.append(float(out[0]))
        return out

    def save(obj, path, *a, **k):
        saves.append((len(losses), {kk: vv.detach().cpu().numpy().copy() for kk, vv in obj.items()}))
        return orig_save(obj, path, *a, **k)

    monkeypatch.setattr(NavieAlgorithm, "train", train)
    monkeypatch.setattr(torch, "save", save)
    random.seed(m["seed"])
    torch.manual_seed(m["seed"])
    np.random.seed(m["seed"])
    argv = ["--data_dir", DATA, "--setting_file", sf, "--model_dir", model_dir, "--output_dir", str(tmp_path) + "/out/"] + m["argv"]
    model, history = driver.main(argv)
    ref_losses = d["losses"]
    assert len(losses) == m["n_steps"] == len(ref_losses)                     # stop rule: only at checkpoint boundaries
    assert abs(losses[0] - ref_losses[0]) <= 1e-5 * max(1.0, abs(ref_losses[0]))  # teacher-forced first step
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-3)                # fp32 trajectory band afterwards
    assert [h[0] for h in history] == [h["global_step"] for h in m["history"]]
    assert [st for st, _ in saves] == m["save_steps"]                        # checkpoint schedule (objective_metric rule)
    for (_, loss, metrics), ref in zip(history, m["history"]):
        assert abs(loss - ref["loss"]) <= 2e-3 * max(1.0, abs(ref["loss"]))
        assert set(metrics) == set(ref["metrics"])
        for k, v in ref["metrics"].items():
            assert abs(metrics[k] - v) <= 1e-6 + (0.0 if k.startswith("ndcg") or k.startswith("mrr") else 1e-3), (k, metrics[k], v)
    # Two parameters are excluded from the saved-tensor comparison: the last LayerNorm's bias and the scorer's bias shift
    # every score of a list by the same amount, which a softmax loss cannot see - their exact gradient is 0, what both
    # implementations compute is w_k * (rounding residue of sum(dscores)), and Adagrad's first steps turn the SIGN of that
    # residue into +-lr moves (the fixture's values for them are sums of +-0.05, +-0.035, +-0.029).  They are checked
    # against that envelope instead of the reference's coin flips.
    top = max(int(k.split("layer_norm")[1].split(".")[0]) for k in m["param_keys"] if "layer_norm" in k)
    noise = {"sequential.layer_norm%d.bias" % top, "sequential.linear%d.bias" % top}
    for i, (st, sd) in enumerate(saves):
        for k in m["param_keys"]:
            if k in noise:
                lr = 0.05
                bound = lr * sum(1.0 / np.sqrt(t + 1.0) for t in range(st)) * 1.05
                assert np.all(np.abs(sd[k] - d["init_" + k]) <= bound), k
                continue
            np.testing.assert_allclose(sd[k], d["save%d_%s" % (i, k)], rtol=5e-3, atol=5e-4, err_msg=k)


def test_bench_plain_run_prints_only_the_headline():
    """A plain `python bench.py --gpus 1 --steps N --warmup W` times the N steps and prints the headline line without measuring any
    secondary figure: those (baselines, other precisions and configs, the eval leg, the plugin API) are `--full`'s."""
    import json
    import subprocess
    import sys
    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == "queries/sec (training step)" and d["unit"] == "queries/sec" and d["higher_is_better"] is True
    assert d["steps"] == 20 and d["warmup"] == 5 and d["n_gpus"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 256 / (1e-3 * d["ms_per_step"])) <= 1e-6 * d["value"] and np.isfinite(d["final_loss"])
    assert d["dtype"].startswith("f32") and d["roofline"]["launches_timed"] >= 1
    for key in ("cpu_baseline", "torch_rocm_baseline", "queries_per_sec_no_host_sync", "fp32_mfma_products", "other_configs", "eval",
                "plugin_queries_per_sec", "end_to_end_queries_per_sec_device_feed"):
        assert key not in d, key


def test_bench_multi_rank_logic_on_one_gpu():
    """`python bench.py --gpus 2 --full` launches its own ranks and prints ONE JSON line carrying both gradient exchanges and the
    checks - exercised here with both ranks on cuda:0 over gloo (ULTR_BENCH_SHARE_GPU=1: a test of bench.py's N > 1 logic, the
    same code the driver's scaling run takes; not a measurement)."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, ULTR_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "40", "--warmup", "5", "--full",
                        "--no-cpu-baseline", "--no-extras"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 512 and d["steps"] == 40
    assert len(d["dp_exchanges"]) == 2 and all("ms_per_step" in v for v in d["dp_exchanges"].values())
    assert d["dp_checks"]["replicas_bit_identical_after_run"] and d["dp_checks"]["peer_exchange_matches_rccl_allreduce"]
    assert d["rccl_ranks"] == 2 and d["value"] > 0
    # the in-run single-GPU figure and what the driver's scaling run is read against (two ranks SHARE one GPU here: no bar on the value)
    assert d["single_gpu_in_run"]["ms_per_step"] > 0 and 0.0 < d["weak_scaling_efficiency"] < 1.5 and "exchange_exposed_us" in d
    # round 6: the exchange self-test under skew (1 000 steps, every rank delayed by its own 0 - 50 us per step) ran in front of the
    # timed region and its verdict, with the exchange's name and the scaling figures, sits in the HEAD of the line
    st = d["dp_selftest"]
    assert st["passed"] and st["replicas_bit_identical"] and st["status_words_zero"] and st["steps"] == 1000 and st["error"] is None
    head = lines[0][:1500]
    for key in ("dp_exchange", "rccl_ranks", "weak_scaling_efficiency", "exchange_exposed_us", "dp_selftest"):
        assert '"%s"' % key in head, key
