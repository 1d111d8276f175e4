"""The SetRank sweep on the GPU (tests/setrank_sweep_cases.py): every case runs one NA and one IPW step through SetRankStepEngine -
forward, loss, backward, update - and is held to the float64 restatement of the step (tests/setrank_dropout_ref.train_step at rate 0)
at the golden bars: scores 1e-5, loss 1e-5 max(1, |loss|), gradients rtol 1e-5 + 2e-6 max(1, max|g|) over the whole vector, and per
parameter tensor max|diff| <= 2e-5 max|tensor| + 1e-6 max|g|.  ultr_setrank_score gives the training forward's scores bit for bit on
every case's route; the knob and mixed-launch cases give the same gradient bits twice; and a last test asserts, from what the route
query (ultr_setrank_route) answered for the cases that ran, that every route flag and every geometry the table is there for was taken.

The reference-alone condition - the torch-fp32 oracle within half of every bar against float64 on every case - is
tests/test_setrank_sweep_cpu.py's; under it a miss here means the kernel.

WHAT THE SWEEP FOUND.  Seven cases first missed ONE bar, the per-tensor bar of the scorer's bias gradient (output_layer.2.bias), at
1.06 .. 2.52 of it - depth nl3 and nl5 at (4,20,24,64,2,.,32), wg_split (64,16,..) and (96,16,..), partials (13,5,13,24,3,1,10),
knobs ULTR_SR_BWD_FUSED=1 and ULTR_SR_BLOCK=2 - with every other figure far inside.  That gradient is the sum of all d scores, and every
list's d scores sum to zero in real arithmetic, so its bar is 1e-6 of the largest gradient entry flat.  The d scores come from the
list-loss launch SetRank shares with the DNN (softmax_ce_kernel, csrc/ultr_loss.hip), which formed d = exp(s - lse) S - w with the
list's weight sum S added up in fp32: a list's d scores then kept S_fp32 - sum(w), about 6e-8 S, whatever SetRank's kernels did with
them (restated in numpy float32 and summed exactly, that formula is over the bar in 21 of 98 steps; with S rounded once, 0 of 98).
The launch now sums S in double and rounds it once, takes p as e / sum(e) and fuses the product (softmax_ce_dscore, ultr_device.h);
ultr_dnn_backward_softmax's prologues, which tests/test_gpu_parity.py holds to the same d score bits, changed with it.  Since then
every case is inside every golden bar: the scorer's bias gradient at most 0.55 of its bar, 0.98 at the 511-list case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import margins  # noqa: E402
from tests import setrank_sweep_cases as C  # noqa: E402
from tests.hipref import dev  # noqa: E402

SEEN = {}  # case id -> dict(route=..., attn=(forward family, backward family)) of the cases that ran


def features_on_device(case, feats):
    """The feature matrix on the device; features_offset_bytes = 4: a view one float into a larger buffer (a caller's slice)."""
    n, F = feats.shape
    if case.features_offset_bytes == 0:
        f = dev(feats)
        assert f.data_ptr() % 16 == 0
        return f
    assert case.features_offset_bytes == 4
    buf = torch.full((n * F + 8,), float("nan"), dtype=torch.float32, device="cuda")
    f = buf[1:1 + n * F].view(n, F)
    f.copy_(torch.from_numpy(np.ascontiguousarray(feats)))
    assert f.is_contiguous() and f.data_ptr() % 16 == 4
    return f


def run_step(case, shape, algo):
    """One step as tests/test_gpu_setrank.run_step runs it: (scores [B, L], gradient / D over the parameters, loss), and the scores of
    ultr_setrank_score on the same inputs."""
    from ultra_pytorch_amd import engine, hip_ops
    inp = C.inputs(case.id)
    B, L = case.B, case.L
    eng = engine.SetRankStepEngine(shape, B, L, torch.device("cuda"), algo="softmax", learning_rate=0.05, max_gradient_norm=5.0)
    p, s = dev(inp.params.copy()), dev(np.zeros_like(inp.params))
    f = features_on_device(case, inp.features)
    i, y = dev(inp.docids.copy(), torch.int32), dev(C.labels_for(case.id, algo).copy(), torch.float32)
    eng.forward(p, f, f.shape[0], i, train=True)
    torch.cuda.synchronize()
    scores = eng.scores.cpu().numpy().copy()
    eng.loss(y, ipw_table=dev(inp.ipw.copy()) if algo == "ipw" else None)
    eng.backward(p, f, f.shape[0], i)
    torch.cuda.synchronize()
    g = eng.grads.cpu().numpy().copy()
    eng.update(p, s)
    torch.cuda.synchronize()
    sc = eng.scalars.cpu().numpy()
    work = torch.full((shape.score_bytes(B * L) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    evaluated = torch.full((B, L), float("nan"), device="cuda")
    hip_ops.setrank_score(shape, dev(inp.params.copy()), f, f.shape[0], i, B, L, evaluated, work)  # (p: updated by now)
    torch.cuda.synchronize()
    eng.close()
    return scores, g[: shape.n_params] / float(sc[3]), float(sc[0]), g, evaluated.cpu().numpy()


@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_step_against_float64(case, monkeypatch):
    from ultra_pytorch_amd import _lib, hip_ops
    shape = C.make_shape(case)
    failures = []
    try:
        C.set_knobs(monkeypatch, case)
        route = shape.route(case.B, case.L)
        attn = (hip_ops.setrank_attn_path(shape, case.L), hip_ops.setrank_attn_path(shape, case.L, backward=True))
        print("%s: route %s attention %s" % (case.id, route, attn))
        for algo in C.ALGOS:
            scores, g, loss, raw, evaluated = run_step(case, shape, algo)
            f = C.figures(case, C.reference(case.id, algo), scores, loss, g)
            print("%s %s: measured / bar  scores %.3f  loss %.3f  grads %.3f  tensor %.3f (%s)"
                  % (case.id, algo, f["scores"], f["loss"], f["grads"], f["tensor"], f["worst_tensor"]))
            failures += ["%s: %s" % (algo, m) for m in C.misses(case.id, algo, f)]
            if not np.array_equal(evaluated, scores):
                failures.append("%s: ultr_setrank_score differs from the training forward by up to %.3g"
                                % (algo, float(np.abs(evaluated - scores).max())))
            for name in C.tensor_bars(case.id, algo):  # a widened bar: the figure is recorded and held to 2 x the committed one
                margins.check("setrank_sweep/%s" % case.id, "%s_%s_over_golden_bar" % (algo, name.split(".", 1)[1]), f["tensors"][name])
            if case.tag in C.DETERMINISM_TAGS:
                again = run_step(case, shape, algo)
                if not (np.array_equal(again[3], raw) and np.array_equal(again[0], scores)):
                    failures.append("%s: a second run from the same state gave other bits" % algo)
        SEEN[case.id] = dict(route=route, attn=attn)
    finally:
        monkeypatch.undo()
        _lib.load().ultr_config_reload()
    assert not failures, (case.id, failures)


def test_the_sweep_reached_every_route_and_geometry():
    """(runs after the cases above: pytest keeps file order)  What the route query answered for the cases that ran, by value."""
    assert set(SEEN) == {c.id for c in C.CASES}, sorted({c.id for c in C.CASES} - set(SEEN))
    R = {cid: v["route"] for cid, v in SEEN.items()}

    def some(pred, what):
        hit = [cid for cid, r in R.items() if pred(r)]
        assert hit, "no case with %s" % what
        return hit

    for b in (0, 1, 2):
        some(lambda r: r["block"] == b, "block = %d" % b)
    some(lambda r: r["block"] != 0 and r["embed"] == 1, "a block kernel behind the fused embedding launch")
    some(lambda r: r["block"] != 0 and r["embed"] == 0, "a block kernel behind the separate embedding launches")
    some(lambda r: r["bwd_embed"] == 0 and r["bwd_blocks"] == 1, "bwd_embed = 0 with bwd_blocks = 1")
    some(lambda r: r["skip_out1"] == 1, "skip_out1 = 1")
    some(lambda r: r["skip_out1"] == 0 and r["block"] != 0, "a block kernel that writes out1")
    some(lambda r: r["bwd_head"] == 1 and r["bwd_blocks"] == 0, "bwd_head without bwd_blocks")
    some(lambda r: r["bwd_blocks"] == 1 and r["bwd_head"] == 0, "bwd_blocks without bwd_head")
    some(lambda r: r["block"] == 0 and r["bwd_blocks"] == 1, "separate forward launches before the fused backward")
    for n in (1, 2, 3):
        some(lambda r: r["wgrad_split"] == n, "wgrad_split = %d" % n)
    families = {v["attn"][0] for v in SEEN.values()} | {v["attn"][1] for v in SEEN.values()}
    assert {"scalar", "mfma", "split_half"} <= families, families
    # every route flag above holds on any device; the geometry the shapes were chosen for needs the 256 compute units of an MI355X
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    geometry = {cid: tuple(r[k] for k in ("rows_per_tile", "tiles", "workgroups", "block_rows", "embed_rows")) for cid, r in R.items()
                if r["block"] != 0}
    if cus != 256:
        print("geometry by case on %d compute units: %s" % (cus, geometry))
        pytest.skip("the device reports %d compute units, the geometry cases are chosen for 256" % cus)
    persistent = lambda r: r["block"] == 2  # noqa: E731
    some(lambda r: persistent(r) and r["rows_per_tile"] == 4, "persistent tiles of 4 rows")
    some(lambda r: persistent(r) and r["rows_per_tile"] == 64, "persistent tiles of 64 rows")
    # fewer tiles than the device has workgroup slots: the launch shrinks to one workgroup per tile
    some(lambda r: persistent(r) and r["tiles"] == r["workgroups"] < cus, "fewer persistent tiles than compute units")
    # more tiles than workgroups: a second round.  (tiles <= rounds x compute units, and below 17 000 rows on 256 compute units the
    # kernels never take a third round: tiles > 2 x workgroups cannot occur in this sweep.)
    some(lambda r: persistent(r) and r["workgroups"] == cus and r["tiles"] > r["workgroups"] and r["rows_per_tile"] < 64,
         "a persistent launch in its second round")
    ragged = R["persistent_geometry-T4097_ragged_last_tile"]
    assert persistent(ragged) and 4097 % ragged["rows_per_tile"] != 0 and ragged["tiles"] * ragged["rows_per_tile"] > 4097, ragged
    round5 = lambda r: r["block"] == 1  # noqa: E731
    some(lambda r: round5(r) and r["block_rows"] == 16, "round-5 workgroups of 16 rows")
    some(lambda r: round5(r) and r["block_rows"] == 32, "round-5 workgroups of 32 rows")
    # the LDS-bound cap of the round-5 kernel at d 256 / dff 128: the most rows the query ever answers for those widths
    cap_case = C.BY_ID["round5_lds_cap-T13312_at_the_cap"]
    cap_shape = C.make_shape(cap_case)
    cap = max(cap_shape.route(B, 16)["block_rows"] for B in range(32, 4097, 32))
    assert 16 < cap < 32, cap
    assert R[cap_case.id]["block"] == 1 and R[cap_case.id]["block_rows"] == cap, (R[cap_case.id], cap)
    assert R["round5_lds_cap-T13328_second_round"]["block_rows"] < cap
    print("routes reached:", {cid: R[cid] for cid in sorted(R)})
