"""DLCM without a GPU: the C ABI's new entries, the parameter layout against the torch twin (tests/dlcm_ref.py), the shape limits, and
how far the twin's own float32 evaluation sits from its float64 one (the room the 1e-5 parity bar of the GPU tests leaves)."""
import ctypes
import os
import re

import pytest
import torch

from tests import dlcm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ultr_dlcm_param_offsets", "ultr_dlcm_saved_bytes", "ultr_dlcm_score_bytes", "ultr_dlcm_workspace_bytes", "ultr_dlcm_forward",
           "ultr_dlcm_backward")


def test_header_table_and_library_agree_on_the_dlcm_entries():
    from ultra_pytorch_amd import _lib, build
    build.build_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ultr_hip.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(ultr_[a-z0-9_]+)\s*\(", src)) if n.startswith("ultr_dlcm_"))
    assert declared == sorted(ENTRIES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    # the argument counts of the header and the ctypes table
    for n in ENTRIES:
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[n][1]), n
    assert re.search(r"typedef struct ultr_dlcm_desc \{\s*int32_t feature_size, hidden_size, num_heads;\s*\} ultr_dlcm_desc;", src)
    assert [f for f, _ in _lib.DlcmDesc._fields_] == ["feature_size", "hidden_size", "num_heads"]
    assert _lib.load().ultr_abi_version() == _lib.ABI_VERSION == 8  # additive: the version stays


@pytest.mark.parametrize("F,H,heads,count", [(12, 20, 3, 3327), (136, 136, 3, 167963), (136, 0, 3, 167963)])
def test_layout_is_the_twins_state_dict(F, H, heads, count):
    from ultra_pytorch_amd import hip_ops
    shape = hip_ops.DlcmShape(F, H, heads)
    twin = R.Twin(F, H, heads)
    sd = twin.state_dict()
    assert [(n, tuple(s)) for n, s, _ in shape.layout()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    off = 0
    for (_, shp, o), v in zip(shape.layout(), sd.values()):
        assert o == off
        off += v.numel()
    assert shape.n_params == off == sum(p.numel() for p in twin.parameters()) == count
    assert shape.saved_bytes(70) > shape.score_bytes(70) > 0 and shape.workspace_bytes(7, 10) > 0


def test_model_state_dict_is_views_of_one_flat_vector_and_loads_into_the_twin():
    from ultra_pytorch_amd.ranking_model import DLCM
    from ultra_pytorch_amd.utils import find_class
    assert find_class("ultra_pytorch_amd.ranking_model.DLCM") is DLCM
    torch.manual_seed(3)
    m = DLCM("hidden_size=20,num_heads=3", 12)
    assert list(m.state_dict()) == list(R.Twin(12, 20, 3).state_dict())
    base = m.flat_params.data_ptr()
    for (name, shp, off), v in zip(m.shape.layout(), m.state_dict().values()):
        assert v.data_ptr() == base + 4 * off and tuple(v.shape) == tuple(shp), name
    twin = R.twin_from(m.state_dict(), 12, 20, 3)
    assert torch.equal(twin.gru.weight_hh_l0.float(), m.state_dict()["gru.weight_hh_l0"])
    # torch's default initialisation: LayerNorm 1 / 0, everything else inside its uniform bound
    assert float(m.state_dict()["layer_norm.weight"].min()) == 1.0 and float(m.state_dict()["layer_norm.bias"].abs().max()) == 0.0
    assert 0.0 < float(m.state_dict()["gru.weight_ih_l0"].abs().max()) <= 20 ** -0.5
    assert 0.0 < float(m.state_dict()["att_v.weight"].abs().max()) <= 3 ** -0.5
    m2 = DLCM("hidden_size=20", 12)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m.flat_params, m2.flat_params)
    with pytest.raises(NotImplementedError):
        m.build([torch.zeros(2, 12)], noisy_params={})
    with pytest.raises(RuntimeError):
        m.build([torch.zeros(2, 12)])  # no GPU fallback: the model sits on the CPU


@pytest.mark.parametrize("F,H", [(13, 20), (12, 18)])
def test_shapes_off_the_4_grid_are_refused_without_a_gpu(F, H):
    from ultra_pytorch_amd import _lib, hip_ops
    from ultra_pytorch_amd.ranking_model import DLCM
    shape = hip_ops.DlcmShape(F, H, 3)  # the layout is defined ...
    assert shape.n_params == sum(v.numel() for v in R.Twin(F, H, 3).state_dict().values())
    for q in (lambda: shape.saved_bytes(10), lambda: shape.score_bytes(10), lambda: shape.workspace_bytes(2, 5),
              lambda: DLCM("hidden_size=%d" % H, F)):
        with pytest.raises(_lib.UltrHipError, match="unsupported shape"):  # ... the kernels do not take it
            q()
    # the calls themselves refuse before they touch a pointer or the device (the addresses below are never read)
    lib, fake = shape.lib, ctypes.c_void_p(4096)
    assert lib.ultr_dlcm_forward(ctypes.byref(shape.desc), fake, fake, 10, fake, 2, 5, fake, fake, None, None) == -2
    assert lib.ultr_dlcm_backward(ctypes.byref(shape.desc), fake, fake, 10, fake, 2, 5, fake, fake, None, 0, fake, fake, None) == -2
    with pytest.raises(ValueError):
        hip_ops.DlcmShape(0, 4, 3)


def test_hidden_sizes_beyond_the_lds_are_refused_without_a_gpu():
    """16 lists x 3 Hp floats of gate gradients must fit 160 KiB in the backward (H <= 848), two states in the forward (H <= 1264)."""
    from ultra_pytorch_amd import hip_ops
    fake = ctypes.c_void_p(4096)
    for H, fwd, bwd in ((852, None, -2), (1268, -2, -2)):
        shape = hip_ops.DlcmShape(12, H, 2)
        assert shape.saved_bytes(6) > 0 and shape.workspace_bytes(2, 3) > 0  # sizes are defined; the calls refuse
        if fwd is not None:
            assert shape.lib.ultr_dlcm_forward(ctypes.byref(shape.desc), fake, fake, 6, fake, 2, 3, fake, fake, None, None) == fwd
        assert shape.lib.ultr_dlcm_backward(ctypes.byref(shape.desc), fake, fake, 6, fake, 2, 3, fake, fake, None, 0, fake, fake, None) == bwd
    wide = hip_ops.DlcmShape(*R.WIDE[2:])
    assert wide.workspace_bytes(3, 3) > hip_ops.DlcmShape(12, 624, 2).workspace_bytes(3, 3)  # (it holds the carried dh)


@pytest.mark.parametrize("B,L,F,H,heads", R.SHAPES)
def test_twin_float32_against_float64(B, L, F, H, heads, record_property):
    """Recorded, with a loose ceiling: stock torch in float32 stays within a few 1e-7 of float64 (relative to each tensor's largest
    magnitude) at the GPU tests' shapes and inputs, so the 1e-5 bar there has room for another summation order and no more."""
    torch.manual_seed(11)
    t32 = R.Twin(F, H, heads)
    feats, ids, dsc = R.make_inputs(B, L, F)
    s64, g64 = R.reference(t32.state_dict(), F, H, heads, feats, ids, dsc)
    s32 = t32(R.gather(feats, ids).float())
    (s32 * dsc).sum().backward()
    worst = R.rel_err(s32, s64)
    for k, p in t32.named_parameters():
        worst = max(worst, R.rel_err(p.grad, g64[k]))
    record_property("twin_fp32_vs_fp64", worst)
    print("twin float32 vs float64 at %s: %.3g" % ((B, L, F, H, heads), worst))
    assert worst < 5e-6
