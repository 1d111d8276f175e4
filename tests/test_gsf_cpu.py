"""GSF without a GPU: the float64 twin (tests/gsf_ref.py) against the DNN oracle at group_size 1 and against a brute-force loop over
groups, the shuffle law's twin, the C ABI's new entries, the parameter layout, and the shape limits."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import gsf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ultr_gsf_param_count", "ultr_gsf_param_offsets", "ultr_gsf_saved_bytes", "ultr_gsf_score_bytes", "ultr_gsf_workspace_bytes",
           "ultr_gsf_shuffle", "ultr_gsf_forward", "ultr_gsf_backward")


def test_twin_at_group_size_1_is_the_dnn_oracle():
    from oracle import ultr_oracle as O
    F, hidden, B, L = 12, [20, 8], 5, 7
    flat = torch.from_numpy(O.init_params(F, hidden, seed=3)).double()
    layout = O.param_layout(F, hidden)
    twin = R.Twin(F, hidden, 1).double()
    assert [(k, tuple(v.shape)) for k, v in twin.state_dict().items()] == [(n, tuple(s)) for n, s, _ in layout]
    twin.load_state_dict({n: flat[o:o + int(np.prod(s))].view(*s) for n, s, o in layout})
    feats, ids, _ = R.make_inputs(B, L, F)
    x = R.gather(feats, ids)
    want = O.dnn_forward(flat, F, hidden, x.reshape(B * L, F)).view(B, L)
    for perm in (None, torch.as_tensor(R.numpy_perm(B, L, 1), dtype=torch.int64)):  # (one document per group: the order cannot matter)
        assert R.rel_err(twin(x, perm), want.detach()) <= 1e-13


@pytest.mark.parametrize("L,m", [(7, 2), (1, 2), (2, 3), (5, 5)])
def test_twin_score_law_against_a_loop_over_groups(L, m):
    B, F = 3, 8
    torch.manual_seed(L * 10 + m)
    twin = R.Twin(F, [12], m).double()
    x = torch.randn(B, L, F, dtype=torch.float64)
    x[B - 1] = 0.0  # a whole-PAD list
    for perm in (None, torch.as_tensor(R.numpy_perm(B, L, 5), dtype=torch.int64)):
        got, want = twin(x, perm).detach(), R.brute_force_scores(twin, x, perm).detach()
        assert R.rel_err(got, want) <= 1e-13
        assert float(got.abs().max()) > 0.0


def test_shuffle_twin_draws_permutations_a_pure_function_of_seed_and_step():
    seed = 0x123456789ABCDEF
    a = R.shuffle(seed, 4, 6, 11)
    assert a.dtype == np.int32 and a.shape == (6, 11)
    for row in a:
        assert sorted(row.tolist()) == list(range(11))
    assert not (a == np.arange(11)).all()
    assert len({tuple(r) for r in a.tolist()}) > 1                    # lists draw differently
    assert (R.shuffle(seed, 4, 6, 11) == a).all()                      # the same (seed, step) repeats
    assert not (R.shuffle(seed, 5, 6, 11) == a).all()                  # two steps differ
    assert not (R.shuffle(seed + 1, 4, 6, 11) == a).all()
    assert (R.shuffle(seed, 4, 3, 11) == a[:3]).all()                  # a list's draw does not depend on the batch
    assert (R.shuffle(seed, 9, 4, 1) == 0).all() and sorted(R.shuffle(seed, 9, 1, 300)[0].tolist()) == list(range(300))
    # the law written out at L = 2: one step, i = 1, word 1 of block 0; the entries swap exactly when (r * 2) >> 32 == 0
    from tests import philox_ref as P
    two = R.shuffle(seed, 4, 8, 2)
    for b in range(8):
        r = int(P.philox4x32(b, 0, 0, R.SHUFFLE_TAG, *P.key(seed, 4))[1])
        assert two[b].tolist() == ([1, 0] if (r * 2) >> 32 == 0 else [0, 1])
    src = open(os.path.join(ROOT, "ultra_pytorch_amd", "csrc", "ultr_device.h")).read()
    assert int(re.search(r"#define ULTR_GSF_SHUFFLE_TAG (0x[0-9A-Fa-f]+)u", src).group(1), 16) == R.SHUFFLE_TAG


def test_header_table_and_library_agree_on_the_gsf_entries():
    from ultra_pytorch_amd import _lib, build
    build.build_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ultr_hip.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(ultr_[a-z0-9_]+)\s*\(", src)) if n.startswith("ultr_gsf_"))
    assert declared == sorted(ENTRIES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[n][1]), n
    assert re.search(r"typedef struct ultr_gsf_desc \{\s*int32_t feature_size, group_size, n_hidden;\s*int32_t hidden\[ULTR_MAX_HIDDEN\];"
                     r"\s*int32_t activation;\s*\} ultr_gsf_desc;", src)
    assert [f for f, _ in _lib.GsfDesc._fields_] == ["feature_size", "group_size", "n_hidden", "hidden", "activation"]
    assert ctypes.sizeof(_lib.GsfDesc) == 4 * (4 + _lib.ULTR_MAX_HIDDEN)
    assert _lib.load().ultr_abi_version() == _lib.ABI_VERSION == 8  # additive: the version stays


@pytest.mark.parametrize("F,hidden,m", [(12, [20, 8], 2), (16, [], 3), (136, [512, 256, 128], 2), (12, [20, 8], 1)])
def test_layout_is_the_twins_state_dict_and_the_librarys_offsets(F, hidden, m):
    from ultra_pytorch_amd import hip_ops
    shape = hip_ops.GsfShape(F, hidden, "elu", m)
    sd = R.Twin(F, hidden, m).state_dict()
    assert [(n, tuple(s)) for n, s, _ in shape.layout()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    offs = (ctypes.c_int64 * (4 * (len(hidden) + 1)))()
    assert shape.lib.ultr_gsf_param_offsets(ctypes.byref(shape.desc), offs) == 0
    off = 0
    for k, ((_, shp, o), v) in enumerate(zip(shape.layout(), sd.values())):
        assert o == off == offs[k]
        off += v.numel()
    assert shape.n_params == off == int(shape.lib.ultr_gsf_param_count(ctypes.byref(shape.desc)))
    assert shape.saved_bytes(70) > shape.score_bytes(70) > 0 and shape.workspace_bytes(7, 10) > 0
    if m == 1:  # the DNN's layout
        dnn = hip_ops.DnnShape(F, hidden)
        assert dnn.layout() == shape.layout() and dnn.n_params == shape.n_params


def test_model_state_dict_is_views_of_one_flat_vector_and_loads_into_the_twin():
    from ultra_pytorch_amd.ranking_model import GSF
    from ultra_pytorch_amd.utils import find_class
    assert find_class("ultra_pytorch_amd.ranking_model.GSF") is GSF
    torch.manual_seed(3)
    m = GSF("hidden_layer_sizes=[20,8],group_size=3", 12)
    assert m.shape.group_size == 3 and m.shape.train_shuffle and m.shape.shuffle_seed == 3 and m.shape.shuffle_step == 0
    assert list(m.state_dict()) == list(R.Twin(12, [20, 8], 3).state_dict())
    base = m.flat_params.data_ptr()
    for (name, shp, off), v in zip(m.shape.layout(), m.state_dict().values()):
        assert v.data_ptr() == base + 4 * off and tuple(v.shape) == tuple(shp), name
    twin = R.twin_from(m.state_dict(), 12, [20, 8], 3)
    assert torch.equal(twin.sequential.linear0.weight.float(), m.state_dict()["sequential.linear0.weight"])
    sd = m.state_dict()
    assert float(sd["sequential.layer_norm0.weight"].min()) == 1.0 and float(sd["sequential.layer_norm2.bias"].abs().max()) == 0.0
    assert tuple(sd["sequential.linear0.weight"].shape) == (20, 36) and tuple(sd["sequential.linear2.weight"].shape) == (3, 8)
    assert 0.0 < float(sd["sequential.linear0.weight"].abs().max()) <= 36 ** -0.5
    # the same draws as the DNN's initialisation at group_size 1
    from ultra_pytorch_amd.ranking_model import DNN
    torch.manual_seed(9)
    g1 = GSF("hidden_layer_sizes=[20,8],group_size=1", 12)
    torch.manual_seed(9)
    assert torch.equal(g1.flat_params, DNN("hidden_layer_sizes=[20,8]", 12).flat_params)
    m2 = GSF("hidden_layer_sizes=[20,8],group_size=3,train_shuffle=false", 12)
    assert not m2.shape.train_shuffle
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m.flat_params, m2.flat_params)
    with pytest.raises(NotImplementedError):
        m.build([torch.zeros(2, 12)], noisy_params={})
    with pytest.raises(RuntimeError):
        m.build([torch.zeros(2, 12)])  # no GPU fallback: the model sits on the CPU
    with pytest.raises(NotImplementedError):
        GSF("norm=batch", 12)
    with pytest.raises(TypeError):
        GSF("activation_func=selu", 12)


@pytest.mark.parametrize("F,hidden,m", [(13, [20], 2), (12, [18], 2), (12, [20], 9)])
def test_shapes_the_kernels_do_not_take_are_refused_without_a_gpu(F, hidden, m):
    from ultra_pytorch_amd import _lib, hip_ops
    from ultra_pytorch_amd.ranking_model import GSF
    shape = hip_ops.GsfShape(F, hidden, "elu", m)  # the layout is defined ...
    assert shape.n_params == sum(v.numel() for v in R.Twin(F, hidden, m).state_dict().values())
    for q in (lambda: shape.saved_bytes(10), lambda: shape.score_bytes(10), lambda: shape.workspace_bytes(2, 5),
              lambda: GSF("hidden_layer_sizes=%s,group_size=%d" % (hidden, m), F)):
        with pytest.raises(_lib.UltrHipError, match="unsupported shape"):  # ... the kernels do not take it
            q()
    # the calls themselves refuse before they touch a pointer or the device (the addresses below are never read)
    lib, fake = shape.lib, ctypes.c_void_p(4096)
    assert lib.ultr_gsf_forward(ctypes.byref(shape.desc), fake, fake, 10, fake, None, 2, 5, fake, fake, None, None) == -2
    assert lib.ultr_gsf_backward(ctypes.byref(shape.desc), fake, fake, 10, fake, None, 2, 5, fake, fake, None, 0, fake, fake, None) == -2
    with pytest.raises(ValueError):
        hip_ops.GsfShape(0, [4], "elu", 2)
    with pytest.raises(ValueError):
        hip_ops.GsfShape(12, [4], "elu", 0)
    assert lib.ultr_gsf_shuffle(1, 2, 0, 5, fake, None) == -1 and lib.ultr_gsf_shuffle(1, 2, 3, 5, None, None) == -1
