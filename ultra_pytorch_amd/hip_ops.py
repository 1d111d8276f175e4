"""Tensor-level wrappers over the C ABI: torch supplies device memory and the stream, nothing else.

Every function takes CUDA(ROCm) float32 / int32 tensors, passes raw pointers + the current
HIP stream to libultr_hip.so and returns immediately (asynchronous w.r.t. the host).
"""
import ctypes
import os
import warnings
import weakref

import torch

from . import _lib
from ._lib import check


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_stream():
    """The current HIP stream's handle as an int: torch's own C getter (what torch.cuda.current_stream().cuda_stream resolves to,
    without building a Stream object and normalising the device argument: ~3 us -> ~0.3 us per call)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _stream():
    return ctypes.c_void_p(raw_stream())


def _req(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise TypeError("%s must be a contiguous %s tensor on the GPU" % (name, dtype))
    return t


class DnnShape:
    """Host-side geometry of one DNN (desc + parameter layout), mirrors DNN.__init__ (DNN.py:25-55)."""

    def __init__(self, feature_size, hidden, activation="elu"):
        self.lib = _lib.load()
        self.feature_size = int(feature_size)
        self.hidden = [int(h) for h in (hidden or [])]
        self.activation = activation
        self.desc = _lib.make_desc(feature_size, self.hidden, activation)
        self.n_params = int(self.lib.ultr_dnn_param_count(ctypes.byref(self.desc)))
        if self.n_params <= 0:
            raise ValueError("bad DNN description")
        nl = len(self.hidden) + 1
        offs = (ctypes.c_int64 * (4 * nl))()
        check(self.lib.ultr_dnn_param_offsets(ctypes.byref(self.desc), offs), "ultr_dnn_param_offsets")
        self.offsets = list(offs)
        dims, k = [], self.feature_size
        for m in self.hidden + [1]:
            dims.append((k, m))
            k = m
        self.dims = dims

    def layout(self):
        """[(state_dict key, shape, offset)] in the reference's parameter order."""
        out = []
        for j, (k, m) in enumerate(self.dims):
            o = self.offsets[4 * j:4 * j + 4]
            out += [("sequential.layer_norm%d.weight" % j, (k,), o[0]), ("sequential.layer_norm%d.bias" % j, (k,), o[1]),
                    ("sequential.linear%d.weight" % j, (m, k), o[2]), ("sequential.linear%d.bias" % j, (m,), o[3])]
        return out

    def saved_bytes(self, n_rows):
        return int(self.lib.ultr_dnn_saved_bytes(ctypes.byref(self.desc), n_rows))

    def bwd_workspace_bytes(self, n_rows):
        return int(self.lib.ultr_dnn_bwd_workspace_bytes(ctypes.byref(self.desc), n_rows))

    def route(self, B, L, n_docs=None, call="step_softmax", operands=None):
        """The kernels one call takes at B lists of L documents gathered from n_docs (default B x L) documents (ultr_dnn_route: the
        route the entry points themselves decide, under the knobs as the library last read them; host-only, launches nothing) as a
        dict of the fields of ultr_dnn_route_info.  `call`: one of _lib.DNN_CALLS.  `operands`: None = what the engines pass (16-byte
        aligned pointers, the weight copies, a dscores buffer), else the names of _lib.DNN_OPERANDS that hold for the call (an
        iterable, or the ULTR_DNN_OP_ bits as an int: ultr_dnn_route_operands).  A call the library would refuse raises UltrHipError
        ("unsupported shape")."""
        info = _lib.DnnRouteInfo()
        if operands is None:
            bits = _lib.DNN_OP_ALL
        elif isinstance(operands, int):
            bits = operands
        else:
            bits = 0
            for name in operands:
                bits |= _lib.DNN_OPERANDS[name]
        check(self.lib.ultr_dnn_route_operands(ctypes.byref(self.desc), int(B), int(L), int(B) * int(L) if n_docs is None else int(n_docs),
                                               _lib.DNN_CALLS.index(call), bits, ctypes.byref(info)), "ultr_dnn_route_operands")
        return {name: int(getattr(info, name)) for name, _ in _lib.DnnRouteInfo._fields_ if name != "reserved"}


class SetRankShape:
    """Host-side geometry of one SetRank model: descriptor + flat parameter layout in the reference's
    state_dict order (SetRank.py:95-103, 130-141).

    `rate` is the dropout rate of TRAINING forwards (SetRank.py:103-117, 141-153).  It lives beside the descriptor, not in it: the
    parameter layout, the buffer sizes and every evaluation are those of the rate-0 model.  The dropout key rides along:
    `dropout_seed` (the owner of the shape sets it; ranking_model.SetRank captures torch.initial_seed()) and `dropout_step`, the count
    of training forwards so far - engines are cached and evicted, so the counter is the model's, shared through this object.

    `attention_backward`: "one_pass" (default) trains lists up to 128 documents on the matrix-core attention kernels (head depth
    16 / 32 / 64) and up to 120 elsewhere; "streaming" sets ULTR_MODEL_SR_STREAM_BWD in the descriptor: beyond those bounds the backward
    AND the forward run the streaming kernels (csrc/ultr_sr_attn_long.hip), so the model trains at any list size.  Below the hand-over
    point nothing changes; at 129 .. 256 documents a streaming model's scores come from the streaming forward instead of the one-pass
    scalar kernel (same values to the 1e-5 bar, other bits)."""

    ATTENTION_BACKWARD = ("one_pass", "streaming")

    def __init__(self, feature_size, d_model=256, num_heads=8, num_layers=2, dff=64, attention_dtype="fp32", rate=0.0,
                 attention_backward="one_pass"):
        rate = float(rate)
        if not 0.0 <= rate < 1.0:
            raise ValueError("rate must be in [0, 1) (got %r)" % rate)
        self.rate, self.dropout_seed, self.dropout_step = rate, 0, 0
        self.lib = _lib.load()
        self.feature_size, self.d_model, self.num_heads = int(feature_size), int(d_model), int(num_heads)
        self.num_layers, self.dff = int(num_layers), int(dff)
        if attention_dtype not in _lib.ATTN_DTYPE:
            raise ValueError("attention_dtype must be one of %s (got %r)" % (sorted(_lib.ATTN_DTYPE), attention_dtype))
        self.attention_dtype = attention_dtype
        if attention_backward not in self.ATTENTION_BACKWARD:
            raise ValueError("attention_backward must be one of %s (got %r)" % (list(self.ATTENTION_BACKWARD), attention_backward))
        self.attention_backward = attention_backward
        self.desc = _lib.SetRankDesc(self.feature_size, self.d_model, self.num_heads, self.num_layers, self.dff,
                                     _lib.ATTN_DTYPE[attention_dtype])
        if attention_backward == "streaming":
            self.desc.flags = int(self.desc.flags) | _lib.MODEL_SR_STREAM_BWD
        self.n_params = int(self.lib.ultr_setrank_param_count(ctypes.byref(self.desc)))
        if self.n_params <= 0:
            raise ValueError("bad SetRank description (d_model must be a multiple of num_heads, 1..8 layers)")

    def layout(self):
        F, d, dff = self.feature_size, self.d_model, self.dff
        out, off = [], 0

        def add(name, shape):
            nonlocal off
            out.append((name, tuple(shape), off))
            n = 1
            for v in shape:
                n *= v
            off += n

        e = "Encoder_layer."
        add(e + "input_layer_norm.weight", (F,)); add(e + "input_layer_norm.bias", (F,))
        add(e + "input_embedding.0.weight", (dff, F)); add(e + "input_embedding.0.bias", (dff,))
        add(e + "input_embedding.2.weight", (d, dff)); add(e + "input_embedding.2.bias", (d,))
        add(e + "output_layer.0.weight", (dff, d)); add(e + "output_layer.0.bias", (dff,))
        add(e + "output_layer.2.weight", (1, dff)); add(e + "output_layer.2.bias", (1,))
        for i in range(self.num_layers):
            l = e + "enc_layers.encoder%d." % i
            add(l + "mha.dense.weight", (d, d)); add(l + "mha.dense.bias", (d,))
            add(l + "ffn.0.weight", (dff, d)); add(l + "ffn.0.bias", (dff,))
            add(l + "ffn.2.weight", (d, dff)); add(l + "ffn.2.bias", (d,))
            add(l + "layernorm1.weight", (d,)); add(l + "layernorm1.bias", (d,))
            add(l + "layernorm2.weight", (d,)); add(l + "layernorm2.bias", (d,))
        assert off == self.n_params
        return out

    def saved_bytes(self, n_rows):
        return int(self.lib.ultr_setrank_saved_bytes(ctypes.byref(self.desc), n_rows))

    def workspace_bytes(self, n_rows):
        return int(self.lib.ultr_setrank_workspace_bytes(ctypes.byref(self.desc), n_rows))

    def dropout_workspace_bytes(self, n_rows):
        """The backward's extra buffer of a dropout step (ultr_setrank_dropout::scratch)."""
        return int(self.lib.ultr_setrank_dropout_workspace_bytes(ctypes.byref(self.desc), n_rows))

    def next_dropout_step(self):
        """The step number of the training forward about to run; counts it."""
        step = self.dropout_step
        self.dropout_step = step + 1
        return step

    def range_flag_offset(self, n_rows):
        """Float offset in `saved` of the range word of the split-half planes (ultr_update_desc::range_flag)."""
        return int(self.lib.ultr_setrank_range_flag_offset(ctypes.byref(self.desc), n_rows))

    def score_bytes(self, n_rows):
        """Bytes of setrank_score's buffer: the live activations (their size does not grow with num_layers), the planes, the range word."""
        return int(self.lib.ultr_setrank_score_bytes(ctypes.byref(self.desc), n_rows))

    def route(self, B, L, dropout=False):
        """The launches one step takes at B lists of L documents (ultr_setrank_route: the library's own plan and route under the knobs
        as it last read them; host-only, launches nothing) as a dict of the fields of ultr_setrank_route_info."""
        info = _lib.SetRankRouteInfo()
        check(self.lib.ultr_setrank_route(ctypes.byref(self.desc), int(B), int(L), 1 if dropout else 0, ctypes.byref(info)),
              "ultr_setrank_route")
        return {name: int(getattr(info, name)) for name, _ in _lib.SetRankRouteInfo._fields_ if name != "reserved"}

    def score_range_flag_offset(self, n_rows):
        """Float offset in setrank_score's buffer of the range word of the split-half planes."""
        return int(self.lib.ultr_setrank_score_range_flag_offset(ctypes.byref(self.desc), n_rows))


def setrank_dropout(rate, seed, step, stream=0, scratch=None):
    """ultr_setrank_dropout for one step: the forward reads (rate, seed, step, stream), the backward of the same step the scratch too."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError("rate must be in [0, 1) (got %r)" % rate)
    d = _lib.SetRankDropout()
    d.rate, d.seed, d.step, d.stream = rate, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(stream)
    d.scratch = scratch.data_ptr() if scratch is not None else None
    d.scratch_bytes = scratch.numel() * scratch.element_size() if scratch is not None else 0
    return d


def setrank_forward(shape, params, features, n_docs, docids, B, L, scores, saved, dropout=None):
    if dropout is not None:
        check(shape.lib.ultr_setrank_forward_dropout(ctypes.byref(shape.desc), _p(params), _p(features), int(n_docs), _p(docids), int(B),
                                                     int(L), _p(scores), _p(saved), ctypes.byref(dropout), _stream()),
              "ultr_setrank_forward_dropout")
        return
    check(shape.lib.ultr_setrank_forward(ctypes.byref(shape.desc), _p(params), _p(features), int(n_docs), _p(docids), int(B),
                                         int(L), _p(scores), _p(saved), _stream()), "ultr_setrank_forward")


def setrank_score(shape, params, features, n_docs, docids, B, L, scores, work):
    """The evaluation forward: setrank_forward's scores bit for bit, no record for a backward.  `work`: shape.score_bytes(B * L) bytes."""
    check(shape.lib.ultr_setrank_score(ctypes.byref(shape.desc), _p(params), _p(features), int(n_docs), _p(docids), int(B), int(L),
                                       _p(scores), _p(work), int(work.numel() * work.element_size()), _stream()), "ultr_setrank_score")


def setrank_backward(shape, params, B, L, saved, dscores, loss_ws, n_loss_parts, ws, grads, dropout=None):
    if dropout is not None:
        check(shape.lib.ultr_setrank_backward_dropout(ctypes.byref(shape.desc), _p(params), int(B), int(L), _p(saved), _p(dscores),
                                                      _p(loss_ws), int(n_loss_parts), _p(ws), _p(grads), ctypes.byref(dropout), _stream()),
              "ultr_setrank_backward_dropout")
        return
    check(shape.lib.ultr_setrank_backward(ctypes.byref(shape.desc), _p(params), int(B), int(L), _p(saved), _p(dscores), _p(loss_ws),
                                          int(n_loss_parts), _p(ws), _p(grads), _stream()), "ultr_setrank_backward")


def setrank_attn_path(shape, L, backward=False):
    """The attention kernel family SetRank's forward (or, backward=True, its backward) takes at list size L, under the knobs as the
    library last read them: one of _lib.SR_ATTN_PATHS - "scalar", "mfma" (fp32 matrix cores), "f16", "split_half" (backward only),
    "long_mfma" / "long_scalar" (the streaming kernels: the forward beyond 256 documents or from ULTR_SR_ATTN_LONG_MIN on; both
    directions of a model with attention_backward="streaming" beyond its one-pass backward's bound).  Host-only: needs no
    GPU and launches nothing.  A refused shape raises UltrHipError, as the call itself would."""
    rc = int(shape.lib.ultr_setrank_attn_path(ctypes.byref(shape.desc), int(L), 1 if backward else 0))
    check(min(rc, 0), "ultr_setrank_attn_path")
    return _lib.SR_ATTN_PATHS[rc]


class _StagedSizes:
    """The size queries of a staged model's shape (DLCM, GSF): ultr_<PREFIX>_saved_bytes / _score_bytes / _workspace_bytes on self.desc.
    A model the kernels do not take raises UltrHipError, as the calls do."""

    PREFIX = None

    def _bytes(self, query, *args):
        fn = "ultr_%s_%s_bytes" % (self.PREFIX, query)
        n = int(getattr(self.lib, fn)(ctypes.byref(self.desc), *args))
        check(min(n, 0), fn)
        return n

    def saved_bytes(self, n_rows):
        return self._bytes("saved", int(n_rows))

    def score_bytes(self, n_rows):
        """Bytes of the scoring form's buffer: what one launch hands to the next, nothing is kept for a backward."""
        return self._bytes("score", int(n_rows))

    def workspace_bytes(self, B, L):
        return self._bytes("workspace", int(B), int(L))


class DlcmShape(_StagedSizes):
    """Host-side geometry of one DLCM model (include/ultr_hip.h: ultr_dlcm_*): descriptor + flat parameter layout in state_dict order.
    `hidden_size` 0 means feature_size (the paper's choice).  feature_size and hidden_size must be multiples of 4: the size queries of
    any other model raise UltrHipError ("unsupported shape"), as the calls do; the layout is defined for every model."""

    NAMES = ("layer_norm.weight", "layer_norm.bias", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0",
             "att_linear.weight", "att_linear.bias", "att_v.weight")
    PREFIX = "dlcm"

    def __init__(self, feature_size, hidden_size=0, num_heads=3):
        self.lib = _lib.load()
        self.feature_size, self.num_heads = int(feature_size), int(num_heads)
        self.hidden_size = int(hidden_size) if int(hidden_size) > 0 else self.feature_size
        self.desc = _lib.DlcmDesc(self.feature_size, self.hidden_size, self.num_heads)
        offs = (ctypes.c_int64 * 10)()
        if int(self.lib.ultr_dlcm_param_offsets(ctypes.byref(self.desc), offs)) != 0:
            raise ValueError("bad DLCM description (feature_size, hidden_size and num_heads must be positive)")
        self.offsets = list(offs)
        self.n_params = int(offs[9])

    def layout(self):
        """[(state_dict key, shape, offset)] in parameter order."""
        F, H, hd = self.feature_size, self.hidden_size, self.num_heads
        shapes = ((F,), (F,), (3 * H, F), (3 * H, H), (3 * H,), (3 * H,), (hd * H, H), (hd * H,), (1, hd))
        return [(n, s, o) for n, s, o in zip(self.NAMES, shapes, self.offsets)]


def dlcm_forward(shape, params, features, n_docs, docids, B, L, scores, saved=None, work=None):
    """saved: the training form; saved None: the scoring form on `work` (shape.score_bytes) - the same scores bit for bit."""
    check(shape.lib.ultr_dlcm_forward(ctypes.byref(shape.desc), _p(params), _p(features) if n_docs > 0 else None, int(n_docs), _p(docids),
                                      int(B), int(L), _p(scores), _p(saved), _p(work), _stream()), "ultr_dlcm_forward")


def dlcm_backward(shape, params, features, n_docs, docids, B, L, saved, dscores, loss_ws, n_loss_parts, ws, grads):
    check(shape.lib.ultr_dlcm_backward(ctypes.byref(shape.desc), _p(params), _p(features) if n_docs > 0 else None, int(n_docs), _p(docids),
                                       int(B), int(L), _p(saved), _p(dscores), _p(loss_ws), int(n_loss_parts), _p(ws), _p(grads),
                                       _stream()), "ultr_dlcm_backward")


class GsfShape(_StagedSizes):
    """Host-side geometry of one GSF model (include/ultr_hip.h: ultr_gsf_*): descriptor + flat parameter layout, the DNN's keys in the
    DNN's order with layer 0 reading group_size * feature_size inputs and the last layer writing group_size outputs.  feature_size and
    every hidden width must be multiples of 4 and group_size at most 8: the size queries of any other model raise UltrHipError
    ("unsupported shape"), as the calls do; the layout is defined for every model.

    The training shuffle's key rides along, as SetRankShape's dropout key does: `train_shuffle`, `shuffle_seed` (the owner of the shape
    sets it; ranking_model.GSF captures torch.initial_seed()) and `shuffle_step`, the count of shuffled training forwards so far -
    engines are per batch shape, cached and evicted, so the counter is the model's, shared through this object."""

    PREFIX = "gsf"

    def __init__(self, feature_size, hidden, activation="elu", group_size=2, train_shuffle=True):
        self.lib = _lib.load()
        self.feature_size, self.group_size = int(feature_size), int(group_size)
        self.hidden = [int(h) for h in (hidden or [])]
        self.activation = activation
        if len(self.hidden) > _lib.ULTR_MAX_HIDDEN:
            raise ValueError("at most %d hidden layers are supported" % _lib.ULTR_MAX_HIDDEN)
        if activation not in _lib.ACT:
            raise ValueError("activation_func must be one of %s (got %r)" % (sorted(_lib.ACT), activation))
        d = self.desc = _lib.GsfDesc()
        d.feature_size, d.group_size, d.n_hidden, d.activation = self.feature_size, self.group_size, len(self.hidden), _lib.ACT[activation]
        for i, h in enumerate(self.hidden):
            d.hidden[i] = h
        self.n_params = int(self.lib.ultr_gsf_param_count(ctypes.byref(d)))
        if self.n_params <= 0:
            raise ValueError("bad GSF description (feature_size, group_size and the hidden widths must be positive)")
        nl = len(self.hidden) + 1
        offs = (ctypes.c_int64 * (4 * nl))()
        check(self.lib.ultr_gsf_param_offsets(ctypes.byref(d), offs), "ultr_gsf_param_offsets")
        self.offsets = list(offs)
        dims, k = [], self.feature_size * self.group_size
        for m in self.hidden + [self.group_size]:
            dims.append((k, m))
            k = m
        self.dims = dims
        self.train_shuffle, self.shuffle_seed, self.shuffle_step = bool(train_shuffle), 0, 0

    layout = DnnShape.layout

    def next_shuffle_step(self):
        """The step number of the shuffled training forward about to run; counts it."""
        step = self.shuffle_step
        self.shuffle_step = step + 1
        return step


def gsf_shuffle(seed, step, B, L, perm):
    """perm [B, L] int32: the Philox Fisher-Yates draw of (seed, step), one permutation of 0 .. L - 1 per list."""
    _req(perm, torch.int32, "perm")
    check(_lib.load().ultr_gsf_shuffle(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(B), int(L), _p(perm), _stream()),
          "ultr_gsf_shuffle")


def gsf_forward(shape, params, features, n_docs, docids, B, L, scores, perm=None, saved=None, work=None):
    """perm [B, L] int32 or None (the identity).  saved: the training form; saved None: the scoring form on `work` (shape.score_bytes) -
    the same scores bit for bit."""
    check(shape.lib.ultr_gsf_forward(ctypes.byref(shape.desc), _p(params), _p(features) if n_docs > 0 else None, int(n_docs), _p(docids),
                                     _p(perm), int(B), int(L), _p(scores), _p(saved), _p(work), _stream()), "ultr_gsf_forward")


def gsf_backward(shape, params, features, n_docs, docids, B, L, saved, dscores, loss_ws, n_loss_parts, ws, grads, perm=None):
    check(shape.lib.ultr_gsf_backward(ctypes.byref(shape.desc), _p(params), _p(features) if n_docs > 0 else None, int(n_docs), _p(docids),
                                      _p(perm), int(B), int(L), _p(saved), _p(dscores), _p(loss_ws), int(n_loss_parts), _p(ws), _p(grads),
                                      _stream()), "ultr_gsf_backward")


def tail_floats(L):
    return int(_lib.load().ultr_step_tail_floats(int(L)))


def loss_workspace_bytes(B, L):
    return int(_lib.load().ultr_loss_workspace_bytes(int(B), int(L)))


def loss_part_count(B):
    """Step-tail partials a stand-alone loss kernel writes for B lists."""
    return int(_lib.load().ultr_loss_part_count(int(B)))


def loss_lds_bytes(algo, L):
    """Dynamic LDS in bytes the stand-alone loss kernel of `algo` (a _lib.ALGO_* id) requests at list size L (ultr_loss_lds_bytes).
    Host-only: needs no GPU and launches nothing.  A list size the entry would refuse raises UltrHipError, as the call itself would."""
    n = int(_lib.load().ultr_loss_lds_bytes(int(algo), int(L)))
    check(min(n, 0), "ultr_loss_lds_bytes")
    return n


def loss_long_lds_bytes(algo, L):
    """Dynamic LDS in bytes the LONG-list loss kernel of `algo` (ALGO_PAIRDEBIAS, ALGO_LAMBDARANK, ALGO_PRS) requests at list size L
    (ultr_loss_long_lds_bytes).  Host-only.  Raises UltrHipError beyond its bound, or for an algorithm without a long kernel."""
    n = int(_lib.load().ultr_loss_long_lds_bytes(int(algo), int(L)))
    check(min(n, 0), "ultr_loss_long_lds_bytes")
    return n


def loss_long_max_list(algo):
    """The longest list the long-list loss kernel of `algo` accepts (ultr_loss_long_max_list).  Host-only."""
    n = int(_lib.load().ultr_loss_long_max_list(int(algo)))
    check(min(n, 0), "ultr_loss_long_max_list")
    return n


def loss_route(algo, L):
    """Which stand-alone loss kernel of `algo` (a _lib.ALGO_* id) a list of L documents runs: "short" for every list the short
    kernel takes, "long" only for a list it refuses and the long kernel (PairDebias, LambdaRank, PRSrank) takes.  Raises
    UltrHipError where neither does.  The rule ultr_train_step follows, read from the same LDS layouts; host-only."""
    lib = _lib.load()
    n = int(lib.ultr_loss_lds_bytes(int(algo), int(L)))
    if n >= 0:
        return "short"
    if n == -2 and int(lib.ultr_loss_long_lds_bytes(int(algo), int(L))) >= 0:  # (ULTR_E_UNSUPPORTED: the short layout does not fit)
        return "long"
    check(n, "ultr_loss_lds_bytes")


H3_KNOBS = ("ULTR_FB_H3", "ULTR_FWD_H3", "ULTR_BWD_H3")
SR_H3_KNOBS = ("ULTR_SR_H3",)


def knob_on(name, default=1):
    """An integer knob as the LIBRARY reads it (csrc: atoi of the environment string - 'false' or 'off' parse as 0 there, so they
    do here; an unset or empty variable is the default)."""
    v = os.environ.get(name, "")
    if v == "":
        return default != 0
    v = v.strip()
    sign = -1 if v.startswith("-") else 1
    digits = ""
    for ch in v.lstrip("+-"):
        if not ch.isdigit():
            break
        digits += ch
    return (sign * int(digits) if digits else 0) != 0


def split_half_enabled(shape=None):
    """Does any split-half (fp16 hi / lo) product read THIS model's weights?  Process-wide knobs AND the model's own switch
    (ultr_dnn_desc / ultr_setrank_desc ::flags)."""
    if shape is not None and (int(shape.desc.flags) & _lib.MODEL_FP32_PRODUCTS):
        return False
    knobs = SR_H3_KNOBS if isinstance(shape, SetRankShape) else H3_KNOBS
    return any(knob_on(k) for k in knobs)


def fall_back_to_fp32_products(shape, why):
    """Switch THIS model's products from the split-half (fp16 hi / lo) weight copies to the fp32 matrix cores - a flag in the
    model's descriptor (ULTR_MODEL_FP32_PRODUCTS), read by every later call that takes the descriptor; other models of the
    process keep their plan and nothing is written to the environment.  The reference computes in fp32 at any weight
    magnitude (DNN.py:58-88, base_algorithm.py:208-226); the copies cover |w| < 128 only.  In a data-parallel run the replicas
    are bit-identical and read their step reports in lockstep, so every rank switches at the same step.  Returns True when
    the model was on the split-half plan until now."""
    if not split_half_enabled(shape):
        return False
    shape.desc.flags = int(shape.desc.flags) | _lib.MODEL_FP32_PRODUCTS
    warnings.warn("ultra_pytorch_amd: %s - the products of this model now run on the fp32 matrix cores (ULTR_MODEL_FP32_PRODUCTS): "
                  "same results to the 1e-5 parity bar, a few per cent slower steps" % why, RuntimeWarning, stacklevel=3)
    return True


class WeightCopy:
    """The k-major copy of the hidden Linear weights the fast forward reads (ultr_dnn_build_wt).  Rebuilt whenever
    torch reports an in-place modification of `params` (load_state_dict, .copy_, init); ultr_apply_update keeps it
    current on its own (it writes through raw pointers, which does not bump the tensor version)."""

    def __init__(self, shape):
        self.shape = shape
        self.n = int(shape.lib.ultr_dnn_wt_floats(ctypes.byref(shape.desc)))
        self.wt, self.key, self.ref = None, None, None
        self.check = os.environ.get("ULTR_CHECK_WT", "0") == "1"

    def invalidate(self):
        """Force a rebuild on the next use.  torch's version counter sees every in-place tensor op (copy_, load_state_dict,
        optimizers), but NOT writes through `.data`, raw pointers (other than this library's own update kernel, which
        maintains the copy itself) or DLPack aliases: whoever writes the parameters that way must call this
        (`ranking_model.DNN.invalidate_weight_copy()`); ULTR_CHECK_WT=1 verifies the copy on every use (debug, synchronises)."""
        self.key = None

    def _verify(self, params):
        fresh = torch.empty_like(self.wt)
        check(self.shape.lib.ultr_dnn_build_wt(ctypes.byref(self.shape.desc), _p(params), _p(fresh), _stream()), "ultr_dnn_build_wt")
        if not torch.equal(fresh, self.wt):
            raise RuntimeError("stale k-major weight copy: the parameters were written behind torch's version counter "
                               "(.data / raw pointer); call invalidate_weight_copy() after such writes")

    def get(self, params):
        # identity of the tensor OBJECT (weakref: a freed tensor's address and version 0 can both be reused)
        key = (params.data_ptr(), params._version)
        same = self.ref is not None and self.ref() is params and key == self.key
        if self.wt is None or self.wt.device != params.device:
            self.wt = torch.zeros(self.n, dtype=torch.float32, device=params.device)  # alignment gaps stay zero
            same = False
        if not same:
            check(self.shape.lib.ultr_dnn_build_wt(ctypes.byref(self.shape.desc), _p(params), _p(self.wt), _stream()),
                  "ultr_dnn_build_wt")
            self.key, self.ref = key, weakref.ref(params)
            # parameters that arrived from outside (checkpoint, init, a test) may be out of the split-half copies' range: look
            # once (a stream synchronisation - this branch runs after external writes only) and switch to the fp32 products
            # BEFORE a kernel reads the copies; training drift is caught by the step report instead (engine.StepEngine)
            if split_half_enabled(self.shape):
                rng = int(self.shape.lib.ultr_dnn_wt_range(ctypes.byref(self.shape.desc), _p(self.wt), _stream()))
                if rng < 0:
                    check(rng, "ultr_dnn_wt_range")
                if rng > 0:
                    fall_back_to_fp32_products(self.shape, "a hidden weight of magnitude >= 64 was loaded (the split-half weight "
                                               "copies cover |w| < 128)")
        elif self.check:
            self._verify(params)
        return self.wt


def weight_copy(shape):
    if getattr(shape, "_wcopy", None) is None:
        shape._wcopy = WeightCopy(shape)
    return shape._wcopy


def dnn_forward(shape, params, features, n_docs, docids, B, L, scores, saved=None, wt=None):
    lib = shape.lib
    _req(params, torch.float32, "params"), _req(docids, torch.int32, "docids"), _req(scores, torch.float32, "scores")
    if n_docs > 0:
        _req(features, torch.float32, "features")
    if wt is None:
        wt = weight_copy(shape).get(params)
    check(lib.ultr_dnn_forward(ctypes.byref(shape.desc), _p(params), _p(wt), _p(features) if n_docs > 0 else None,
                               int(n_docs), _p(docids), int(B), int(L), _p(scores), _p(saved), _stream()), "ultr_dnn_forward")


def dnn_backward(shape, params, features, n_docs, docids, B, L, saved, dscores, loss_ws, bwd_ws, grads):
    lib = shape.lib
    check(lib.ultr_dnn_backward(ctypes.byref(shape.desc), _p(params), _p(features) if n_docs > 0 else None, int(n_docs),
                                _p(docids), int(B), int(L), _p(saved), _p(dscores), _p(loss_ws), _p(bwd_ws), _p(grads),
                                _stream()), "ultr_dnn_backward")


def dnn_backward_softmax(shape, params, features, n_docs, docids, B, L, saved, scores, labels, loss_ws, bwd_ws, grads,
                         pw=None, ipw_table=None, dscores_out=None):
    n_ipw = 0 if ipw_table is None else int(ipw_table.numel())
    check(shape.lib.ultr_dnn_backward_softmax(ctypes.byref(shape.desc), _p(params), _p(features) if n_docs > 0 else None,
                                              int(n_docs), _p(docids), int(B), int(L), _p(saved), _p(scores), _p(labels), _p(pw),
                                              _p(ipw_table), n_ipw, _p(dscores_out), _p(loss_ws), _p(bwd_ws), _p(grads),
                                              _stream()), "ultr_dnn_backward_softmax")


def grad_sumsq(grads, n_params, L, bwd_ws):
    check(_lib.load().ultr_grad_sumsq(_p(grads), int(n_params), int(L), _p(bwd_ws), _stream()), "ultr_grad_sumsq")


def softmax_ce(scores, labels, B, L, dscores, loss_ws, pw=None, ipw_table=None):
    n_ipw = 0 if ipw_table is None else int(ipw_table.numel())
    check(_lib.load().ultr_softmax_ce(_p(scores), _p(labels), _p(pw), _p(ipw_table), n_ipw, int(B), int(L), _p(dscores),
                                      _p(loss_ws), _stream()), "ultr_softmax_ce")


def dla_loss(scores, labels, prop_params, logits_to_prob, B, L, dscores, loss_ws):
    check(_lib.load().ultr_dla_loss(_p(scores), _p(labels), _p(prop_params), int(logits_to_prob), int(B), int(L),
                                    _p(dscores), _p(loss_ws), _stream()), "ultr_dla_loss")


def pairdebias_loss(scores, labels, t_plus, t_minus, B, L, batch_total, dscores, loss_ws):
    check(_lib.load().ultr_pairdebias_loss(_p(scores), _p(labels), _p(t_plus), _p(t_minus), int(B), int(L),
                                           int(batch_total), _p(dscores), _p(loss_ws), _stream()), "ultr_pairdebias_loss")


def lambdarank_loss(scores, labels, t_plus, t_minus, sigma, B, L, dscores, loss_ws):
    check(_lib.load().ultr_lambdarank_loss(_p(scores), _p(labels), _p(t_plus), _p(t_minus), float(sigma), int(B), int(L),
                                           _p(dscores), _p(loss_ws), _stream()), "ultr_lambdarank_loss")


def prs_loss(scores, labels, ipw_table, sigma, B, L, dscores, loss_ws):
    """PRSrank: propensity-ratio-scored, delta-NDCG-weighted pairwise BCE on the sorted list; ipw_table = the IPW_list (fp32)."""
    check(_lib.load().ultr_prs_loss(_p(scores), _p(labels), _p(ipw_table), int(ipw_table.numel()), float(sigma), int(B), int(L),
                                    _p(dscores), _p(loss_ws), _stream()), "ultr_prs_loss")


def prs_loss_pw(scores, labels, ipw_bl, sigma, B, L, dscores, loss_ws):
    """PRSrank with a weight per list entry: ipw_bl [B, L] (presentation order) instead of the position table (history_pw)."""
    check(_lib.load().ultr_prs_loss_pw(_p(scores), _p(labels), _p(ipw_bl), float(sigma), int(B), int(L), _p(dscores), _p(loss_ws),
                                       _stream()), "ultr_prs_loss_pw")


# The long-list kernels (csrc/ultr_loss_long.hip): the arguments of the short wrappers above, every L from 1 up to loss_long_max_list.
def pairdebias_loss_long(scores, labels, t_plus, t_minus, B, L, batch_total, dscores, loss_ws):
    check(_lib.load().ultr_pairdebias_loss_long(_p(scores), _p(labels), _p(t_plus), _p(t_minus), int(B), int(L),
                                                int(batch_total), _p(dscores), _p(loss_ws), _stream()), "ultr_pairdebias_loss_long")


def lambdarank_loss_long(scores, labels, t_plus, t_minus, sigma, B, L, dscores, loss_ws):
    check(_lib.load().ultr_lambdarank_loss_long(_p(scores), _p(labels), _p(t_plus), _p(t_minus), float(sigma), int(B), int(L),
                                                _p(dscores), _p(loss_ws), _stream()), "ultr_lambdarank_loss_long")


def prs_loss_long(scores, labels, ipw_table, sigma, B, L, dscores, loss_ws):
    check(_lib.load().ultr_prs_loss_long(_p(scores), _p(labels), _p(ipw_table), int(ipw_table.numel()), float(sigma), int(B), int(L),
                                         _p(dscores), _p(loss_ws), _stream()), "ultr_prs_loss_long")


def prs_loss_pw_long(scores, labels, ipw_bl, sigma, B, L, dscores, loss_ws):
    check(_lib.load().ultr_prs_loss_pw_long(_p(scores), _p(labels), _p(ipw_bl), float(sigma), int(B), int(L), _p(dscores), _p(loss_ws),
                                            _stream()), "ultr_prs_loss_pw_long")


def pdgd_loss(scores, labels, docids, n_docs, tau, cutoff, B, L, dscores, loss_ws):
    """PDGD: the pairs of clicked documents with lower-labelled ones above them (or just below), each weighted by the
    Plackett-Luce probability ratio of the swapped ranking; docids [L, B] int32 mark the PADs (== n_docs)."""
    check(_lib.load().ultr_pdgd_loss(_p(scores), _p(labels), _p(docids), int(n_docs), float(tau), int(cutoff), int(B), int(L),
                                     _p(dscores), _p(loss_ws), _stream()), "ultr_pdgd_loss")


def regem_loss(scores, labels, propensity, B, L, dscores, loss_ws, uniforms=None, seed=0, step=0, pseudo_out=None):
    """RegressionEM estimation + BCE loss; uniforms [B, L] teacher-forces the Bernoulli draw."""
    check(_lib.load().ultr_regem_loss(_p(scores), _p(labels), _p(propensity), _p(uniforms), int(seed), int(step), int(B),
                                      int(L), _p(dscores), _p(pseudo_out), _p(loss_ws), _stream()), "ultr_regem_loss")


def twotower_loss(scores, labels, bias_logits, B, L, dscores, loss_ws, combination="product", docids=None, n_docs=0):
    """TwoTower: the click log-likelihood of sigmoid(s) sigmoid(theta_l) ("product") or sigmoid(s + theta_l) ("sum"), bias_logits [L]
    = theta.  docids [L, B] int32 with n_docs masks the PAD positions (id < 0 or >= n_docs); None: every position counts."""
    if combination not in ("product", "sum"):
        raise ValueError("tower_combination must be 'product' or 'sum', got %r" % (combination,))
    check(_lib.load().ultr_twotower_loss(_p(scores), _p(labels), _p(bias_logits), _lib.TWOTOWER_SUM if combination == "sum" else 0,
                                         _p(docids), int(n_docs), int(B), int(L), _p(dscores), _p(loss_ws), _stream()),
          "ultr_twotower_loss")


def plrank_loss(scores, labels, docids, n_docs, B, L, dscores, loss_ws, n_samples=64, cutoff=0, gain="linear", seed=0, step=0, pw=None,
                ipw_table=None, perm_out=None):
    """PLRank: the sampled Plackett-Luce policy gradient of the expected DCG@cutoff (0: the whole list) from n_samples rankings per
    list, drawn under Philox(seed, step).  Relevance estimates rho = w * gain(labels): w from pw [B, L], else ipw_table (the IPW_list),
    else 1; gain "linear" or "exp2".  docids [L, B] int32 with n_docs mark the PADs.  perm_out [B, n_samples, L] int32 (optional)
    receives the sampled orders."""
    if gain not in _lib.PLRANK_GAIN:
        raise ValueError("gain must be one of %s, got %r" % (sorted(_lib.PLRANK_GAIN), gain))
    if perm_out is not None:
        _req(perm_out, torch.int32, "perm_out")
    n_ipw = 0 if ipw_table is None else int(ipw_table.numel())
    check(_lib.load().ultr_plrank_loss(_p(scores), _p(labels), _p(pw), _p(ipw_table), n_ipw, _p(docids), int(n_docs), int(cutoff),
                                       int(n_samples), _lib.PLRANK_GAIN[gain], int(seed) & 0xFFFFFFFFFFFFFFFF,
                                       int(step) & 0xFFFFFFFFFFFFFFFF, int(B), int(L), _p(dscores), _p(perm_out), _p(loss_ws),
                                       _stream()), "ultr_plrank_loss")


def affine_loss(scores, labels, alpha, beta, B, L, dscores, loss_ws, docids=None, n_docs=0):
    """AffineRank: the listwise softmax loss with the affine-corrected clicks w = (c - beta_k) / alpha_k, k = min(l, n - 1), at every
    position (alpha, beta: float32 [n] each, alpha > 0).  docids [L, B] int32 with n_docs mark the PADs (w = 0 there); None: every
    position counts.  Weights, their sum and the loss may be negative."""
    _req(alpha, torch.float32, "alpha")
    _req(beta, torch.float32, "beta")
    if alpha.numel() != beta.numel():
        raise ValueError("alpha and beta must have one length, got %d and %d" % (alpha.numel(), beta.numel()))
    check(_lib.load().ultr_affine_loss(_p(scores), _p(labels), _p(alpha), _p(beta), int(alpha.numel()), _p(docids), int(n_docs), int(B),
                                       int(L), _p(dscores), _p(loss_ws), _stream()), "ultr_affine_loss")


def apply_update(shape, udesc, params, state, grads, aux, bwd_ws, scalars):
    wt = weight_copy(shape).get(params)  # the update kernel writes the new weights into both layouts
    check(shape.lib.ultr_apply_update(ctypes.byref(udesc), ctypes.byref(shape.desc), _p(params), _p(wt), _p(state), _p(grads),
                                      _p(aux), _p(bwd_ws), _p(scalars), _stream()), "ultr_apply_update")


def ndcg(scores, labels, docids, n_docs, B, L, topn, ndcg_out, ndcg_ws, order_out=None, masked_out=None):
    arr = (ctypes.c_int32 * len(topn))(*[int(t) for t in topn])
    check(_lib.load().ultr_ndcg(_p(scores), _p(labels), _p(docids), int(n_docs), int(B), int(L), arr, len(topn),
                                _p(ndcg_out), _p(order_out), _p(masked_out), _p(ndcg_ws), _stream()), "ultr_ndcg")


def propensity_count(labels, lengths, exam, n_exam, cprob, click_model, seed, first_session, n_sessions, click_count):
    """n_sessions randomized click sessions (ultr_propensity_count) ADDED to click_count [lmax, lmax] int64: labels [n_queries, lmax]
    float32 with row q valid in [0, lengths[q]), lengths [n_queries] int32, exam / cprob as the device feeds upload them."""
    _req(labels, torch.float32, "labels"), _req(lengths, torch.int32, "lengths"), _req(exam, torch.float32, "exam")
    _req(cprob, torch.float32, "cprob"), _req(click_count, torch.int64, "click_count")
    n_queries, lmax = labels.shape
    if lengths.numel() != n_queries or tuple(click_count.shape) != (lmax, lmax):
        raise ValueError("propensity_count: labels [n_queries, lmax] needs lengths [n_queries] and click_count [lmax, lmax]")
    a = _lib.PropensityArgs()
    a.labels, a.lengths, a.n_queries, a.lmax = labels.data_ptr(), lengths.data_ptr(), int(n_queries), int(lmax)
    a.exam_prob, a.n_exam, a.click_prob, a.n_rel = exam.data_ptr(), int(n_exam), cprob.data_ptr(), int(cprob.numel())
    a.click_model, a.seed, a.first_session, a.n_sessions = int(click_model), int(seed), int(first_session), int(n_sessions)
    a.click_count = click_count.data_ptr()
    check(_lib.load().ultr_propensity_count(ctypes.byref(a), _stream()), "ultr_propensity_count")


def history_pw(labels, table, pw_out, all_positions, args=None):
    """pw_out [B, L] = the weights of a click model with a click history (ultr_history_pw): labels [L, B] clicks, table [L, L] from
    OraclePropensityEstimator.weight_table; all_positions False: clicked positions only (IPWrank), True: every position (PRSrank).
    Queued on the current stream.  args: a _lib.HistoryPwArgs the caller keeps between calls (a step loop: no struct per step)."""
    _req(labels, torch.float32, "labels"), _req(table, torch.float32, "table"), _req(pw_out, torch.float32, "pw_out")
    L, B = labels.shape
    if tuple(table.shape) != (L, L) or tuple(pw_out.shape) != (B, L):
        raise ValueError("history_pw: labels [L, B] needs table [L, L] and pw_out [B, L]")
    a = _lib.HistoryPwArgs() if args is None else args
    a.labels, a.table, a.pw_out = labels.data_ptr(), table.data_ptr(), pw_out.data_ptr()
    a.batch, a.list_size, a.all_positions = int(B), int(L), 1 if all_positions else 0
    check(_lib.load().ultr_history_pw(ctypes.byref(a), _stream()), "ultr_history_pw")
