"""DLCM - Deep Listwise Context Model (Ai, Bi, Guo, Croft, SIGIR 2018): the ranking model the reference's README and shipped settings
name (`ultra.ranking_model.DLCM`) and never shipped.  This is the model as DESIGN.md section 3d fixes it:

    xh_l    = LayerNorm_F(x_l), eps 1e-5; a PAD (document id n_docs) is the zero row, so it comes out as beta
    o_l     = a one-layer GRU (torch.nn.GRU's law and layout) reading the list from the LAST position to the FIRST from h = 0;
              o_l is the state after position l, s = o_0 the state after the top document
    score_l = o_l . m,  m = sum_j v_j M_j,  M = tanh(W_phi s + b_phi) viewed as [num_heads, H]      (the paper's eq. 6, folded)

Constructor `(hparams_str, feature_size)`; hparams `hidden_size` (0: feature_size, the paper's choice) and `num_heads`.  All parameters
are views into ONE flat fp32 tensor in state_dict order (`layer_norm`, `gru`, `att_linear`, `att_v`) - the layout ultr_dlcm_forward /
ultr_dlcm_backward consume - initialised as torch initialises those modules, from the global generator.  Not here: LSTM cells, input
abstraction layers, forward-order reading, dropout, noisy parameters, data parallelism.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import engine, hip_ops
from ..utils.hparams import HParams


def init_dlcm_params(shape):
    """torch's own initialisation of nn.LayerNorm, nn.GRU, nn.Linear(H, num_heads H) and nn.Linear(num_heads, 1, bias=False), drawn in
    that order from the global generator (torch.manual_seed controls it), in the flat layout."""
    F, H, hd = shape.feature_size, shape.hidden_size, shape.num_heads
    mods = {"layer_norm": nn.LayerNorm(F), "gru": nn.GRU(F, H, batch_first=True), "att_linear": nn.Linear(H, hd * H),
            "att_v": nn.Linear(hd, 1, bias=False)}
    flat = torch.empty(shape.n_params, dtype=torch.float32)
    with torch.no_grad():
        for name, shp, off in shape.layout():
            mod, par = name.split(".")
            flat[off:off + int(np.prod(shp))] = getattr(mods[mod], par).reshape(-1)
    return flat


class _Node(nn.Module):
    """Bare container of the parameters of one sub-module name."""


class DLCM(nn.Module):
    step_engine_cls = engine.DlcmStepEngine
    eval_engine_cls = engine.DlcmEvalEngine

    def __init__(self, hparams_str, feature_size=None):
        super().__init__()
        print("build DLCM")
        self.hparams = HParams(hidden_size=0, num_heads=3)
        self.hparams.parse(hparams_str)
        self.feature_size = int(feature_size)
        self.shape = hip_ops.DlcmShape(self.feature_size, int(self.hparams.hidden_size), int(self.hparams.num_heads))
        self.shape.saved_bytes(1)  # a model the kernels do not take (feature_size / hidden_size off the 4 grid) is refused here
        self._bind(init_dlcm_params(self.shape))
        self._fwd_work = {}

    def _bind(self, flat):
        self.flat_params = flat
        root = _Node()
        for name, shp, off in self.shape.layout():
            mod, par = name.split(".")
            if mod not in root._modules:
                root.add_module(mod, _Node())
            n = int(np.prod(shp))
            root._modules[mod].register_parameter(par, nn.Parameter(flat[off:off + n].view(*shp), requires_grad=False))
        for mod, node in root._modules.items():
            setattr(self, mod, node)

    def _apply(self, fn, *a, **k):
        flat = fn(self.flat_params.detach())
        self._bind(flat.contiguous().to(torch.float32))
        self._fwd_work = {}
        return self

    def load_state_dict(self, state_dict, strict=True):
        own = dict(self.state_dict())
        missing = [k for k in own if k not in state_dict]
        unexpected = [k for k in state_dict if k not in own]
        if strict and (missing or unexpected):
            raise RuntimeError("load_state_dict: missing %s unexpected %s" % (missing, unexpected))
        with torch.no_grad():
            for k, v in state_dict.items():
                if k in own:
                    own[k].copy_(v.to(own[k].device, torch.float32))
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def build(self, input_list, noisy_params=None, noise_rate=0.05, is_training=False, **kwargs):
        """Scores for a list of L tensors [B, F] -> list of L tensors [B, 1]."""
        if noisy_params is not None:
            raise NotImplementedError("DLCM has no support for noisy parameters")
        if not self.flat_params.is_cuda:
            raise RuntimeError("ultra_pytorch_amd.ranking_model.DLCM.build needs the model on the GPU; there is no CPU fallback")
        dev = self.flat_params.device
        L, B = len(input_list), int(input_list[0].shape[0])
        x = torch.cat([t.to(dev, torch.float32) for t in input_list], dim=0).contiguous()  # position-major rows
        docids = torch.arange(L * B, dtype=torch.int32, device=dev)
        scores = torch.empty(B, L, dtype=torch.float32, device=dev)
        key = (B, L)
        if key not in self._fwd_work:
            self._fwd_work[key] = torch.empty(max(self.shape.score_bytes(B * L) // 4, 1), dtype=torch.float32, device=dev)
        hip_ops.dlcm_forward(self.shape, self.flat_params, x, L * B, docids, B, L, scores, work=self._fwd_work[key])
        return list(torch.split(scores.t().contiguous().view(L * B, 1), B, dim=0))
