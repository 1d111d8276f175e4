"""GSF - Groupwise Scoring Function (Ai, Wang, Bendersky et al., ICTIR 2019): the ranking model the reference's README lists and never
shipped (`# from .GSF import *`).  This is the model as DESIGN.md section 3e fixes it, for one list of L presented positions and
m = group_size:

    place p holds presented position perm[p] (the identity, or - a training step with train_shuffle - a Philox Fisher-Yates draw)
    group g (one per place) holds in slot j the document at place (g + j) mod L: the circular windows of the shuffled list, so every
              document fills every slot exactly once; a PAD (document id n_docs) is the zero row
    u_g     = LayerNorm_{mF}(the m rows side by side), eps 1e-5
    o_g     = the DNN on it: [Linear -> act -> LayerNorm] x k -> Linear(H_k, m)
    score[perm[p]] = sum_j o_{(p - j) mod L}[j]         (every group output that names the document; no 1 / m)

Constructor `(hparams_str, feature_size)`; hparams `hidden_layer_sizes`, `activation_func`, `norm` (the DNN's), `group_size`,
`train_shuffle`.  All parameters are views into ONE flat fp32 tensor with the DNN's state_dict keys in the DNN's order - the layout
ultr_gsf_forward / ultr_gsf_backward consume - initialised as torch initialises nn.LayerNorm / nn.Linear, from the global generator; at
group_size = 1 the layout, and the model, are the DNN's.  The shuffle's key is the model's: `shape.shuffle_seed` (torch.initial_seed()
at construction, settable) and `shape.shuffle_step`, the count of shuffled training forwards.  Not here: all L^m groups, shuffling at
evaluation or of the non-PAD prefix only, averaging, dropout, noisy parameters, data parallelism.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import engine, hip_ops
from ..utils.hparams import HParams
from .dnn import init_flat_params


class GSF(nn.Module):
    step_engine_cls = engine.GsfStepEngine
    eval_engine_cls = engine.GsfEvalEngine

    DEFAULT_HIDDEN = [512, 256, 128]

    def __init__(self, hparams_str, feature_size=None):
        super().__init__()
        print("build GSF")
        self.hparams = HParams(hidden_layer_sizes=list(self.DEFAULT_HIDDEN), activation_func="elu", norm="layer", group_size=2,
                               train_shuffle=True)
        self.hparams.parse(hparams_str)
        if self.hparams.norm != "layer":
            raise NotImplementedError("norm=%r: only 'layer' is supported, as for the DNN" % self.hparams.norm)
        if self.hparams.activation_func == "selu":
            raise TypeError("activation_func='selu' raises for the DNN too (base_ranking_model.selu is not a Module subclass)")
        if self.hparams.activation_func not in ("elu", "relu", "tanh", "sigmoid"):
            raise NotImplementedError("activation_func=%r: base_ranking_model.py:63-69 knows elu, relu, tanh, sigmoid"
                                      % self.hparams.activation_func)
        self.feature_size = int(feature_size)
        self.shape = hip_ops.GsfShape(self.feature_size, list(self.hparams.hidden_layer_sizes), self.hparams.activation_func,
                                      int(self.hparams.group_size), bool(self.hparams.train_shuffle))
        self.shape.saved_bytes(1)  # a model the kernels do not take (a width off the 4 grid, group_size > 8) is refused here
        self.shape.shuffle_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self._bind(init_flat_params(self.shape))
        self._fwd_work = {}

    def _bind(self, flat):
        """(Re)create the parameter views over `flat` (device moves re-bind)."""
        self.flat_params = flat
        self.sequential = nn.Module()
        mods = {}
        for name, shp, off in self.shape.layout():
            _, mod, leaf = name.split(".")
            n = int(np.prod(shp))
            p = nn.Parameter(flat[off:off + n].view(*shp), requires_grad=False)
            mods.setdefault(mod, nn.Module()).register_parameter(leaf, p)
        for mod, m in mods.items():
            self.sequential.add_module(mod, m)

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
        """Scores for a list of L tensors [B, F] -> list of L tensors [B, 1], in presented order (no shuffle: the scoring form)."""
        if noisy_params is not None:
            raise NotImplementedError("GSF has no support for noisy parameters")
        if not self.flat_params.is_cuda:
            raise RuntimeError("ultra_pytorch_amd.ranking_model.GSF.build needs the model on the GPU; there is no CPU fallback")
        dev = self.flat_params.device
        L, B = len(input_list), int(input_list[0].shape[0])
        x = torch.cat([t.to(dev, torch.float32) for t in input_list], dim=0).contiguous()  # position-major rows
        docids = torch.arange(L * B, dtype=torch.int32, device=dev)
        scores = torch.empty(B, L, dtype=torch.float32, device=dev)
        key = (B, L)
        if key not in self._fwd_work:
            self._fwd_work[key] = torch.empty(max(self.shape.score_bytes(B * L) // 4, 1), dtype=torch.float32, device=dev)
        hip_ops.gsf_forward(self.shape, self.flat_params, x, L * B, docids, B, L, scores, work=self._fwd_work[key])
        return list(torch.split(scores.t().contiguous().view(L * B, 1), B, dim=0))
