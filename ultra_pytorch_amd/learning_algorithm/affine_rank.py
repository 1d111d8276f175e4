"""AffineRank — counterfactual learning to rank from clicks with trust bias: the listwise softmax loss with the affine-corrected clicks
(Agarwal et al., WWW 2019; Vardasbi et al., CIKM 2020).  The project's own algorithm - the reference has no such class.

    P(click | rank k, relevance gamma) = alpha_k gamma + beta_k,  beta_k > 0    (click_models.TrustBiasModel)
    w_l  = (click_l - beta_k) / alpha_k,  k = min(l, n - 1)                    at EVERY position, clicked or not:  E[w_l] = gamma
    loss = mean over lists of  sum_l w_l (-log softmax(scores)_l)

Under that law inverse propensity weighting is biased whatever its table; the affine estimate is not.  The weights of unclicked
positions are negative, so the loss value may be negative too: its gradient is what is unbiased.  `affine_estimator_json` is a table
({"alpha": [...], "beta": [...]}) or a click model (the model's own JSON, or a file with a "click_model" entry), answered by
OraclePropensityEstimator.affine_table.  The loss runs in ultr_affine_loss; the law is DESIGN.md section 4e.  Estimating (alpha, beta)
from clicks and data parallelism are not part of it."""
import json

import numpy as np
import torch

from ..utils import HParams
from .base_algorithm import BaseAlgorithm
from .ipw_rank import resolve_estimator_json


def load_affine_table(path, list_size, affine_clip=0.0):
    """(alpha[n], beta[n]) as float32 numpy from `path` (needs no GPU): a table file gives its own entries (the kernel saturates at
    the last one), a click model the first `list_size` entries of OraclePropensityEstimator.affine_table.  alpha_k <= 0 raises
    ValueError; affine_clip > 0 sets alpha_k = max(alpha_k, affine_clip), beta is untouched."""
    from ..utils import click_models as CM
    from ..utils.propensity_estimator import OraclePropensityEstimator
    with open(resolve_estimator_json(path)) as fin:
        data = json.load(fin)
    if "alpha" in data and "beta" in data:
        alpha, beta = np.asarray(data["alpha"], np.float32), np.asarray(data["beta"], np.float32)
    elif "click_model" in data or "model_name" in data:
        model = CM.loadModelFromJson(data["click_model"] if "click_model" in data else data)
        alpha, beta = OraclePropensityEstimator(model).affine_table(list_size)
    else:
        raise KeyError("%s holds neither an \"alpha\" / \"beta\" table nor a click model" % path)
    if alpha.ndim != 1 or alpha.shape != beta.shape or alpha.size == 0:
        raise ValueError("alpha and beta must be two lists of one length >= 1, got %r and %r" % (alpha.shape, beta.shape))
    if not np.isfinite(alpha).all() or not np.isfinite(beta).all() or (alpha <= 0).any():
        raise ValueError("the affine correction divides by alpha_k: every alpha_k must be finite and > 0, got %r" % (alpha.tolist(),))
    if affine_clip > 0:
        alpha = np.maximum(alpha, np.float32(affine_clip))
    return alpha, beta


class AffineRank(BaseAlgorithm):
    ENGINE_ALGO = "affine"

    @staticmethod
    def parse_hparams(hparam_string):
        """The algorithm's hyper-parameters from a settings string (needs no GPU).  A negative affine_clip raises ValueError."""
        hp = HParams(affine_estimator_json="./example/ClickModel/trust_0.1_1.0_4_1.0.json", affine_clip=0.0, mask_padding=True,
                     learning_rate=0.05, max_gradient_norm=5.0, l2_loss=0.0, grad_strategy="ada")
        hp.parse(hparam_string)
        if float(hp.affine_clip) < 0:
            raise ValueError("affine_clip must be >= 0 (0: no clipping of alpha), got %r" % (hp.affine_clip,))
        return hp

    def __init__(self, data_set, exp_settings):
        print("Build the affine-corrected listwise ranker (trust bias).")
        print(exp_settings["learning_algorithm_hparams"])
        self.hparams = self.parse_hparams(exp_settings["learning_algorithm_hparams"])
        if exp_settings.get("process_group", None) is not None:
            raise NotImplementedError("AffineRank does not train data parallel: run it without a process_group")
        # (the table is read before the model is built: a bad one raises with nothing on the GPU)
        self.alpha, self.beta = load_affine_table(
            self.hparams.affine_estimator_json, int(exp_settings.get("selection_bias_cutoff", exp_settings["max_candidate_num"])),
            float(self.hparams.affine_clip))
        self._setup(data_set, exp_settings)
        self.affine_table = torch.from_numpy(np.concatenate([self.alpha, self.beta])).to(self.cuda)  # [alpha(n) | beta(n)]

    def _engine_kwargs(self):
        return dict(mask_padding=bool(self.hparams.mask_padding))

    def write_affine_table(self, path):
        """The table in use (after the clip) as the JSON affine_estimator_json loads."""
        with open(path, "w") as f:
            f.write(json.dumps({"alpha": [float(x) for x in self.alpha], "beta": [float(x) for x in self.beta]}, indent=4, sort_keys=True))

    def train(self, input_feed):
        """One step: forward, the affine-corrected loss, backward, update; global_step is incremented after the step."""
        if not self.model.training:  # (nn.Module.train() walks every submodule: ~10 us a 47 us step does not have)
            self.model.train()
        L = self.rank_list_size
        self.create_input_feed(input_feed, L)
        eng = self._train_engine(self.batch_size, L)
        eng.train_step(self.model.flat_params, self.state_sum, self.letor_features, self.n_docs, self.docid_inputs, self.labels_LB,
                       ipw_table=self.affine_table)
        self.loss = eng.read_loss()  # the only host sync: the reference's loss.item()
        self.global_step += 1
        print("Loss %f at global step %d" % (self.loss, self.global_step))
        return self.loss, None, self.train_summary
