"""TwoTower — the pointwise two-tower click model: a relevance tower (the ranking model) and an observation tower (one logit per
position), trained jointly by maximum likelihood on the clicks (PAL's "shallow tower"; the pointwise baseline of the ULTR
benchmarks).  The project's own algorithm - the reference has no such class; its dead `sigmoid_loss` branches stay refused.

    P(click at position l) = sigmoid(s) * sigmoid(theta_l)   tower_combination="product" (default)
                           = sigmoid(s + theta_l)            tower_combination="sum"
    loss = mean over lists of the sum over positions of  -c log p - (1 - c) log(1 - p),  c = min(label, 1)

It has RegressionEM's click model fitted by gradient steps instead of EM with sampled pseudo-labels, and it is the pointwise twin of
DLA.  The loss runs in ultr_twotower_loss, the step of both towers in the update launch."""
import json
import math

import torch

from ..utils import HParams
from .base_algorithm import BaseAlgorithm

COMBINATIONS = ("product", "sum")


class TwoTower(BaseAlgorithm):
    ENGINE_ALGO = "twotower"

    @staticmethod
    def parse_hparams(hparam_string):
        """The algorithm's hyper-parameters from a settings string (needs no GPU).  Any tower_combination but 'product' / 'sum' raises."""
        hp = HParams(learning_rate=0.05, max_gradient_norm=5.0, l2_loss=0.0, grad_strategy="ada", tower_combination="product",
                     propensity_learning_rate=-1.0, mask_padding=True)
        hp.parse(hparam_string)
        if hp.tower_combination not in COMBINATIONS:
            raise ValueError("tower_combination must be one of %s, got %r" % (COMBINATIONS, hp.tower_combination))
        return hp

    def __init__(self, data_set, exp_settings):
        print("Build the two-tower click model.")
        print(exp_settings["learning_algorithm_hparams"])
        self.hparams = self.parse_hparams(exp_settings["learning_algorithm_hparams"])
        self._setup(data_set, exp_settings)
        plr = float(self.hparams.propensity_learning_rate)
        self.propensity_learning_rate = self.learning_rate if plr < 0 else plr
        # the observation tower theta [L]: an examination probability of 0.9 where RegressionEM starts (product), 0 for the sum
        init = math.log(9.0) if self.hparams.tower_combination == "product" else 0.0
        self.bias_logits = torch.full((self.rank_list_size,), init, dtype=torch.float32, device=self.cuda)

    def _engine_kwargs(self):
        return dict(propensity_learning_rate=self.propensity_learning_rate, tower_combination=self.hparams.tower_combination,
                    mask_padding=bool(self.hparams.mask_padding))

    @property
    def propensity(self):
        """The examination probabilities sigmoid(theta) as [1, L]; the additive form has none."""
        if self.hparams.tower_combination != "product":
            raise ValueError("tower_combination='sum' has no examination probability: read bias_logits")
        return torch.sigmoid(self.bias_logits).view(1, -1)

    def export_propensity(self, path):
        """Write the learned table as the {"IPW_list": [...]} JSON of utils.propensity_estimator, IPW_list[l] = sigmoid(theta_0) /
        sigmoid(theta_l): IPWrank and PRSrank then train on it (propensity_estimator_json)."""
        p = self.propensity.view(-1).double().cpu()
        table = [float(p[0] / v) for v in p]
        with open(path, "w") as f:
            f.write(json.dumps({"IPW_list": table}, indent=4, sort_keys=True))
        return table

    def train(self, input_feed):
        """One step: forward, the joint click likelihood, backward, and one update launch that clips and steps both towers;
        global_step is incremented after the step, as RegressionEM.train does."""
        if not self.model.training:  # (nn.Module.train() walks every submodule: ~10 us a 47 us step does not have)
            self.model.train()
        self.create_input_feed(input_feed, self.rank_list_size)
        eng = self._train_engine(self.batch_size, self.rank_list_size)
        eng.train_step(self.model.flat_params, self.state_sum, self.letor_features, self.n_docs, self.docid_inputs,
                       self.labels_LB, aux=self.bias_logits)
        self.loss = eng.read_loss()  # the only host sync: the reference's loss.item()
        self.global_step += 1
        print("Loss %f at global step %d" % (self.loss, self.global_step))
        return self.loss, None, self.train_summary
