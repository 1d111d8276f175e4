"""PLRank — counterfactual learning of a ranking metric itself: the ranker's scores are a Plackett-Luce policy and a step follows the
sampled, low-variance policy gradient of PL-Rank (Oosterhuis, SIGIR 2021) of the expected DCG@K, with the IPW-weighted clicks as
relevance estimates.  The project's own algorithm - the reference has no such class.

    reward of a list = E_{y ~ PL(scores)} [ sum_{k < K} rho_{y_k} / log2(k + 2) ],   rho_l = w_l * gain(click_l)
    loss             = minus the mean over lists of the reward, estimated from num_samples sampled rankings per list

w_l is IPWrank's weight (the estimator's table, or the Oracle estimator's per-click weight), gain is the click itself (`linear`) or
2^y - 1 for graded labels (`exp2`, with DirectLabelFeed).  Sampling, the four scans per sample and the gradient run in one kernel
(ultr_plrank_loss); the law is DESIGN.md section 4d.  Data parallelism is not part of it."""
import torch

from .. import _lib
from ..utils import HParams
from .base_algorithm import BaseAlgorithm
from .ipw_rank import PropensitySource


class PLRank(BaseAlgorithm):
    ENGINE_ALGO = "plrank"

    @staticmethod
    def parse_hparams(hparam_string):
        """The algorithm's hyper-parameters from a settings string (needs no GPU).  An unknown gain, or num_samples outside
        1 .. 4095, raises ValueError."""
        hp = HParams(propensity_estimator_type="ultra.utils.propensity_estimator.RandomizedPropensityEstimator",
                     propensity_estimator_json="./example/PropensityEstimator/randomized_pbm_0.1_1.0_4_1.0.json",
                     learning_rate=0.05, max_gradient_norm=5.0, l2_loss=0.0, grad_strategy="ada", num_samples=64, cutoff=0,
                     gain="linear")
        hp.parse(hparam_string)
        if hp.gain not in _lib.PLRANK_GAIN:
            raise ValueError("gain must be one of %s, got %r" % (sorted(_lib.PLRANK_GAIN), hp.gain))
        if not 1 <= int(hp.num_samples) <= _lib.PLRANK_MAX_SAMPLES:
            raise ValueError("num_samples must be in 1 .. %d, got %r" % (_lib.PLRANK_MAX_SAMPLES, hp.num_samples))
        if int(hp.cutoff) < 0:
            raise ValueError("cutoff must be >= 0 (0: the whole list), got %r" % (hp.cutoff,))
        return hp

    def __init__(self, data_set, exp_settings):
        print("Build the Plackett-Luce policy-gradient ranker (PL-Rank).")
        print(exp_settings["learning_algorithm_hparams"])
        self.hparams = self.parse_hparams(exp_settings["learning_algorithm_hparams"])
        if exp_settings.get("process_group", None) is not None:
            raise NotImplementedError("PLRank does not train data parallel: run it without a process_group")
        self._setup(data_set, exp_settings)
        self.propensity = PropensitySource(self.hparams.propensity_estimator_type, self.hparams.propensity_estimator_json, self.cuda,
                                           all_positions=False)
        self.ipw_table = None if self.propensity.oracle else self.propensity._ipw_table
        # the draws of step t: Philox(rng_seed, t), t counted here beside the model - engines come and go with the batch shapes
        self.rng_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF  # as DBGD keys its noise
        self.draw_steps = 0

    def _engine_kwargs(self):
        return dict(num_samples=int(self.hparams.num_samples), cutoff=int(self.hparams.cutoff), gain=self.hparams.gain,
                    rng_seed=self.rng_seed)

    def train(self, input_feed):
        """One step: forward, the sampled policy gradient, backward, update; global_step is incremented after the step."""
        if not self.model.training:  # (nn.Module.train() walks every submodule: ~10 us a 47 us step does not have)
            self.model.train()
        L = self.rank_list_size
        self.create_input_feed(input_feed, L)
        eng = self._train_engine(self.batch_size, L)
        eng.set_draw_step(self.draw_steps)
        self.draw_steps += 1
        ipw_table, pw = self.ipw_table, None
        if self.propensity.oracle:
            ipw_table, pw = self.propensity.step_weights(eng, self.labels_LB, L)
        eng.train_step(self.model.flat_params, self.state_sum, self.letor_features, self.n_docs, self.docid_inputs, self.labels_LB,
                       ipw_table=ipw_table, pw=pw)
        self.loss = eng.read_loss()  # the only host sync: the reference's loss.item()
        self.global_step += 1
        print("Loss %f at global step %d" % (self.loss, self.global_step))
        return self.loss, None, self.train_summary
