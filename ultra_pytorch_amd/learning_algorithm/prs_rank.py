"""PRSrank — propensity-ratio-scored LambdaRank: delta-NDCG-weighted pairwise BCE on the sorted list, each pair weighted by
ipw_i / ipw_j of the two presentation positions.  Drop-in for ultra.learning_algorithm.PRSrank (reference prs_rank.py:23-251)."""
from ..utils import HParams
from .base_algorithm import BaseAlgorithm
from .ipw_rank import PropensitySource, _LazyColumn, _LazyEstimatorWeights


class PRSrank(BaseAlgorithm):
    """The reference's train() also prints three debug tensors (the sorted ipw / pw of list 0 and its L x L prs matrix,
    prs_rank.py:129-136); they are not reproduced - each would force a device synchronisation inside the step.  The loss line
    is printed as the reference prints it, with the step number BEFORE the increment (0-based)."""
    ENGINE_ALGO = "prs"
    # prs_rank.py:43-50 (no l2_loss: a settings string that names one gets it reported and ignored, as there)
    DEFAULT_HPARAMS = dict(
        propensity_estimator_type="ultra.utils.propensity_estimator.RandomizedPropensityEstimator",
        propensity_estimator_json="./example/PropensityEstimator/randomized_pbm_0.1_1.0_4_1.0.json",
        learning_rate=0.05, max_gradient_norm=5.0, grad_strategy="ada", sigma=1.0)

    def __init__(self, data_set, exp_settings):
        self.hparams = HParams(**self.DEFAULT_HPARAMS)
        print(exp_settings["learning_algorithm_hparams"])
        self.hparams.parse(exp_settings["learning_algorithm_hparams"])
        self._check_hparams()
        self._setup(data_set, exp_settings)
        self.sigma = float(self.hparams.sigma)
        self.propensity = PropensitySource(self.hparams.propensity_estimator_type, self.hparams.propensity_estimator_json, self.cuda,
                                           all_positions=True)
        self.propensity_estimator = self.propensity.estimator
        self.IPW_list = self.propensity.IPW_list  # None for the Oracle: it has no table
        self.ipw_table = None if self.propensity.oracle else self.propensity._ipw_table
        self._pw_names = ["propensity_weights{0}".format(l) for l in range(self.max_candidate_num)]

    def _engine_kwargs(self):
        return dict(sigma=self.sigma)

    def train(self, input_feed):
        """prs_rank.py:94-176.  The per-list propensity loop (getPropensityForOneList with use_non_clicked_data=True) is folded
        into the loss kernel: ipw[l] = IPW_list[min(l, len - 1)] for every position (the Oracle on a user-browsing model: a weight per
        list entry from hip_ops.history_pw, ipw_rank.PropensitySource); the host feed still gets the `propensity_weights{l}` entries
        the reference adds (prs_rank.py:108-119)."""
        self.rank_list_size = self.exp_settings["selection_bias_cutoff"]
        if not self.model.training:
            self.model.train()
        L = self.rank_list_size
        clicks = self.create_input_feed(input_feed, L)  # None for a device feed
        if clicks is not None and self.propensity.oracle:  # the Oracle reads the list's clicks: materialised when first read
            lazy = _LazyEstimatorWeights(clicks.copy(), self.propensity)
            for l in range(L):
                input_feed[self._pw_names[l]] = _LazyColumn(lazy, l)
        elif clicks is not None:
            B, n = clicks.shape[1], len(self.IPW_list)
            for l in range(L):
                input_feed[self._pw_names[l]] = [self.IPW_list[min(l, n - 1)]] * B
        eng = self._train_engine(self.batch_size, L)
        ipw_table, pw = self.ipw_table, None
        if self.propensity.oracle:
            ipw_table, pw = self.propensity.step_weights(eng, self.labels_LB, L)
        eng.train_step(self.model.flat_params, self.state_sum, self.letor_features, self.n_docs, self.docid_inputs,
                       self.labels_LB, ipw_table=ipw_table, pw=pw)
        self.loss = eng.read_loss()
        print(" Loss %f at Global Step %d: " % (self.loss, self.global_step))
        self.global_step += 1
        return self.loss, None, self.train_summary
