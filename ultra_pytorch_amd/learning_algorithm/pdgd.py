"""PDGD — Pairwise Differentiable Gradient Descent, the online learner of Oosterhuis & de Rijke (CIKM 2018).
Drop-in for ultra.learning_algorithm.PDGD (reference pdgd.py:27-215)."""
from .. import engine
from ..utils import HParams
from .base_algorithm import BaseAlgorithm


class PDGD(BaseAlgorithm):
    """Each clicked document is paired with every lower-labelled document above it and the one just below it; a pair is
    weighted by how likely the current model's Plackett-Luce ranking would show it the other way round, and the loss is the
    weighted sum of -e^{s_l} / (e^{s_l} + e^{s_k}).  The pair construction, the weights and the loss gradient at the list
    positions run in one HIP kernel (ultr_pdgd.hip), the rest of the step is the shared forward / backward / update.

    Defaults as pdgd.py:47-54.  `tau` is an int hyper-parameter there and here.  Unlike IPWrank and its siblings (SURVEY
    Appendix A.8), PDGD hands opt_step a FRESH model.parameters() after its L2 loop (pdgd.py:206-212), so the gradient, L2 term
    included, IS clipped at max_gradient_norm (1.0 by default) although l2_loss > 0 by default; ultr_apply_update does the same.

    Works with the DNN and Linear ranking models only.  The reference scores the pairs by running the model on two-document
    "lists" (get_ranking_scores on [positive, negative] docids); for a per-document model that equals the score at the list
    position, so the gradient can be taken there.  SetRank's score depends on the rest of the list, so for it the reference's
    pair scores are a different function of the parameters than the list forward: it is refused."""
    ENGINE_ALGO = "pdgd"
    DEFAULT_HPARAMS = dict(learning_rate=0.05, tau=1, max_gradient_norm=1.0, l2_loss=0.005, grad_strategy="ada")

    def __init__(self, data_set, exp_settings):
        print("Build Pairwise Differentiable Gradient Descent (PDGD) algorithm.")
        self.hparams = HParams(**self.DEFAULT_HPARAMS)
        print(exp_settings["learning_algorithm_hparams"])
        self.hparams.parse(exp_settings["learning_algorithm_hparams"])
        self._check_hparams()
        self._setup(data_set, exp_settings)
        if getattr(self.model, "step_engine_cls", engine.StepEngine) is not engine.StepEngine:
            raise NotImplementedError(
                "PDGD supports the DNN and Linear ranking models only: the reference scores its pairs with the model on "
                "two-document lists, which for %s is a different function of the parameters than the list forward"
                % type(self.model).__name__)
        if not hasattr(self, "rank_list_size"):
            self.rank_list_size = self.max_candidate_num
        self.tau = float(self.hparams.tau)

    def _engine_kwargs(self):
        return dict(sigma=self.tau, cutoff=int(self.rank_list_size))

    def train(self, input_feed):
        """pdgd.py:97-192: the forward covers max_candidate_num positions (a DeviceClickFeed batch: its own L), the pairs stop at
        selection_bias_cutoff.  The loss line is printed with global_step AFTER the increment, as there."""
        if not self.model.training:
            self.model.train()
        if input_feed.get("device_feed", False):
            L = int(input_feed["docids"].shape[0])
        else:
            L = self.max_candidate_num
        self.create_input_feed(input_feed, L)
        eng = self._train_engine(self.batch_size, L)
        eng.train_step(self.model.flat_params, self.state_sum, self.letor_features, self.n_docs, self.docid_inputs,
                       self.labels_LB)
        self.loss = eng.read_loss()
        self.global_step += 1
        print(" Loss %f at Global Step %d: " % (self.loss, self.global_step))
        return self.loss, None, self.train_summary
