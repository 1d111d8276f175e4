"""DBGD and MGD - Dueling Bandit Gradient Descent (Yue & Joachims, ICML 2009) and Multileave Gradient Descent (Schuth et al.,
WSDM 2016), the weight-perturbing online learners.  Drop-in for ultra.learning_algorithm.DBGD / MGD (reference dbgd.py:27-330,
mgd.py:23-232, team_draft_interleave.py)."""
import torch

from .. import engine
from ..utils import HParams
from ..utils import click_models
from .base_algorithm import BaseAlgorithm

CLICK_MODEL_IDS = click_models.CLICK_MODEL_IDS


class DBGD(BaseAlgorithm):
    """Each step perturbs the Linear parameters of the current model along R random unit directions (R = 1 here, ranker_num for
    MGD), scores the batch with the current model and every candidate, and lets simulated users pick the winners: per list a
    team-draft multileave of the R + 1 rankings, clicks from this algorithm's own click model on the labels in that order, and each
    ranker's share of the clicks.  The model then steps toward the winning directions.  Without interleaving the winners are the
    candidates whose batch NDCG beats the current model's.  The noise, the multileave, the clicks and the gradient run as HIP kernels
    (csrc/ultr_dbgd.hip) around one validation forward per ranker; clip and optimizer are the shared update (engine.DbgdEngine).

    Defaults as dbgd.py:47-56, plus `tau` (int, default 1) - the Plackett-Luce temperature of interleave_strategy='Stochastic', which
    the reference reads but never defines.  Kept and changed quirks: DESIGN.md section 8.  Works with the DNN and Linear ranking
    models; SetRank and data parallelism are refused."""
    ENGINE_ALGO = "dbgd"
    INTERLEAVES_IN_TRAIN = True  # the online feeds accept need_interleave=True from this algorithm
    MAX_SAMPLE_ROUND_NUM = 100
    DEFAULT_HPARAMS = dict(click_model_json="./example/ClickModel/pbm_0.1_1.0_4_1.0.json", learning_rate=0.5,
                           max_gradient_norm=5.0, need_interleave=True, interleave_strategy="Stochastic", grad_strategy="sgd", tau=1)
    BANNER = "Build Dueling Bandit Gradient Descent (DBGD) algorithm."

    def __init__(self, data_set, exp_settings):
        print(self.BANNER)
        self.hparams = HParams(**self.DEFAULT_HPARAMS)
        print(exp_settings["learning_algorithm_hparams"])
        self.hparams.parse(exp_settings["learning_algorithm_hparams"])
        if exp_settings.get("process_group", None) is not None:
            raise NotImplementedError("%s runs on one GPU: data-parallel training is not implemented" % type(self).__name__)
        self._check_hparams()
        self._setup(data_set, exp_settings)
        if getattr(self.model, "step_engine_cls", engine.StepEngine) is not engine.StepEngine:
            raise NotImplementedError("%s supports the DNN and Linear ranking models only (its candidates perturb the Linear "
                                      "parameters of the flat DNN layout), not %s" % (type(self).__name__, type(self.model).__name__))
        if not hasattr(self, "rank_list_size"):
            self.rank_list_size = self.max_candidate_num
        self.n_rankers = int(getattr(self.hparams, "ranker_num", 1))  # R candidates: DBGD 1, MGD ranker_num
        self.winners_name = "winners"
        self.interleaving_strategy = self.hparams.interleave_strategy
        self.rng_seed = int(torch.initial_seed())  # the step's draws: Philox(rng_seed, global_step)
        self._load_click_model()

    def _load_click_model(self):
        _, self.click_model, self.click_model_id = click_models.load_for_device(self.hparams.click_model_json, type(self).__name__)
        self.exam, self.n_exam, self.cprob = click_models.device_tables(self.click_model, self.click_model_id, self.cuda)

    def _optimizer(self):
        return "sgd" if self.hparams.grad_strategy == "sgd" else "ada"  # (engine.DbgdEngine knows these two)

    def _dbgd_engine(self, B, M):
        key = (B, M)
        eng = self._train_engines.get(key)
        if eng is None:
            eng = self._train_engines[key] = self._make_engine(
                self.model.shape, B, M, min(int(self.rank_list_size), M), self.n_rankers, self.cuda,
                need_interleave=bool(self.hparams.need_interleave), stochastic=self.interleaving_strategy == "Stochastic",
                tau=float(self.hparams.tau), noise_rate=float(self.hparams.learning_rate), learning_rate=self.learning_rate,
                max_gradient_norm=float(self.hparams.max_gradient_norm),
                optimizer=self._optimizer(), click_model=self.click_model_id,
                exam=self.exam, n_exam=self.n_exam, cprob=self.cprob, seed=self.rng_seed, max_redraws=self.MAX_SAMPLE_ROUND_NUM)
            while len(self._train_engines) > self.MAX_ENGINES:
                self._train_engines.popitem(last=False)
        else:
            self._train_engines.move_to_end(key)
        return eng

    def _make_engine(self, *args, **kw):
        return engine.DbgdEngine(*args, **kw)

    def train(self, input_feed):
        """dbgd.py:125-187: every list of max_candidate_num positions (a device feed: its own length); the loss is
        1 - NDCG@rank_list_size of the current model on the feed's labels, PADs unmasked, as a batch mean."""
        if not self.model.training:
            self.model.train()
        if input_feed.get("device_feed", False):
            M = int(input_feed["docids"].shape[0])
        else:
            M = self.max_candidate_num
        self.create_input_feed(input_feed, M)
        eng = self._dbgd_engine(self.batch_size, M)
        eng.train_step(self.model.flat_params, self.state_sum, self.letor_features, self.n_docs, self.docid_inputs, self.labels_LB,
                       step=self.global_step)
        self.loss = eng.read_loss()
        self._report()
        return self.loss, None, self.train_summary

    def _report(self):
        print(" Loss %f at Global Step %d: " % (self.loss, self.global_step))  # dbgd.py:184-185: printed, then counted
        self.global_step += 1


class MGD(DBGD):
    """MGD: DBGD with ranker_num candidates, multileaved (mgd.py:23-232).  The reference cannot construct it (is_cuda_avail is never
    set) nor train it (input_feed["winners"], click_simulation_winners called with the wrong arguments); here it is DBGD's step with
    R = ranker_num, and it takes DBGD's interleave_strategy, tau and click_model_json as well."""
    DEFAULT_HPARAMS = dict(DBGD.DEFAULT_HPARAMS, ranker_num=4)
    BANNER = "Build Multileave Gradient Descent (DBGD) algorithm."

    def _report(self):
        self.global_step += 1  # mgd.py:130-131: counted, then printed
        print(" Loss %f at Global Step %d: " % (self.loss, self.global_step))
