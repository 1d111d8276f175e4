"""Click simulators (host side): position-biased, user-browsing and cascade models driven by Python's `random` stream, so that
a seeded run draws the same clicks as the reference's simulators (ultra/utils/click_models.py:7-16, 68-110, 113-186, 187-236):
one `random.random()` per list position, click iff u < exam_prob * click_prob[label].  TrustBiasModel is the project's own: the
one model here that leaves the examination hypothesis.  Below them: how a model reaches the GPU
(CLICK_MODEL_IDS, load_for_device, device_tables) - the device feeds, DBGD / MGD / NSGD and the propensity estimator all go through it."""
import json
import os
import random


class ClickModel(object):
    model_name = "click_model"

    def __init__(self, neg_click_prob=0.0, pos_click_prob=1.0, relevance_grading_num=1, eta=1.0):
        self.exam_prob = None
        self.setExamProb(eta)
        b = (pos_click_prob - neg_click_prob) / (pow(2, relevance_grading_num) - 1)
        a = neg_click_prob - b
        self.click_prob = [a + pow(2, i) * b for i in range(relevance_grading_num + 1)]

    def setExamProb(self, eta):
        self.eta = eta

    def getModelJson(self):
        return {"model_name": self.model_name, "eta": self.eta, "click_prob": self.click_prob, "exam_prob": self.exam_prob}

    def getExamProb(self, rank):
        return self.exam_prob[rank if rank < len(self.exam_prob) else -1]

    def sampleClick(self, rank, relevance_label):
        relevance_label = int(relevance_label) if relevance_label > 0 else 0
        exam_p = self.getExamProb(rank)
        click_p = self.click_prob[relevance_label if relevance_label < len(self.click_prob) else -1]
        return (1 if random.random() < exam_p * click_p else 0), exam_p, click_p


class PositionBiasedModel(ClickModel):
    model_name = "position_biased_model"
    ORIGINAL_EXAM_PROB = [0.68, 0.61, 0.48, 0.34, 0.28, 0.20, 0.11, 0.10, 0.08, 0.06]

    def setExamProb(self, eta):
        self.eta = eta
        self.exam_prob = [pow(x, eta) for x in self.ORIGINAL_EXAM_PROB]

    def sampleClicksForOneList(self, label_list):
        out = [self.sampleClick(rank, label) for rank, label in enumerate(label_list)]
        return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]

    def estimatePropensityWeightsForOneList(self, click_list, use_non_clicked_data=False):
        return [(1.0 / self.getExamProb(r) * self.getExamProb(0)) if (use_non_clicked_data or c > 0) else 0.0
                for r, c in enumerate(click_list)]


class TrustBiasModel(PositionBiasedModel):
    """Trust bias (Agarwal et al. 2019; Vardasbi et al. 2020): an examined document is clicked with a probability that depends on the
    rank as well as on its perceived relevance - trust_pos[k] (epsilon+) if perceived relevant, trust_neg[k] (epsilon-) if not:

        P(click | rank k, label y) = exam[k] * (trust_neg[k] + (trust_pos[k] - trust_neg[k]) * click_prob[y]) = alpha_k gamma + beta_k

    with gamma = click_prob[y], alpha_k = exam[k] (trust_pos[k] - trust_neg[k]), beta_k = exam[k] trust_neg[k].  The rank saturates
    at the tables' last entry and the label is clamped, as in the base class.  The default tables are this project's."""
    model_name = "trust_bias_model"

    def __init__(self, neg_click_prob=0.0, pos_click_prob=1.0, relevance_grading_num=1, eta=1.0, trust_pos=None, trust_neg=None):
        PositionBiasedModel.__init__(self, neg_click_prob, pos_click_prob, relevance_grading_num, eta)
        n = len(self.exam_prob)
        self.trust_pos = [1.0 - (r + 1) / 100 for r in range(n)] if trust_pos is None else [float(x) for x in trust_pos]
        self.trust_neg = [0.65 / (r + 1) for r in range(n)] if trust_neg is None else [float(x) for x in trust_neg]
        self.check_tables()

    def check_tables(self):
        """ValueError unless exam_prob, trust_pos and trust_neg have one length and 0 <= trust_neg[k] < trust_pos[k] <= 1."""
        if not (len(self.exam_prob) == len(self.trust_pos) == len(self.trust_neg)) or not self.exam_prob:
            raise ValueError("trust_bias_model: exam_prob, trust_pos and trust_neg must have one length, got %d, %d and %d"
                             % (len(self.exam_prob), len(self.trust_pos), len(self.trust_neg)))
        for k, (tp, tn) in enumerate(zip(self.trust_pos, self.trust_neg)):
            if not 0.0 <= tn < tp <= 1.0:
                raise ValueError("trust_bias_model: 0 <= trust_neg[k] < trust_pos[k] <= 1 does not hold at k = %d (%r, %r)" % (k, tn, tp))

    def getModelJson(self):
        desc = PositionBiasedModel.getModelJson(self)
        desc["trust_pos"], desc["trust_neg"] = self.trust_pos, self.trust_neg
        return desc

    def _rank(self, rank):
        return rank if rank < len(self.exam_prob) else len(self.exam_prob) - 1

    def sampleClick(self, rank, relevance_label):
        """(click, examination probability, click probability given examination): one random.random(), as the base class draws."""
        relevance_label = int(relevance_label) if relevance_label > 0 else 0
        k = self._rank(rank)
        exam_p = self.exam_prob[k]
        gamma = self.click_prob[relevance_label if relevance_label < len(self.click_prob) else -1]
        click_p = self.trust_neg[k] + (self.trust_pos[k] - self.trust_neg[k]) * gamma
        return (1 if random.random() < exam_p * click_p else 0), exam_p, click_p

    def affine_parameters(self, list_size):
        """(alpha[list_size], beta[list_size]) in Python floats: P(click at rank k) = alpha_k click_prob[label] + beta_k."""
        ks = [self._rank(r) for r in range(int(list_size))]
        return ([self.exam_prob[k] * (self.trust_pos[k] - self.trust_neg[k]) for k in ks],
                [self.exam_prob[k] * self.trust_neg[k] for k in ks])

    def estimateAffineWeightsForOneList(self, click_list):
        """The affine correction (c - beta_k) / alpha_k of every position, clicked or not: its expectation is click_prob[label]."""
        alpha, beta = self.affine_parameters(len(click_list))
        return [(c - b) / a for c, a, b in zip(click_list, alpha, beta)]


class UserBrowsingModel(ClickModel):
    """Examination depends on the rank AND on how far back the last click was (reference click_models.py:113-186): a triangular
    table exam[rank][distance - 1], distance = rank - last_click_rank (last_click_rank = -1 before the first click).  Beyond the
    table's last row the last row is reused: a distance that reaches back before the list start takes its last entry ("no click
    so far"), any other distance its own column, saturating at the second-to-last."""
    model_name = "user_browsing_model"
    RD_EXAM_TABLE = [
        [1.0],
        [0.98, 1.0],
        [1.0, 0.62, 0.95],
        [1.0, 0.77, 0.42, 0.82],
        [1.0, 0.92, 0.55, 0.31, 0.69],
        [1.0, 0.96, 0.63, 0.4, 0.22, 0.54],
        [1.0, 0.99, 0.73, 0.46, 0.29, 0.17, 0.47],
        [1.0, 1.0, 0.89, 0.52, 0.35, 0.24, 0.14, 0.43],
        [1.0, 1.0, 0.95, 0.68, 0.4, 0.29, 0.19, 0.12, 0.41],
        [1.0, 1.0, 1.0, 0.96, 0.52, 0.36, 0.27, 0.18, 0.12, 0.43],
    ]

    def setExamProb(self, eta):
        self.eta = eta
        self.exam_prob = [[pow(x, eta) for x in row] for row in self.RD_EXAM_TABLE]

    def getExamProb(self, rank, last_click_rank=-1):
        distance = rank - last_click_rank
        if rank < len(self.exam_prob):
            return self.exam_prob[rank][distance - 1]
        last = self.exam_prob[-1]
        if distance > rank:
            return last[-1]
        return last[distance - 1 if distance < len(last) - 1 else -2]

    def sampleClick(self, rank, last_click_rank, relevance_label):
        relevance_label = int(relevance_label) if relevance_label > 0 else 0
        exam_p = self.getExamProb(rank, last_click_rank)
        click_p = self.click_prob[relevance_label if relevance_label < len(self.click_prob) else -1]
        return (1 if random.random() < exam_p * click_p else 0), exam_p, click_p

    def sampleClicksForOneList(self, label_list):
        clicks, exams, cps, last = [], [], [], -1
        for rank, label in enumerate(label_list):
            click, exam_p, click_p = self.sampleClick(rank, last, label)
            last = rank if click > 0 else last
            clicks.append(click)
            exams.append(exam_p)
            cps.append(click_p)
        return clicks, exams, cps

    def estimatePropensityWeightsForOneList(self, click_list, use_non_clicked_data=False):
        out, last = [], -1
        for r, c in enumerate(click_list):
            out.append(1.0 / self.getExamProb(r, last) if (use_non_clicked_data or c > 0) else 0.0)
            last = r if c > 0 else last
        return out


class CascadeModel(ClickModel):
    model_name = "cascade_model"

    def setExamProb(self, eta):
        self.eta = eta
        self.exam_prob = [1.0 for _ in range(10)]

    def sampleClicksForOneList(self, label_list):
        clicks, exams, cps, has_click = [], [], [], False
        for rank, label in enumerate(label_list):
            click, exam_p, click_p = self.sampleClick(rank, label)  # the uniform is drawn even after a click
            clicks.append(0.0 if has_click else click)
            exams.append(0.0 if has_click else exam_p)
            cps.append(click_p)
            has_click = has_click or click > 0
        return clicks, exams, cps

    def estimatePropensityWeightsForOneList(self, click_list, use_non_clicked_data=False):
        return [(1.0 / self.getExamProb(r) * self.getExamProb(0)) if (use_non_clicked_data or c > 0) else 0.0
                for r, c in enumerate(click_list)]


def loadModelFromJson(model_desc):
    name = model_desc["model_name"]
    model = {"cascade_model": CascadeModel, "user_browsing_model": UserBrowsingModel,
             "trust_bias_model": TrustBiasModel}.get(name, PositionBiasedModel)()
    model.eta = model_desc["eta"]
    model.click_prob = model_desc["click_prob"]
    model.exam_prob = model_desc["exam_prob"]
    if name == "trust_bias_model":
        model.trust_pos, model.trust_neg = [float(x) for x in model_desc["trust_pos"]], [float(x) for x in model_desc["trust_neg"]]
        model.check_tables()
    return model


# The click models the GPU simulates (include/ultr_hip.h: ULTR_CLICK_PBM / _CASCADE / _UBM / _TRUST), and how one gets there.
CLICK_MODEL_IDS = {"position_biased_model": 0, "cascade_model": 1, "user_browsing_model": 2, "trust_bias_model": 3}


def load_for_device(path, who):
    """(desc, model, model_id) of the click-model JSON at `path`; a path that does not exist falls back to the file of that name in the
    package's data/ (the reference's defaults are relative to its repository root; the same files ship here).  `who` is the subject
    of the refusal of a model the GPU does not simulate."""
    if not os.path.exists(path):
        alt = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", os.path.basename(path))
        path = alt if os.path.exists(alt) else path
    with open(path) as fin:
        desc = json.load(fin)
    if desc["model_name"] not in CLICK_MODEL_IDS:
        raise NotImplementedError("%s simulates the position-biased, the cascade and the user-browsing model (and the trust-bias "
                                  "model)" % who)
    return desc, loadModelFromJson(desc), CLICK_MODEL_IDS[desc["model_name"]]


def device_tables(model, model_id, device):
    """(exam tensor, n_exam, cprob tensor) of `model` on `device` as the kernels read them: the examination table [n] for PBM /
    cascade, a dense [n][n] image of the triangular rank x distance table for the user-browsing model, a dense [2][n] image for the
    trust-bias model (row 0 alpha_k, row 1 beta_k: each the Python-float product rounded to float32 once); the click probabilities
    [n_rel]."""
    import torch
    ep = model.exam_prob
    n = len(ep)
    if model_id == CLICK_MODEL_IDS["user_browsing_model"]:
        ep = [[(row[c] if c < len(row) else 0.0) for c in range(n)] for row in ep]
    if model_id == CLICK_MODEL_IDS["trust_bias_model"]:
        ep = [list(x) for x in model.affine_parameters(n)]
    return (torch.tensor(ep, dtype=torch.float32, device=device).contiguous(), n,
            torch.tensor(model.click_prob, dtype=torch.float32, device=device))
