"""Inverse-propensity tables (reference ultra/utils/propensity_estimator.py): a JSON file with "IPW_list", loaded by IPWrank and
PRSrank, and the estimators that make one: RandomizedPropensityEstimator runs the reference's randomized click experiment
(:95-132) on the GPU (ultr_propensity_count: the session loop, the shuffle and the click histogram are one HIP kernel), the
OraclePropensityEstimator (:149-180) answers from the click model itself (weight_table: what IPWrank / PRSrank upload).

    python -m ultra_pytorch_amd.utils.propensity_estimator <click_model.json> <data_dir> <output_dir> [--sessions N] [--seed S]

writes <output_dir>/randomized_<click model file stem>.json, as the reference's main() does."""
import argparse
import json
import os

from . import click_models as CM

CLICK_MODEL_IDS = CM.CLICK_MODEL_IDS
SESSIONS_PER_CALL = 1 << 24  # sessions per ultr_propensity_count call: the counter is (seed, session), the split changes nothing


class BasicPropensityEstimator(object):
    def __init__(self, file_name=None):
        self.IPW_list = []
        if file_name:
            self.loadEstimatorFromFile(file_name)

    def getPropensityForOneList(self, click_list, use_non_clicked_data=False):
        """weight_r = IPW_list[min(r, len-1)] if clicked (or use_non_clicked_data) else 0   (:22-42)"""
        last = len(self.IPW_list) - 1
        return [self.IPW_list[min(r, last)] if (use_non_clicked_data or c > 0) else 0.0 for r, c in enumerate(click_list)]

    def loadEstimatorFromFile(self, file_name):
        with open(file_name) as f:
            self.IPW_list = json.load(f)["IPW_list"]

    def outputEstimatorToFile(self, file_name):
        with open(file_name, "w") as f:
            f.write(json.dumps({"IPW_list": self.IPW_list}, indent=4, sort_keys=True))


def ipw_from_click_count(click_count):
    """The reference's table from its counts (:119-131): click_count[y][x] = clicks on position x of lists of length y + 1;
    first[x] = sum_{y >= x} click_count[y][0], agg[x] = sum_{y >= x} click_count[y][x],
    IPW_list[x] = min(first[x] / (agg[x] + 10e-6), first[x]) in Python floats from the integer counts."""
    n = len(click_count)
    first, agg = [0] * n, [0] * n
    for x in range(n):
        for y in range(x, n):
            first[x] += int(click_count[y][0])
            agg[x] += int(click_count[y][x])
    return [min(first[x] / (agg[x] + 10e-6), first[x]) for x in range(n)]


class RandomizedPropensityEstimator(BasicPropensityEstimator):
    """The table estimated from randomized click sessions (:69-146), or loaded from a file that holds one.  Under the trust-bias
    model the experiment estimates the examination-only table (clicks on position 0 over clicks on position x): the weights that
    are biased under that model whatever the table, kept as the baseline the affine correction is held against."""

    def __init__(self, file_name=None):
        self.click_model = None
        BasicPropensityEstimator.__init__(self, file_name)

    def loadEstimatorFromFile(self, file_name):
        with open(file_name) as f:
            data = json.load(f)
        self.click_model = CM.loadModelFromJson(data["click_model"]) if "click_model" in data else None
        self.IPW_list = data["IPW_list"]

    def estimateParametersFromModel(self, click_model, data_set, session_num=10_000_000, seed=0, device=None):
        """session_num times on the GPU: pick a label list of data_set uniformly, shuffle it, sample clicks with click_model, count
        them by (list length, position); then IPW_list[x] = clicks on position 0 / clicks on position x over the lists that have a
        position x.  Sets click_model, IPW_list (length data_set.rank_list_size) and click_count (int64 [L, L] numpy)."""
        import numpy as np
        import torch
        from .. import hip_ops
        if getattr(click_model, "model_name", None) not in CLICK_MODEL_IDS:
            raise NotImplementedError("RandomizedPropensityEstimator simulates the position-biased, the cascade and the user-browsing model "
                                      "(and the trust-bias model)")
        L, label_lists = int(data_set.rank_list_size), data_set.labels
        if any(len(x) > L for x in label_lists):
            raise ValueError("a label list is longer than rank_list_size = %d" % L)
        if not label_lists or L <= 0 or session_num < 0:
            raise ValueError("estimateParametersFromModel needs at least one label list, rank_list_size > 0 and session_num >= 0")
        if not torch.cuda.is_available():
            raise RuntimeError("RandomizedPropensityEstimator.estimateParametersFromModel needs a GPU; there is no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        labels = np.zeros((len(label_lists), L), np.float32)
        for q, lab in enumerate(label_lists):
            labels[q, :len(lab)] = lab
        model_id = CLICK_MODEL_IDS[click_model.model_name]
        with torch.cuda.device(device):
            d_labels = torch.tensor(labels, device=device)
            d_lengths = torch.tensor([len(x) for x in label_lists], dtype=torch.int32, device=device)
            d_exam, n_exam, d_cprob = CM.device_tables(click_model, model_id, device)
            d_count = torch.zeros(L, L, dtype=torch.int64, device=device)
            for first in range(0, int(session_num), SESSIONS_PER_CALL):
                hip_ops.propensity_count(d_labels, d_lengths, d_exam, n_exam, d_cprob, model_id, seed, first,
                                         min(SESSIONS_PER_CALL, int(session_num) - first), d_count)
            self.click_count = d_count.cpu().numpy()
        self.click_model = click_model
        self.IPW_list = ipw_from_click_count(self.click_count)

    def outputEstimatorToFile(self, file_name):
        with open(file_name, "w") as f:
            f.write(json.dumps({"click_model": self.click_model.getModelJson(), "IPW_list": self.IPW_list}, indent=4, sort_keys=True))


class OraclePropensityEstimator(BasicPropensityEstimator):
    """The click model's own weights (:149-180): no table to estimate.  Built from a click-model object or from the path of a JSON
    file with a "click_model" entry - what outputEstimatorToFile writes, and what a randomized_*.json carries next to its table.
    (Changed: the reference's find_class(type)(json_path) hands the file NAME to the constructor as its click model)

    An examination probability of 0 at an entry a list can reach raises ValueError here: the step would divide by it."""

    def __init__(self, click_model):
        if isinstance(click_model, (str, bytes, os.PathLike)):
            self.loadEstimatorFromFile(os.fspath(click_model))
        else:
            self.click_model = click_model
            if click_model is not None:  # (None: an empty estimator for loadEstimatorFromFile, as the base class allows)
                self._check()

    def loadEstimatorFromFile(self, file_name):
        with open(file_name) as f:
            data = json.load(f)
        if "click_model" not in data:
            raise KeyError("%s has no \"click_model\" entry: OraclePropensityEstimator needs the click model itself" % file_name)
        self.click_model = CM.loadModelFromJson(data["click_model"])
        self._check()

    def _check(self):
        name = getattr(self.click_model, "model_name", None)
        if name not in CLICK_MODEL_IDS:
            raise NotImplementedError("OraclePropensityEstimator answers for the position-biased, the cascade and the user-browsing "
                                      "model, and for the trust-bias model (got %r)" % name)
        ep = self.click_model.exam_prob
        used = [x for row in ep for x in row] if name == "user_browsing_model" else list(ep)
        if any(float(x) == 0.0 for x in used):
            raise ValueError("the click model has an examination probability of 0: its inverse propensity weight is undefined")

    def weight_table(self, list_size):
        """The weights of every list of `list_size` positions as float32 numpy, each entry the reference's own expression in Python
        floats rounded to float32 once (what torch.as_tensor(list of floats) does, ipw_rank.py:138, prs_rank.py:116):
          position-biased / cascade / trust-bias (its examination-only weights, PBM's expression):
                                     ("position", w[list_size]),            w[r] = 1.0 / getExamProb(r) * getExamProb(0)
          user-browsing:             ("history", w[list_size, list_size]),  w[r][c] = 1.0 / getExamProb(r, c - 1) for c <= r, else 0
        (row = rank, column = rank of the last click before it + 1, column 0 = no click so far).  getExamProb fills the table, so
        its rules for ranks beyond the model's rows (click_models.py:174-185) are expanded here and the GPU only looks up."""
        import numpy as np
        cm, L = self.click_model, int(list_size)
        if L <= 0:
            raise ValueError("list_size must be positive")
        if cm.model_name == "user_browsing_model":
            w = np.zeros((L, L), np.float32)
            for r in range(L):
                for c in range(r + 1):
                    w[r, c] = np.float32(1.0 / cm.getExamProb(r, c - 1))
            return "history", w
        return "position", np.asarray([1.0 / cm.getExamProb(r) * cm.getExamProb(0) for r in range(L)], np.float32)

    def affine_table(self, list_size):
        """(alpha[list_size], beta[list_size]) as float32 numpy: P(click at rank k) = alpha_k click_prob[label] + beta_k, what the
        affine correction (c - beta_k) / alpha_k of AffineRank divides by and subtracts.  The trust-bias model gives its two rows
        (each the Python-float product rounded to float32 once), the position-biased model (exam[k], 0).  The cascade and the
        user-browsing model raise NotImplementedError: their examination depends on the clicks of the list, no position table holds it."""
        import numpy as np
        cm, L = self.click_model, int(list_size)
        if L <= 0:
            raise ValueError("list_size must be positive")
        if cm.model_name == "trust_bias_model":
            alpha, beta = cm.affine_parameters(L)
        elif cm.model_name == "position_biased_model":
            alpha, beta = [cm.getExamProb(r) for r in range(L)], [0.0] * L
        else:
            raise NotImplementedError("affine_table: the examination of the %s depends on the clicks of the list" % cm.model_name)
        return np.asarray(alpha, np.float32), np.asarray(beta, np.float32)

    def getPropensityForOneList(self, click_list, use_non_clicked_data=False):
        return self.click_model.estimatePropensityWeightsForOneList(click_list, use_non_clicked_data)

    def outputEstimatorToFile(self, file_name):
        with open(file_name, "w") as f:
            f.write(json.dumps({"click_model": self.click_model.getModelJson()}, indent=4, sort_keys=True))


def main(argv=None):
    from . import data_utils
    ap = argparse.ArgumentParser(prog="python -m ultra_pytorch_amd.utils.propensity_estimator",
                                 description="Estimate an inverse-propensity table from randomized click sessions on the GPU.")
    ap.add_argument("click_model_json")
    ap.add_argument("data_dir")
    ap.add_argument("output_dir")
    ap.add_argument("--sessions", type=int, default=10_000_000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    os.makedirs(args.output_dir, exist_ok=True)  # before the run, not after 10^7 sessions
    print("Load data from " + args.data_dir)
    train_set = data_utils.read_data(args.data_dir, "train")
    with open(args.click_model_json) as fin:
        click_model = CM.loadModelFromJson(json.load(fin))
    print("Estimating...")
    estimator = RandomizedPropensityEstimator()
    estimator.estimateParametersFromModel(click_model, train_set, session_num=args.sessions, seed=args.seed)
    print("Output results...")
    stem = os.path.splitext(os.path.basename(args.click_model_json))[0]
    output_file = os.path.join(args.output_dir, "randomized_" + stem + ".json")
    estimator.outputEstimatorToFile(output_file)
    print(output_file)


if __name__ == "__main__":
    main()
