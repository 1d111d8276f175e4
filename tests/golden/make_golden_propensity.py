#!/usr/bin/env python3
"""Golden propensity table of the reference's RandomizedPropensityEstimator, recorded by RUNNING it on the CPU.

The reference's estimateParametersFromModel (ultra/utils/propensity_estimator.py:95-132) is run once, with Python's `random`
seeded, on the click model pbm_0.1_1.0_4_1.0 (the JSON shipped in ultra_pytorch_amd/data/) and a small synthetic Raw_data:
50 label lists, lengths 1 .. 12 with every length present, labels 0 .. 4.  Its 10^7-session loop is hard-coded, so this
takes minutes of CPU.  Stored in propensity_ref.npz:

  labels      int32 [50, 12]   row q valid in [0, lengths[q]), 0 beyond
  lengths     int32 [50]
  IPW_list    float64 [12]     the reference's output
  seconds     float64          wall time of the reference's loop (sessions/s = sessions / seconds)
  sessions    int64            10^7, the reference's constant
  seed        int64            the seed given to random.seed

Usage:  python tests/golden/make_golden_propensity.py
"""
import json
import os
import random
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

N_LISTS, LMAX, SEED = 50, 12, 20260117
CLICK_MODEL_JSON = os.path.join(HERE, "..", "..", "ultra_pytorch_amd", "data", "pbm_0.1_1.0_4_1.0.json")


def make_label_lists():
    rng = np.random.RandomState(7)
    lens = list(range(1, LMAX + 1)) + [int(v) for v in rng.randint(1, LMAX + 1, size=N_LISTS - LMAX)]
    rng.shuffle(lens)
    return [[int(v) for v in rng.randint(0, 5, size=n)] for n in lens]


def main():
    with open(CLICK_MODEL_JSON) as f:
        desc = json.load(f)
    ultra = import_reference()
    from ultra.utils import click_models as CM
    from ultra.utils.propensity_estimator import RandomizedPropensityEstimator
    ds = ultra.utils.data_utils.Raw_data()
    ds.labels = make_label_lists()
    ds.initial_list_lengths = [len(x) for x in ds.labels]
    ds.rank_list_size = LMAX
    assert sorted(set(ds.initial_list_lengths)) == list(range(1, LMAX + 1))
    labels = np.zeros((N_LISTS, LMAX), np.int32)
    for q, lab in enumerate(ds.labels):
        labels[q, :len(lab)] = lab
    est = RandomizedPropensityEstimator()
    random.seed(SEED)
    t0 = time.time()
    est.estimateParametersFromModel(CM.loadModelFromJson(desc), ds)
    seconds = time.time() - t0
    # the reference shuffles a deep copy: the dataset's own lists are as recorded above
    assert all(list(labels[q, :len(lab)]) == lab for q, lab in enumerate(ds.labels))
    out = os.path.join(HERE, "propensity_ref.npz")
    np.savez(out, labels=labels, lengths=np.asarray(ds.initial_list_lengths, np.int32),
             IPW_list=np.asarray(est.IPW_list, np.float64), seconds=np.float64(seconds),
             sessions=np.int64(10_000_000), seed=np.int64(SEED))
    print("wrote %s: %.1f s, %.0f sessions/s" % (out, seconds, 1e7 / seconds))
    print("IPW_list", est.IPW_list)


if __name__ == "__main__":
    main()
