"""Writes tests/golden/metrics_frozen.npz: the output bits of the metric launches at the cases of tests/test_gpu_metrics_frozen.py,
which owns the cases and the code that runs one (that test compares a later library with this file).  Needs the GPU and the built
library; run it from a tree whose metric kernels are the ones to freeze:
    python tests/golden/make_metrics_frozen.py
Keys are "<case id>/<means | per_list | order | masked | host_report>"; float outputs are stored as their uint32 views."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import test_gpu_metrics_frozen as T  # noqa: E402


def main():
    out = {}
    for case in T.CASES:
        for what, a in T.run_case(case).items():
            out["%s/%s" % (T.case_id(case), what)] = a
    np.savez_compressed(T.FIXTURE, **out)
    size = os.path.getsize(T.FIXTURE)
    assert size < 256 * 1024, "the fixture is %d bytes" % size
    print("wrote %s: %d arrays of %d cases, %d bytes" % (T.FIXTURE, len(out), len(T.CASES), size))


if __name__ == "__main__":
    main()
