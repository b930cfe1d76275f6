"""Record the oracle's greedy on the 1040 x 1024 basis of tests/test_deim_truth_gpu.py's size limit (oracle.deim_greedy:
1023 dense solves, about 10 s - and a long-double certificate of it some 20 s, too long to repeat in every run of the
suite) as tests/golden/deim_limit_1024.npz:

    python -m tests.golden.make_deim_limit

``probe`` is a sample of the input, so that the tests can tell that the basis they build is the basis this record is of.
No step may be a near-tie: the device has to return these very indices."""
import os

import numpy as np

from oracle import romtime_oracle as oracle
from tests import deim_cases as dc

if __name__ == "__main__":
    B = dc.basis(**dc.LIMIT)
    dofs, _, margin = oracle.deim_greedy(B)
    print("smallest margin", margin.min(), "multiplier bound - 1", dc.multiplier_bound(B, dofs) - 1.0)
    assert margin.min() > 1e-6, "a near-tie: take another seed in tests.deim_cases.LIMIT"
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "deim_limit_1024.npz"), dofs=dofs,
                        margin=margin, probe=B[dc.LIMIT_PROBE].copy(), **dc.LIMIT)
