"""Record the oracle's POD of the 2200 x 2048 set of tests/test_wide_eig_gpu.py (oracle.orth: dgesvd, about a minute
on 16 cores - too long to repeat in every run of the suite) as tests/golden/wide_eig_limit_2048.npz:

    python -m tests.golden.make_wide_eig

``probe`` is a sample of the input, so that the test can tell that the set it builds is the set this reference is of."""
import os

import numpy as np

from oracle import romtime_oracle as oracle
from tests.test_wide_eig_gpu import LIMIT_KW, PROBE, _input

if __name__ == "__main__":
    X = _input("limit_2048")
    Q, s, energy = oracle.orth(X, **LIMIT_KW)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "wide_eig_limit_2048.npz"), Q=Q, s=s,
                        energy=energy, probe=X[PROBE].copy())
