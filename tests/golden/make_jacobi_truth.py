"""Record, for every matrix of tests/jacobi_cases.py, its eigenvalues in long double (``compute_truth``: the round-robin
Jacobi restated in np.longdouble, minutes at n = 512) and what rt_host_jacobi_eigh achieves on it (``compute_host_reference``:
the three ratios and its sweep count; a second at n = 512) as tests/golden/jacobi_truth.npz:

    python -m tests.golden.make_jacobi_truth

``probe`` is a sample of the matrix, so that a test can tell that the matrix it builds is the one the record is of.  The
library must be built (the host routine is part of it).  tests/test_jacobi_eig_cpu.py recomputes the records of the small
matrices and holds the file to them."""
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from tests import jacobi_cases as jc


def record(case):
    kind, n = case
    G, _ = jc.matrix(kind, n)
    lam = jc.compute_truth(G)
    hi, lo = jc.split(lam)
    host = jc.compute_host_reference(G, lam)
    key = jc.label(kind, n)
    print(key, host, flush=True)
    return {key + "/hi": hi, key + "/lo": lo, key + "/probe": G[jc.PROBE].copy(),
            key + "/host": np.array([host["lam"], host["orth"], host["res"], host["sweeps"]])}


if __name__ == "__main__":
    out = {}
    todo = sorted(jc.cases(jc.GPU_SIZES), key=lambda c: -c[1])   # the long ones first
    with ProcessPoolExecutor(max_workers=8) as pool:
        for part in pool.map(record, todo):
            out.update(part)
    np.savez_compressed(jc.GOLDEN, **out)
