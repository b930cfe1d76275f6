"""Writes tests/golden/eig_lapack.json: the figures of ``np.linalg.eigh`` (LAPACK, the reference's library) on every
matrix of the tridiagonal eigensolver's truth tests, measured by ``tests.eig_cases.measure`` over
``tests.eig_cases.columns(n)``.  The device's bars are four times the larger of 1 and these (at most 20); the host test
recomputes the sizes up to 257 and holds the record to them.  Run from the repository root:

    python -m tests.golden.make_eig_lapack
"""
import json

import numpy as np

from tests import eig_cases as ec


def main():
    figures = {}
    for label in ec.all_labels():
        got = ec.compute_lapack_reference(label)
        figures[label] = {key: round(float(got[key]), 6) for key in ec.FIGURES if key in got}
        print(ec.format_line("EIG-LAPACK", label, got, got), flush=True)
    with open(ec.GOLDEN, "w") as fh:
        json.dump(dict(numpy=np.__version__, figures=figures), fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
