"""The device Jacobi eigensolver (csrc/symjacobi.hip, rt_sym_jacobi_eigh) as far as a host without a GPU can check it:
the entry point in the header, the binding table and the library; its argument check; the round-robin order; and the
premises the GPU bars rest on - the NumPy restatement of the kernel's arithmetic (tests/jacobi_cases.py) against the
long-double truth, next to rt_host_jacobi_eigh on the same matrices, whose figures are the reference of those bars.

Figures of rt_host_jacobi_eigh on these matrices (n = 7, 64, 129; graded with delta 1e-3 and 1e-1, the 1e-6 cluster, the
singular tail), in units of n eps: eigenvalues 0.046 ... 0.150, |W^T W - I| 0.342 ... 0.699, residual 0.007 ... 0.113;
2 to 4 sweeps by its own count (which leaves the closing sweep out).  The restatement: 0.054 ... 0.179, 0.278 ... 1.017,
0.009 ... 0.037; 4 or 5 sweeps with the closing one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import jacobi_cases as jc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG = -1


def _read(*parts):
    with open(os.path.join(REPO, *parts)) as fh:
        return fh.read()


# ---- binding and limits -----------------------------------------------------------------------------------------------
def test_header_binding_table_and_version_carry_the_entry_point():
    from romtime_amd import _lib

    header = _read("include", "romtime_hip.h")
    decl = re.search(r"int rt_sym_jacobi_eigh\(([^;]*)\);", header)
    assert decl, "include/romtime_hip.h does not declare rt_sym_jacobi_eigh"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert args == ["rt_ctx* ctx", "const double* A", "int64_t n", "double* lam", "double* W", "int max_sweeps",
                    "int* sweeps_done", "int* status"], args
    doc = header[header.index("Two-sided Jacobi eigen-decomposition"):decl.start()]
    assert "1 <= n <= 2048" in doc and "RT_ERR_UNSUPPORTED" in doc and "rt_last_launch_info" in doc
    res, argtypes = _lib.SIGNATURES["rt_sym_jacobi_eigh"]
    assert res is C.c_int and len(argtypes) == 8
    assert argtypes[2] is C.c_int64 and argtypes[5] is C.c_int and argtypes[6] == C.POINTER(C.c_int)
    assert "rt_host_jacobi_eigh" in _lib.SIGNATURES and "int rt_host_jacobi_eigh(" in header    # the host routine stays
    assert int(re.search(r"int rt_version\(void\) \{ return (\d+); \}", _read("romtime_amd", "csrc", "api.hip")).group(1)) >= 360
    assert "symjacobi.hip" in _read("romtime_amd", "build.py")


def test_library_exports_the_entry_point_and_refuses_a_null_ctx():
    """Without a GPU no ctx can be made: the null-ctx refusal is the argument check that runs here (the others, and the
    n > 2048 refusal with the limit in rt_last_error, need a ctx: tests/test_jacobi_eig_gpu.py)."""
    from romtime_amd import _lib, ops, pod

    lib = _lib.load()
    assert lib.rt_version() >= 360
    assert hasattr(lib, "rt_sym_jacobi_eigh")
    buf = np.zeros(4)
    sweeps = C.c_int(-7)
    rc = lib.rt_sym_jacobi_eigh(None, buf.ctypes.data, 2, buf.ctypes.data, buf.ctypes.data, 60, C.byref(sweeps), buf.ctypes.data)
    assert rc == RT_ERR_ARG and sweeps.value == -7 and not buf.any()
    assert callable(pod.jacobi_eigh) and callable(ops.sym_jacobi_eigh)


# ---- the order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 64, 65, 129, 130])
def test_round_robin_order(n):
    """n - 1 rounds for even n, n for odd n; the pairs of a round are disjoint and cover every index; a sweep meets
    every pair once; for odd n exactly one pair per round holds the idle index n; and the columns of consecutive pairs
    are consecutive (one wrap per side aside) - what makes a wave's accesses whole lines."""
    m = n + n % 2
    rs = list(jc.rounds(n))
    assert len(rs) == (n - 1 if n % 2 == 0 else n) == m - 1
    met = set()
    for p, q in rs:
        both = np.r_[p, q]
        assert sorted(both) == list(range(m))
        assert int(np.sum(both >= n)) == n % 2
        for a, b in zip(p, q):
            key = (min(a, b), max(a, b))
            assert key not in met
            met.add(key)
        if len(p) > 2:
            assert np.sum(np.diff(p[1:]) != 1) <= 1 and np.sum(np.diff(q[1:]) != -1) <= 1
    assert len(met) == m * (m - 1) // 2


# ---- the restatement and the host routine against the truth ---------------------------------------------------------------
@pytest.mark.parametrize("kind,n", jc.cases(jc.CPU_SIZES), ids=[jc.label(k, n) for k, n in jc.cases(jc.CPU_SIZES)])
def test_restatement_and_host_routine_against_the_truth(kind, n):
    """The premises of the GPU bars.  The long-double truth and the host routine's figures are recomputed and the record
    (tests/golden/jacobi_truth.npz) is held to them; the restated kernel arithmetic meets the bars the device is held to
    (four times the larger of 1 and the host's ratio, at most 20; at most two sweeps more than the host); every sweep
    leaves the work matrix exactly symmetric."""
    G, _ = jc.matrix(kind, n)
    truth = jc.compute_truth(G)
    host = jc.compute_host_reference(G, truth)
    print(f"JACOBI-HOST {jc.label(kind, n)} lam={host['lam']:.3f} orth={host['orth']:.3f} res={host['res']:.3f} "
          f"sweeps={host['sweeps']}")
    recorded = jc.truth(kind, n)
    assert np.array_equal(recorded, truth), "the recorded truth is not the truth of this matrix"
    rec_host = jc.host_reference(kind, n)
    assert rec_host["sweeps"] == host["sweeps"]
    for key in ("lam", "orth", "res"):
        assert abs(rec_host[key] - host[key]) <= 1e-9 * max(host[key], 1e-3), (key, rec_host, host)
    assert np.all(truth[:-1] >= truth[1:]) and truth[-1] >= 0
    if kind == "singular_tail":
        assert np.count_nonzero(truth == 0) == max(n // 4, 1)          # exactly singular: exact zeros in the truth

    work = []
    lam, W, sweeps, applied = jc.restated(G, work_out=work)
    got = jc.ratios(G, lam, W, truth)
    print(f"JACOBI-RESTATED {jc.label(kind, n)} lam={got['lam']:.3f} orth={got['orth']:.3f} res={got['res']:.3f} "
          f"sweeps={sweeps} applied={applied}")
    for A in work:
        assert np.array_equal(A, A.T)
    assert applied[-1] == 0 and sweeps == len(applied)
    for key in ("lam", "orth", "res"):
        assert got[key] <= jc.bar(host[key]), (key, got, host)
    assert sweeps <= host["sweeps"] + jc.MAX_EXTRA_SWEEPS
    # the host routine itself is within the convention's cap: the bars mean something
    assert max(host["lam"], host["orth"], host["res"]) <= jc.BAR_CAP / jc.BAR_FACTOR


def test_restatement_on_exact_cases():
    """Diagonal input: no rotation, one sweep, the sorted diagonal, the permutation with ties in index order.  Blocks
    [[a, b], [b, a]]: one rotating sweep, exactly a +- b, entries of W 0 or +-1/sqrt(2) as rounded by 1 / sqrt(2)."""
    d = np.array([3.0, 0.0, 7.0, 3.0, 0.0, 5.0, 7.0])
    lam, W, sweeps, applied = jc.restated(np.diag(d))
    order = np.argsort(-d, kind="stable")
    assert sweeps == 1 and applied == [0]
    assert np.array_equal(lam, d[order]) and np.array_equal(W, np.eye(7)[:, order])
    G = np.zeros((5, 5))
    for (i, j), (a, b) in {(0, 3): (5.0, 2.0), (1, 4): (9.0, 4.0)}.items():
        G[i, i] = G[j, j] = a
        G[i, j] = G[j, i] = b
    G[2, 2] = 6.0
    lam, W, sweeps, applied = jc.restated(G)
    assert sweeps == 2 and applied == [2, 0]
    assert np.array_equal(lam, [13.0, 7.0, 6.0, 5.0, 3.0])
    assert set(np.abs(W).ravel()) == {0.0, 1.0, 1.0 / np.sqrt(2.0)}
