"""Shared pieces of the greedy-against-the-truth tests (tests/test_deim_truth_cpu.py, tests/test_deim_truth_gpu.py).
Plain module, not a conftest; everything here runs on the host.

* ``certify``: the extended-precision certificate of ONE pivot sequence.  It walks the sequence it is given in
  ``np.longdouble`` (r_k = phi_k reduced by the earlier residual columns at their pivots) and reports, per step, the true
  maximum of |r_k|, how far the pick falls short of it, the true margin and argmax and the running magnitude S_k.  It never
  looks at a second sequence: after a legitimate near-tie the picks of another greedy say nothing about this one's.
* ``accepted`` / ``condition``: the rule a pick is held to, |r_k[p_k]| >= (1 - 1e-9) max|r_k| (1e-9 is the near-tie threshold
  of tests/test_configs_gpu.py and tests/test_full_size_gpu.py), and the number that keeps the rule meaningful: float64
  rounding moves an entry of r_k by about (k + 2) eps S_k, and every case of the tables below has
  (k + 2) eps S_k / max|r_k| <= 1e-11 at every step (asserted in tests/test_deim_truth_cpu.py), a hundred times below 1e-9.
  Wherever the true margin exceeds 1e-9 the rule therefore forces the pick to be the true argmax.
* ``basis``: the input families, deterministic from (family, N, m, seed): ``random``, ``sine``, ``dup_pair`` / ``dup_half`` /
  ``dup_mirror`` (exact ties at every step), ``near_mirror`` (a tie to a few ulps at every step), ``scaled``, ``permuted``.
* ``multiplier_bound``: the float64 form of the greedy's defining property for sizes whose long-double certificate would
  take too long: with U from an unpivoted LU of Phi[idx], every entry of Phi U^-1 is a multiplier r_k[i] / r_k[p_k].

Out of scope: a basis with an exactly zero residual column (a rank-deficient Phi).  The reference raises LinAlgError
there and what the device does is unspecified."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np
from scipy.linalg import solve_triangular

from tests.svd_cases import _need_extended

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
NEAR_TIE = 1e-9           # the project's near-tie threshold
CONDITION = 1e-11         # (k + 2) eps S_k / max|r_k| of every case stays below this


# ---- the certificate --------------------------------------------------------------------------------------------------
@dataclass
class Certificate:
    top: np.ndarray         # long double: max_i |r_k[i]|
    shortfall: np.ndarray   # long double: top - |r_k[p_k]|
    margin: np.ndarray      # float64: (top1 - top2) / top1 of the true |r_k|
    argmax: np.ndarray      # int64: the true argmax, lowest index on ties
    S: np.ndarray           # long double: max_i (|phi_k[i]| + sum_j |r_j[i]| |c_j|)


def certify(B, idx, keep_residuals=False):
    """The certificate of the pivot sequence ``idx`` on the basis ``B`` (N x m), N m^2 / 2 long-double operations.
    With ``keep_residuals`` the residual columns (N x m, long double) are returned beside it."""
    _need_extended()
    A = np.asarray(B, dtype=LD)
    N, m = A.shape
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.shape == (m,) and idx.min() >= 0 and idx.max() < N
    R = np.empty((m, N), dtype=LD)                 # residual columns as rows: contiguous updates
    piv = np.empty(m, dtype=LD)
    cert = Certificate(np.empty(m, LD), np.empty(m, LD), np.empty(m), np.empty(m, np.int64), np.empty(m, LD))
    for k in range(m):
        t = A[:, k].copy()
        S = np.abs(t)
        for j in range(k):
            c = t[idx[j]] / piv[j]
            t -= R[j] * c
            S += np.abs(R[j]) * np.abs(c)
        R[k] = t
        piv[k] = t[idx[k]]
        a = np.abs(t)
        i = int(np.argmax(a))                      # the first maximum
        top = a[i]
        a[i] = -1
        second = a.max() if N > 1 else LD(0)
        cert.top[k], cert.argmax[k], cert.S[k] = top, i, S.max()
        cert.shortfall[k] = top - np.abs(piv[k])
        cert.margin[k] = float((top - second) / top) if top > 0 else 0.0
    return (cert, R.T) if keep_residuals else cert


def accepted(cert):
    """Per step: the pick is within 1e-9 (relative) of the true maximum of its own residual."""
    return cert.top - cert.shortfall >= (LD(1) - LD(NEAR_TIE)) * cert.top


def condition(cert):
    """Per step (k + 2) eps S_k / max|r_k|: what float64 rounding can move an entry by, relative to the maximum."""
    k = np.arange(len(cert.top))
    return ((k + 2) * EPS * cert.S / cert.top).astype(np.float64)


def shortfall_in_eps(cert):
    """Per step shortfall / (eps S_k): information for DESIGN.md, not a bar."""
    return (cert.shortfall / (EPS * cert.S)).astype(np.float64)


def assert_certified(B, idx, show=print, label="", cert=None):
    """certify (unless ``cert`` is the certificate of ``idx`` already) + the acceptance rule on every step + distinct
    indices in range; returns the certificate."""
    idx = np.asarray(idx)
    N, m = B.shape
    assert idx.min() >= 0 and idx.max() < N and len(set(idx.tolist())) == m, (label, idx)
    cert = cert or certify(B, idx)
    ok = accepted(cert)
    rel = (cert.shortfall / cert.top).astype(np.float64)
    show(f"DEIM-TRUTH {label} {N}x{m} worst shortfall/top={rel.max():.3g} shortfall/(eps S)={shortfall_in_eps(cert).max():.3g} "
         f"min margin={cert.margin.min():.3g} condition={condition(cert).max():.3g}")
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (label, "steps whose pick is not the residual's maximum", bad[:8], rel[bad[:8]],
                           idx[bad[:8]], cert.argmax[bad[:8]])
    # wherever the truth is no near-tie the pick IS the true argmax
    clear = cert.margin > NEAR_TIE
    assert np.array_equal(idx[clear], cert.argmax[clear]), label
    return cert


# ---- input families -------------------------------------------------------------------------------------------------
DUP_FAMILIES = ("dup_pair", "dup_half", "dup_mirror")


def _rng(family, N, m, seed):
    return np.random.RandomState(zlib.crc32(f"{family}-{N}-{m}-{seed}".encode()) & 0x7FFFFFFF)


def _random(N, m, seed):
    return np.linalg.qr(_rng("random", N, m, seed).standard_normal((N, m)))[0]


def dup_partner(family, N):
    """(low, high): rows ``high`` duplicate rows ``low`` (low[i] < high[i], every row in exactly one pair; N even).
    ``dup_pair``: 2i -> 2i + 1, the two slots of one thread's pair of rows.  ``dup_half``: i -> i + 512 inside every full
    1024-row column workgroup, the rows a thread takes in its two halves; what is left over at the end is paired 2i ->
    2i + 1.  ``dup_mirror``: i -> N - 1 - i, across workgroups."""
    assert N % 2 == 0
    if family == "dup_pair":
        low = np.arange(0, N, 2)
        return low, low + 1
    if family == "dup_mirror":
        low = np.arange(N // 2)
        return low, N - 1 - low
    if family == "dup_half":
        full = N // 1024 * 1024
        low = (np.arange(full).reshape(-1, 1024)[:, :512]).ravel()
        rest = np.arange(full, N, 2)
        return np.r_[low, rest], np.r_[low + 512, rest + 1]
    raise ValueError(family)


def assert_exact_ties(family, N, idx, margin):
    """On a ``dup`` family every step is an exact tie between the two rows of a pair: the pick is the lower row (the first
    maximum, np.argmax's rule) and the margin is 0.0 to the last bit."""
    low, _ = dup_partner(family, N)
    idx, margin = np.asarray(idx), np.asarray(margin)
    high_picks = np.nonzero(~np.isin(idx, low))[0]
    assert high_picks.size == 0, (family, "steps that took the higher row of a pair", high_picks[:8], idx[high_picks[:8]])
    assert np.all(margin == 0.0), (family, "margins of exact ties that are not 0.0", np.nonzero(margin != 0.0)[0][:8])


def column_exponents(N, m, seed=0):
    return _rng("exponents", N, m, seed).randint(-40, 41, size=m)


def row_permutation(N, m, seed=0):
    return _rng("permutation", N, m, seed).permutation(N)


def basis(family, N, m, seed=0):
    """The float64 N x m basis of a family (C order)."""
    if family == "random":
        return _random(N, m, seed)
    if family == "sine":
        x = np.arange(1, N + 1) / (N + 1.0)
        return np.sqrt(2.0 / (N + 1)) * np.sin(np.pi * x[:, None] * np.arange(1, m + 1)[None, :])
    if family in DUP_FAMILIES:
        B = _random(N, m, seed)
        low, high = dup_partner(family, N)
        sign = _rng(family, N, m, seed).choice([-1.0, 1.0], size=len(low))
        B[high] = sign[:, None] * B[low]
        return B
    if family == "near_mirror":  # dup_mirror with the copy a few ulps off: a true margin of some 1e-16 at EVERY step
        B = basis("dup_mirror", N, m, seed)
        low, high = dup_partner("dup_mirror", N)
        ulps = _rng(family, N, m, seed).choice([-2.0, -1.0, 1.0, 2.0], size=len(high))
        B[high] *= (1.0 + ulps * EPS)[:, None]
        return B
    if family == "scaled":       # random with column k times 2^e_k: exact in float64
        return _random(N, m, seed) * np.ldexp(1.0, column_exponents(N, m, seed))[None, :]
    if family == "permuted":     # row i of the result is row perm[i] of random
        return np.ascontiguousarray(_random(N, m, seed)[row_permutation(N, m, seed)])
    raise ValueError(family)


# ---- the tables of tests/test_deim_truth_gpu.py -----------------------------------------------------------------------
# BLK = 8 columns per block, 512-row sweeps, 1024-row column workgroups, 128-wide passes and 16 waves in the block start:
# every m either side of those, each with an N from {m itself; 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 2049}
RANDOM_SHAPES = [(1, 1), (15, 1), (2, 2), (16, 2), (7, 7), (17, 7), (8, 8), (511, 8), (9, 9), (512, 9), (16, 16), (513, 16),
                 (17, 17), (1023, 17), (1024, 24), (1025, 63), (511, 64), (2049, 64), (513, 65), (512, 128), (1023, 129),
                 (1024, 136), (1025, 137), (2049, 264), (1025, 265)]
SINE_SHAPES = [(1023, 64), (1025, 137)]
NEAR_MIRROR_CASE = ("near_mirror", 2050, 40, 0)
SLICE_SHAPES = [(513, 17), (1025, 137)]
DUP_CASES = [("dup_pair", 2050, 40), ("dup_half", 2050, 40), ("dup_mirror", 2050, 40), ("dup_pair", 1026, 9)]
SCALED_CASE = ("scaled", 1025, 65, 0)
PERMUTED_CASE = ("permuted", 2049, 24, 0)
TABLE = ([("random", N, m, 0) for N, m in RANDOM_SHAPES] + [("sine", N, m, 0) for N, m in SINE_SHAPES]
         + [(f, N, m, 0) for f, N, m in DUP_CASES] + [NEAR_MIRROR_CASE, SCALED_CASE, PERMUTED_CASE])
LIMIT = dict(family="random", N=1040, m=1024, seed=0)      # tests/golden/make_deim_limit.py
LIMIT_PROBE = (slice(0, 1040, 97), slice(0, 1024, 89))     # a sample of the input, stored beside its reference
# LAPACK's blocked QR is not the same to the last bit on every host (threads, kernels picked per CPU): the rebuilt basis
# matches the recorded one to rounding (entries are about 0.03; differences seen: below 1e-15), which the recorded picks
# - no margin below 1e-4 - do not feel
LIMIT_PROBE_ATOL = 1e-13


def label(case):
    return "{}-{}x{}-s{}".format(*case)


# ---- the float64 multiplier certificate -------------------------------------------------------------------------------
def unpivoted_upper(A, nb=64):
    """U of A = L U without pivoting (L unit lower), right-looking in panels of ``nb`` columns: the panel by rank-1
    updates, the rest at BLAS speed."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    assert A.shape == (n, n)
    for k0 in range(0, n, nb):
        k1 = min(k0 + nb, n)
        for k in range(k0, k1):
            A[k + 1:, k] /= A[k, k]
            A[k + 1:, k + 1:k1] -= np.outer(A[k + 1:, k], A[k, k + 1:k1])
        if k1 < n:
            L11 = np.tril(A[k0:k1, k0:k1], -1) + np.eye(k1 - k0)
            A[k0:k1, k1:] = solve_triangular(L11, A[k0:k1, k1:], lower=True, unit_diagonal=True)
            A[k1:, k1:] -= A[k1:, k0:k1] @ A[k0:k1, k1:]
    return np.triu(A)


def multiplier_bound(Phi, idx):
    """max |Phi U^-1| with U from the unpivoted LU of Phi[idx]: column k of Phi U^-1 is r_k / r_k[p_k] along ``idx``, so a
    greedy sequence has 1 (the pivots themselves) and a sequence with a pick that was not the maximum has more."""
    Phi = np.asarray(Phi, dtype=np.float64)
    U = unpivoted_upper(Phi[np.asarray(idx)])
    X = solve_triangular(U, Phi.T, trans="T", lower=False)      # U^T X = Phi^T
    return float(np.abs(X).max())
