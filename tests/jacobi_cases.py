"""Shared pieces of the device Jacobi eigensolver's tests (tests/test_jacobi_eig_cpu.py, tests/test_jacobi_eig_gpu.py).
Plain module, not a conftest; everything here runs on the host.

* ``rounds`` / ``restated``: the round-robin order of csrc/symjacobi.hip and its arithmetic restated in NumPy, block by
  block: the new 2 x 2 block of row pair i and column pair j from the old block alone, column rotation first above the
  diagonal of pairs and row rotation first below it, no fused multiply-add.  ``J^T A J`` is never formed as dense
  products (that destroys the relative accuracy of the small entries).  In ``np.float64`` it gives the kernel's bits,
  in ``np.longdouble`` the truth.
* ``matrix``: the test matrices.  Graded positive definite G = F^T F, F = Q (I + delta E) diag(s) (Q drops out of G), s over 12 decades,
  E uniform with entries of variance 1/n (so ||E||_2 is about 2 at every n and delta measures the departure of G's
  scaled form from the identity: its condition number stays below ((1 + 2 delta) / (1 - 2 delta))^2 = 2.25 at delta =
  0.1, which is what makes the small eigenvalues well determined, Demmel & Veselic 1992); a 1e-6 cluster at the top;
  an exactly singular tail.  G is the product in long double, rounded once and mirrored.
* ``truth`` / ``host_reference``: eigenvalues of G as stored (``restated`` in long double) and what
  ``rt_host_jacobi_eigh`` achieves on the same matrix.  Both are recorded in tests/golden/jacobi_truth.npz
  (tests/golden/make_jacobi_truth.py writes it; the long-double runs at n = 257 and 512 take minutes); the CPU test
  recomputes the small ones and holds the record to them.
* ``ratios``: the three figures every bar is about.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)          # 2.2e-16: the unit of every ratio (n eps)
STOP_EPS = 1.1102230246251565e-16              # the stopping rule's eps, as csrc/host_dense.cpp and csrc/symjacobi.hip have it
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jacobi_truth.npz")

KINDS = ("graded_1e-3", "graded_1e-1", "cluster", "singular_tail")
CPU_SIZES = (7, 64, 129)
GPU_SIZES = CPU_SIZES + (257, 512)
BAR_FACTOR, BAR_CAP = 4.0, 20.0                # a bar: BAR_FACTOR max(1, host's ratio), at most BAR_CAP
MAX_EXTRA_SWEEPS = 2
PROBE = (slice(None, None, 17), slice(None, None, 13))


# ---- the order --------------------------------------------------------------------------------------------------------
def player(pos, rnd, m):
    """Who sits at position ``pos`` in round ``rnd`` of a tournament of m (even) players."""
    pos = np.asarray(pos)
    return np.where(pos == 0, 0, (pos - 1 - rnd) % (m - 1) + 1)


def rounds(n):
    """The rounds of a sweep: (p, q) index arrays of the m / 2 pairs, m = n rounded up to even; for odd n the pair that
    holds index n idles.  n - 1 rounds for even n, n for odd n; a function of n alone."""
    m = n + (n % 2)
    pairs = np.arange(m // 2)
    for rnd in range(m - 1):
        yield player(pairs, rnd, m), player(m - 1 - pairs, rnd, m)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------
def _rot(c, s, x, y, on):
    """(c x - s y, s x + c y) where ``on``, (x, y) elsewhere; c, s, on broadcast against the blocks."""
    return np.where(on, c * x - s * y, x), np.where(on, s * x + c * y, y)


def restated(G, dtype=np.float64, max_sweeps=60, stop_eps=None, work_out=None):
    """(lam, W, sweeps, applied): the device solver restated.  ``sweeps`` counts the closing sweep without rotations,
    ``applied`` lists the rotations applied per sweep.  ``work_out``: a list that receives the work matrix after every
    sweep (what the rounds leave of G: exactly symmetric, exact zeros where a pair was rotated last)."""
    n = G.shape[0]
    m = n + (n % 2)
    one = dtype(1.0)
    eps = dtype(STOP_EPS if stop_eps is None else stop_eps)
    A = np.zeros((m, m), dtype=dtype)               # an odd n plays with a zero row and column that never rotate
    A[:n, :n] = np.triu(G) + np.triu(G, 1).T
    W = np.zeros((m, m), dtype=dtype)
    W[:n, :n] = np.eye(n, dtype=dtype)
    P = m // 2
    upper = np.arange(P)[:, None] < np.arange(P)[None, :]
    diag = np.arange(P)
    applied, sweeps = [], 0
    while sweeps < max_sweeps:
        count = 0
        for p, q in rounds(n):
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            on = (p < n) & (q < n) & (apq != 0) & ~(np.abs(apq) <= eps * np.sqrt(np.abs(app) * np.abs(aqq)))
            safe = np.where(on, apq, one)
            theta = (aqq - app) / (dtype(2.0) * safe)
            t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
            c = one / np.sqrt(t * t + one)
            s = t * c
            c, s, t = np.where(on, c, one), np.where(on, s, dtype(0.0)), np.where(on, t, dtype(0.0))
            count += int(on.sum())
            Bpr, Bps, Bqr, Bqs = A[np.ix_(p, p)], A[np.ix_(p, q)], A[np.ix_(q, p)], A[np.ix_(q, q)]
            ci, si, oi = c[:, None], s[:, None], on[:, None]
            cj, sj, oj = c[None, :], s[None, :], on[None, :]
            # above the diagonal of pairs: columns first, then rows
            u_pr, u_ps = _rot(cj, sj, Bpr, Bps, oj)
            u_qr, u_qs = _rot(cj, sj, Bqr, Bqs, oj)
            u_pr, u_qr = _rot(ci, si, u_pr, u_qr, oi)
            u_ps, u_qs = _rot(ci, si, u_ps, u_qs, oi)
            # below it: rows first, then columns - the transposed operations on the transposed block
            l_pr, l_qr = _rot(ci, si, Bpr, Bqr, oi)
            l_ps, l_qs = _rot(ci, si, Bps, Bqs, oi)
            l_pr, l_ps = _rot(cj, sj, l_pr, l_ps, oj)
            l_qr, l_qs = _rot(cj, sj, l_qr, l_qs, oj)
            Npr, Nps = np.where(upper, u_pr, l_pr), np.where(upper, u_ps, l_ps)
            Nqr, Nqs = np.where(upper, u_qr, l_qr), np.where(upper, u_qs, l_qs)
            # a pair's own block, as rt_host_jacobi_eigh writes it
            tq = t * apq
            Npr[diag, diag] = np.where(on, app - tq, app)
            Nqs[diag, diag] = np.where(on, aqq + tq, aqq)
            Nps[diag, diag] = np.where(on, dtype(0.0), apq)
            Nqr[diag, diag] = np.where(on, dtype(0.0), A[q, p])
            A[np.ix_(p, p)], A[np.ix_(p, q)], A[np.ix_(q, p)], A[np.ix_(q, q)] = Npr, Nps, Nqr, Nqs
            wp, wq = _rot(cj, sj, W[:, p], W[:, q], oj)
            W[:, p], W[:, q] = wp, wq
        sweeps += 1
        applied.append(count)
        if work_out is not None:
            work_out.append(A[:n, :n].copy())
        if count == 0:
            break
    d = np.diagonal(A)[:n].copy()
    order = np.argsort(-d, kind="stable")
    return d[order], W[:n, :n][:, order], sweeps, applied


# ---- matrices ---------------------------------------------------------------------------------------------------------
def spectrum(kind, n):
    """2^-x_i, x_i = 40 i / (n - 1) (twelve decades), the power between two integers interpolated linearly: divisions,
    floor and ldexp only, so the values do not depend on a mathematical library."""
    x = 40.0 * np.arange(n) / max(n - 1, 1)
    s = np.ldexp(1.0 - 0.5 * (x - np.floor(x)), -np.floor(x).astype(np.int64))
    if kind == "cluster" and n > 4:
        s[:4] = [1.0, 1.0 - 1e-6, 1.0 - 2e-6, 1.0 - 3e-6]
    if kind == "singular_tail":
        s[n - max(n // 4, 1):] = 0.0
    return s


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    """(G, F): G = F^T F in long double, rounded once, exactly symmetric; F = (I + delta E) diag(s) in float64.  The
    orthogonal factor Q drops out of F^T F, so it is left out, and E is uniform on [-sqrt(3 / n), sqrt(3 / n)] (variance
    1 / n) from integer draws: every operation here is an IEEE elementwise operation or a long-double product (no BLAS,
    no LAPACK, no logarithm or power), so the matrix is the same bit for bit wherever it is built - the recorded truth
    is the truth of exactly this matrix."""
    rng = np.random.RandomState(100 * n + KINDS.index(kind))
    delta = 1e-1 if kind == "graded_1e-1" else 1e-3
    E = rng.randint(-(1 << 30), (1 << 30) + 1, size=(n, n)).astype(np.float64) / float(1 << 30) * np.sqrt(3.0 / n)
    F = (np.eye(n) + delta * E) * spectrum(kind, n)
    FL = F.astype(LD)
    G = (FL.T @ FL).astype(np.float64)
    G = np.triu(G) + np.triu(G, 1).T
    G.setflags(write=False)
    return G, F


def cases(sizes):
    return [(kind, n) for n in sizes for kind in KINDS]


def label(kind, n):
    return f"{kind}-{n}"


# ---- the truth, and the host routine on the same matrices -----------------------------------------------------------------
def compute_truth(G):
    """Eigenvalues of G as stored, in long double (descending): ``restated`` with long double's own eps."""
    if not np.finfo(LD).eps < 2e-19:
        raise RuntimeError("the truth needs x86 extended precision (np.longdouble eps < 2e-19)")
    lam, _, sweeps, _ = restated(G, dtype=LD, stop_eps=float(np.finfo(LD).eps) / 2)
    assert sweeps < 60, "the long-double sweeps did not converge"
    return lam


def host_jacobi(G, max_sweeps=60):
    """(lam, W, sweeps) of rt_host_jacobi_eigh; ``sweeps`` is its own count (sweeps that rotated)."""
    from romtime_amd import _lib

    lib = _lib.load()
    n = G.shape[0]
    A = np.array(G, dtype=np.float64, order="C", copy=True)
    W, lam, sweeps = np.empty((n, n)), np.empty(n), C.c_int(0)
    rc = lib.rt_host_jacobi_eigh(A.ctypes.data, n, W.ctypes.data, lam.ctypes.data, max_sweeps, C.byref(sweeps))
    assert rc == 0, rc
    return lam, W, int(sweeps.value)


def ratios(G, lam, W, truth):
    """dict(lam, orth, res): max_i |lam_i - truth_i| / (n eps truth_i) over the positive eigenvalues of the truth,
    max |W^T W - I| / (n eps), max_i ||G w_i - lam_i w_i||_2 / (n eps ||G||_2).  Products in long double: the figures
    are the solver's, not the check's."""
    n = G.shape[0]
    pos = truth > 0
    lam_l, Wl, Gl = lam.astype(LD), W.astype(LD), G.astype(LD)
    rl = float(np.max(np.abs(lam_l[pos] - truth[pos]) / truth[pos])) / (n * EPS) if pos.any() else 0.0
    ro = float(np.max(np.abs(Wl.T @ Wl - np.eye(n, dtype=LD)))) / (n * EPS)
    norm2 = float(np.max(truth))               # ||G||_2 of a symmetric positive semi-definite matrix
    rr = float(np.max(np.sqrt(np.sum((Gl @ Wl - Wl * lam_l) ** 2, axis=0)))) / (n * EPS * norm2)
    return dict(lam=rl, orth=ro, res=rr)


def compute_host_reference(G, truth):
    lam, W, sweeps = host_jacobi(G)
    out = ratios(G, lam, W, truth)
    out["sweeps"] = sweeps
    return out


def split(x):
    """A long-double vector as two float64 vectors (value = hi + lo exactly for x86 extended precision's 64 bits)."""
    hi = x.astype(np.float64)
    return hi, (x - hi.astype(LD)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def truth(kind, n):
    """Recorded long-double eigenvalues of ``matrix(kind, n)[0]``; refuses a record of another matrix."""
    g, key = _golden(), label(kind, n)
    G, _ = matrix(kind, n)
    if not np.array_equal(G[PROBE], g[key + "/probe"]):
        raise AssertionError(f"{key}: tests/golden/jacobi_truth.npz belongs to another matrix (regenerate it)")
    return g[key + "/hi"].astype(LD) + g[key + "/lo"].astype(LD)


def host_reference(kind, n):
    """Recorded dict(lam, orth, res, sweeps) of rt_host_jacobi_eigh on ``matrix(kind, n)[0]``."""
    v = _golden()[label(kind, n) + "/host"]
    return dict(lam=float(v[0]), orth=float(v[1]), res=float(v[2]), sweeps=int(v[3]))


def bar(host_ratio):
    return min(BAR_FACTOR * max(1.0, host_ratio), BAR_CAP)
