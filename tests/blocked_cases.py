"""Shared pieces of the block Rayleigh-Ritz tests (tests/test_blocked_eig_cpu.py, tests/test_blocked_eig_gpu.py; the
route: csrc/symeig_blocked.hip).  Plain module, not a conftest; everything here runs on the host.

Truth without an extended-precision SVD at n > 2048: X = A diag(s) B^T in long double, rounded to float64.  A holds the
first k orthonormal DCT-II vectors of length N, B the first k of length n with its rows pushed through a fixed
permutation, so that no block sees a zero panel.  (s, A, B) is the exact SVD of the unrounded X; rounding moves it by at
most eps ||X||_F.  With ``normalize`` the matrix decomposed is X D^-1 = A (diag(s) B^T D^-1): a k x n factor whose
long-double SVD costs O(n k^2).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import svd_cases as svd

LD = svd.LD
EPS = svd.EPS
N_ROWS = 4096
K = 24


def dct_columns(N, k):
    """The first k orthonormal DCT-II vectors of length N, in long double."""
    i = (np.arange(N, dtype=LD) + LD(0.5))[:, None]
    j = np.arange(k, dtype=LD)[None, :]
    pi = 4 * np.arctan(LD(1))
    A = np.cos(pi * i * j / LD(N)) * np.sqrt(LD(2) / LD(N))
    A[:, 0] /= np.sqrt(LD(2))
    return A


@dataclass(frozen=True)
class Case:
    n: int
    smin: float = 1e-5          # s geometric from 1 down to smin
    outer_scale: float = 1.0    # the rows of B outside the last block scaled by this (and B orthonormalised again)

    @property
    def label(self):
        return f"dct-{N_ROWS}x{self.n}-smin{self.smin:.0e}" + (f"-outer{self.outer_scale:.0e}" if self.outer_scale != 1.0 else "")


SPREAD_2049 = Case(2049)
SPREAD_4097 = Case(4097)
# the last block carries all the energy but 2^-80 of it: lam_max comes from it, and the first block keeps nothing
LAST_2049 = Case(2049, outer_scale=2.0 ** -40)
# ... all but 1e-6 of it: the first block's eigenvalues straddle the floor, so the blocks discard part of the signal
STRADDLE_2049 = Case(2049, outer_scale=1e-3)
DEEP_2049 = Case(2049, smin=1e-9)


@functools.lru_cache(maxsize=None)
def factors(case: Case):
    """(A, s, B) in long double: N x K, K, n x K."""
    from romtime_amd import pod_rules

    A = dct_columns(N_ROWS, K)
    s = LD(case.smin) ** (np.arange(K, dtype=LD) / LD(K - 1))
    B = dct_columns(case.n, K)[np.random.RandomState(case.n).permutation(case.n)]
    if case.outer_scale != 1.0:
        widths = pod_rules.block_partition(case.n)
        B = B.copy()
        B[: case.n - widths[-1]] *= LD(case.outer_scale)
        B, _, _ = svd.longdouble_svd(B)          # orthonormal columns with the same span
    return A, s, B


@functools.lru_cache(maxsize=None)
def snapshots(case: Case):
    """X (float64, N x n, C order, read-only)."""
    A, s, B = factors(case)
    X = np.ascontiguousarray(((A * s) @ B.T).astype(np.float64))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def gram_host(case: Case):
    """B diag(s^2) B^T in long double, rounded: the Gram matrix of the unrounded X."""
    _, s, B = factors(case)
    G = ((B * (s * s)) @ B.T).astype(np.float64)
    G = 0.5 * (G + G.T)
    G.setflags(write=False)
    return G


def gram_apply(case: Case):
    """W -> G W in long double through the factors: O(n K k)."""
    _, s, B = factors(case)
    return lambda Wl: B @ ((s * s)[:, None] * (B.T @ Wl))


@functools.lru_cache(maxsize=None)
def pod_truth(case: Case, normalize: bool):
    """(U, sig): the K left singular vectors (N x K) and singular values of X, or of X D^-1, in long double."""
    A, s, B = factors(case)
    if not normalize:
        return A, s
    d = np.sqrt(np.sum((B * s) ** 2, axis=1))            # column norms of X
    Mt = (B * s) / d[:, None]                              # (diag(s) B^T D^-1)^T, n x K
    _, sig, V = svd.longdouble_svd(Mt)                     # M^T = U' sig V^T: the left vectors of M are V
    return A @ V, sig


def spectrum_n(sig, n):
    sf = np.zeros(n)
    sf[: len(sig)] = np.asarray(sig, dtype=np.float64)
    return sf


def level_tops(sf, num, tol):
    """s_L per entry: the largest singular value of the deflated level that produces it (the tail: the last level's)."""
    tops = np.full(len(sf), sf[0])
    for first, _ in svd.level_plan(sf, num, tol):
        tops[first:] = sf[first]
    return tops


def pod_bars(case: Case, normalize, num, tol):
    """dict(r, sf, s_bar, col_bar, dist_bar) for ``orth`` on the case through the blocked route with deflated levels:
    the bars of svd_cases.model_sigma / model_columns with F_S / F_COL, plus the Rayleigh-Ritz terms p tau_L^2 / (2 s_i)
    and p tau_L^2 / gap_i with tau_L^2 = n eps s_L^2 >= n eps lam_max of the level.  ``dist_bar`` is the root sum of
    squares of the column bars over the kept modes: a subspace distance is at most the Frobenius norm of the column
    errors."""
    from romtime_amd import pod_rules

    n = case.n
    _, sig = pod_truth(case, normalize)
    sf = spectrum_n(sig, n)
    energy = np.cumsum(sf * sf) / np.sum(sf * sf)
    r = svd.truncation_rank(sf, energy, num or 0, tol or 0.0)
    if tol:
        assert np.all(np.abs(energy - tol) > 0.1 * (1.0 - tol)), (case.label, "an energy within 10 % of 1 - tol of tol")
    p = len(pod_rules.block_partition(n))
    tops = level_tops(sf, num or 0, tol or 0.0)
    tau2 = p * n * EPS * tops ** 2                                    # p tau_L^2 per entry
    s_bar = svd.F_S * svd.model_sigma(sf, tops)
    s_bar[:K] += tau2[:K] / (2.0 * sf[:K])
    lam = np.r_[sf[:K] ** 2, 0.0]
    gap = np.array([np.min(np.abs(np.delete(lam, i) - lam[i])) for i in range(K)])
    col_bar = svd.F_COL * np.maximum(svd.model_columns(sig), n * EPS) + tau2[:K] / gap
    return dict(r=r, sf=sf, s_bar=s_bar, col_bar=col_bar, dist_bar=float(np.sqrt(np.sum(col_bar[:r] ** 2))), p=p)
