"""Shared pieces of the tridiagonal eigensolver's truth tests (tests/test_sym_eig_truth_cpu.py,
tests/test_sym_eig_truth_gpu.py; the solver: csrc/symeig.hip).  Plain module, not a conftest; everything here runs on
the host.

* ``exact``: matrices whose eigen-decomposition is known exactly at every size.  G = H D H, H = I - 2 v v^T / P a
  Householder matrix, v nonzero small integers whose squares sum to a power of two P >= n, D distinct positive integers
  below 2^20 in no order.  P^2 G is formed in int64 (below 2^53, asserted) and divided by P^2: G is exact in float64 and
  exactly symmetric, its eigenvalues are exactly D and its eigenvectors exactly the columns of H - at n = 2048 as at
  n = 4, with no extended-precision run, the same bit for bit wherever it is built.  v_0 = +-1, so that
  H_00 = 1 - 2 / P != 0: e_0 then has a component along every eigenvector and the tridiagonal matrix that a Householder
  reduction from row 0 leaves is irreducible (n - 2 real reflectors).
  The squares 1, 4, 9 (entries +-1, +-2, +-3) reach a power of two at every size of the tests but two.  n = 6 needs one
  +-4 (16 + 9 + 4 + 1 + 1 + 1 = 32; no six squares of 1 ... 3 sum to 8, 16 or 32).  At n = 3 no nonzero integers do at
  all (a sum of squares that is divisible by 4 has only even terms, so it reduces to 1 or 2 = three nonzero squares):
  there v = (+-1, +-1, +-1), P = 3 and the matrix is the integer matrix P^2 G itself - still exact, eigenvalues 9 D,
  eigenvectors the columns of H, which are then kept in long double.
* ``measure``: the figures every bar is about, all products in long double on the solver's output (as
  ``jacobi_cases.ratios``): eigenvalues, per-vector residuals, norms, gap-scaled orthogonality and - where the
  eigenvectors are known - the gap-scaled distance of every vector from the truth.
* ``tridiagonalise`` / ``back_transform``: the Householder reduction of csrc/symeig.hip (dsytd2 recurrences from row 0)
  and its blocked back-transformation ``s_u = tau_u (a_u - sum_w c_uw s_w)`` restated in NumPy.
* ``lapack_reference``: the same figures for ``np.linalg.eigh`` on the same matrix; recorded in
  tests/golden/eig_lapack.json (tests/golden/make_eig_lapack.py writes it, the host test recomputes the small sizes).
  A bar is ``BAR_FACTOR max(1, LAPACK's ratio)``, at most ``BAR_CAP`` (``bar``).
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from tests import jacobi_cases as jc

LD = jc.LD
EPS = jc.EPS
BAR_FACTOR, BAR_CAP = jc.BAR_FACTOR, jc.BAR_CAP
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eig_lapack.json")

SPECTRA = ("spread", "graded")
# both sides of the one-workgroup form (64 / 65), of every NM class (128, 256, 512, 1024), of the 32- and 128-workgroup
# teams (512 / 513) and of the wide route (1024 / 1025); every residue of (n - 2) % 4, and of % 2 beyond 1024
EXACT_SIZES = (3, 4, 5, 6, 7, 10, 63, 64, 65, 66, 128, 129, 130, 256, 257, 512, 513, 1024, 1025, 1026, 2047, 2048)
CPU_SIZES = tuple(n for n in EXACT_SIZES if n <= 257)      # LAPACK's figures are recomputed on the host up to here
FULL_K_MAX = 512                                           # up to here every vector is requested and measured
LARGE_KS = (1, 2, 63, 64, 65, 128)                         # beyond: these k, long-double products on those columns only
SLICES = {130: (37, 50), 1026: (700, 65)}                  # (first, count) of the slices passed as lam + first
FIGURES = ("lam", "res", "norm", "orth", "vec")
SEPARATED_BOUND = 2e-12                                    # what pod_rules.separated's docstring states
CLUSTER = 4                                                # jacobi_cases' ``cluster``: the leading four within 3e-6


# ---- the exact family -------------------------------------------------------------------------------------------------
def fill(n):
    """(P, (a, b, c)): the smallest power of two P >= n with P - n = 3 a + 8 b + 15 c, a entries +-2, b entries +-3 and
    c entries +-4 among n - 1 (the first stays +-1), the fewest +-4 first; None where there is none (n = 3)."""
    P = 1
    while P < n:
        P *= 2
    while P <= 16 * n:
        r = P - n
        for c in range(r // 15 + 1):
            for b in range((r - 15 * c) // 8 + 1):
                rem = r - 15 * c - 8 * b
                if rem % 3 == 0 and rem // 3 + b + c <= n - 1:
                    return P, (rem // 3, b, c)
        P *= 2
    return None


def graded_integers(n):
    """floor(2^20 2^-x_i), x_i = 20 i / (n - 1), the power between two integers interpolated linearly (divisions, floor
    and ldexp only, as jacobi_cases.spectrum), below 2^20 and made strictly decreasing from the small end upwards."""
    x = 20.0 * np.arange(n) / max(n - 1, 1)
    s = np.ldexp(1.0 - 0.5 * (x - np.floor(x)), -np.floor(x).astype(np.int64))
    d = np.minimum(np.floor(s * float(1 << 20)).astype(np.int64), (1 << 20) - 1)
    d = np.maximum(d, 1)
    for i in range(n - 2, -1, -1):
        d[i] = max(d[i], d[i + 1] + 1)
    assert d[0] < (1 << 20) and np.all(np.diff(d) < 0)
    return d


class Exact:
    """One matrix of the exact family.  ``G`` float64 (read-only), ``truth`` its eigenvalues in descending order (long
    double, exact), ``vectors(cols)`` the eigenvectors of those eigenvalues (long double, exact wherever P is a power of
    two), ``apply(W)`` G W in long double through H D H - O(n k) instead of O(n^2 k)."""

    def __init__(self, spectrum, n):
        assert spectrum in SPECTRA and n >= 3
        rng = np.random.RandomState(7000 * (1 + SPECTRA.index(spectrum)) + n)
        found = fill(n)
        if found is None:
            P, counts, self.scale = n, (0, 0, 0), 1          # the integer matrix P^2 G itself
        else:
            (P, counts), self.scale = found, None
        a, b, c = counts
        mag = np.r_[np.ones(n - 1 - a - b - c, dtype=np.int64), np.full(a, 2), np.full(b, 3), np.full(c, 4)].astype(np.int64)
        v = np.r_[1, mag[rng.permutation(n - 1)]] * (2 * rng.randint(0, 2, size=n) - 1)
        assert int(np.sum(v * v)) == P and np.all(v != 0) and abs(int(v[0])) == 1
        if spectrum == "spread":
            D = rng.choice((1 << 20) - 1, size=n, replace=False).astype(np.int64) + 1
        else:
            D = graded_integers(n)[rng.permutation(n)]
        assert len(set(D.tolist())) == n and D.min() >= 1 and D.max() < (1 << 20)
        self.spectrum, self.n, self.P, self.v, self.D = spectrum, n, int(P), v, D
        S = int(np.sum(v * v * D))
        vv = np.outer(v, v)
        M = -2 * P * vv * (D[:, None] + D[None, :]) + 4 * vv * S          # int64, exact
        M[np.arange(n), np.arange(n)] += P * P * D
        assert int(np.abs(M).max()) < (1 << 53), "P^2 G does not fit float64's integers"
        self.M = M                                                       # P^2 G
        G = M.astype(np.float64)
        if self.scale is None:
            assert P & (P - 1) == 0
            G = G / float(P * P)                                         # a power of two: exact
            self.factor = 1
        else:
            self.factor = P * P
        assert np.array_equal(G, G.T)
        G.setflags(write=False)
        self.G = G
        self.order = np.argsort(-D, kind="stable")
        self.truth = (D[self.order] * self.factor).astype(LD)

    def vectors(self, cols):
        """Columns ``cols`` (indices into the descending spectrum) of H, in long double."""
        p = self.order[np.asarray(cols)]
        vl = self.v.astype(LD)
        Hc = -2 * vl[:, None] * vl[p][None, :] / LD(self.P)
        Hc[p, np.arange(len(p))] += 1
        return Hc

    def apply(self, Wl):
        vl = self.v.astype(LD)[:, None]
        Y = Wl - vl * (2 * (vl * Wl).sum(axis=0) / LD(self.P))
        Y = Y * (self.D.astype(LD) * self.factor)[:, None]
        return Y - vl * (2 * (vl * Y).sum(axis=0) / LD(self.P))


@functools.lru_cache(maxsize=None)
def exact(spectrum, n):
    return Exact(spectrum, n)


def exact_cases(sizes=EXACT_SIZES):
    return [(s, n) for n in sizes for s in SPECTRA]


def exact_label(spectrum, n):
    return f"exact-{spectrum}-{n}"


def recorded_label(kind, n):
    return f"recorded-{kind}-{n}"


def columns(n):
    """The columns the figures of a size are taken over (LAPACK's record and the device alike): all of them up to
    ``FULL_K_MAX``, beyond it the leading 128 and the slice, if the size has one."""
    if n <= FULL_K_MAX:
        return np.arange(n)
    cols = np.arange(max(LARGE_KS))
    if n in SLICES:
        first, count = SLICES[n]
        cols = np.r_[cols, np.arange(first, first + count)]
    return cols


# ---- what is measured ---------------------------------------------------------------------------------------------------
def measure(truth, lam_idx, lam, cols, W, apply_G, H=None, skip=()):
    """dict(lam, res, norm, orth, vec, vec_abs) of eigenvalues ``lam`` (those of the indices ``lam_idx`` of the descending
    spectrum) and vectors ``W`` (those of the indices ``cols``, a subset of ``lam_idx``), n = len(truth):
    lam   max_i |lam_i - truth_i| / (n eps lam_1)                                  absolute: a Householder reduction promises no more
    res   max_i ||G w_i - lam_i w_i||_2 / (n eps lam_1)                           the returned columns, no QR first
    norm  max_i | ||w_i||_2 - 1 | / eps
    orth  max_{i != j} |w_i . w_j| min(|truth_i - truth_j| / lam_1, 1) / (n eps)  pairs inside ``skip`` (a cluster) left out
    vec   max_i ||w_i - s h_i||_2 gap_i / (n eps lam_1), s = sign(w_i . h_i),     ``H``: the true vectors of ``cols``;
          gap_i the distance from truth_i to the rest of the spectrum; ``vec_abs``: ||w_i - s h_i||_2 per column
    Every product in long double: the figures are the solver's, not the check's."""
    n = len(truth)
    truth = np.asarray(truth, dtype=LD)
    lam_idx, cols = np.asarray(lam_idx), np.asarray(cols)
    lam1 = truth[0]
    unit = n * EPS * lam1
    lam_l, Wl = np.asarray(lam).astype(LD), np.asarray(W).astype(LD)
    assert lam_l.shape == lam_idx.shape and Wl.shape == (n, len(cols))
    out = dict(lam=float(np.max(np.abs(lam_l - truth[lam_idx])) / unit))
    where = {int(i): q for q, i in enumerate(lam_idx)}
    lam_c = lam_l[[where[int(i)] for i in cols]]
    R = apply_G(Wl) - Wl * lam_c
    out["res"] = float(np.max(np.sqrt(np.sum(R * R, axis=0))) / unit)
    out["norm"] = float(np.max(np.abs(np.sqrt(np.sum(Wl * Wl, axis=0)) - 1)) / EPS)
    t = truth[cols]
    weight = np.minimum(np.abs(t[:, None] - t[None, :]) / lam1, 1)
    np.fill_diagonal(weight, 0)
    inside = np.isin(cols, np.asarray(skip, dtype=np.int64))
    weight[np.ix_(inside, inside)] = 0
    out["orth"] = float(np.max(np.abs(Wl.T @ Wl) * weight) / (n * EPS)) if len(cols) > 1 else 0.0
    if H is not None:
        s = np.where(np.sum(Wl * H, axis=0) < 0, -1, 1).astype(LD)
        dist = np.sqrt(np.sum((Wl - H * s) ** 2, axis=0))
        srt = np.sort(truth)
        pos = np.searchsorted(srt, t)
        lo = np.where(pos > 0, t - srt[np.maximum(pos - 1, 0)], np.inf)
        hi = np.where(pos < n - 1, srt[np.minimum(pos + 1, n - 1)] - t, np.inf)
        gap = np.minimum(lo, hi)
        out["vec"] = float(np.max(dist * gap) / unit)
        out["vec_abs"] = dist.astype(np.float64)
    return out


def dense_apply(G):
    Gl = np.asarray(G).astype(LD)
    return lambda Wl: Gl @ Wl


def separated_prefix(truth, limit=None):
    """The largest k <= ``limit`` for which ``pod_rules.separated(truth, k)`` holds (0: none)."""
    from romtime_amd import pod_rules

    t = np.asarray(truth, dtype=np.float64)
    best = 0
    for k in range(1, (len(t) if limit is None else min(limit, len(t))) + 1):
        if pod_rules.separated(t, k):
            best = k
    return best


def format_line(tag, label, got, ref):
    parts = [f"{key}={got[key]:.3f} ({ref[key]:.3f})" for key in FIGURES if key in got and key in ref]
    return f"{tag} {label} " + " ".join(parts)


# ---- the reduction and the blocked back-transformation, restated ------------------------------------------------------------
def tridiagonalise(G):
    """(d, e, V, tau) of the Householder reduction of csrc/symeig.hip in float64: step k takes row k, entries j > k
    (dlarfg), p = tau A v, w = p - (tau / 2)(p . v) v, A -= v w^T + w v^T.  Row k of V holds the reflector of step k
    (V[k, k + 1] = 1); e[k] is the off-diagonal entry between k and k + 1."""
    A = np.array(G, dtype=np.float64)
    n = A.shape[0]
    d, e, tau, V = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, n))
    for k in range(n - 2):
        x = A[k, k + 1:].copy()
        alpha, part = x[0], float(np.sum(x[1:] ** 2))
        d[k] = A[k, k]
        if part == 0.0:
            e[k] = alpha
            continue
        beta = -np.copysign(np.sqrt(alpha * alpha + part), alpha)
        tau[k] = (beta - alpha) / beta
        v = np.r_[1.0, x[1:] / (alpha - beta)]
        V[k, k + 1:] = v
        e[k] = beta
        B = A[k + 1:, k + 1:]
        p = tau[k] * (B @ v)
        w = p - 0.5 * tau[k] * (p @ v) * v
        B -= np.outer(v, w) + np.outer(w, v)
    d[n - 2], e[n - 2], d[n - 1] = A[n - 2, n - 2], A[n - 2, n - 1], A[n - 1, n - 1]
    return d, e, V, tau


def back_transform(V, tau, Z, rb=4, zero_block=None):
    """x = H_0 H_1 ... H_{n-3} z for every column of Z, the reflectors taken ``rb`` at a time from the last, as
    symeig_vectors_kernel does: a_u = v_u . z for the incoming z, s_u = tau_u (a_u - sum_{w<u} (v_u . v_w) s_w),
    z -= sum_u s_u v_u; reflectors past the first (k < 0, the last, partial block) are zero.  rb = 1 is the
    reflector-by-reflector application.  ``zero_block``: the block whose cross products are zeroed (a broken kernel)."""
    n = V.shape[0]
    Z = np.array(Z, dtype=V.dtype)
    blk = 0
    for k0 in range(n - 3, -1, -rb):
        ks = [k0 - u for u in range(rb)]
        vs = [V[k] if k >= 0 else np.zeros(n, dtype=V.dtype) for k in ks]
        ts = [tau[k] if k >= 0 else 0.0 for k in ks]
        a = [v @ Z for v in vs]
        s = []
        for u in range(rb):
            r = a[u]
            for w in range(u):
                c = 0.0 if blk == zero_block else vs[u] @ vs[w]
                r = r - c * s[w]
            s.append(ts[u] * r)
        for u in range(rb):
            Z -= np.outer(vs[u], s[u])
        blk += 1
    return Z


# ---- LAPACK on the same matrices ---------------------------------------------------------------------------------------------
def lapack_eigh(G):
    lam, W = np.linalg.eigh(np.asarray(G))
    return lam[::-1].copy(), W[:, ::-1].copy()


def compute_lapack_reference(label):
    """LAPACK's figures on the matrix of ``label`` over ``columns(n)``."""
    family, kind, n = label.split("-", 1)[0], label.split("-", 1)[1].rsplit("-", 1)[0], int(label.rsplit("-", 1)[1])
    cols = columns(n)
    if family == "exact":
        ex = exact(kind, n)
        lam, W = lapack_eigh(ex.G)
        return measure(ex.truth, np.arange(n), lam, cols, W[:, cols], ex.apply, H=ex.vectors(cols))
    G, _ = jc.matrix(kind, n)
    lam, W = lapack_eigh(G)
    skip = np.arange(CLUSTER) if kind == "cluster" and n > CLUSTER else ()
    return measure(jc.truth(kind, n), np.arange(n), lam, cols, W[:, cols], dense_apply(G), skip=skip)


def all_labels():
    return [exact_label(s, n) for s, n in exact_cases()] + [recorded_label(k, n) for k, n in jc.cases(jc.GPU_SIZES)]


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def lapack_reference(label):
    """Recorded dict(lam, res, norm, orth[, vec]) of np.linalg.eigh on the matrix of ``label``."""
    return dict(_golden()["figures"][label])


def bar(ref_ratio, factor=BAR_FACTOR):
    return min(factor * max(1.0, ref_ratio), BAR_CAP)
