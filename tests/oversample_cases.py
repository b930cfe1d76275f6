"""Shared pieces of the oversampled-(M)DEIM tests (tests/test_oversample_cpu.py, tests/test_oversample_step_gpu.py,
tests/test_oversample_classes_gpu.py).  Plain module, not a conftest; everything here runs on the host.

The rule under test is GappyPOD+E (Peherstorfer, Drmac, Gugercin, SIAM J. Sci. Comput. 42, 2020): starting from the m greedy
entries p of the N x m basis U, until len(p) == m_s,
    1. thin SVD of A = U[p, :];  g = sigma_{m-1}^2 - sigma_m^2,  w = the right singular vector of sigma_m;
    2. rho_i = ||U[i, :]||^2,  c_i = U[i, :] . w,  a_i = g + rho_i,
       score_i = 4 g c_i^2 / (a_i + sqrt(max(a_i^2 - 4 g c_i^2, 0)));
    3. append the argmax over the rows not in p, the lowest index on ties.

* ``direction`` / ``scores`` / ``oversample``: the NumPy restatement of the loop (float64).
* ``certify``: the long-double certificate of ONE pick sequence.  Per step it takes (w, g) from ``np.linalg.svd`` of the
  rows of THAT sequence, in the sequence's order - the float64 numbers any implementation of step 1 hands to step 2 - forms
  every score in ``np.longdouble`` and reports the top score, the pick's shortfall, the true margin and the argmax.
* ``accepted``: the project's rule (tests/deim_cases.py): the pick's score is at least (1 - 1e-9) of the top, which forces
  the true argmax wherever the true margin exceeds 1e-9.
* ``condition``: what keeps the rule meaningful.  float64 rounding of the tiny SVD moves w by about eps sigma_max / gap, i.e.
  a score by about eps sigma_max^2 / g relative to the top; the row sums move c_i by at most (m + 1) eps |U[i, :]| . |w| and
  rho_i by (m + 1) eps rho_i, and the score formula adds a few eps.  ``condition`` is
      eps sigma_max^2 / g + (2 m + 10) eps (|U[i*, :]| . |w|) / |c_i*|       (i* the true argmax),
  and every case of ``TABLE`` stays at or below 1e-11 at every step (asserted in tests/test_oversample_cpu.py), a hundred
  times below 1e-9.
* ``basis``: input families, deterministic from (family, N, m, seed): ``random`` (orthonormal), ``sine`` (orthonormalised
  perturbed sines) and ``bumps`` (leading left singular vectors of shifted Gaussian bumps).
* ``stiff_case``: one step on rows whose norm dwarfs the gap, where the paper's a - sqrt(a^2 - 4 g c^2) cancels to zero in
  float64 and the rewritten quotient does not."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import deim_cases as dc
from tests.svd_cases import _need_extended

LD = np.longdouble
EPS = dc.EPS
NEAR_TIE = dc.NEAR_TIE      # 1e-9, the project's near-tie threshold
CONDITION = 1e-11


# ---- the restatement ----------------------------------------------------------------------------------------------------
def direction(rows):
    """(w, g, sigma) of the rows picked so far (n x m, n >= m >= 2): step 1, with the gap formed as a product."""
    _, s, Vt = np.linalg.svd(np.asarray(rows, dtype=np.float64), full_matrices=False)
    m = rows.shape[1]
    return np.ascontiguousarray(Vt[m - 1]), float((s[m - 2] - s[m - 1]) * (s[m - 2] + s[m - 1])), s


def scores(B, w, g, dtype=np.float64):
    """Step 2 for every row of B in ``dtype`` (float64: the restatement; long double: the truth of a given (w, g))."""
    B, w, g = np.asarray(B, dtype=dtype), np.asarray(w, dtype=dtype), dtype(g)
    rho = (B * B).sum(axis=1)
    c = B @ w
    a = g + rho
    q = dtype(4) * g * c * c
    den = a + np.sqrt(np.maximum(a * a - q, dtype(0)))
    out = np.zeros(B.shape[0], dtype=dtype)
    np.divide(q, den, out=out, where=q > 0)
    return out


def cancelling_scores(B, w, g, dtype=np.float64):
    """The score as the paper writes it, a - sqrt(a^2 - 4 g c^2): a planted fault (tests/test_oversample_cpu.py)."""
    B, w, g = np.asarray(B, dtype=dtype), np.asarray(w, dtype=dtype), dtype(g)
    a = g + (B * B).sum(axis=1)
    c = B @ w
    return a - np.sqrt(np.maximum(a * a - dtype(4) * g * c * c, dtype(0)))


def _top2(score, taken):
    """(argmax, top1, top2) over the rows that are not taken, the lowest index on ties; top2 = -1 where there is none."""
    s = np.where(taken, -np.ones((), dtype=score.dtype), score)
    i = int(np.argmax(s))
    top = s[i]
    if top < 0:
        return -1, s.dtype.type(-1), s.dtype.type(-1)
    s = s.copy()
    s[i] = -1
    return i, top, s.max() if s.size > 1 else s.dtype.type(-1)


def oversample(B, idx, m_s, score_fn=scores, direction_fn=direction, rank=0, allow_taken=False):
    """The loop: ``(idx, PT_U, margin, sigma_min)`` as ``ops.deim_oversample`` returns them.  ``score_fn``,
    ``direction_fn``, ``rank`` (take the rank-th best instead of the best) and ``allow_taken`` plant faults."""
    B = np.asarray(B, dtype=np.float64)
    N, m = B.shape
    idx = [int(i) for i in idx]
    assert len(idx) == m and m >= 2 and m <= m_s <= N
    margin, sigma_min = [], []
    while len(idx) < m_s:
        w, g, s = direction_fn(B[idx])
        sigma_min.append(s[m - 1])
        sc = score_fn(B, w, g)
        taken = np.zeros(N, dtype=bool)
        if not allow_taken:
            taken[idx] = True
        i, top, second = _top2(sc, taken)
        for _ in range(rank):
            taken[i] = True
            i = _top2(sc, taken)[0]
        margin.append(float((top - max(second, 0.0)) / top) if top > 0 else 0.0)
        idx.append(i)
    sigma_min.append(np.linalg.svd(B[idx], compute_uv=False)[m - 1])
    return np.array(idx, dtype=np.int64), B[idx], np.array(margin), np.array(sigma_min)


# ---- the certificate ---------------------------------------------------------------------------------------------------
@dataclass
class Certificate:
    top: np.ndarray          # long double: the largest true score among the free rows
    shortfall: np.ndarray    # long double: top - score of the pick (top + 1 where the pick was not free)
    margin: np.ndarray       # float64: (top1 - top2) / top1 of the true scores
    argmax: np.ndarray       # int64: the true argmax, lowest index on ties
    gap_term: np.ndarray     # float64: eps sigma_max^2 / g
    sum_term: np.ndarray     # float64: (2 m + 10) eps (|U[i*]| . |w|) / |c_i*|
    sigma_min: np.ndarray    # float64: sigma_m before every step and after the last


def step_truth(B, w, g, taken):
    """(long-double scores of every row, argmax, top, second) of one step for the float64 (w, g) an implementation was
    handed and the rows ``taken`` (bool mask)."""
    _need_extended()
    sc = scores(B, w, g, dtype=LD)
    i, top, second = _top2(sc, np.asarray(taken, dtype=bool))
    return sc, i, top, second


def certify(B, idx, m):
    """The certificate of the entries ``idx[m:]`` added to ``idx[:m]`` on the basis B (N x m)."""
    B = np.asarray(B, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    N = B.shape[0]
    assert B.shape[1] == m and idx.min() >= 0 and idx.max() < N
    steps = len(idx) - m
    cert = Certificate(np.empty(steps, LD), np.empty(steps, LD), np.empty(steps), np.empty(steps, np.int64), np.empty(steps),
                       np.empty(steps), np.empty(steps + 1))
    for k in range(steps):
        n = m + k
        w, g, s = direction(B[idx[:n]])
        taken = np.zeros(N, dtype=bool)
        taken[idx[:n]] = True
        sc, i, top, second = step_truth(B, w, g, taken)
        p = idx[n]
        cert.top[k], cert.argmax[k] = top, i
        cert.shortfall[k] = top + 1 if taken[p] else top - sc[p]
        cert.margin[k] = float((top - max(second, LD(0))) / top) if top > 0 else 0.0
        cert.gap_term[k] = EPS * s[0] ** 2 / g if g > 0 else np.inf
        c = float(abs(B[i] @ w))
        cert.sum_term[k] = (2 * m + 10) * EPS * float(np.abs(B[i]) @ np.abs(w)) / c if c > 0 else np.inf
        cert.sigma_min[k] = s[m - 1]
    cert.sigma_min[steps] = np.linalg.svd(B[idx], compute_uv=False)[m - 1]
    return cert


def accepted(cert):
    return cert.top - cert.shortfall >= (LD(1) - LD(NEAR_TIE)) * cert.top


def condition(cert):
    return cert.gap_term + cert.sum_term


def assert_certified(B, idx, m, show=print, label="", cert=None):
    """certify + the acceptance rule on every step + distinct entries in range + sigma_min non-decreasing (interlacing: a
    row more cannot lower it; 4 eps sigma_max covers the rounding of the two small SVDs).  Returns the certificate."""
    idx = np.asarray(idx)
    N = B.shape[0]
    assert idx.min() >= 0 and idx.max() < N and len(set(idx.tolist())) == len(idx), (label, idx)
    cert = cert or certify(B, idx, m)
    rel = (cert.shortfall / cert.top).astype(np.float64)
    show(f"OVERSAMPLE-TRUTH {label} {N}x{m}->{len(idx)} worst shortfall/top={rel.max():.3g} min margin={cert.margin.min():.3g} "
         f"condition={condition(cert).max():.3g} sigma_min {cert.sigma_min[0]:.3g}->{cert.sigma_min[-1]:.3g}")
    bad = np.nonzero(~accepted(cert))[0]
    assert bad.size == 0, (label, "steps whose pick is not the top score", bad[:8], rel[bad[:8]], idx[m + bad[:8]],
                           cert.argmax[bad[:8]])
    clear = cert.margin > NEAR_TIE
    assert np.array_equal(idx[m:][clear], cert.argmax[clear]), label
    smax = np.linalg.svd(B[idx], compute_uv=False)[0]
    assert np.all(np.diff(cert.sigma_min) >= -4 * EPS * smax), (label, cert.sigma_min)
    return cert


# ---- input families -----------------------------------------------------------------------------------------------------
def basis(family, N, m, seed=0):
    """The float64 N x m basis of a family (C order, orthonormal columns)."""
    if family == "random":
        return dc.basis("random", N, m, seed)
    if family == "sine":
        noise = dc._rng("sine-noise", N, m, seed).standard_normal((N, m))
        return np.linalg.qr(dc.basis("sine", N, m, seed) + 1e-2 / np.sqrt(N) * noise)[0]
    if family == "bumps":
        x = np.linspace(0.0, 1.0, N)
        centres = np.linspace(0.0, 1.0, 3 * m)
        X = np.exp(-((x[:, None] - centres[None, :]) * m) ** 2)
        return np.ascontiguousarray(np.linalg.svd(X, full_matrices=False)[0][:, :m])
    raise ValueError(family)


def greedy(B):
    """The m greedy DEIM entries the loop starts from (the oracle's restatement of deim.py:517-561)."""
    from oracle import romtime_oracle as oracle

    return np.asarray(oracle.deim_greedy(np.asarray(B, dtype=np.float64))[0], dtype=np.int64)


SHAPES = [(257, 8, 16), (1000, 16, 32), (4099, 32, 48), (4099, 64, 128)]
FAMILIES = ("random", "sine", "bumps")
TABLE = [(f, N, m, m_s) for N, m, m_s in SHAPES for f in FAMILIES]


def label(case):
    return "{}-{}x{}-to-{}".format(*case)


def stiff_case(N=64):
    """(B, idx, m): picked rows diag(1, 1/2) - so w = +-e_2 and g = 3/4 - and free rows (2^20, c_i), 1/2 <= c_i <= 1, the
    largest c not at the lowest free index.  True scores are about 3 c_i^2 / 2^41: the rewritten quotient resolves them,
    a - sqrt(a^2 - q) is 0.0 for every row (q / a^2 is below eps)."""
    c = 0.5 + 0.5 * dc._rng("stiff", N, 2, 0).random_sample(N)
    B = np.stack([np.full(N, 2.0 ** 20), c], axis=1)
    B[0], B[1] = (1.0, 0.0), (0.0, 0.5)
    B[2, 1] = 0.5                                   # the lowest free row is the worst
    return B, np.array([0, 1], dtype=np.int64), 2
