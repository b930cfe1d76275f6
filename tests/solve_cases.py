"""Shared pieces of the reduced-solve tests (tests/test_reduced_solves_cpu.py, tests/test_reduced_solves_gpu.py and the
sweep tests of tests/test_kernels_gpu.py).  Plain module, not a conftest; everything here runs on the host.

* ``exact_lu_system`` and ``wilkinson_system``: systems whose pivoted LU is exact in float64, so that the device answer
  must equal the known solution bit for bit; ``retiring_lu_solve`` restates the elimination of ``lu_solve_lds``
  (solve.hip) and ``lu_waves`` its thread mapping, to prove the premise on the host; ``tied=True`` puts two equal
  pivot candidates in different waves, of which only the kernel's documented choice keeps the answer exact.
* ``conditioned_system``, ``reference_solve`` and ``solve_errors``: systems of a chosen condition number, their
  solution to 50 digits (mpmath) and the two error measures the ratio bar compares with LAPACK's.
* ``tracked_model``: a NumPy restatement of the decisions of ``newton_solve_kernel``.  It is used to CHOOSE inputs
  that take a wanted route with a margin; it is not the reference of any answer.
* ``synthetic_hrom_terms``: random interpolation terms for ``hrom_bdf_sweep`` / ``oracle.hrom_solve``.
* ``GuardedInt32``: the int32 twin of ``tests.guarded.GuardedOutput`` for the kernels' ``info`` arrays.
"""
from __future__ import annotations

import mpmath
import numpy as np
import torch

from romtime_amd._lib import WARN_SINGULAR  # noqa: F401  (RT_WARN_SINGULAR; loading the binding needs no GPU)

EPS = 2.2e-16

# The ratio bar: error <= F * max(LAPACK's error on the same system, r EPS), (forward, backward) per entry point.
# F = ten times the worst ratio measured on an MI355X over the cases of tests/test_reduced_solves_gpu.py and of
# tests/test_kernels_gpu.py::test_dense_solve (figures in the docstrings there), never more than 100.  Worst ratios:
# batched 1.34 / 0.079, multi 1.25 / 0.060, tracked 2.7 / 0.275.
F_BATCHED = (13.4, 0.79)
F_MULTI = (12.5, 0.6)
F_TRACKED = (27.0, 2.75)

# ---- sizes -----------------------------------------------------------------------------------------------------------
# rt_dense_solve_batched / _multi: both sides of every change of parts = min(8, 256 / r), the second back-substitution
# slot (r = 65) and the ends
LU_SIZES = [1, 2, 31, 32, 33, 36, 37, 42, 43, 51, 52, 63, 64, 65, 85, 86, 127, 128]
WILKINSON_SIZES = [20, 50]            # entries of the factors stay below 2^53
TIED_SIZES = [20, 50, 128]            # a tied first column across the waves of the LU kernels (256 threads)
FALLBACK_SIZES = [12, 50, 64, 80]     # in-kernel LU of the tracked solve (512 threads)
LADDER_SIZES = [5, 16, 40, 50, 64, 80]  # tile layouts 1, 1, 3, 4, 4, 5; 16, 64 and 80 take the 16-byte path
SOLVE_THREADS, NS_THREADS = 256, 512


def lu_parts(r, threads=SOLVE_THREADS):
    return min(8, threads // r)


def lu_waves(rows, r, threads=SOLVE_THREADS):
    """The wave of lu_solve_lds that owns each of ``rows``: thread = row * parts + part, 64 threads per wave."""
    return (np.asarray(rows) * lu_parts(r, threads)) // 64


# ---- systems whose LU is exact -----------------------------------------------------------------------------------------
def small_integers(rng, shape):
    """Nonzero integers in [-8, 8] as float64."""
    return (rng.randint(1, 9, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float64)


def exact_lu_system(r, rng, tiny_last=False, tied=False):
    """K, b, x with K = (L U)[perm]: L unit lower triangular with multipliers in {0, +-1/4, +-1/2}, U upper triangular
    with integers in [-3, 3] above a diagonal of +-2^k (k = 2..4), x nonzero integers in [-8, 8] (a zero unknown comes
    out as +0 or -0 with the sign of the pivot, which a bitwise comparison would have to excuse), b = K x.

    Every multiplier is below 1 in modulus: partial pivoting meets a strictly largest candidate in every column and
    recovers these factors.  Every intermediate is a small multiple of 1/4 and every diagonal a power of two, so each
    product, sum, quotient and reciprocal is exact in float64 in any order, with or without FMA.

    ``tiny_last``: the last column of U is 2^-60 e_r (condition number about 2^60; Newton-Schulz cannot reach its
    residual, the LU is still exact).  The last column of K is then 2^-60 in one row and zero elsewhere, and the last
    unknown is an integer times 2^60, so that b stays exactly representable.

    ``tied`` (r > 1): the pivot of column 0 sits in row 0 of K and the LAST row of K gets the multiplier +-1, so the
    first pivot search meets two equal candidates in different waves.  Taking row 0 - the (|value| desc, row asc) order
    of the kernel, and LAPACK's - is the exact factorisation above.  Taking the other one is a valid factorisation
    too, but its Schur complement is no longer the designed one: the next pivots are no powers of two, the multipliers
    no dyadic fractions, and the answer comes out rounded.  Only the documented order returns x bit for bit."""
    mult = np.array([0.0, 0.25, -0.25, 0.5, -0.5])
    L = np.tril(mult[rng.randint(0, 5, size=(r, r))], -1) + np.eye(r)
    U = np.triu(rng.randint(-3, 4, size=(r, r)).astype(np.float64), 1)
    U += np.diag(rng.choice([-1.0, 1.0], size=r) * 2.0 ** rng.randint(2, 5, size=r))
    x = small_integers(rng, r)
    if tiny_last:
        U[:, r - 1] = 0.0
        U[r - 1, r - 1] = 2.0 ** -60
        x[r - 1] = float(rng.randint(1, 9)) * 2.0 ** 60
    perm = rng.permutation(r)
    if tied and r > 1:
        perm = np.r_[0, perm[perm != 0]]
        L[perm[-1], 0] = rng.choice([-1.0, 1.0])
    K = (L @ U)[perm]
    return K, K @ x, x


def wilkinson_system(r, rng):
    """The growth matrix: unit diagonal, -1 below it, last column 1.  Every column's candidates tie at 1, the lowest
    row (the diagonal) wins, no rows are exchanged and the last column doubles at every step (2^(r-1) < 2^53).  (Not a
    test of the order among equals: all multipliers are +-1, so any choice stays exact - ``exact_lu_system(tied=True)`` is.)
    x nonzero integers in [-8, 8]; b and every update of it are integers that float64 holds exactly (checked on the host
    by tests/test_reduced_solves_cpu.py)."""
    K = np.eye(r) - np.tril(np.ones((r, r)), -1)
    K[:, r - 1] = 1.0
    x = small_integers(rng, r)
    return K, K @ x, x


def retiring_lu_solve(K, b, other_tie_order=False, threads=SOLVE_THREADS):
    """The elimination of lu_solve_lds on the host: rows are not exchanged but retired once they have served as
    pivot; the pivot of column c is the live row with the largest |entry| and, among equals, the lowest index.
    Returns x, the pivot row of every column, and (best, runner-up) candidate moduli per column (runner-up -1 when
    one row is left).  ``other_tie_order``: among equal candidates of different waves (of a workgroup of ``threads``)
    take the highest wave's - the order the kernel must NOT have; the host test uses it to show that the tied systems
    then lose their exact answer."""
    A = np.array(K, dtype=np.float64)
    y = np.array(b, dtype=np.float64)
    r = A.shape[0]
    live = np.ones(r, dtype=bool)
    piv, margins = [], []
    for c in range(r):
        cand = np.where(live, np.abs(A[:, c]), -1.0)
        p = int(np.argmax(cand))                     # first occurrence of the maximum: lowest row among equals
        if other_tie_order:
            tied = np.nonzero(cand == cand[p])[0]
            waves = lu_waves(tied, r, threads)
            p = int(tied[waves == waves.max()][0])
        rest = np.delete(cand, p)
        margins.append((float(cand[p]), float(rest.max()) if rest.size else -1.0))
        piv.append(p)
        live[p] = False
        rows = np.nonzero(live)[0]
        l = A[rows, c] / A[p, c]
        A[rows, c + 1:] -= l[:, None] * A[p, c + 1:][None, :]
        y[rows] -= l * y[p]
    x = np.zeros(r)
    for c in range(r - 1, -1, -1):
        p = piv[c]
        x[c] = (y[p] - A[p, c + 1:] @ x[c + 1:]) / A[p, c]
    return x, np.array(piv), margins


# ---- conditioned systems and the 50-digit reference ------------------------------------------------------------------------
def conditioned_system(r, e, rng):
    """K = U diag(s) V^T with s geometric from 1 to 10^-e, and a random right-hand side."""
    U, _ = np.linalg.qr(rng.standard_normal((r, r)))
    V, _ = np.linalg.qr(rng.standard_normal((r, r)))
    s = 10.0 ** (-e * np.arange(r) / max(r - 1, 1))
    return (U * s) @ V.T, rng.standard_normal(r)


def _mp_array(a):
    flat = [mpmath.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]
    out = np.empty(len(flat), dtype=object)
    out[:] = flat
    return out.reshape(np.shape(a))


def reference_solve(K, b, digits=50):
    """The solution of K x = b (the float64 data taken as exact) to ``digits`` digits, rounded to float64.

    Iterative refinement whose residuals b - K x are formed in ``digits``-digit arithmetic (mpmath) and whose
    corrections come from LAPACK: every pass gains about 16 - log10(cond) digits, and the loop ends when a correction
    is below 10^-(digits - 15) of the iterate - checked, so a system too ill-conditioned for this fails loudly instead
    of returning a poor reference.  Far cheaper than an LU in mpmath (r^2 instead of r^3 multi-precision operations per
    pass), which is what lets every answer of the tests be compared with it."""
    K = np.asarray(K, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    with mpmath.workprec(int(digits * 3.33) + 8):
        Km, bm = _mp_array(K), _mp_array(b)
        x = _mp_array(np.zeros_like(b))
        for _ in range(60):
            res = bm - Km.dot(x)
            d = np.linalg.solve(K, np.array([float(v) for v in res.reshape(-1)]).reshape(b.shape))
            x = x + _mp_array(d)
            xn = max(abs(float(v)) for v in x.reshape(-1))
            if np.abs(d).max() <= 10.0 ** -(digits - 15) * xn:
                break
        else:
            raise AssertionError("reference_solve did not converge: the system is singular to working precision")
        return np.array([float(v) for v in x.reshape(-1)]).reshape(b.shape)


def solve_errors(K, b, x, x_ref):
    """(forward error relative to the reference, normwise backward error |b - K x| / (|K|_2 |x| + |b|))."""
    x = np.asarray(x, dtype=np.float64)
    fwd = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    res = (b.astype(np.longdouble) - K.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64)
    bwd = np.linalg.norm(res) / (np.linalg.norm(K, 2) * np.linalg.norm(x) + np.linalg.norm(b))
    return float(fwd), float(bwd)


def error_ratios(K, b, x, x_ref):
    """The device's forward and backward error over max(LAPACK's on the same system, r eps): what the bar F bounds."""
    r = K.shape[0]
    dev = solve_errors(K, b, x, x_ref)
    lap = solve_errors(K, b, np.linalg.solve(K, b), x_ref)
    return tuple(d / max(l, r * EPS) for d, l in zip(dev, lap))


# ---- the decisions of newton_solve_kernel, restated --------------------------------------------------------------------
NS_MAX_ITER, NS_REFINE_MAX, NS_REFRESH_AFTER = 100, 8, 5
NS_REFINE_TOL, NS_REFINE_RATE = 2e-15, 0.3


def _safe_start(K):
    return K.T / (np.abs(K).sum(axis=0).max() * np.abs(K).sum(axis=1).max())


def tracked_model(K, b, X=None):
    """Which way newton_solve_kernel goes for K x = b from the carried inverse ``X`` (None: first call), in float64
    NumPy.  Returns a dict: ``route`` ("first", "refine", "refine_refresh", "newton", "restart", "fallback", or
    "refresh_failed" where the refinement has solved but the refresh then does not converge),
    ``newton_iterations``, ``restarts``, ``lu_fallbacks`` as the kernel counts them, ``refine_steps`` (None when the
    refinement did not solve), ``refine_res`` (|b - K x| / |b| at every refinement test), ``ns_res`` (|I - K X|_F at
    every Newton-Schulz test), and ``X`` (the inverse the kernel would leave; zeros after a fallback)."""
    r = K.shape[0]
    have_prev = X is not None
    X = _safe_start(K) if X is None else np.array(X)
    out = dict(refine_steps=None, refine_res=[], ns_res=[], newton_iterations=0, restarts=0, lu_fallbacks=0)
    solved = False
    if have_prev:
        bn2 = b @ b
        x = X @ b
        prev = 1e300
        for it in range(NS_REFINE_MAX + 1):
            e = b - K @ x
            rn2 = e @ e
            out["refine_res"].append(float(np.sqrt(rn2 / bn2)))
            if not rn2 == rn2:
                break
            if rn2 <= NS_REFINE_TOL ** 2 * bn2 or (it > 0 and rn2 >= 0.25 * prev and rn2 <= 1e-26 * bn2):
                solved, out["refine_steps"] = True, it
                break
            if it == NS_REFINE_MAX or rn2 > NS_REFINE_RATE ** 2 * prev:
                break
            prev = rn2
            x = x + X @ e
        if solved and out["refine_steps"] <= NS_REFRESH_AFTER:
            return dict(out, route="refine", X=X)
    restarted, status = not have_prev, WARN_SINGULAR
    for _ in range(NS_MAX_ITER):
        out["newton_iterations"] += 1
        T = K @ X
        res = np.linalg.norm(np.eye(r) - T)
        out["ns_res"].append(float(res))
        if res != res:
            break
        if not restarted and not res < 0.7:
            restarted, out["restarts"] = True, 1
            X = _safe_start(K)
            continue
        X = 2.0 * X - X @ T
        if res < 1e-6:
            status = 0
            break
    if status != 0:
        if solved:
            return dict(out, route="refresh_failed", X=np.zeros_like(K))
        return dict(out, route="fallback", lu_fallbacks=1, X=np.zeros_like(K))
    route = "refine_refresh" if solved else ("first" if not have_prev else ("restart" if out["restarts"] else "newton"))
    return dict(out, route=route, X=X)


def scaled_permutation_system(r, rng):
    """K with one nonzero per row and column, K[i, s(i)] = k_i (1 <= |k_i| <= 4), a right-hand side, and s.

    Every sum in newton_solve_kernel then has a single nonzero term, so each entry of every Newton-Schulz iterate is the
    outcome of a few correctly rounded scalar operations that ``scaled_permutation_first_call`` repeats on the host:
    the inverse the kernel leaves and its answer are known bit for bit.  T = K X is diagonal, and s is drawn so that the
    nonzeros of X and of X T fall in every full 16 x 16 tile (and in as many of the partial ones at the edge as the
    draw gives): a tile of a product that no wave computes, that two waves compute, or that comes out scaled shows in
    the bits of Xinv.  The k_i are redrawn until no residual the kernel tests against 1e-6 lies within a factor ten of
    it, so that the iteration count does not hang on the order of a sum."""
    full = max(r // 16, 1) if r >= 16 else 0
    for _ in range(10000):
        s = rng.permutation(r)
        K = np.zeros((r, r))
        K[np.arange(r), s] = rng.uniform(1.0, 4.0, size=r) * rng.choice([-1.0, 1.0], size=r)
        b = rng.standard_normal(r)
        tiles = {(int(j) // 16, i // 16) for i, j in enumerate(s)}
        covered = all((a, c) in tiles for a in range(full) for c in range(full))
        if covered and all(v < 1e-7 or v > 1e-5 for v in scaled_permutation_first_call(K, b)[3]):
            return K, b, s
    raise AssertionError("no permutation with an entry in every full tile")


def scaled_permutation_first_call(K, b):
    """A first call of newton_solve_kernel on a ``scaled_permutation_system``, operation by operation: returns x, Xinv,
    the number of Newton-Schulz iterations and the residual |I - K X|_F at every test."""
    r = K.shape[0]
    rows = np.arange(r)
    s = np.abs(K).argmax(axis=1)
    k = K[rows, s]
    sc = 1.0 / (np.abs(k).max() * np.abs(k).max())    # 1 / (|K|_1 |K|_inf)
    x = k * sc                                        # X[s(i), i]
    res_all = []
    for _ in range(NS_MAX_ITER):
        t = k * x                                     # T = K X, diagonal
        res_all.append(float(np.sqrt(np.sum((1.0 - t) ** 2))))
        x = 2.0 * x - x * t                           # X <- 2 X - X T
        if res_all[-1] < 1e-6:
            break
    X = np.zeros((r, r))
    X[s, rows] = x
    x1 = x * b                                        # x = X b, then one refinement step against K
    e = b - k * x1
    sol = np.zeros(r)
    sol[s] = x1 + x * e
    return sol, X, len(res_all), res_all


def ladder_systems(r, B=4):
    """The moving matrices of the tracked-solve ladder: K0 = randn / sqrt(r) + 2 I and a direction dK = randn / sqrt(r)
    for each of B systems, and the generator the right-hand sides are drawn from afterwards."""
    rng = np.random.RandomState(1000 + r)
    K0 = rng.standard_normal((B, r, r)) / np.sqrt(r) + 2.0 * np.eye(r)
    dK = rng.standard_normal((B, r, r)) / np.sqrt(r)
    return K0, dK, rng


# the ladder: (d, route every system must take, from the inverse the previous rung left).  d = 0.03 and 0.3 sit on a
# threshold and change route with r; REFRESH_D is chosen by tests/test_reduced_solves_cpu.py's margin check.
REFRESH_D = 2e-2
LADDER = [(0.0, "refine"), (1e-6, "refine"), (1e-4, "refine"), (1e-3, "refine"), (REFRESH_D, "refine_refresh"),
          (0.1, "newton"), (1.0, "restart"), (3.0, "restart")]


def ladder_calls(r, B=4):
    """Every call of the ladder at size r as (K [B,r,r], b [B,r], route or "first"): a first call with K0, then each
    rung K0 + d dK - each tracked from the inverse a call with K0 leaves, so the rungs do not depend on one another."""
    K0, dK, rng = ladder_systems(r, B)
    calls = [(K0, rng.standard_normal((B, r)), "first")]
    for d, route in LADDER:
        calls.append((K0 + d * dK, rng.standard_normal((B, r)), route))
    return calls


# ---- synthetic interpolation terms for the hyper-reduced sweep ---------------------------------------------------------
def synthetic_hrom_terms(rng, r, nt, n_mu, m_mass, lin, m_nl, m_rhs, wobble_tables=False):
    """Random interpolation terms (mass, lin, nl, rhs) for ``hrom_bdf_sweep`` and ``oracle.hrom_solve``.

    A matrix term is operator(mu, t) = (1 + wobble(mu, t)) * base + small random modes, written as an m-mode
    interpolation expansion.  ``lin``: (m, "spd" | "general") per linear term.  ``wobble_tables``: the wobble of a term
    is a table drawn before the term's modes (and identically zero for the mass); otherwise it is drawn with the
    term's coefficients.  The order of the draws is part of the contract: a given generator state gives the same
    terms every time."""
    spd = lambda: (lambda a: a @ a.T + r * np.eye(r))(rng.standard_normal((r, r)))
    wob = lambda: 0.1 * rng.standard_normal((nt, n_mu))

    def matrix_term(m, base, wobble=None):
        cols = np.concatenate([base.reshape(-1, 1), 0.05 * rng.standard_normal((r * r, m - 1))], axis=1)
        PT_U, _ = np.linalg.qr(rng.standard_normal((m, m)))
        lead = 1.0 + (0.1 * rng.standard_normal((nt, n_mu, 1)) if wobble is None else wobble[..., None])
        theta = np.concatenate([lead, 0.1 * rng.standard_normal((nt, n_mu, m - 1))], axis=-1)
        return dict(PT_U=PT_U, basis_rom=cols, F=theta @ PT_U.T)

    def make(m, kind, zero_wobble=False):
        base = spd() if kind == "spd" else rng.standard_normal((r, r))
        if not wobble_tables:
            return matrix_term(m, base)
        w = wob()
        return matrix_term(m, base, 0.0 * w if zero_wobble else w)

    mass = make(m_mass, "spd", zero_wobble=True)
    lin_terms = [make(m, kind) for m, kind in lin]
    PTn, _ = np.linalg.qr(rng.standard_normal((m_nl, m_nl)))
    nl = dict(PT_U=PTn, basis_rom=0.3 * rng.standard_normal((r * r, m_nl)), W=0.2 * rng.standard_normal((m_nl, r)),
              C=0.1 * rng.standard_normal((nt, n_mu, m_nl)), S=1.0 + 0.1 * rng.standard_normal((nt, n_mu)))
    PTf, _ = np.linalg.qr(rng.standard_normal((m_rhs, m_rhs)))
    rhs = [dict(PT_U=PTf, basis_rom=rng.standard_normal((r, m_rhs)), F=rng.standard_normal((nt, n_mu, m_rhs)))]
    return mass, lin_terms, nl, rhs


# ---- placing operands --------------------------------------------------------------------------------------------------
INT_CANARY = 0x5BADC0DE


class GuardedInt32:
    """``n`` int32 words (``t``) inside a buffer of a fixed pattern: ``check()`` lists pattern words changed outside
    the view and view words never written - tests.guarded.GuardedOutput for the kernels' ``info`` arrays."""

    def __init__(self, n, device="cuda", guard=64):
        self.buf = torch.full((n + 2 * guard,), INT_CANARY, dtype=torch.int32, device=device)
        self.t = self.buf[guard:guard + n]
        self.n, self.guard = n, guard

    def check(self):
        host = self.buf.cpu().numpy()
        inside = np.zeros(host.size, dtype=bool)
        inside[self.guard:self.guard + self.n] = True
        problems = []
        outside = np.nonzero((host != INT_CANARY) & ~inside)[0]
        if outside.size:
            problems.append(f"{outside.size} words written outside info, offsets from its start {(outside[:4] - self.guard).tolist()}")
        unwritten = np.nonzero(host[inside] == INT_CANARY)[0]
        if unwritten.size:
            problems.append(f"{unwritten.size} info words never written, first {int(unwritten[0])}")
        return problems


def place(host, misalign=False, device="cuda"):
    """``host`` as a contiguous float64 tensor whose base address is 16-byte aligned, or 8 bytes past that."""
    host = np.ascontiguousarray(host, dtype=np.float64)
    buf = torch.empty(host.size + 2, dtype=torch.float64, device=device)
    off = (buf.data_ptr() // 8) % 2 + (1 if misalign else 0)
    view = buf[off:off + host.size].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == (8 if misalign else 0)
    return view
