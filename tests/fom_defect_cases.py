"""Cases and references of the certified full-order sweep tests (test_fom_defect_cpu.py, test_fom_defect_gpu.py):
rt_p1_fom_bdf_sweep_certified holds a step by the componentwise backward error of its solve,

    omega = max_i |rhs_i - (l_i x_{i-1} + d_i x_i + u_i x_{i+1})| / (|l_i x_{i-1}| + |d_i x_i| + |u_i x_{i+1}| + |rhs_i|),

not by diagonal dominance.  The convective cases are MockBurgers at alpha_0 = 1e-6 .. 1e-4 (CFL 3 to 90 at these sizes):
dominance is lost from nx = 65 on, and the unpivoted elimination is as good as ever.  The flag cases are linear problems
whose diagonal all but vanishes in one step of one point: regular systems that an unpivoted elimination solves badly.

``step_rows`` forms a step's rows in float64 by the formulas of include/romtime_hip.h; ``omega_of`` evaluates the
residual in np.longdouble.  ``OMEGA_REF`` is the worst omega of a float64 sequential (Thomas, unpivoted) elimination over
the convective cases - what the arithmetic gives without any partitioning.  Truth, host loop and bar are those of
tests/fom_cases.py, unchanged.  Plain module, not a conftest."""
from __future__ import annotations

import functools

import numpy as np

from romtime_amd.testing.mock import MockBurgers
from tests import fom_cases as fc

DT = 1.0 / 24.0
NT = 12
CONV_MUS = [dict(alpha_0=1e-6, delta=0.1, omega=6.0), dict(alpha_0=1e-4, delta=0.15, omega=4.0),
            dict(alpha_0=1e-5, delta=0.3, omega=9.0)]
# a single row, inactive lanes, one row per partition (pure cyclic reduction), the first two-row partitioning with a
# short last partition, a full one, and three rows per partition
CONV_NX = [2, 3, 4, 65, 1024, 1025, 1026, 2049, 2050, 3100]
FLAG_NX = [5, 1027, 2051]
FLAG_EPS = 1e-10
DEFECT_TOL = 1e-10


def _Lt(t, **mu):
    return 1.0 - 0.1 * np.sin(mu["omega"] * t)


def make_fom(nx, nt, bdf2, T=None):
    fom = MockBurgers(domain=dict(L0=1.0, nx=nx, T=DT * nt if T is None else T, nt=nt), Lt=_Lt, bdf2=bdf2)
    fom.setup()
    return fom


# ---- a step's rows and the defect of a state ---------------------------------------------------------------------------------
def step_rows(nx, row7, dt, two, state_in_w, un, un1):
    """(l, d, u, rhs), each (n_mu, nx - 1) float64: the interior rows of one step by the header's formulas, from the table
    rows ``row7`` (n_mu, 7) and the two older states (n_mu, nx + 1); l_1 = u_{nx-1} = 0."""
    Nh = nx + 1
    h, alpha, c0, c1, a0, a1, a2 = (np.asarray(row7, dtype=np.float64)[:, q][:, None] for q in range(7))
    bdf = 1.5 if two else 1.0
    ustar = 2 * un - un1 if two else un
    past = 2 * un - un1 / 2 if two else un
    ramp = (np.arange(Nh) / np.float64(nx))[None, :]
    with np.errstate(all="ignore"):
        w = (ustar if state_in_w else 0 * ustar) + c0 + c1 * ramp
        a = (2 * w[:, :-1] + w[:, 1:]) / 6
        b = (w[:, :-1] + 2 * w[:, 1:]) / 6
        lo = bdf * h / 6 + dt * (-alpha / h - b[:, :-1])
        di = bdf * 4 * h / 6 + dt * (2 * alpha / h + b[:, :-1] - a[:, 1:])
        up = bdf * h / 6 + dt * (-alpha / h + a[:, 1:])
        x = np.arange(Nh)[None, :] * h
        f = lambda z: a0 + a1 * z + a2 * z * z
        load = h / 3 * (f(x - h / 2) + f(x) + f(x + h / 2))
        r = h / 6 * (past[:, :-2] + 4 * past[:, 1:-1] + past[:, 2:]) + dt * load[:, 1:-1]
    lo, up = lo.copy(), up.copy()
    lo[:, 0] = 0.0
    up[:, -1] = 0.0
    return lo, di, up, r


def omega_of(lo, di, up, r, x, normwise=False):
    """(n_mu,) componentwise backward error of the states ``x`` (n_mu, nx + 1, zero ends) for the float64 rows, residual
    and denominator in np.longdouble; 0/0 = 0, +inf where anything is not finite.  ``normwise``: the normwise one,
    max|res| / (max_i (|l_i| + |d_i| + |u_i|) max|x| + max|rhs|), for the record only."""
    L = lambda v: np.asarray(v, dtype=np.longdouble)
    lo, di, up, r, x = L(lo), L(di), L(up), L(r), L(x)
    with np.errstate(all="ignore"):
        tl, tc, tr = lo * x[:, :-2], di * x[:, 1:-1], up * x[:, 2:]
        res = np.abs(r - (tl + tc + tr))
        den = np.abs(tl) + np.abs(tc) + np.abs(tr) + np.abs(r)
        q = np.where(den > 0, res / np.where(den > 0, den, 1), 0)
        if normwise:
            scale = (np.abs(lo) + np.abs(di) + np.abs(up)).max(axis=1) * np.abs(x).max(axis=1) + np.abs(r).max(axis=1)
            q = res / np.where(scale > 0, scale, 1)[:, None]
    finite = np.isfinite(res).all(axis=1) & np.isfinite(den).all(axis=1) & np.isfinite(x).all(axis=1)
    return np.where(finite, q.max(axis=1), np.inf).astype(np.float64)


def thomas(lo, di, up, r):
    """Sequential elimination without pivoting in float64, vectorised over the points: (n_mu, n) -> (n_mu, n)."""
    lo, di, up, r = (np.ascontiguousarray(v.T) for v in (lo, di, up, r))
    n = di.shape[0]
    c, d = np.empty_like(di), np.empty_like(di)
    with np.errstate(all="ignore"):
        c[0], d[0] = up[0] / di[0], r[0] / di[0]
        for k in range(1, n):
            den = di[k] - lo[k] * c[k - 1]
            c[k], d[k] = up[k] / den, (r[k] - lo[k] * d[k - 1]) / den
        x = np.empty_like(di)
        x[-1] = d[-1]
        for k in range(n - 2, -1, -1):
            x[k] = d[k] - c[k] * x[k + 1]
    return x.T


def _older(U, u_init, s):
    """u^n and u^{n-1} of step s of the block U (n_mu, nt, N_h) that starts from ``u_init`` (n_mu, 2, N_h) or zero."""
    zero = np.zeros_like(U[:, 0])
    first = zero if u_init is None else u_init[:, 0]
    second = zero if u_init is None else u_init[:, 1]
    return (U[:, s - 1] if s >= 1 else first), (U[:, s - 2] if s >= 2 else (first if s == 1 else second))


def step_defects(nx, tab, dt, bdf2, state_in_w, U, u_init=None, first_step=0, normwise=False):
    """omega_test (n_mu, nt): every step of ``U`` held on its own - the rows formed from the two states before it IN U."""
    tab, U = np.asarray(tab, dtype=np.float64), np.asarray(U, dtype=np.float64)
    out = np.empty((U.shape[0], U.shape[1]))
    for s in range(U.shape[1]):
        un, un1 = _older(U, u_init, s)
        out[:, s] = omega_of(*step_rows(nx, tab[s], dt, bool(bdf2) and first_step + s > 0, state_in_w, un, un1), U[:, s],
                             normwise=normwise)
    return out


def sequential_sweep(nx, tab, dt, bdf2, state_in_w):
    """(U, omega): the recipe as a float64 loop with the sequential unpivoted elimination, and each step's defect."""
    tab = np.asarray(tab, dtype=np.float64)
    nt, n_mu = tab.shape[:2]
    U, om = np.zeros((n_mu, nt, nx + 1)), np.empty((n_mu, nt))
    for s in range(nt):
        un, un1 = _older(U, None, s)
        rows = step_rows(nx, tab[s], dt, bool(bdf2) and s > 0, state_in_w, un, un1)
        U[:, s, 1:-1] = thomas(*rows)
        om[:, s] = omega_of(*rows, U[:, s])
    return U, om


# ---- convective cases ------------------------------------------------------------------------------------------------------------
def _case(fom, mus):
    rec = fc.recipe(fom, mus)
    nx = int(fom.nx)
    T, margin, flags = fc.truth(nx, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"])
    host, _, _ = fc.host_solutions(fom, mus)
    _, om = sequential_sweep(nx, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"])
    return dict(fom=fom, mus=mus, rec=rec, nx=nx, dt=fom.dt, bdf2=rec["bdf2"], state_in_w=rec["state_in_w"], truth=T,
                margin=margin, flags=flags, host=host, d_host=fc.rel(host, T), seq_omega=om)


@functools.lru_cache(maxsize=None)
def conv_case(nx, bdf2):
    return _case(make_fom(nx, NT, bdf2), [dict(mu) for mu in CONV_MUS])


@functools.lru_cache(maxsize=None)
def piston_case():
    """The sizes of the reference's own piston runs: nx = 1000, nt = 100, T = 1, alpha_0 = 1e-6."""
    return _case(make_fom(1000, 100, True, T=1.0), [dict(CONV_MUS[0])])


@functools.lru_cache(maxsize=None)
def size_case():
    """N_h = 1e5, where 2 alpha dt / h^2 outgrows the CFL number from alpha_0 = 1e-5 on: both points at alpha_0 = 1e-6."""
    return _case(make_fom(100_000, 6, True), [dict(CONV_MUS[0]), dict(CONV_MUS[2], alpha_0=1e-6)])


def conv_keys():
    return [(nx, bdf2) for nx in CONV_NX for bdf2 in (False, True)]


def all_conv_cases():
    """(name, case) of every convective case, the two large ones last."""
    for nx, bdf2 in conv_keys():
        yield f"nx{nx}-bdf{2 if bdf2 else 1}", conv_case(nx, bdf2)
    yield "piston-nx1000-nt100", piston_case()
    yield "size-nx100000", size_case()


@functools.lru_cache(maxsize=None)
def omega_ref():
    """OMEGA_REF: the worst defect of the float64 sequential elimination over the convective cases."""
    return float(max(c["seq_omega"].max() for _, c in all_conv_cases()))


# ---- flag cases: a diagonal that all but vanishes ------------------------------------------------------------------------------------
def flag_table(nx, eps=FLAG_EPS):
    """(tab (3, 2, 7), dt): linear problems (state_in_w = 0, BDF1), h = 1/nx, alpha = 1e-3, f = 1; point 0 has at step 1 a
    ramp c1 that puts d = -(4h/6 + 2 dt alpha/h) eps against |l|, |u| of 0.4 to 260.  Every other (point, step) is pure
    diffusion, strictly dominant."""
    h, alpha = 1.0 / nx, 1e-3
    tab = np.zeros((3, 2, 7))
    tab[:, :, 0], tab[:, :, 1], tab[:, :, 4] = h, alpha, 1.0
    tab[1, 0, 3] = (4 * h / 6 + 2 * DT * alpha / h) * 3 * nx / DT * (1 + eps)
    return tab, DT
