"""Cases, extended-precision truth and bars of the trajectory-residual tests (test_residual_cpu.py, test_residual_gpu.py).

rt_trajectory_residuals (include/romtime_hip.h) lifts x^t = V a[t] (nodes 0 and nx taken as 0), forms the interior rows
of step s of the full-order sweep from x^{s-1} and x^{s-2} and returns

    res[j, s] = sqrt(sum_i r_i^2),  r_i = rhs_i - (l_i x_{i-1} + d_i x_i + u_i x_{i+1}),
    scale[j, s] = sqrt(sum_i s_i^2),  s_i = |l_i x_{i-1}| + |d_i x_i| + |u_i x_{i+1}| + |rhs_i|.

``truth`` is exactly that, written on the row expressions of ``fom_cases.truth``, in ``np.longdouble`` from the float64
inputs.  Distances are per step and relative to the truth's scale, ``dist(x, t, scale) = |x - t| / scale``; ``d_np`` is
the distance of the same function run with ``dtype=np.float64`` from the long-double truth, its maximum over the case's
steps, and the device has to stay within the project's bar ``8 d_np + 64 eps``.  No bar is derived from the code under
test.  Plain module, not a conftest."""
from __future__ import annotations

import functools

import numpy as np

from tests import fom_cases as fc

EPS = fc.EPS


def truth(nx, tab, dt, bdf2, state_in_w, V, a, a_init=None, first_step=0, dtype=np.longdouble):
    """(res, scale, omega), (n_traj, nt) each in ``dtype``: omega = max_i |r_i| / s_i (0/0 = 0), the componentwise
    companion.  tab (nt, n_traj, 7); V (nx + 1, k), rows 0 and nx not looked at; a (n_traj, nt, k); a_init (n_traj, 2, k):
    the coefficients of the two steps before this call's first, newest first, None = zero."""
    tab = np.asarray(tab, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    nt, n = tab.shape[:2]
    Nh = nx + 1
    T = lambda v: np.asarray(v, dtype=dtype)
    Vt = T(np.asarray(V, dtype=np.float64)).copy()
    Vt[0] = Vt[-1] = 0

    def lift(c):
        """(..., k) -> (..., N_h), one column after the other: every value is the same chain of operations whatever the
        shape of the block (a BLAS product is not), so a horizon cut into calls has the bits of the whole."""
        c = T(c)
        out = np.zeros(c.shape[:-1] + (Nh,), dtype)
        for q in range(c.shape[-1]):
            out += c[..., q, None] * Vt[:, q]
        return out

    X = lift(a)
    X[..., 0] = X[..., -1] = 0
    older = np.zeros((n, 2, Nh), dtype) if a_init is None else lift(np.asarray(a_init, dtype=np.float64))
    older[..., 0] = older[..., -1] = 0
    dt = T(dt)
    ramp = (np.arange(Nh).astype(dtype) / dtype(nx))[None, :]
    node = np.arange(Nh).astype(dtype)[None, :]
    res, scale, omega = (np.empty((n, nt), dtype) for _ in range(3))
    for s in range(nt):
        un = X[:, s - 1] if s >= 1 else older[:, 0]
        un1 = X[:, s - 2] if s >= 2 else (older[:, 0] if s == 1 else older[:, 1])
        x = X[:, s]
        h, alpha, c0, c1, a0, a1, a2 = (T(tab[s, :, q])[:, None] for q in range(7))
        two = bool(bdf2) and (first_step + s) > 0
        bdf = dtype(1.5) if two else dtype(1)
        with np.errstate(all="ignore"):
            ustar = 2 * un - un1 if two else un
            past = 2 * un - un1 / 2 if two else un
            w = (ustar if state_in_w else 0 * ustar) + c0 + c1 * ramp
            ae = (2 * w[:, :-1] + w[:, 1:]) / 6
            be = (w[:, :-1] + 2 * w[:, 1:]) / 6
            lo = bdf * h / 6 + dt * (-alpha / h - be[:, :-1])
            di = bdf * 4 * h / 6 + dt * (2 * alpha / h + be[:, :-1] - ae[:, 1:])
            up = bdf * h / 6 + dt * (-alpha / h + ae[:, 1:])
            xs = node * h
            f = lambda z: a0 + a1 * z + a2 * z * z
            load = h / 3 * (f(xs - h / 2) + f(xs) + f(xs + h / 2))
            r = h / 6 * (past[:, :-2] + 4 * past[:, 1:-1] + past[:, 2:]) + dt * load[:, 1:-1]
            lo, up = lo.copy(), up.copy()
            lo[:, 0] = 0
            up[:, -1] = 0
            tl, tc, tr = lo * x[:, :-2], di * x[:, 1:-1], up * x[:, 2:]
            ri = r - (tl + tc + tr)
            si = np.abs(tl) + np.abs(tc) + np.abs(tr) + np.abs(r)
            res[:, s] = np.sqrt((ri * ri).sum(axis=1))
            scale[:, s] = np.sqrt((si * si).sum(axis=1))
            omega[:, s] = np.where(si > 0, np.abs(ri) / np.where(si > 0, si, 1), 0).max(axis=1)
    return res, scale, omega


def dist(x, t, scale):
    """|x - t| / scale per step (the truth rounded to float64 first)."""
    t, scale = np.asarray(t).astype(np.float64), np.asarray(scale).astype(np.float64)
    return np.abs(np.asarray(x, dtype=np.float64) - t) / scale


def bar(d_np):
    return 8.0 * d_np + 64.0 * EPS


# ---- what the plan says -----------------------------------------------------------------------------------------------------------
def plan(nx, k=1, nt=1, n_traj=1, num_cus=256):
    from romtime_amd import ops

    return ops.trajectory_residuals_plan(nx, k, nt, n_traj, num_cus)


def stage_rows():
    """Rows a stage evaluates (the row seams lie at its multiples inside a slice), read from the plan."""
    return plan(100)[2] // 1000


def block_steps():
    """Steps a block evaluates (the step seams lie at its multiples), read from the plan."""
    return plan(100)[2] % 1000


@functools.lru_cache(maxsize=None)
def slice_length():
    """The planned slice length s: the largest number of interior rows that is still one slice on a full device (read
    from the plan query by bisection, never hard-coded)."""
    lo, hi = 1, 1 << 20                                          # one slice at lo, more at hi
    assert plan(lo + 1)[1] == 1 and plan(hi + 1)[1] > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(mid + 1)[1] == 1 else (lo, mid)
    return lo


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def basis(rng, Nh, k):
    """Random N_h x k with orthonormal columns (where N_h >= k; scaled random otherwise), NaN in rows 0 and nx."""
    G = rng.standard_normal((Nh, k))
    V = np.linalg.qr(G)[0] if Nh >= k else G / np.sqrt(Nh)
    V = np.ascontiguousarray(V)
    V[0] = V[-1] = np.nan
    return V


@functools.lru_cache(maxsize=None)
def case(kind, nx, nt, k, n_traj, flags=None, with_init=False, seed=0):
    """One case, computed once and shared: the model's recipe (``flags`` = (bdf2, state_in_w) overrides its flags, as
    fom_cases.step_case_keys does), a random basis and random coefficients of size 1, the truth and d_np."""
    fom = fc.make_fom(kind, nx, nt)
    rec = fc.recipe(fom, fc.mus_of(kind, n_traj))
    bdf2, state = (rec["bdf2"], rec["state_in_w"]) if flags is None else flags
    rng = np.random.default_rng(1000 * nx + 10 * nt + k + seed)
    V = basis(rng, nx + 1, k)
    a = rng.uniform(-1.0, 1.0, (n_traj, nt, k))
    a_init = rng.uniform(-1.0, 1.0, (n_traj, 2, k)) if with_init else None
    first = 7 if with_init else 0
    c = dict(kind=kind, nx=nx, nt=nt, k=k, tab=np.ascontiguousarray(rec["tab"]), dt=fom.dt, bdf2=bool(bdf2), state_in_w=bool(state),
             V=V, a=a, a_init=a_init, first_step=first)
    c.update(reference(c))
    return c


def reference(c):
    """truth and d_np (res and scale) of a case dict."""
    args = (c["nx"], c["tab"], c["dt"], c["bdf2"], c["state_in_w"], c["V"], c["a"])
    kw = dict(a_init=c.get("a_init"), first_step=c.get("first_step", 0))
    res, scale, omega = truth(*args, **kw)
    r64, s64, _ = truth(*args, dtype=np.float64, **kw)
    return dict(res=res, scale=scale, omega=omega, d_np_res=float(dist(r64, res, scale).max()),
                d_np_scale=float(dist(s64, scale, scale).max()))


def row_counts():
    """Interior row counts: one and two rows, the stage seams of 32-row and of the plan's stages, and the slice seams."""
    s, e = slice_length(), stage_rows()
    return sorted({1, 2, 31, 32, 33, 63, 64, 65, e - 1, e, e + 1, 2 * e - 1, 2 * e, 2 * e + 1, s - 1, s, s + 1, 2 * s + 1})


def row_case_keys():
    return [(kind, n + 1, 3, 5, 1) for kind in ("burgers", "heat") for n in row_counts()]


STEP_NX = 70
STEP_NTS = (1, 2, 3, 63, 64, 65, 66, 130)


def step_case_keys():
    return [("burgers" if state else "heat", STEP_NX, nt, 6, 3, (bdf2, state))
            for nt in STEP_NTS for bdf2 in (False, True) for state in (False, True)]


K_NX = 200
KS = (1, 3, 4, 5, 127, 128)


def k_case_keys():
    return [("burgers", K_NX, 5, k, 2, None, True) for k in KS]


SIZE_KEY = ("burgers", 20000, 66, 16, 2)


# ---- the FOM's own trajectory -------------------------------------------------------------------------------------------------------
OWN_NX = (5, 33, 127)
OWN_NT = 9


def own_bound(defect, scale, Nh):
    """res <= omega scale (1 + 4 N_h eps): |r_i| <= omega s_i row by row, two sums of N_h non-negative terms with at most
    N_h eps of relative rounding each, one square root."""
    return defect * scale * (1.0 + 4.0 * Nh * EPS)


# ---- host stand-in of the device operator (with tests/cpu_stub.py: the host-logic tests) --------------------------------------------
def stub_trajectory_residuals(V, uN, nx, tab, dt, bdf2, state_in_w, a_init=None, first_step=0):
    import torch

    n = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    a = n(uN)
    a = a[None] if a.ndim == 2 else a
    res, scale, _ = truth(int(nx), n(tab), dt, bdf2, state_in_w, n(V), a, a_init=n(a_init), first_step=first_step, dtype=np.float64)
    return torch.from_numpy(res), torch.from_numpy(scale)


def install_stubs(monkeypatch):
    from romtime_amd import ops
    from tests import cpu_stub

    cpu_stub.install(monkeypatch)
    monkeypatch.setattr(ops, "trajectory_residuals", stub_trajectory_residuals)
