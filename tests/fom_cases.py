"""Cases, extended-precision truth and bars of the full-order sweep tests (test_fom_cpu.py, test_fom_gpu.py).

Truth is the recipe of rt_p1_fom_bdf_sweep (include/romtime_hip.h) evaluated in ``np.longdouble`` on the float64 table the
kernel gets, each step solved by a sequential Thomas pass.  Distances are relative L2 distances over a whole trajectory
block.  ``d_host`` is the distance of the host loop (``mock.solve()``: SciPy CSR assembly + SuperLU in float64) from that
truth; the device has to stay within ``8 d_host + 64 eps`` - the partitioned elimination orders its operations unlike
both, all three are backward stable, and a real defect (a wrong coupling row, a lost boundary, a wrong BDF switch) shows
as 1e-6 or worse.  Plain module, not a conftest."""
from __future__ import annotations

import functools

import numpy as np

from romtime_amd.testing.mock import MockBurgers, MockHeatEquation

EPS = float(np.finfo(np.float64).eps)
DT = 1.0 / 24.0

BURGERS_MUS = [dict(alpha_0=0.05, delta=0.4, omega=9.0), dict(alpha_0=0.11, delta=0.25, omega=5.0),
               dict(alpha_0=0.02, delta=0.33, omega=12.0)]
HEAT_MUS = [dict(delta=0.5, beta=2.0, alpha_0=0.4, omega=2.0), dict(delta=0.8, beta=1.1, alpha_0=0.15, omega=3.5),
            dict(delta=0.3, beta=3.0, alpha_0=0.9, omega=1.2)]


def _burgers_Lt(t, **mu):
    return 1.0 - 0.1 * np.sin(mu["omega"] * t)


def _heat_Lt(t, **mu):
    return 1.0 - 0.3 * np.sin(mu["omega"] * t)


def _heat_dLt(t, **mu):
    return -0.3 * mu["omega"] * np.cos(mu["omega"] * t)


def make_fom(kind, nx, nt, bdf2=True, moving=True):
    """The two problems of testing/mock.py on a (moving) interval, dt = 1/24 (Burgers) or 1/12 (heat)."""
    if kind == "burgers":
        fom = MockBurgers(domain=dict(L0=1.3, nx=nx, T=DT * nt, nt=nt), Lt=_burgers_Lt if moving else None, bdf2=bdf2)
    else:
        fom = MockHeatEquation(domain=dict(L0=1.5, nx=nx, T=2.0 * DT * nt, nt=nt), Lt=_heat_Lt if moving else None,
                               dLt_dt=_heat_dLt if moving else None)
    fom.setup()
    return fom


def mus_of(kind, n_mu):
    base = BURGERS_MUS if kind == "burgers" else HEAT_MUS
    return [dict(base[j % 3]) for j in range(n_mu)]


def recipe(fom, mus):
    ts = fom.dt * np.arange(1, int(fom.domain["nt"]) + 1)
    return fom.p1_fom_recipe(mus, ts)


def truth(nx, tab, dt, bdf2, state_in_w, dtype=np.longdouble, u_init=None, first_step=0):
    """(U, margin, flags): U (n_mu, nt, nx + 1) in ``dtype``; margin = min over every row of (|d| - |l| - |u|) / max|d|
    (positive: strictly diagonally dominant); flags (n_mu) as the kernel's info.  Vectorised over the points, sequential
    over the rows."""
    tab = np.asarray(tab, dtype=np.float64)
    nt, n_mu = tab.shape[:2]
    Nh = nx + 1
    T = lambda v: np.asarray(v, dtype=dtype)
    dt = T(dt)
    un, un1 = np.zeros((n_mu, Nh), dtype), np.zeros((n_mu, Nh), dtype)
    if u_init is not None:
        un, un1 = T(u_init[:, 0]).copy(), T(u_init[:, 1]).copy()
    ramp = (np.arange(Nh).astype(dtype) / dtype(nx))[None, :]
    node = np.arange(Nh).astype(dtype)[None, :]
    out = np.zeros((n_mu, nt, Nh), dtype)
    margin, flags = np.inf, np.zeros(n_mu, dtype=np.int64)
    for s in range(nt):
        h, alpha, c0, c1, a0, a1, a2 = (T(tab[s, :, q])[:, None] for q in range(7))
        two = bool(bdf2) and (first_step + s) > 0
        bdf = dtype(1.5) if two else dtype(1)
        ustar = 2 * un - un1 if two else un
        past = 2 * un - un1 / 2 if two else un
        w = (ustar if state_in_w else 0 * ustar) + c0 + c1 * ramp
        a = (2 * w[:, :-1] + w[:, 1:]) / 6
        b = (w[:, :-1] + 2 * w[:, 1:]) / 6
        lo = bdf * h / 6 + dt * (-alpha / h - b[:, :-1])
        di = bdf * 4 * h / 6 + dt * (2 * alpha / h + b[:, :-1] - a[:, 1:])
        up = bdf * h / 6 + dt * (-alpha / h + a[:, 1:])
        x = node * h
        f = lambda z: a0 + a1 * z + a2 * z * z
        load = h / 3 * (f(x - h / 2) + f(x) + f(x + h / 2))
        r = h / 6 * (past[:, :-2] + 4 * past[:, 1:-1] + past[:, 2:]) + dt * load[:, 1:-1]
        slack = np.abs(di) - np.abs(lo) - np.abs(up)
        margin = min(margin, float(np.min(slack / np.max(np.abs(di), axis=1, keepdims=True))))
        bad = (slack < 0).any(axis=1)
        n = nx - 1
        c, d = np.empty((n, n_mu), dtype), np.empty((n, n_mu), dtype)
        lo, di, up, r = lo.T.copy(), di.T.copy(), up.T.copy(), r.T.copy()
        with np.errstate(all="ignore"):
            c[0], d[0] = up[0] / di[0], r[0] / di[0]
            for k in range(1, n):
                den = di[k] - lo[k] * c[k - 1]
                c[k], d[k] = up[k] / den, (r[k] - lo[k] * d[k - 1]) / den
            xs = np.empty((n, n_mu), dtype)
            xs[-1] = d[-1]
            for k in range(n - 2, -1, -1):
                xs[k] = d[k] - c[k] * xs[k + 1]
        bad |= ~np.isfinite(xs.astype(np.float64)).all(axis=0)
        flags = np.where((flags == 0) & bad, 1 + first_step + s, flags)
        u = np.zeros((n_mu, Nh), dtype)
        u[:, 1:-1] = xs.T
        un1, un = un, u
        out[:, s] = u
    return out, margin, flags


def host_solutions(fom, mus):
    """(n_mu, nt, N_h) homogeneous snapshots, (n_mu, nt, N_h) lifted solutions and the list of nonlinear snapshot sets
    (or None) of ``fom.solve()``."""
    homog, full, nl = [], [], []
    for mu in mus:
        fom.setup()
        fom.update_parametrization(mu)
        fom.solve()
        homog.append(fom.solutions.snapshots.T.copy())
        full.append(fom.solutions.fom.T.copy())
        sets = getattr(fom, "nonlinear_snapshots", None)
        if sets is not None and len(sets) > 1:
            snaps = np.array(sets[1:]).T
            snaps[0, :] = 0.0
            nl.append(snaps)
    return np.array(homog), np.array(full), (nl or None)


def superlu_sweep(nx, tab, dt, bdf2, state_in_w):
    """The recipe as a host loop of the kind ``mock.solve()`` is - float64 rows, SciPy CSC, SuperLU - for the flag
    combinations no mock problem has (a BDF2 heat problem)."""
    from scipy.sparse import diags
    from scipy.sparse.linalg import spsolve

    tab = np.asarray(tab, dtype=np.float64)
    nt, n_mu = tab.shape[:2]
    Nh = nx + 1
    out = np.zeros((n_mu, nt, Nh))
    ramp = np.arange(Nh) / nx
    for j in range(n_mu):
        un, un1 = np.zeros(Nh), np.zeros(Nh)
        for s in range(nt):
            h, alpha, c0, c1, a0, a1, a2 = tab[s, j]
            two = bool(bdf2) and s > 0
            bdf = 1.5 if two else 1.0
            ustar = 2 * un - un1 if two else un
            past = 2 * un - un1 / 2 if two else un
            w = (ustar if state_in_w else 0.0) + c0 + c1 * ramp
            a, b = (2 * w[:-1] + w[1:]) / 6, (w[:-1] + 2 * w[1:]) / 6
            lo = bdf * h / 6 + dt * (-alpha / h - b[:-1])
            di = bdf * 4 * h / 6 + dt * (2 * alpha / h + b[:-1] - a[1:])
            up = bdf * h / 6 + dt * (-alpha / h + a[1:])
            x = np.arange(Nh) * h
            f = lambda z: a0 + a1 * z + a2 * z * z
            load = h / 3 * (f(x - h / 2) + f(x) + f(x + h / 2))
            r = h / 6 * (past[:-2] + 4 * past[1:-1] + past[2:]) + dt * load[1:-1]
            K = diags([lo[1:], di, up[:-1]], [-1, 0, 1], format="csc")
            u = np.zeros(Nh)
            u[1:-1] = spsolve(K, r) if nx > 2 else r / di
            un1, un = un, u
            out[j, s] = u
    return out


def rel(a, b):
    """Relative L2 distance of the block ``a`` from the truth ``b`` (the truth rounded to float64 first)."""
    b = np.asarray(b).astype(np.float64)
    return float(np.linalg.norm((np.asarray(a, dtype=np.float64) - b).ravel()) / np.linalg.norm(b.ravel()))


def bar(d_host):
    return 8.0 * d_host + 64.0 * EPS


@functools.lru_cache(maxsize=None)
def case(kind, nx, nt, bdf2=True, n_mu=1, flags=None):
    """One case, computed once and shared: the model, its points and recipe, the truth and d_host.  ``flags`` =
    (bdf2, state_in_w) overrides the recipe's flags (the kernel's four combinations on one table); the host reference is
    then the SuperLU loop of the recipe where no mock problem solves that combination."""
    fom = make_fom(kind, nx, nt, bdf2=bdf2)
    mus = mus_of(kind, n_mu)
    rec = recipe(fom, mus)
    f_bdf2, f_state = (rec["bdf2"], rec["state_in_w"]) if flags is None else flags
    T, margin, info = truth(nx, rec["tab"], fom.dt, f_bdf2, f_state)
    if (f_bdf2, f_state) == (rec["bdf2"], rec["state_in_w"]):
        host, host_full, host_nl = host_solutions(fom, mus)
    else:
        host, host_full, host_nl = superlu_sweep(nx, rec["tab"], fom.dt, f_bdf2, f_state), None, None
    return dict(fom=fom, mus=mus, rec=rec, bdf2=f_bdf2, state_in_w=f_state, truth=T, margin=margin, info=info, host=host,
                host_full=host_full, host_nl=host_nl, d_host=rel(host, T))


def row_counts(P):
    """Interior row counts at which the partitioning changes: below, at and above one row per partition, two and three
    rows per partition (c = 3)."""
    return [1, 2, P - 1, P, P + 1, 2 * P + 1, 3 * P - 1, 3 * P, 3 * P + 1]


def flag_table(nx, nt, bad_step):
    """A table of three heat-type points whose middle one has alpha = 0 and, at ``bad_step``, a ramp c1 so large that
    d_i < |l_i| + |u_i| in the rows near the right end; its neighbours (and its other steps) are dominant."""
    fom = make_fom("heat", nx, nt)
    mus = mus_of("heat", 3)
    rec = recipe(fom, mus)
    tab = rec["tab"].copy()
    tab[:, 1, 1] = 0.0
    tab[:, 1, 3] = 0.0
    h = tab[bad_step, 1, 0]
    # alpha = 0, w = c1 i/nx: l = h/6 - dt b, u = h/6 + dt a with a, b about c1 i/(2 nx); dt c1/2 = h makes |l| + |u| about
    # 2h against d about 4h/6 at the right end
    tab[bad_step, 1, 3] = 2.0 * h / fom.dt
    return fom, mus, dict(rec, tab=tab)


# ---- host stand-ins of the two device operators fom.py calls (with tests/cpu_stub.py: the host-logic tests) ---------------
def stub_p1_fom_bdf_sweep(nx, tab, dt, bdf2, state_in_w, u_init=None, first_step=0):
    import torch

    tab = tab.numpy() if isinstance(tab, torch.Tensor) else np.asarray(tab)
    ui = None if u_init is None else (u_init.numpy() if isinstance(u_init, torch.Tensor) else np.asarray(u_init))
    U, _, flags = truth(nx, tab, dt, bdf2, state_in_w, dtype=np.float64, u_init=ui, first_step=first_step)
    return torch.from_numpy(U), torch.from_numpy(flags.astype(np.int32))


def stub_p1_local_assembly(kind, nx, rows, cols, h, coef=None, state=None, ramp=None, poly=None):
    import torch

    assert kind == "trilinear" and state is not None
    w = state.numpy()
    rows, cols = np.asarray(rows), np.asarray(cols)
    out = np.zeros((w.shape[0], rows.size))
    for e, (i, j) in enumerate(zip(rows, cols)):
        if i in (0, nx):
            out[:, e] = 1.0 if i == j else 0.0
            continue
        bp, ai = (w[:, i - 1] + 2 * w[:, i]) / 6, (2 * w[:, i] + w[:, i + 1]) / 6
        out[:, e] = -bp if j == i - 1 else (bp - ai if j == i else ai)
    return torch.from_numpy(out)


def install_stubs(monkeypatch):
    from romtime_amd import ops

    monkeypatch.setattr(ops, "p1_fom_bdf_sweep", stub_p1_fom_bdf_sweep)
    monkeypatch.setattr(ops, "p1_local_assembly", stub_p1_local_assembly)


# ---- the cases of test_fom_gpu.py, listed here so that test_fom_cpu.py can hold every one of them to strict dominance --------
def partitions():
    """Partitions per system where every partition holds several rows (read from the plan, never hard-coded)."""
    from romtime_amd import ops

    return ops.p1_fom_plan(1 << 20)[1]


def row_case_keys():
    return [(kind, n + 1, 3, True, 1, None) for kind in ("burgers", "heat") for n in row_counts(partitions())]


def step_case_keys():
    nx = 2 * partitions() + 2
    return [("burgers" if state else "heat", nx, nt, True, 3, (bdf2, state))
            for nt in (1, 2, 3, 9) for bdf2 in (False, True) for state in (False, True)]


SIZE_NX = 100_000


def size_case_keys():
    return [(kind, SIZE_NX, 3, True, 2, None) for kind in ("burgers", "heat")]
