"""Shared inputs of tests/test_collect_cpu.py and tests/test_collect_gpu.py: the three closed-form mock FOMs at nx = 100
with their parameter points, a reductor for every operator they have a closed form for, a counter around every
``assemble_*`` of a FOM, and a NumPy restatement of ``ops.p1_snapshot_sets`` for the host-logic tests (the closed forms in
long double of tests/test_p1_assembly_gpu.py on the replicated operands, rounded to float64)."""
import numpy as np
import torch

NX = 100
TS = [0.15, 0.4, 0.7, 0.95]                                     # 4 instants
N_PSI = 5

SOLVER_MUS = [dict(alpha_0=0.6, gamma=0.2), dict(alpha_0=1.0, gamma=0.5), dict(alpha_0=1.5, gamma=0.9)]      # no delta / omega
HEAT_MUS = [dict(delta=0.4 + 0.3 * q, beta=2.0 + 1.5 * q, alpha_0=0.3 + 0.25 * q, omega=1.0 + q) for q in range(3)]
BURGERS_MUS = [dict(alpha_0=0.05 + 0.03 * q, delta=0.3 + 0.1 * q, omega=9.0 + 1.5 * q) for q in range(3)]

MATRIX_KINDS = ("mass", "stiffness", "convection", "nonlinear_lifting")
VECTOR_KINDS = ("forcing", "lifting", "rhs")
# (fom, kind) pairs with a closed form: every kind of every FOM that p1_closed_form() carries the scalars for
CASES = [("solver", "mass"), ("solver", "stiffness"), ("solver", "convection"),
         ("heat", "mass"), ("heat", "stiffness"), ("heat", "convection"), ("heat", "forcing"), ("heat", "lifting"), ("heat", "rhs"),
         ("burgers", "mass"), ("burgers", "stiffness"), ("burgers", "convection"), ("burgers", "nonlinear_lifting"),
         ("burgers", "lifting"), ("burgers", "trilinear")]


def make_fom(which, nx=NX, nt=40):
    from romtime_amd.testing.mock import MockBurgers, MockHeatEquation, MockSolver

    if which == "solver":
        fom = MockSolver(domain=dict(L0=1.3, nx=nx, T=1.0, nt=nt), Lt=lambda t, **mu: 1.0 + 0.2 * mu["gamma"] * t)
    elif which == "heat":
        fom = MockHeatEquation(domain=dict(L0=2.0, nx=nx, T=1.0, nt=nt), Lt=lambda t, **mu: 1.0 - 0.25 * np.sin(mu["omega"] * t),
                               dLt_dt=lambda t, **mu: -0.25 * mu["omega"] * np.cos(mu["omega"] * t))
    else:
        fom = MockBurgers(domain=dict(L0=1.0, nx=nx, T=1.0, nt=nt), Lt=lambda t, **mu: 1.0 - 0.1 * np.sin(mu["omega"] * t))
    fom.setup()
    return fom


def mus_of(which):
    return [dict(m) for m in dict(solver=SOLVER_MUS, heat=HEAT_MUS, burgers=BURGERS_MUS)[which]]


def states(nx=NX, n=N_PSI):
    """Smooth, strictly increasing states: every entry of the trilinear operator's topology stays nonzero."""
    x = np.linspace(0.0, 1.0, nx + 1)
    return np.stack([(1.0 + x) ** (k + 1) + 0.1 * np.sin((k + 1) * np.pi * x) for k in range(n)], axis=1)


def make_reductor(fom, kind, mus, ts=TS, params=None, grid=None):
    """The reductor class that goes with ``kind`` around ``fom.assemble_<kind>``, its report reset and its topology read
    off one sample operator (no sampling space needed)."""
    from romtime_amd import (DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation,
                             MatrixDiscreteEmpiricalInterpolationNonlinear)
    from romtime_amd.base import Reductor

    p = dict({"ts": list(ts), "num_snapshots": len(mus)}, **(params or {}))
    callback = getattr(fom, "assemble_" + kind)
    if kind in VECTOR_KINDS:
        red = DiscreteEmpiricalInterpolation(assemble=callback, grid=grid, tree_walk_params=p, name=kind)
        Reductor.setup(red, rnd=np.random.RandomState(0))
    elif kind == "trilinear":
        red = MatrixDiscreteEmpiricalInterpolationNonlinear(assemble=callback, grid=grid, tree_walk_params=p, name=kind)
        Reductor.setup(red, rnd=np.random.RandomState(0))
        red.rows, red.cols = red.get_matrix_topology(mu=mus[0], t=1.0, u_n=np.linspace(0.0, 1.0, fom.Nh))
        red.u_n = states(fom.nx)
    else:
        red = MatrixDiscreteEmpiricalInterpolation(assemble=callback, grid=grid, tree_walk_params=p, name=kind)
        Reductor.setup(red, rnd=np.random.RandomState(0))
        red.rows, red.cols = red.get_matrix_topology(mu=mus[0], t=0.3)
    return red


def callback_columns(red, mus, ts, u_n=None):
    """The stacked ``assemble_snapshot`` columns in the order (mu, t[, psi]): N x S."""
    if u_n is not None:
        cols = [red.assemble_snapshot(mu=mu, t=t, u_n=u_n[:, i]) for mu in mus for t in ts for i in range(u_n.shape[1])]
    else:
        cols = [red.assemble_snapshot(mu, t) for mu in mus for t in ts]
    return np.array(cols).T


class Counted:
    """Every ``assemble_*`` of a FOM wrapped by a counter (instance attributes; a wrapper keeps the ``__self__`` and the
    names of the bound method it stands for, so it resolves as the method does)."""

    def __init__(self, fom):
        self.calls = 0
        self.depth = 0
        self.fom = fom
        for name in [n for n in dir(fom) if n.startswith("assemble_")]:
            setattr(fom, name, self._wrap(getattr(fom, name)))

    def _wrap(self, method):
        def counted(*a, **kw):
            if self.depth == 0:                    # a callback that calls others of the FOM (rhs) is one call
                self.calls += 1
            self.depth += 1
            try:
                return method(*a, **kw)
            finally:
                self.depth -= 1

        counted.__self__ = method.__self__
        counted.__name__ = method.__name__
        counted.__qualname__ = method.__qualname__
        return counted


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def numpy_p1_snapshot_sets(kind, nx, rows, cols, h, coef=None, ramp=None, poly=None, fun=None, zero_first=False, out=None,
                           beta=0.0):
    """``ops.p1_snapshot_sets`` on the host: the operands replicated to one row per column (p, f), the long-double closed
    forms of tests/test_p1_assembly_gpu.py, one rounding to float64."""
    from tests.test_p1_assembly_gpu import _closed_form_longdouble

    rows = _np(rows).astype(np.int64)
    cols = None if cols is None else _np(cols).astype(np.int64)
    h = np.atleast_1d(_np(h)).astype(np.float64).reshape(-1)
    n_par = h.size
    c = np.ones(n_par) if coef is None else np.atleast_1d(_np(coef)).astype(np.float64).reshape(-1)
    n_fun, nodal = 1, None
    width = 2 * nx + 1 if kind == "load_p2" else nx + 1
    if fun is not None:
        f = _np(fun).astype(np.float64)
        n_fun = f.shape[0]
        nodal = np.tile(f, (n_par, 1))
    elif ramp is not None:
        nodal = np.atleast_1d(_np(ramp)).reshape(-1)[:, None] * (np.arange(nx + 1) / nx)[None, :]
    elif poly is not None:
        a = _np(poly).astype(np.longdouble)
        x = ((0.5 * h[:, None]) * np.arange(width)[None, :]).astype(np.longdouble)
        nodal = a[:, :1] + a[:, 1:2] * x + a[:, 2:3] * x * x
    ref = _closed_form_longdouble(kind, nx, rows, cols, np.repeat(h, n_fun), np.repeat(c, n_fun), nodal)
    v = np.ascontiguousarray(np.asarray(ref, dtype=np.float64))
    if zero_first:
        v[:, 0] = 0.0
    res = torch.from_numpy(v)
    if out is not None:
        out.copy_(res if beta == 0.0 else beta * out + res)
        return out
    return res
