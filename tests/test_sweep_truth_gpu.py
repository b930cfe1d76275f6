"""Every step of both online sweeps against an extended-precision one-step defect (tests/sweep_cases.py), inside
NaN-poisoned operands and a canary-guarded trajectory.

Each case builds its rt_hsweep_desc / rt_sweep_desc itself and calls the library directly, so that uN_out and every
table, matrix and value vector sit in guarded buffers (tests/guarded.py).  Per case, in this order: the route where it
is observable (the step's expansion: the last GEMM-class launch of a hyper-reduced sweep, whatever the solver - the
solve kernels leave launch_info alone), the defect bar at every step and point, the guard checks.  The measure, the
cases and the planted faults that prove the measure are in tests/sweep_cases.py and tests/test_sweep_truth_cpu.py.

Index arrays (indptr, indices) are guarded by words holding the valid index 0 and checked for writes: a poisoned guard
would turn an over-read into a wild gather on a machine others share, where a NaN cannot stand in for an index."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import guarded as gd
from tests import sweep_cases as sc
from tests.guarded import guarded_operand, guarded_output

pytestmark = pytest.mark.gpu
SCHEMES = [pytest.param(False, id="bdf1"), pytest.param(True, id="bdf2")]


@pytest.fixture(scope="module", autouse=True)
def _defaults_only():
    try:
        gd.require_clean_env()
    except RuntimeError as exc:
        pytest.fail(str(exc))


@pytest.fixture(scope="module")
def ctx():
    from romtime_amd._lib import Context

    return Context.current()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _report(**kw):
    print(json.dumps(kw))


def _cases(table):
    return [pytest.param(name, kw, id=name) for name, kw in table.items()]


class Placed:
    """The operands of one sweep in guarded buffers, and the trajectory in a canary buffer."""

    INDEX_GUARD = 256

    def __init__(self, c):
        self.c, self.ops, self.idx = c, [], []
        self.out = guarded_output((c.n_mu * c.nt, c.r))

    def mat(self, a):
        """A table, matrix or vector (None stays None) as a contiguous guarded operand; returns the device view."""
        if a is None:
            return None
        a = np.asarray(a, dtype=np.float64)
        host = np.ascontiguousarray(a.reshape(1, -1) if a.ndim == 1 else a.reshape(-1, a.shape[-1]))
        view = guarded_operand(host)
        self.ops.append((view, host))
        return view

    def index(self, a):
        g = self.INDEX_GUARD
        buf = torch.zeros(a.size + 2 * g, dtype=torch.int64, device="cuda")
        buf[g:g + a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()
        self.idx.append((buf, a))
        return buf[g:g + a.size]

    def trajectory(self):
        torch.cuda.synchronize()
        c = self.c
        return self.out.t.cpu().numpy().reshape(c.n_mu, c.nt, c.r)

    def clean(self):
        torch.cuda.synchronize()
        assert self.out.check() == [], self.out.check()
        for view, host in self.ops:
            assert gd.operand_intact(view, host) == [], gd.operand_intact(view, host)
        g = self.INDEX_GUARD
        for buf, a in self.idx:
            want = np.zeros(a.size + 2 * g, dtype=np.int64)
            want[g:g + a.size] = a
            assert np.array_equal(buf.cpu().numpy(), want), "an index array or its guard was written"


def run_sweep(ctx, c, solver="direct"):
    """One sweep of the case through the C ABI.  Returns (trajectory, the Placed operands for the guard checks)."""
    from romtime_amd._lib import HSweepDesc, SweepDesc
    from romtime_amd.sweep import reduced_solver

    p = Placed(c)
    if c.kind == "hrom":
        desc = HSweepDesc(r=c.r, n_mu=c.n_mu, nt=c.nt, dt=c.dt, bdf2=int(c.bdf2), m_mass=c.mm, m_lin=c.ml, m_nl=c.mn, m_rhs=c.mf,
                          Z=P(p.mat(c.Z)), Zf=P(p.mat(c.Zf)), F_mass=P(p.mat(c.F_mass)), F_lin=P(p.mat(c.F_lin)),
                          F_rhs=P(p.mat(c.F_rhs)), W=P(p.mat(c.W)), C_nl=P(p.mat(c.C)), S_nl=P(p.mat(c.S)))
        fn, what = ctx.lib.rt_hrom_bdf_sweep, "rt_hrom_bdf_sweep"
    else:
        desc = SweepDesc(N=c.N, nnz=c.nnz, r=c.r, n_mu=c.n_mu, nt=c.nt, dt=c.dt, bdf2=int(c.bdf2), indptr=P(p.index(c.indptr)),
                         indices=P(p.index(c.indices)), V=P(p.mat(c.V)), mass_values=P(p.mat(c.mass)), n_terms=c.n_terms,
                         term_values=P(p.mat(c.terms)), term_coef=P(p.mat(c.term_coef)), tril_values=P(p.mat(c.tril)),
                         n_rhs=c.n_rhs, rhs_terms=P(p.mat(c.rhs_terms)), rhs_coef=P(p.mat(c.rhs_coef)))
        fn, what = ctx.lib.rt_rom_bdf_sweep, "rt_rom_bdf_sweep"
    with reduced_solver(ctx, solver, None, c.r):
        ctx.check(fn(ctx.handle, C.byref(desc), P(p.out.t)), what)
    return p.trajectory(), p


def expansion_taken(c):
    """rt_expansion_gemm's own conditions (sweep.hip) for the stacked [K_N; M_N] = G Z of a hyper-reduced step."""
    M, rr = c.depth, c.r * c.r
    return 2 * c.n_mu <= 64 and M >= 2 and rr >= 2 and M % 2 == 0 and rr % 2 == 0


def assert_expansion_route(ctx, cus, c):
    M, rr = c.depth, c.r * c.r
    generic = gd.gemm_plan(2 * c.n_mu, rr, M, False, False, cus)
    want = gd.expansion_plan(rr) if expansion_taken(c) else generic
    # (at 64 stacked rows and r = 16 the generic GEMM would launch the same grid and tile: launch_info cannot tell the
    # two apart there - points_32 - and tells them apart everywhere else the expansion is taken)
    assert want != generic or not expansion_taken(c) or (2 * c.n_mu, rr) == (64, 256)
    assert ctx.launch_info() == want, (ctx.launch_info(), want)


def assert_defect_bar(c, uN, F, label):
    m = sc.measure(c, uN)
    w, b, s, i = sc.worst(m)
    _report(case=label, worst=round(w, 4), point=b, step=s, entry=i, ratio_device=round(float(m.ratio.max()), 4),
            ratio_numpy=round(float(m.ratio_numpy.max()), 4))
    assert np.isfinite(uN).all()
    bad = np.argwhere(m.ratio > F * np.maximum(m.ratio_numpy, 1.0))
    assert bad.size == 0, (f"defect above the bar at (point, step) {bad[:4].tolist()}; worst {w:.3g} at point {b}, step {s}, "
                           f"entry {i}")
    return m


# ---- hyper-reduced sweep -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name,kw", _cases(sc.H_CASES))
def test_hyper_reduced_sweep_step_defect(ctx, cus, name, kw, bdf2):
    c = sc.build("hrom", name, kw, bdf2)
    uN, placed = run_sweep(ctx, c)
    assert_expansion_route(ctx, cus, c)
    assert_defect_bar(c, uN, sc.F_HSWEEP, f"hrom-{name}-bdf{1 + bdf2}")
    placed.clean()


@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name,kw", _cases(sc.H_GRAPH_CASES))
def test_hyper_reduced_sweep_graph_replay_is_bit_equal(ctx, cus, name, kw, bdf2):
    """nt = 3 is the smallest horizon the graph takes, nt = 2 runs eagerly whatever the option says."""
    c = sc.build("hrom", name, kw, bdf2)
    eager, placed = run_sweep(ctx, c)
    placed.clean()
    ctx.set_option("sweep_graph", 1)
    try:
        replay, placed = run_sweep(ctx, c)
    finally:
        ctx.set_option("sweep_graph", 0)
    assert_expansion_route(ctx, cus, c)
    assert gd.bits_equal(replay, eager), gd.mismatch(replay, eager)
    assert_defect_bar(c, replay, sc.F_HSWEEP, f"hrom-graph-{name}-bdf{1 + bdf2}")
    placed.clean()


def assert_gmres_bar(ctx, c, uN, label):
    assert ctx.counter("sweep_gmres_unconverged") == 0
    m = sc.measure(c, uN)
    slack = m.d2 - (np.maximum(sc.GMRES_TOL, sc.GMRES_TOL * m.b2) + m.floor)
    _report(case=label, worst_defect=float(m.d2.max()), worst_over_tolerance=float((m.d2 / np.maximum(sc.GMRES_TOL, sc.GMRES_TOL * m.b2)).max()))
    assert np.isfinite(uN).all() and (slack <= 0.0).all(), np.argwhere(slack > 0)[:4].tolist()


@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name,kw", _cases(sc.H_GMRES_CASES))
def test_hyper_reduced_sweep_gmres_defect(ctx, cus, name, kw, bdf2):
    """The stopping rule is the bar here: |d|_2 <= max(atol, rtol |b_N|_2) + floor at every step and point."""
    c = sc.build("hrom", name, kw, bdf2)
    uN, placed = run_sweep(ctx, c, solver="gmres")
    assert_expansion_route(ctx, cus, c)
    assert_gmres_bar(ctx, c, uN, f"hrom-gmres-{name}-bdf{1 + bdf2}")
    placed.clean()


@pytest.mark.parametrize("solver", ["direct", "gmres"])
@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name,kw", _cases(sc.H_ZERO_CASES))
def test_hyper_reduced_sweep_without_a_source_stays_zero(ctx, name, kw, bdf2, solver):
    c = sc.build("hrom", name, kw, bdf2)
    assert c.Zf is None and c.F_rhs is None and c.mf == 0
    uN, placed = run_sweep(ctx, c, solver=solver)
    assert (uN == 0.0).all()                                 # either sign of zero
    placed.clean()


# ---- direct sweep --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name,kw", _cases(sc.D_CASES))
def test_direct_sweep_step_defect(ctx, name, kw, bdf2):
    c = sc.build("direct", name, kw, bdf2)
    uN, placed = run_sweep(ctx, c)
    stats = ctx.sweep_stats()
    if c.r <= 80:                                            # beyond, the plain LU solves and counts nothing
        assert stats["solves"] == c.n_mu * c.nt and stats["lu_fallbacks"] == 0, stats   # all on the tracked inverse
    assert_defect_bar(c, uN, sc.F_SWEEP, f"direct-{name}-bdf{1 + bdf2}")
    placed.clean()


@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name,kw", _cases(sc.D_GMRES_CASES))
def test_direct_sweep_gmres_defect(ctx, name, kw, bdf2):
    c = sc.build("direct", name, kw, bdf2)
    uN, placed = run_sweep(ctx, c, solver="gmres")
    assert_gmres_bar(ctx, c, uN, f"direct-gmres-{name}-bdf{1 + bdf2}")
    placed.clean()


@pytest.mark.parametrize("solver", ["direct", "gmres"])
@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name,kw", _cases(sc.D_ZERO_CASES))
def test_direct_sweep_without_a_source_stays_zero(ctx, name, kw, bdf2, solver):
    c = sc.build("direct", name, kw, bdf2)
    assert c.rhs_terms is None and c.n_rhs == 0
    uN, placed = run_sweep(ctx, c, solver=solver)
    assert (uN == 0.0).all()
    placed.clean()
