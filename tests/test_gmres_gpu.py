"""The device GMRES reduced solver (rt_gmres_batched, and the sweeps' RT_SOLVER_GMRES mode) against SciPy's gmres, the
solver of the reference's online loop (rom.py:36,414-425,492): the same inner-iteration counts and info for every
system, the same iterate up to rounding, and the reference's own trajectories to 1e-10."""
import ctypes as C
import re
import time

import numpy as np
import pytest
import torch
from scipy.sparse.linalg import gmres as scipy_gmres

from oracle import romtime_oracle as oracle
from tests import guarded as gd
from tests.test_configs_gpu import _report

pytestmark = pytest.mark.gpu
EPS = 2.2e-16
CASES = ["r10_bdf1", "r10_bdf2", "r24_bdf1", "r24_bdf2"]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def P(t):
    return C.c_void_p(t.data_ptr())


def scipy_solve(K, b, o):
    """SciPy's gmres with the options the device solver runs (a GmresOpts), and its inner-iteration count: the
    "pr_norm" callback fires once per inner iteration with presid / |b|."""
    hist = []
    x, info = scipy_gmres(K, b, rtol=o.rtol, atol=o.atol, restart=int(o.restart), maxiter=int(o.maxiter),
                          callback=hist.append, callback_type="pr_norm")
    return x, info, hist


class CountingGmres:
    """oracle.reduced_solve (the reference's gmres call, rom.py:36,492) with its inner iterations counted."""

    def __init__(self):
        self.iters, self.unconverged, self.solves, self.max_iters = 0, 0, 0, 0

    def __call__(self, K, b):
        hist = []
        x, info = scipy_gmres(K, b, callback=hist.append, callback_type="pr_norm", **oracle.GMRES_OPTIONS)
        self.iters += len(hist)
        self.unconverged += int(info != 0)
        self.solves += 1
        self.max_iters = max(self.max_iters, len(hist))
        return x


# ---- systems -----------------------------------------------------------------------------------------------------
def _bdf_like(r, rng):
    """1.5 M + dt A: an SPD mass-like matrix and a nonsymmetric stiffness / convection part."""
    Q, _ = np.linalg.qr(rng.standard_normal((r, r)))
    M = (Q * rng.uniform(0.5, 2.0, r)) @ Q.T
    A = rng.standard_normal((r, r)) / np.sqrt(r)
    return 1.5 * M + 0.05 * (A @ A.T + 2.0 * (A - A.T))


def _convection(r, rng, sign=1.0):
    """Upwinded convection-diffusion stencil (positive-definite symmetric part, strongly nonnormal): restarted GMRES
    needs many cycles on it."""
    K = 2.1 * np.eye(r) - 1.9 * np.eye(r, k=-1) - 0.1 * np.eye(r, k=1)
    return sign * (K + 0.01 * rng.standard_normal((r, r)) / np.sqrt(r))


def _systems(r, rng):
    """32 systems of every kind: BDF-like, convection-dominated (f > 0 and, negated, f < 0 rotations), the identity
    (breakdown at once, g = 0), b an exact eigenvector (upper-triangular K, b = 3 e_0: breakdown after one step), a
    permutation (f = 0, then g = 0 with f < 0), b = 0, and |b| below atol."""
    out = []
    for i in range(32):
        kind = ("bdf", "conv", "conv_neg", "identity", "eigvec", "swap", "zero", "tiny")[i % 8]
        b = rng.standard_normal(r)
        if kind == "bdf":
            K = _bdf_like(r, rng)
        elif kind == "conv":
            K = _convection(r, rng)
        elif kind == "conv_neg":
            K = _convection(r, rng, -1.0)
        elif kind == "identity":
            K = np.eye(r)
        elif kind == "eigvec":
            K = np.triu(rng.standard_normal((r, r))) + 3.0 * np.eye(r)
            b = 3.0 * np.eye(r)[0]
        elif kind == "swap":
            K = np.eye(r)[np.r_[1, 0, 2:r]] if r >= 2 else np.eye(r)
            b = np.eye(r)[0]
        elif kind == "zero":
            K, b = _bdf_like(r, rng), np.zeros(r)
        else:
            K, b = _bdf_like(r, rng), 1e-13 * b
        out.append((kind, K, b))
    return out


R_LIST = [1, 2, 7, 10, 20, 21, 24, 64, 80, 128]
TOLS = {"reference": dict(tol=1e-10, atol=1e-10, maxiter=1e6), "loose": dict(rtol=1e-6, atol=0.0)}


@pytest.mark.parametrize("tol", sorted(TOLS))
@pytest.mark.parametrize("restart", [5, 20, "r"])
@pytest.mark.parametrize("r", R_LIST)
def test_kernel_against_scipy(r, restart, tol):
    """Every system: inner iterations and info equal to SciPy's; |x - x_scipy| <= 1e-12 |x_scipy| up to cond(K) = 1e4
    (a bar growing with cond(K) eps above); the same bits whatever the batch size and the system's place in it."""
    from romtime_amd import ops
    from romtime_amd.gmres import gmres_opts

    rng = np.random.RandomState(1000 * r + (0 if restart == "r" else restart))
    opts = dict(TOLS[tol], restart=r if restart == "r" else restart)
    systems = _systems(r, rng)
    Ks = np.stack([K for _, K, _ in systems])
    bs = np.stack([b for _, _, b in systems])
    x, info, iters = ops.gmres_solve(ops.to_device(Ks), ops.to_device(bs), opts)
    x, info, iters = x.cpu().numpy(), info.cpu().numpy(), iters.cpu().numpy()
    o = gmres_opts(opts, r)
    for i, (kind, K, b) in enumerate(systems):
        xs, info_s, hist = scipy_solve(K, b, o)
        where = f"system {i} ({kind}), r={r}, restart={opts['restart']}, {tol}"
        tail = [f"{h:.3e}" for h in hist[-3:]]
        assert iters[i] == len(hist) and info[i] == info_s, (where, int(iters[i]), len(hist), int(info[i]), info_s,
                                                             "SciPy presid/|b| at the end:", tail)
        nx = np.linalg.norm(xs)
        if nx == 0.0:
            assert np.all(x[i] == 0.0), where
            continue
        bar = 1e-12 * max(1.0, np.linalg.cond(K) / 1e4)
        assert np.linalg.norm(x[i] - xs) <= bar * nx, (where, np.linalg.norm(x[i] - xs) / nx, bar)
    # bit-identical whatever B and position
    for idx in ([0], [31], [5, 6, 7], [30, 1, 17]):
        xs, infos, its = ops.gmres_solve(ops.to_device(Ks[idx]), ops.to_device(bs[idx]), opts)
        assert gd.bits_equal(xs.cpu().numpy(), x[idx]), (idx, gd.mismatch(xs.cpu().numpy(), x[idx]))
        assert np.array_equal(infos.cpu().numpy(), info[idx]) and np.array_equal(its.cpu().numpy(), iters[idx])


def test_maxiter_ends_unconverged_like_scipy():
    """maxiter = 2 cycles of restart 5 on systems that need more: info = 2 on both sides, same iterate."""
    from romtime_amd import ops
    from romtime_amd.gmres import gmres_opts

    rng = np.random.RandomState(7)
    for r in (24, 80, 128):
        Ks = np.stack([_convection(r, rng, s) for s in (1.0, -1.0, 1.0)])
        bs = rng.standard_normal((3, r))
        opts = dict(tol=1e-10, atol=1e-10, restart=5, maxiter=2)
        x, info, iters = ops.gmres_solve(ops.to_device(Ks), ops.to_device(bs), opts)
        for i in range(3):
            xs, info_s, hist = scipy_solve(Ks[i], bs[i], gmres_opts(opts, r))
            assert info_s == 2 and int(info[i]) == 2 and int(iters[i]) == len(hist) == 10
            assert np.linalg.norm(x[i].cpu().numpy() - xs) <= 1e-12 * np.linalg.norm(xs)


def test_single_system_and_bad_arguments():
    from romtime_amd import ops
    from romtime_amd._lib import Context, GmresOpts, RomtimeHipError

    rng = np.random.RandomState(3)
    K, b = _bdf_like(12, rng), rng.standard_normal(12)
    x, info, iters = ops.gmres_solve(ops.to_device(K), ops.to_device(b), dict(tol=1e-10, atol=1e-10))
    assert x.shape == (12,) and int(info) == 0 and int(iters) > 0
    assert np.linalg.norm(K @ x.cpu().numpy() - b) <= 1e-10 * np.linalg.norm(b)
    ctx = Context.current()
    Kd = torch.zeros((1, 129, 129), dtype=torch.float64, device="cuda")
    bd = torch.zeros((1, 129), dtype=torch.float64, device="cuda")
    good = GmresOpts(rtol=1e-6, atol=0.0, restart=20, maxiter=10)
    assert ctx.lib.rt_gmres_batched(ctx.handle, P(Kd), P(bd), P(bd), 129, 1, C.byref(good), None, None) == -3
    for bad in (GmresOpts(rtol=-1.0, atol=0.0, restart=20, maxiter=10), GmresOpts(rtol=1e-6, atol=0.0, restart=0, maxiter=10),
                GmresOpts(rtol=1e-6, atol=0.0, restart=20, maxiter=0), GmresOpts(rtol=float("nan"), atol=0.0, restart=2, maxiter=1)):
        assert ctx.lib.rt_gmres_batched(ctx.handle, P(Kd), P(bd), P(bd), 8, 1, C.byref(bad), None, None) == -1
        assert ctx.lib.rt_ctx_set_reduced_solver(ctx.handle, 1, C.byref(bad)) == -1
    assert ctx.lib.rt_ctx_set_reduced_solver(ctx.handle, 2, C.byref(good)) == -1
    assert ctx.lib.rt_ctx_set_reduced_solver(ctx.handle, 0, None) == 0
    with pytest.raises(RomtimeHipError):
        ops.gmres_solve(torch.zeros((3, 4), dtype=torch.float64, device="cuda"), bd[:, :3])


# ---- guarded buffers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,restart", [(24, 20), (80, 20), (128, 20), (128, 128)])
def test_guarded_buffers(r, restart):
    """K and b inside NaN-poisoned buffers (8-byte-misaligned bases), x / info / iters inside canaries; the Krylov basis
    in LDS (r = 24, 80 with restart 20) and in the global work area (r = 128).  Bits equal to the plain call's."""
    from romtime_amd import ops
    from romtime_amd._lib import Context
    from romtime_amd.gmres import gmres_opts

    ctx = Context.current()
    rng = np.random.RandomState(r + restart)
    B = 6
    Ks = np.stack([_bdf_like(r, rng) if i % 2 == 0 else _convection(r, rng) for i in range(B)])
    bs = rng.standard_normal((B, r))
    opts = dict(tol=1e-10, atol=1e-10, restart=restart, maxiter=1e6)
    x_ref, info_ref, it_ref = ops.gmres_solve(ops.to_device(Ks), ops.to_device(bs), opts)
    Kg = gd.guarded_operand(Ks.reshape(B * r, r), "C", 0, misalign=True)
    bg = gd.guarded_operand(bs, "C", 0, misalign=(r % 3 == 0))
    xo = gd.guarded_output((B, r), misalign=True)
    io = gd.guarded_output((B,), dtype=torch.int64)
    to = gd.guarded_output((B // 2,))   # B int32 counts fill B / 2 canary words
    o = gmres_opts(opts, r)
    assert ctx.lib.rt_gmres_batched(ctx.handle, P(Kg), P(bg), P(xo.t), r, B, C.byref(o), P(io.t), P(to.t)) == 0
    torch.cuda.synchronize()
    for out in (xo, io, to):
        assert out.check() == [], out.check()
    assert gd.operand_intact(Kg, Ks.reshape(B * r, r)) == [] and gd.operand_intact(bg, bs) == []
    assert gd.bits_equal(xo.t.cpu().numpy(), x_ref.cpu().numpy()), gd.mismatch(xo.t.cpu().numpy(), x_ref.cpu().numpy())
    assert np.array_equal(io.t.cpu().numpy(), info_ref.cpu().numpy())
    assert np.array_equal(to.t.view(torch.int32).cpu().numpy(), it_ref.cpu().numpy())


# ---- the reference's own trajectories ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_class_surface_reproduces_the_reference_trajectories(golden_rom, monkeypatch, case):
    """RomConstructorNonlinear with REDUCED_SOLVER = "gmres": the golden trajectories of the reference's own run and the
    oracle loop with the reference's solver (oracle.reduced_solve) to 1e-10.  The direct path is 1e-8 .. 4e-8 away."""
    from romtime_amd import RomConstructorNonlinear
    from tests.test_surface import _burgers

    g = golden_rom
    a, d, w = g["mu"]
    mu = dict(alpha_0=a, delta=d, omega=w)
    got = {}
    for solver in ("gmres", "direct"):
        monkeypatch.setattr(RomConstructorNonlinear, "REDUCED_SOLVER", solver)
        fom = _burgers(case.endswith("bdf2"))
        rom = RomConstructorNonlinear(fom=fom, grid=None, name="golden")
        rom.setup(rnd=0)
        rom.basis = g[f"V__{case}"]
        rom.solve(mu=mu, step="online")
        got[solver] = (rom.solutions.rom, rom.solutions.fom)
    ref_rom, ref_fom = oracle.rom_solve_nonlinear(_burgers(case.endswith("bdf2")), g[f"V__{case}"], mu,
                                                  solver=oracle.reduced_solve)
    uN, uh = got["gmres"]
    d = dict(golden_rom=_rel(uN, g[f"rom__{case}"]), golden_fom=_rel(uh, g[f"fom__{case}"]),
             oracle_rom=_rel(uN, ref_rom), oracle_fom=_rel(uh, ref_fom))
    _report(test="class surface, REDUCED_SOLVER=gmres vs the reference's trajectories", case=case, **d,
            direct_path_golden_fom=_rel(got["direct"][1], g[f"fom__{case}"]))
    assert max(d.values()) <= 1e-10, d


# ---- sweeps ------------------------------------------------------------------------------------------------------
def _hrom_case(nt, n_mu, r, bars, label, check_mus):
    from romtime_amd._lib import Context
    from romtime_amd.sweep import hrom_bdf_sweep
    from romtime_amd.testing.workloads import c5_hyper_reduced

    terms, _, _, _ = c5_hyper_reduced(nt=nt, n_mu=n_mu, r=r)
    args = (terms["mass"], terms["lin"], terms["nl"], terms["rhs"], terms["dt"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    uN = hrom_bdf_sweep(*args, bdf2=True, solver="gmres")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ctx = Context.current()
    iters, unconv, solves = (ctx.counter("sweep_gmres_iterations"), ctx.counter("sweep_gmres_unconverged"),
                             ctx.counter("sweep_solves"))
    uN = uN.cpu().numpy()
    assert uN.shape == (n_mu, nt, r) and np.all(np.isfinite(uN))
    total, worst, worst_last = 0, 0.0, 0.0
    for b in check_mus:
        solver = CountingGmres()
        ref = oracle.hrom_solve(*args[:4], b, r, nt, terms["dt"], True, solver=solver)
        whole, last = _rel(uN[b].T, ref), _rel(uN[b, -1], ref[:, -1])
        worst, worst_last = max(worst, whole), max(worst_last, last)
        assert whole <= bars and last <= bars, (b, whole, last)
        total += solver.iters
        assert solver.unconverged == 0
    assert unconv == 0 and solves == nt * n_mu
    return dict(config=label, rel_l2_whole=worst, rel_l2_last_step=worst_last, gmres_iterations=iters,
                iterations_per_solve=iters / solves, unconverged=unconv, solves=solves, steps_per_s=nt / wall,
                oracle_iterations_checked_mus=total), iters, total


def test_hrom_sweep_gmres_mode():
    """c5_hyper_reduced(n_mu = 4, r = 80), 500 BDF2 steps in GMRES mode against oracle.hrom_solve with the reference's
    gmres for all four parameter points: 1e-10 rel-L2 (whole trajectory and last step), the same iteration total."""
    rep, iters, total = _hrom_case(500, 4, 80, 1e-10, "hyper-reduced sweep, GMRES mode, 500 steps x 4 mu, r=80", range(4))
    _report(**rep)
    assert iters == total, (iters, total)


def test_direct_sweep_gmres_mode():
    """c5_direct(N = 3000, r = 24) in GMRES mode against oracle.rom_solve_nonlinear with the reference's gmres: restart
    20 < r = 24, so a system may need a second cycle (reported)."""
    from romtime_amd._lib import Context
    from romtime_amd.sweep import rom_bdf_sweep
    from romtime_amd.testing.workloads import c5_direct

    nt, N, r = 1000, 3000, 24
    fom, V, _, _ = c5_direct(N=N, r=r, n_mu=1, nt=nt, dt=1e-3, seed=3)
    mus = [dict(alpha=0.5 + 0.2 * i, beta=1.0 - 0.1 * i, delta=0.3 + 0.05 * i, omega=7.0 + i) for i in range(3)]
    d = fom.descriptor(mus)
    uN = rom_bdf_sweep(V, d["indptr"], d["indices"], d["mass"], d["terms"], d["term_coef"], d["tril"], d["rhs_terms"],
                       d["rhs_coef"], d["dt"], bdf2=True, solver="gmres")
    ctx = Context.current()
    iters, unconv, solves = (ctx.counter("sweep_gmres_iterations"), ctx.counter("sweep_gmres_unconverged"),
                             ctx.counter("sweep_solves"))
    uN = uN.cpu().numpy()
    total, worst, max_iters = 0, 0.0, 0
    for i, mu in enumerate(mus):
        solver = CountingGmres()
        ref, _ = oracle.rom_solve_nonlinear(fom, V, mu, solver=solver)
        whole, last = _rel(uN[i].T, ref), _rel(uN[i, -1], ref[:, -1])
        worst = max(worst, whole, last)
        assert whole <= 1e-10 and last <= 1e-10, (i, whole, last)
        total += solver.iters
        max_iters = max(max_iters, solver.max_iters)
    assert iters == total and unconv == 0 and solves == nt * len(mus), (iters, total, unconv, solves)
    _report(config="direct sweep, GMRES mode, 1000 steps N=3000 r=24", rel_l2=worst, iterations_per_solve=iters / solves,
            most_inner_iterations_of_a_solve=max_iters, second_cycle_needed=bool(max_iters > 20))


def test_hrom_sweep_gmres_mode_full_size():
    """C5 hyper-reduced sweep in GMRES mode at its stated size: 1e4 steps x 32 mu, r = 80; three mu against the
    oracle's GMRES loop at 1e-10."""
    rep, iters, total = _hrom_case(10_000, 32, 80, 1e-10, "C5 hyper-reduced sweep, GMRES mode, 1e4 steps x 32 mu r=80",
                                   (0, 13, 31))
    _report(**rep)


def _small_hrom():
    from romtime_amd.testing.workloads import c5_hyper_reduced

    terms, d, V, _ = c5_hyper_reduced(N=20_000, nt=60, n_mu=4, r=24)
    return (terms["mass"], terms["lin"], terms["nl"], terms["rhs"], terms["dt"]), d, V


def test_default_sweeps_unchanged_after_gmres_mode():
    """A default sweep after a GMRES-mode call is bit-identical to one before it, and the GMRES counters read 0."""
    from romtime_amd._lib import Context
    from romtime_amd.sweep import hrom_bdf_sweep, rom_bdf_sweep

    ctx = Context.current()
    args, d, V = _small_hrom()
    dargs = (V, d["indptr"], d["indices"], d["mass"], d["terms"], d["term_coef"], d["tril"], d["rhs_terms"],
             d["rhs_coef"], d["dt"])
    h0, r0 = hrom_bdf_sweep(*args).cpu().numpy(), rom_bdf_sweep(*dargs).cpu().numpy()
    hg = hrom_bdf_sweep(*args, solver="gmres").cpu().numpy()
    assert ctx.counter("sweep_gmres_iterations") > 0 and ctx.reduced_solver[0] == 0
    rg = rom_bdf_sweep(*dargs, solver="gmres", gmres_options=dict(tol=1e-12, atol=0.0)).cpu().numpy()
    # the reference's tolerance (1e-10) leaves GMRES trajectories up to ~1e-7 from the exact ones (golden cases: 1e-8 ..
    # 4e-8); a tolerance of 1e-12 brings them to the exact solve
    assert not gd.bits_equal(hg, h0) and _rel(hg, h0) <= 1e-6
    assert _rel(rg, r0) <= 1e-9
    h1 = hrom_bdf_sweep(*args).cpu().numpy()
    assert ctx.counter("sweep_gmres_iterations") == 0 and ctx.counter("sweep_gmres_unconverged") == 0
    r1 = rom_bdf_sweep(*dargs).cpu().numpy()
    assert ctx.counter("sweep_gmres_iterations") == 0 and ctx.counter("sweep_gmres_unconverged") == 0
    assert gd.bits_equal(h1, h0) and gd.bits_equal(r1, r0)
    with pytest.raises(ValueError):
        hrom_bdf_sweep(*args, solver="gmres", gmres_options=dict(callback=print))
    assert ctx.reduced_solver[0] == 0


def test_piston_workflow_in_gmres_mode(tmp_path, monkeypatch, capsys):
    """The reference's HyperReducedPiston driver sequence with RomConstructorNonlinear.REDUCED_SOLVER = "gmres": its
    existing bars hold (the direct path is 2.5e-15 from the reference's run)."""
    from romtime_amd import RomConstructorNonlinear
    from tests.conftest import load_golden
    from tests.test_hrom_flow import check_piston_workflow

    monkeypatch.setattr(RomConstructorNonlinear, "REDUCED_SOLVER", "gmres")
    check_piston_workflow(load_golden("hrom.npz"), tmp_path, monkeypatch)
    out = capsys.readouterr().out
    m = re.search(r"within ([0-9.e+-]+) rel-L2", out)
    with capsys.disabled():
        _report(test="piston workflow, REDUCED_SOLVER=gmres", worst_rel_l2_fom_space=float(m.group(1)) if m else None,
                direct_path=2.5e-15)
