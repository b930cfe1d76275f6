"""The GMRES reduced solver without a GPU: how the reference's option dictionary becomes ``rt_gmres_opts``, and the
class wiring of ``REDUCED_SOLVER = "gmres"`` on the CPU stub with SciPy's gmres standing in for the device kernel."""
import numpy as np
import pytest
import torch
from scipy.sparse.linalg import gmres as scipy_gmres

from romtime_amd.gmres import gmres_opts

CASES = ["r10_bdf1", "r10_bdf2", "r24_bdf1", "r24_bdf2"]


def _fields(o):
    return (o.rtol, o.atol, o.restart, o.maxiter)


@pytest.mark.parametrize("r", [1, 5, 10, 20, 24, 80, 128])
def test_reference_options(r):
    """rom.py:36 as the reference passes it: tol / atol 1e-10, restart min(20, r), maxiter 1e6 as an integer."""
    assert _fields(gmres_opts(dict(atol=1e-10, tol=1e-10, maxiter=1e6), r)) == (1e-10, 1e-10, min(20, r), 1_000_000)


def test_spellings_and_defaults():
    assert _fields(gmres_opts(dict(rtol=1e-6), 30)) == (1e-6, 0.0, 20, 300)          # SciPy >= 1.14 spelling
    assert _fields(gmres_opts(None, 7)) == (1e-5, 0.0, 7, 70)                          # SciPy's defaults
    assert _fields(gmres_opts({}, 50)) == (1e-5, 0.0, 20, 500)
    assert _fields(gmres_opts(dict(restart=None, maxiter=None), 3)) == (1e-5, 0.0, 3, 30)
    assert _fields(gmres_opts(dict(tol=1e-8, rtol=1e-8, restart=5, maxiter=3), 50)) == (1e-8, 0.0, 5, 3)
    assert _fields(gmres_opts(dict(restart=128, maxiter=np.int64(4), atol=np.float64(2.0)), 128)) == (1e-5, 2.0, 128, 4)


@pytest.mark.parametrize("bad", [dict(tol=1e-8, rtol=1e-9), dict(x0=np.zeros(3)), dict(M=None), dict(callback=print),
                                 dict(callback_type="pr_norm"), dict(tolerance=1e-8), dict(maxiter=2.5), dict(maxiter=0),
                                 dict(maxiter=True), dict(restart=0), dict(restart=-3), dict(atol=-1.0),
                                 dict(rtol=float("nan")), dict(atol=float("inf")), dict(rtol="1e-6")])
def test_bad_options_raise(bad):
    with pytest.raises(ValueError):
        gmres_opts(bad, 10)


def _scipy_gmres_solve(calls):
    """ops.gmres_solve on the host: SciPy's gmres with the options as the device solver reads them."""

    def solve(K, b, opts=None):
        Kn = K.detach().cpu().numpy()
        bn = b.detach().cpu().numpy()
        single = Kn.ndim == 2
        Kn, bn = Kn.reshape(-1, Kn.shape[-2], Kn.shape[-1]), bn.reshape(Kn.shape[0] if Kn.ndim == 3 else 1, -1)
        o = gmres_opts(opts, Kn.shape[-1])
        xs, infos, iters = [], [], []
        for k, rhs in zip(Kn, bn):
            hist = []
            x, info = scipy_gmres(k, rhs, rtol=o.rtol, atol=o.atol, restart=o.restart, maxiter=o.maxiter,
                                  callback=hist.append, callback_type="pr_norm")
            xs.append(x)
            infos.append(info)
            iters.append(len(hist))
        calls.append(len(xs))
        x, info, it = torch.from_numpy(np.array(xs)), torch.tensor(infos, dtype=torch.int64), torch.tensor(iters, dtype=torch.int32)
        return (x[0], info[0], it[0]) if single else (x, info, it)

    return solve


def _count_dense(calls, dense):
    def solve(K, b):
        calls.append(1)
        return dense(K, b)

    return solve


def _online(g, case, cls):
    from tests.test_surface import _burgers

    fom = _burgers(case.endswith("bdf2"))
    a, d, w = g["mu"]
    rom = cls(fom=fom, grid=None, name="golden")
    rom.setup(rnd=0)
    rom.basis = g[f"V__{case}"]
    rom.solve(mu=dict(alpha_0=a, delta=d, omega=w), step="online")
    return rom, fom


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("case", CASES)
def test_gmres_mode_reproduces_the_reference_trajectories(cpu_ops, golden_rom, monkeypatch, case):
    """RomConstructorNonlinear with REDUCED_SOLVER = "gmres" calls ops.gmres_solve once per step with the class's
    GMRES_OPTIONS; with SciPy's gmres behind it the online loop IS the reference's: the golden trajectories (produced by
    the reference's own code) to 1e-12.  The direct path is 1e-8 .. 4e-8 away from them."""
    from romtime_amd import RomConstructorNonlinear, ops

    gm, dense = [], []
    monkeypatch.setattr(ops, "gmres_solve", _scipy_gmres_solve(gm))
    monkeypatch.setattr(ops, "dense_solve", _count_dense(dense, ops.dense_solve))
    monkeypatch.setattr(RomConstructorNonlinear, "REDUCED_SOLVER", "gmres")
    rom, fom = _online(golden_rom, case, RomConstructorNonlinear)
    nt = fom.domain["nt"]
    assert gm == [1] * nt and dense == []
    assert _rel(rom.solutions.rom, golden_rom[f"rom__{case}"]) <= 1e-12
    assert _rel(rom.solutions.fom, golden_rom[f"fom__{case}"]) <= 1e-12


def test_default_class_still_solves_directly(cpu_ops, golden_rom, monkeypatch):
    from romtime_amd import RomConstructorNonlinear, ops

    gm, dense = [], []
    monkeypatch.setattr(ops, "gmres_solve", _scipy_gmres_solve(gm))
    monkeypatch.setattr(ops, "dense_solve", _count_dense(dense, ops.dense_solve))
    assert RomConstructorNonlinear.REDUCED_SOLVER == "direct"
    rom, fom = _online(golden_rom, "r10_bdf2", RomConstructorNonlinear)
    assert gm == [] and len(dense) == fom.domain["nt"]


def test_selection_is_read_at_setup_and_survives_truncate(cpu_ops, golden_rom, monkeypatch):
    from romtime_amd import RomConstructorNonlinear, ops
    from tests.test_surface import _burgers

    gm, dense = [], []
    monkeypatch.setattr(ops, "gmres_solve", _scipy_gmres_solve(gm))
    monkeypatch.setattr(ops, "dense_solve", _count_dense(dense, ops.dense_solve))
    rom = RomConstructorNonlinear(fom=_burgers(True), grid=None, name="srom")
    rom.REDUCED_SOLVER = "gmres"
    rom.GMRES_OPTIONS = dict(tol=1e-6, restart=5)
    rom.setup(rnd=0)
    rom.basis = golden_rom["V__r24_bdf2"]
    small = rom.truncate(4)
    assert small.N == 20 and small.REDUCED_SOLVER == "gmres" and small.GMRES_OPTIONS == dict(tol=1e-6, restart=5)
    assert small.GMRES_OPTIONS is not rom.GMRES_OPTIONS
    x, info = small.algebraic_solver(A=np.eye(20) * 2.0, b=np.ones(20))
    assert gm == [1] and dense == [] and info == 0 and np.allclose(x, 0.5)
    rom.GMRES_OPTIONS["x0"] = None          # changed after setup: the solver built at setup is unaffected
    rom.algebraic_solver(A=np.eye(24), b=np.ones(24))
    with pytest.raises(ValueError):
        rom.setup(rnd=0)                    # ... and the next setup reads (and rejects) it
    bad = RomConstructorNonlinear(fom=_burgers(True), grid=None, name="bad")
    bad.REDUCED_SOLVER = "lu"
    with pytest.raises(ValueError):
        bad.setup(rnd=0)


class _FakeCtx:
    def __init__(self):
        self.reduced_solver = (0, None)
        self.calls = []

    def set_reduced_solver(self, kind, opts=None):
        self.calls.append(kind)
        self.reduced_solver = (kind, opts)


def test_sweep_solver_selection_is_scoped_and_restored_on_error():
    from romtime_amd.sweep import reduced_solver

    ctx = _FakeCtx()
    with pytest.raises(RuntimeError):
        with reduced_solver(ctx, "gmres", None, 24):
            kind, o = ctx.reduced_solver
            assert kind == 1 and (o.rtol, o.atol, o.restart, o.maxiter) == (1e-10, 1e-10, 20, 1_000_000)
            raise RuntimeError("sweep failed")
    assert ctx.reduced_solver == (0, None) and ctx.calls == [1, 0]
    with reduced_solver(ctx, "direct", None, 24):     # already direct: the ctx is not touched
        pass
    assert ctx.calls == [1, 0]
    with reduced_solver(ctx, "gmres", dict(rtol=1e-6, restart=5), 80):
        assert ctx.reduced_solver[1].restart == 5 and ctx.reduced_solver[1].maxiter == 800
    for solver, opts in (("lu", None), ("direct", dict(tol=1e-6)), ("gmres", dict(x0=0))):
        with pytest.raises(ValueError):
            with reduced_solver(ctx, solver, opts, 24):
                pass
    assert ctx.reduced_solver == (0, None)
