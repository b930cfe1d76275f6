"""The classes' online stage on the device (romtime_amd/online.py, ONLINE_ON = "device"): ``solve`` / ``solve_many`` of the
three classes on every route against the oracle's loops and the classes' own host loop, ``online.evaluate`` against the
per-step host functions, and the fold cache.  Bars: 1e-10 against the oracle (tests/test_surface.py:311), 1e-9 for the
host loop against the oracle (:305), hence 1.1e-9 between the two routes of one object."""
import numpy as np
import pytest

from oracle import romtime_oracle as oracle
from tests.online_cases import AFFINE_MUS, HideClosedForm, affine_rom, heat_rom, host_storages, rel

pytestmark = pytest.mark.gpu

ORACLE_BAR = 1e-10
ROUTES_BAR = 1.1e-9
ONLINE = "online"


@pytest.fixture(scope="module")
def piston():
    """tests.test_surface._fully_hyper_reduced_rom() (nx = 60, nt = 14, 3 points, r <= 8) with, per point, the oracle's
    trajectory on the hrom_terms_from_rom tables and the storage the host loop leaves."""
    from romtime_amd.sweep import hrom_terms_from_rom
    from tests.test_surface import _fully_hyper_reduced_rom

    fom, rom, mus = _fully_hyper_reduced_rom()
    tm = hrom_terms_from_rom(rom, mus)
    r, nt = rom.N, fom.domain["nt"]
    refs = [oracle.hrom_solve(tm["mass"], tm["lin"], tm["nl"], tm["rhs"], b, r, nt, tm["dt"], tm["bdf2"]) for b in range(len(mus))]
    rom.mu_space[ONLINE] = []
    host = host_storages(rom, mus, ONLINE)
    return dict(fom=fom, rom=rom, mus=mus, refs=refs, host=host, host_space=list(rom.mu_space[ONLINE]))


@pytest.fixture
def device_piston(piston, monkeypatch):
    rom = piston["rom"]
    monkeypatch.setattr(rom, "ONLINE_ON", "device", raising=False)
    monkeypatch.setattr(rom, "mu_space", dict(rom.mu_space, **{ONLINE: []}))
    return piston


def _check_storage(got, want, bar, what):
    assert got.rom.shape == want.rom.shape and got.fom.shape == want.fom.shape, what
    assert got.rom.dtype == want.rom.dtype and got.fom.dtype == want.fom.dtype
    d = dict(rom=rel(got.rom, want.rom), fom=rel(got.fom, want.fom))
    print(f"{what}: {d}")
    assert max(d.values()) <= bar, (what, d)
    assert np.array_equal(got.ts, want.ts) and np.array_equal(got.domain, want.domain) and got.mu == want.mu, what


@pytest.mark.parametrize("route", ["closed_form", "callbacks"])
def test_piston_solve(device_piston, monkeypatch, route):
    """Device ``solve`` per point on both routes of the piston model (the callbacks route through a FOM that hides its
    closed forms, as a FEniCS solver would): the oracle on the host tables at 1e-10, the same object's host loop at
    1.1e-9 for ``solutions.rom`` and ``solutions.fom``, equal ``ts`` / ``domain``, the same indices and ``mu_space``."""
    from romtime_amd import online

    p = device_piston
    rom = p["rom"]
    if route == "callbacks":
        monkeypatch.setattr(rom, "fom", HideClosedForm(p["fom"]))
    assert online.plan(rom) == route
    for b, mu in enumerate(p["mus"]):
        idx = rom.solve(mu=mu, step=ONLINE)
        host_idx, host = p["host"][b]
        assert idx == host_idx
        d = rel(rom.solutions.rom, p["refs"][b])
        print(f"{route} point {b} vs oracle: {d:.3e}")
        assert d <= ORACLE_BAR, (b, d)
        _check_storage(rom.solutions, host, ROUTES_BAR, f"{route} point {b} vs host loop")
    assert rom.mu_space[ONLINE] == p["host_space"]


@pytest.mark.parametrize("chunk", [None, 2])
def test_solve_many(device_piston, chunk):
    """Three points in one sweep and in chunks of two: every trajectory within 1e-10 of the oracle, ``storage(j)`` what
    ``solve(mus[j])`` leaves within the same bar (not the same bits: the direct solver's bits may depend on the batch),
    ``solutions`` the last point's."""
    p = device_piston
    rom, mus = p["rom"], p["mus"]
    many = rom.solve_many(mus, chunk=chunk)
    assert many.idx == [i for i, _ in p["host"]] and many.mus == mus and rom.mu_space[ONLINE] == p["host_space"]
    assert many.uN.is_cuda and tuple(many.uN.shape) == (3, p["fom"].domain["nt"], rom.N)
    assert np.array_equal(many.ts, p["host"][0][1].ts)
    uN = many.uN.cpu().numpy()
    last = rom.solutions
    _check_storage(last, many.storage(2), ORACLE_BAR, "solutions after solve_many vs storage(2)")
    for b, mu in enumerate(mus):
        d = rel(uN[b].T, p["refs"][b])
        print(f"solve_many chunk={chunk} point {b} vs oracle: {d:.3e}")
        assert d <= ORACLE_BAR, (b, d)
        rom.solve(mu=mu, step=ONLINE)
        _check_storage(many.storage(b), rom.solutions, ORACLE_BAR, f"storage({b}) vs solve")


@pytest.mark.parametrize("bdf2", [False, True], ids=["bdf1", "bdf2"])
@pytest.mark.parametrize("size", [(96, 6, 5), (40, 12, 1)], ids=lambda s: "N%d_nt%d_r%d" % s)
def test_affine_route(size, bdf2):
    """AffineBurgers, no reductor: device ``solve`` against the oracle's direct loop with an exact solver and against
    ``rom_bdf_sweep`` on the descriptor, 1e-10 for ``.rom`` and ``.fom``."""
    from romtime_amd import online, ops
    from romtime_amd.sweep import rom_bdf_sweep

    N, nt, r = size
    fom, rom = affine_rom(N, nt, r, bdf2)
    rom.ONLINE_ON = "device"
    assert online.plan(rom) == "affine"
    d = fom.descriptor(AFFINE_MUS)
    direct = rom_bdf_sweep(rom.basis, d["indptr"], d["indices"], d["mass"], d["terms"], d["term_coef"], d["tril"],
                           d["rhs_terms"], d["rhs_coef"], d["dt"], bdf2=bdf2)
    lifted = ops.gemm_nn(ops.to_device(rom.basis), direct[-1].T.contiguous()).cpu().numpy()
    direct = direct.cpu().numpy()
    for b, mu in enumerate(AFFINE_MUS):
        assert rom.solve(mu=mu, step=ONLINE) == b
        want_rom, want_fom = oracle.rom_solve_nonlinear(fom, rom.basis, mu, solver=np.linalg.solve)
        got = rom.solutions
        assert got.rom.shape == (r, nt) and got.fom.shape == (N, nt) and np.abs(want_rom).max() > 1e-6
        figures = dict(rom=rel(got.rom, want_rom), fom=rel(got.fom, want_fom), sweep=rel(got.rom, direct[b].T))
        print(f"affine N={N} nt={nt} r={r} bdf2={bdf2} point {b}: {figures}")
        assert max(figures.values()) <= ORACLE_BAR, (b, figures)
    assert rel(got.fom, lifted) <= ORACLE_BAR                                # g_h = 0: .fom is V u_N


@pytest.fixture(scope="module", params=["rhs", "split"])
def heat(request):
    """The heat model of tests/test_online_cpu.py with the storages of its host loop, built once per source."""
    fom, rom, mus = heat_rom(request.param)
    return dict(source=request.param, fom=fom, rom=rom, mus=mus, host=host_storages(rom, mus, ONLINE))


@pytest.mark.parametrize("route", ["closed_form", "callbacks"])
def test_heat_classes(heat, monkeypatch, route):
    """RomConstructorMoving on the moving-mesh heat problem (tests/test_online_cpu.py), both sources and both routes:
    device ``solve`` and ``solve_many`` against the host loop at 1.1e-9."""
    from romtime_amd import online

    source, fom, rom, mus, host = heat["source"], heat["fom"], heat["rom"], heat["mus"], heat["host"]
    monkeypatch.setattr(rom, "mu_space", dict(rom.mu_space, **{ONLINE: []}))
    monkeypatch.setattr(rom, "ONLINE_ON", "device", raising=False)
    if route == "callbacks":
        monkeypatch.setattr(rom, "fom", HideClosedForm(fom))
    assert online.plan(rom) == route
    many = rom.solve_many(mus)
    for b, mu in enumerate(mus):
        assert rom.solve(mu=mu, step=ONLINE) == host[b][0]
        _check_storage(rom.solutions, host[b][1], ROUTES_BAR, f"heat {source} {route} point {b} vs host loop")
        _check_storage(many.storage(b), host[b][1], ROUTES_BAR, f"heat {source} {route} solve_many point {b} vs host loop")


def test_gmres_follows_reduced_solver(device_piston, monkeypatch):
    """REDUCED_SOLVER = "gmres" with ONLINE_ON = "device" against the host class loop with the same setting, on the piston
    case.  The bar is that of tests/test_gmres_gpu.py::test_hrom_sweep_gmres_mode, the existing comparison of
    hrom_bdf_sweep(solver="gmres") with a host GMRES loop: 1e-10 rel-L2 of the whole trajectory."""
    from romtime_amd._lib import Context

    p = device_piston
    rom = p["rom"]
    monkeypatch.setattr(rom, "REDUCED_SOLVER", "gmres", raising=False)
    monkeypatch.setattr(rom, "algebraic_solver", rom.create_algebraic_solver())
    host = host_storages(rom, p["mus"], ONLINE)
    direct = [s for _, s in p["host"]]
    many = rom.solve_many(p["mus"])
    assert Context.current().counter("sweep_gmres_iterations") > 0               # the sweep did run GMRES
    for b in range(len(p["mus"])):
        got, want = many.storage(b), host[b][1]
        figures = dict(rom=rel(got.rom, want.rom), fom=rel(got.fom, want.fom), host_gmres_vs_direct=rel(want.rom, direct[b].rom))
        print(f"gmres point {b}: {figures}")
        assert figures["rom"] <= 1e-10 and figures["fom"] <= 1e-10, (b, figures)


def test_evaluate_against_the_per_step_host_functions(piston):
    """``online.evaluate`` of a ROM / S-ROM pair (the helper's reductors, copied and projected on each basis; the S-ROM has
    two modes more) with which = ONLINE, so the FOM truth is the device sweep: each of the three curves against the
    per-step host functions (Reductor._compute_error, utils.compute_rom_difference) on the host-route solutions and the
    same FOM trajectories.  Per-step bar: the l2 distance of the two routes' ``solutions.fom`` over sqrt(N_h) - of the ROM,
    of the S-ROM, of both for the estimator, which is their difference - plus tests.certify_cases.error_bar of the
    operands: a triangle inequality.  The mass payload equals outputs.mass_conservation called by hand on the same uN."""
    from romtime_amd import fom as device_fom
    from romtime_amd import online, outputs
    from romtime_amd.conventions import Errors, MassConservation, ProblemType
    from romtime_amd.rom import _HYPER_SLOTS
    from romtime_amd.utils import compute_rom_difference
    from tests.certify_cases import error_bar

    fom, srom = piston["fom"], piston["rom"]
    rom = srom.truncate(2)
    assert srom.N == rom.N + 2
    for which, slot in _HYPER_SLOTS.items():
        if getattr(srom, slot):
            rom.add_hyper_reductor(getattr(srom, slot), which)
    rom.project_reductors()
    mus = [dict(mu, a0=14.0 + 2.0 * j) for j, mu in enumerate(piston["mus"])]
    keep_space, keep_on = dict(srom.mu_space), srom.__dict__.get("ONLINE_ON")
    try:
        host = {}
        for name, model in (("rom", rom), ("srom", srom)):
            model.mu_space = dict(model.mu_space, **{ONLINE: []})
            host[name] = [s for _, s in host_storages(model, mus, ONLINE)]
            model.mu_space = dict(model.mu_space, **{ONLINE: []})
            model.ONLINE_ON = "device"
        ev = online.evaluate(rom, srom, mus, ONLINE, probes=[0.0, 0.5, np.inf], chunk=2)
    finally:
        srom.mu_space = keep_space
        if keep_on is None:
            srom.__dict__.pop("ONLINE_ON", None)
        else:
            srom.ONLINE_ON = keep_on
    assert sorted(ev) == [0, 1, 2]
    ts = online.times(fom)
    rec = device_fom.recipe(fom, mus)
    (_, U), = device_fom.fom_sweep(fom, mus, rec=rec)
    full = device_fom.full_solution(U, rec["lift"]).cpu().numpy()                  # (n_mu, nt, N_h)
    U = U.cpu().numpy()
    Nh, nt = fom.Nh, len(ts)
    uN = np.concatenate([s.uN.cpu().numpy() for s in ev.solutions[ProblemType.ROM]])
    uNs = np.concatenate([s.uN.cpu().numpy() for s in ev.solutions[ProblemType.SROM]])
    dev = {"rom": [s.storage(j) for s in ev.solutions[ProblemType.ROM] for j in range(len(s))],
           "srom": [s.storage(j) for s in ev.solutions[ProblemType.SROM] for j in range(len(s))]}
    worst = 0.0
    for j in range(3):
        assert set(ev[j]) == {Errors.ESTIMATOR, Errors.ROM, Errors.SACRIFICIAL}
        uh = full[j].T
        route = {k: np.linalg.norm(dev[k][j].fom - host[k][j].fom, axis=0) / np.sqrt(Nh) for k in ("rom", "srom")}
        for key, k, V, a in ((Errors.ROM, "rom", rom.basis, uN[j]), (Errors.SACRIFICIAL, "srom", srom.basis, uNs[j])):
            want = np.array([rom._compute_error(u=host[k][j].fom[:, t], ue=uh[:, t]) for t in range(nt)])
            bar = route[k] + error_bar(V, a, U[j].T, want)
            got = ev[j][key]
            worst = max(worst, float(np.max(np.abs(got - want) / bar)))
            assert got.shape == want.shape and np.all(np.abs(got - want) <= bar), (key, j, np.abs(got - want).max(), bar.min())
        want = np.array([compute_rom_difference(host["rom"][j].rom[:, t], host["srom"][j].rom[:, t], srom.basis) for t in range(nt)])
        d = uNs[j].copy()
        d[:, : rom.N] -= uN[j]
        bar = route["rom"] + route["srom"] + error_bar(srom.basis, d, None, want)
        got = ev[j][Errors.ESTIMATOR]
        worst = max(worst, float(np.max(np.abs(got - want) / bar)))
        assert got.shape == want.shape and np.all(np.abs(got - want) <= bar), ("estimator", j, np.abs(got - want).max(), bar.min())
        assert np.max(ev[j][Errors.ROM]) > 1e-6                                     # errors of a truncated basis, not rounding
    print(f"evaluate: worst |curve - truth| / bar = {worst:.3f}")
    # mass conservation and probes: the same calls by hand on the same uN
    L = np.ascontiguousarray(fom.p1_closed_form(mus, ts)["h"].T) * fom.nx
    lift = online.lifting(fom, mus, ts)
    by_hand = outputs.mass_conservation(rom.basis, uN, mus, fom.dt, L, gamma=1.4, lift=lift, ts=ts)
    probes = outputs.probes(rom.basis, uN, [0.0, 0.5, np.inf], L, lift=lift)
    for j in range(3):
        got = ev.mass[j][ProblemType.ROM]
        assert set(got) == set(by_hand[j]) and got[MassConservation.WHICH] == ProblemType.ROM
        for key in (MassConservation.TIMESTEPS, MassConservation.MASS, MassConservation.MASS_CHANGE, MassConservation.OUTFLOW):
            assert got[key].shape == by_hand[j][key].shape == (nt,) and np.array_equal(got[key], by_hand[j][key]), (j, key)
        want = outputs.snapshot_mass_conservation(full[j].T, mus[j], fom.dt, L[j], gamma=1.4, ts=ts)
        got = ev.mass[j][ProblemType.FOM]
        assert set(got) == set(want) and got[MassConservation.WHICH] == ProblemType.FOM
        for key in (MassConservation.MASS, MassConservation.OUTFLOW):        # the same rule on the same trajectory, up to
            assert np.allclose(got[key], want[key], rtol=1e-12, atol=1e-14), (j, key)   # the rounding of adding the lifting
        assert ev.probes[j].shape == (nt, 3) and np.array_equal(ev.probes[j], probes[j])


def test_fold_cache(device_piston, monkeypatch):
    """The second ``solve`` on one object folds nothing (no ops.dense_solve_multi call); after project_reductors() the
    next one folds every reductor again."""
    from romtime_amd import ops

    p = device_piston
    rom, mu = p["rom"], p["mus"][0]
    calls = []
    real = ops.dense_solve_multi
    monkeypatch.setattr(ops, "dense_solve_multi", lambda K, B: (calls.append(tuple(B.shape)), real(K, B))[1])
    rom.project_reductors()
    rom.solve(mu=mu, step=ONLINE)
    assert len(calls) == 6, calls                                  # one fold per reductor of the class
    rom.solve(mu=p["mus"][1], step=ONLINE)
    rom.solve(mu=mu, step=ONLINE)
    assert len(calls) == 6, calls
    assert rel(rom.solutions.rom, p["refs"][0]) <= ORACLE_BAR
    rom.project_reductors()
    rom.solve(mu=mu, step=ONLINE)
    assert len(calls) == 12, calls
    assert rel(rom.solutions.rom, p["refs"][0]) <= ORACLE_BAR
