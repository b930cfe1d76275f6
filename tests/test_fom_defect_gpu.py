"""rt_p1_fom_bdf_sweep_certified on the device (cases and references: tests/fom_defect_cases.py).  Every array of every
call sits in a guarded buffer: ``defect``, ``info`` and ``U`` behind canaries, ``tab`` and ``u_init`` inside quiet NaNs.

1. the same solve: U is bit-equal to rt_p1_fom_bdf_sweep's, on the convective cases and on the dominant cases of
   test_fom_gpu.py;
2. every step held on its own: omega_test, the long-double defect of the device's new state for the float64 rows formed
   from the device's two states before it, is at most F x OMEGA_REF;
3. the reported defect is that defect: at most F x OMEGA_REF on the convective cases, within a factor of two of
   omega_test on the flag cases where omega_test >= 1e-8;
4. the flag rule; 5. trajectories within K d_host + 64 eps of the long-double truth; 6. independence of batch and
   chunking, defects included; 7. the class surface.

F and K.  OMEGA_REF = 2.117e-15 (9.5 eps, the float64 sequential elimination).  Measured on the MI355X over all 22
convective cases: worst omega_test / OMEGA_REF = 15323 (3.244e-11, nx = 2049 BDF1, point alpha_0 = 1e-6) and worst
defect / OMEGA_REF = 15323 (the reported defect is 1.03 - 1.2 times omega_test wherever omega_test is above 1e-15); F is
the next power of two at or above four times that, 65536.  Worst d_dev / d_host = 15.31 (1.317e-13 against 8.603e-15, the
same case), above 4, so K is the next power of two at or above twice it, 32.

The ratio is far above 64, and that is a finding about the solve, not about the defect pass.  By rows per partition m:
nx <= 65 at most 1.1 OMEGA_REF; m = 1 (nx = 1024, 1025: pure cyclic reduction) 88 - 494; m = 2 (nx = 1026, 2049) 3035 -
15323; m = 3 (nx = 2050) 30 - 46; m = 4 (nx = 3100) 1282 - 4062; nx = 1000, nt = 100: 3.6; N_h = 1e5 (m = 98): 1.5.  A
float64 NumPy model of the three passes gives the same figures (2.7e-11 at nx = 2049), and the same model with the
interface system handed to a pivoted banded solve instead of the parallel cyclic reduction gives 1.5e-14: the loss is
in pass B.  With CFL numbers of 40 to 90 the multipliers c = u / pivot reach 10, for m = 2 the interface rows are
f xB_p-1 + (1 - c F) xB_p - c G xB_p+1 with |c G| about 100 against a diagonal of 1 to 2, and cyclic reduction without
pivoting is only normwise stable on such rows; where |x_i| is 1e2 - 1e3 below max |x| the componentwise measure shows
it.  The trajectories stay 1.3e-13 from the truth and every defect below the default tolerance 1e-10, by a factor of
three at the worst: F x OMEGA_REF = 1.4e-10 is above that tolerance, so on these cases the binding check is info == 0.
Every test prints its figures before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import fom_cases as fc
from tests import fom_defect_cases as dc
from tests import guarded

pytestmark = pytest.mark.gpu

WORST_OMEGA_RATIO = 15323.4      # measured: see the docstring
WORST_TRUTH_RATIO = 15.31
F = 65536.0                      # the next power of two at or above 4 WORST_OMEGA_RATIO
K = 32.0                         # the next power of two at or above 2 WORST_TRUTH_RATIO (the project's 8 where that is <= 4)

CONV_NAMES = [f"nx{nx}-bdf{2 if b else 1}" for nx, b in dc.conv_keys()] + ["piston-nx1000-nt100", "size-nx100000"]


def _conv(name):
    if name.startswith("piston"):
        return dc.piston_case()
    if name.startswith("size"):
        return dc.size_case()
    nx, b = name[2:].split("-bdf")
    return dc.conv_case(int(nx), b == "2")


def certified(nx, tab, dt, bdf2, state_in_w, u_init=None, first_step=0, tol=dc.DEFECT_TOL):
    """The C entry on guarded buffers; (U, info, defect) as host arrays, every guard checked."""
    from romtime_amd import _lib
    from romtime_amd._lib import Context

    tab = np.ascontiguousarray(np.asarray(tab, dtype=np.float64))
    nt, n_mu, Nh = tab.shape[0], tab.shape[1], nx + 1
    tab_host = tab.reshape(nt, n_mu * 7)
    tab_d = guarded.guarded_operand(tab_host, misalign=True)
    init_host, init_d = None, None
    if u_init is not None:
        init_host = np.ascontiguousarray(np.asarray(u_init, dtype=np.float64)).reshape(n_mu * 2, Nh)
        init_d = guarded.guarded_operand(init_host, guard=4)
    out = guarded.guarded_output((n_mu * nt, Nh), guard=4)
    defect = guarded.guarded_output((n_mu, nt), misalign=True)
    flags = torch.full((n_mu + 64,), -77, dtype=torch.int32, device="cuda")
    ctx = Context.current()
    desc = _lib.FomDesc(nx, n_mu, nt, int(first_step), float(dt), int(bool(bdf2)), int(bool(state_in_w)),
                        C.c_void_p(tab_d.data_ptr()), None if init_d is None else C.c_void_p(init_d.data_ptr()))
    ctx.check(ctx.lib.rt_p1_fom_bdf_sweep_certified(ctx.handle, C.byref(desc), C.c_void_p(out.t.data_ptr()), Nh, nt * Nh, float(tol),
                                                    C.c_void_p(defect.t.data_ptr()), C.c_void_p(flags[32:].data_ptr())),
              "rt_p1_fom_bdf_sweep_certified")
    torch.cuda.synchronize()
    assert out.check() == [] and defect.check() == [], (out.check(), defect.check())
    assert (flags[:32] == -77).all() and (flags[32 + n_mu:] == -77).all()
    assert guarded.operand_intact(tab_d, tab_host) == []
    if init_d is not None:
        assert guarded.operand_intact(init_d, init_host) == []
    return out.t.cpu().numpy().reshape(n_mu, nt, Nh), flags[32:32 + n_mu].cpu().numpy(), defect.t.cpu().numpy()


def plain(nx, tab, dt, bdf2, state_in_w, **kw):
    from romtime_amd import ops

    U, info = ops.p1_fom_bdf_sweep(nx, np.ascontiguousarray(tab), dt, bdf2, state_in_w, **kw)
    return U.cpu().numpy(), info.cpu().numpy()


def expected_info(defect, tol, first_step=0):
    bad = ~(defect <= tol)
    return np.where(bad.any(axis=1), 1 + first_step + bad.argmax(axis=1), 0)


@functools.lru_cache(maxsize=None)
def device_run(name):
    """One certified and one plain sweep of a convective case, shared by the tests below."""
    c = _conv(name)
    U, info, defect = certified(c["nx"], c["rec"]["tab"], c["dt"], c["bdf2"], c["state_in_w"])
    U0, info0 = plain(c["nx"], c["rec"]["tab"], c["dt"], c["bdf2"], c["state_in_w"])
    om = dc.step_defects(c["nx"], c["rec"]["tab"], c["dt"], c["bdf2"], c["state_in_w"], U)
    return dict(U=U, info=info, defect=defect, U0=U0, info0=info0, omega_test=om)


# ---- 1. the same solve ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONV_NAMES)
def test_same_bits_as_the_dominance_entry_on_convective_cases(name):
    c, d = _conv(name), device_run(name)
    print(f"{name}: dominance entry info {d['info0'].tolist()}, certified info {d['info'].tolist()}")
    assert guarded.bits_equal(d["U"], d["U0"]), guarded.mismatch(d["U"], d["U0"])
    assert (d["U"][:, :, 0] == 0).all() and (d["U"][:, :, -1] == 0).all()
    if c["nx"] >= 65:
        assert d["info0"].all()                                              # what the existing entry makes of these models


def test_same_bits_as_the_dominance_entry_on_its_own_cases():
    nxp = 2 * fc.partitions() + 2
    keys = fc.row_case_keys() + fc.step_case_keys() + fc.size_case_keys()
    keys += [(k, 64, 3, True, 3, None) for k in ("burgers", "heat")] + [(k, 200, 40, True, 3, None) for k in ("burgers", "heat")]
    keys += [(k, nxp, 4, True, 3, (True, k == "burgers")) for k in ("burgers", "heat")] + [("burgers", 200, 9, True, 3, None)]
    for kind, nx, nt, bdf2, n_mu, flags in keys:
        fom = fc.make_fom(kind, nx, nt, bdf2=bdf2)
        rec = fc.recipe(fom, fc.mus_of(kind, n_mu))
        f_bdf2, f_state = (rec["bdf2"], rec["state_in_w"]) if flags is None else flags
        U, info, defect = certified(nx, rec["tab"], fom.dt, f_bdf2, f_state)
        U0, info0 = plain(nx, rec["tab"], fom.dt, f_bdf2, f_state)
        print(f"{kind} nx {nx} nt {nt} bdf2 {f_bdf2} state {f_state}: worst defect {defect.max():.3e}")
        assert guarded.bits_equal(U, U0), (kind, nx, nt, flags, guarded.mismatch(U, U0))
        assert not info.any() and not info0.any() and defect.max() <= dc.DEFECT_TOL


# ---- 2., 3. and 5. on the convective cases --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONV_NAMES)
def test_every_step_held_on_its_own(name):
    c, d, ref = _conv(name), device_run(name), dc.omega_ref()
    worst = float(d["omega_test"].max())
    norm = dc.step_defects(c["nx"], c["rec"]["tab"], c["dt"], c["bdf2"], c["state_in_w"], d["U"], normwise=True).max()
    print(f"{name}: worst omega_test {worst:.3e} = {worst / ref:.3f} OMEGA_REF ({ref:.3e}), bar {F:g} OMEGA_REF; normwise {norm:.3e}")
    assert worst <= F * ref


@pytest.mark.parametrize("name", CONV_NAMES)
def test_reported_defect_on_convective_cases(name):
    d, ref = device_run(name), dc.omega_ref()
    worst = float(d["defect"].max())
    ratio = float(np.max(d["defect"] / np.maximum(d["omega_test"], fc.EPS / 8)))
    print(f"{name}: worst defect {worst:.3e} = {worst / ref:.3f} OMEGA_REF, worst defect / omega_test {ratio:.2f}")
    assert np.isfinite(d["defect"]).all() and (d["defect"] >= 0).all()
    assert worst <= F * ref
    assert not d["info"].any()


@pytest.mark.parametrize("name", CONV_NAMES)
def test_trajectories_against_the_truth(name):
    c, d = _conv(name), device_run(name)
    dist = fc.rel(d["U"], c["truth"])
    bar = K * c["d_host"] + 64.0 * fc.EPS
    print(f"{name}: d_host {c['d_host']:.3e} d_dev {dist:.3e} ratio {dist / c['d_host']:.3f} bar {bar:.3e} margin {c['margin']:.3e}")
    assert dist <= bar


# ---- 3. and 4. on the flag cases ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flag_run(nx):
    tab, dt = dc.flag_table(nx)
    U, info, defect = certified(nx, tab, dt, False, False)
    return dict(tab=tab, dt=dt, U=U, info=info, defect=defect, omega_test=dc.step_defects(nx, tab, dt, False, False, U))


@pytest.mark.parametrize("nx", dc.FLAG_NX)
def test_flag_case(nx):
    r = flag_run(nx)
    tab, dt, defect, om = r["tab"], r["dt"], r["defect"], r["omega_test"]
    print(f"nx {nx}: defect {defect.tolist()} omega_test {om.tolist()} info {r['info'].tolist()}")
    assert np.isfinite(r["U"]).all()
    assert r["info"].tolist() == expected_info(defect, dc.DEFECT_TOL).tolist()
    if om[0, 1] >= 1e-8:                                                     # the reported defect is that defect
        assert 0.5 * om[0, 1] <= defect[0, 1] <= 2.0 * om[0, 1]
    if defect[0, 1] > dc.DEFECT_TOL:
        assert r["info"][0] == 2
    else:                                                                    # a good solve after all: then it is the truth's
        T, _, _ = fc.truth(nx, tab[:, :1], dt, False, False)
        d_host = fc.rel(fc.superlu_sweep(nx, tab[:, :1], dt, False, False), T)
        assert r["info"][0] == 0 and fc.rel(r["U"][:1], T) <= K * d_host + 64.0 * fc.EPS
    others = np.delete(defect.ravel(), 1)
    assert others.max() <= F * dc.omega_ref() and np.delete(om.ravel(), 1).max() <= F * dc.omega_ref()
    # point 1 is not touched by its neighbour's flag
    alone, info1, defect1 = certified(nx, tab[:, 1:], dt, False, False)
    assert r["info"][1] == 0 and info1.tolist() == [0]
    assert guarded.bits_equal(alone[0], r["U"][1]) and guarded.bits_equal(defect1[0], defect[1])


def test_a_flag_case_qualifies():
    qualified = [nx for nx in dc.FLAG_NX if flag_run(nx)["omega_test"][0, 1] >= 1e-8]
    print("flag cases with omega_test >= 1e-8:", qualified, [f"{flag_run(nx)['omega_test'][0, 1]:.3e}" for nx in dc.FLAG_NX])
    assert qualified


def test_flag_rule_at_the_median_defect():
    c, d = dc.conv_case(1025, True), device_run("nx1025-bdf2")
    tol = float(np.median(d["defect"]))
    U, info, defect = certified(c["nx"], c["rec"]["tab"], c["dt"], c["bdf2"], c["state_in_w"], tol=tol)
    want = expected_info(d["defect"], tol)
    print(f"tol = median defect {tol:.3e}: info {info.tolist()} expected {want.tolist()}")
    assert guarded.bits_equal(U, d["U"]) and guarded.bits_equal(defect, d["defect"])
    assert info.tolist() == want.tolist() and want.any()
    # a chunk that starts later reports the global step
    cut = 5
    init = np.stack([d["U"][:, cut - 1], d["U"][:, cut - 2]], axis=1)
    U2, info2, defect2 = certified(c["nx"], c["rec"]["tab"][cut:], c["dt"], c["bdf2"], c["state_in_w"], u_init=init, first_step=cut, tol=tol)
    assert guarded.bits_equal(U2, d["U"][:, cut:]) and guarded.bits_equal(defect2, d["defect"][:, cut:])
    assert info2.tolist() == expected_info(d["defect"][:, cut:], tol, first_step=cut).tolist()


def test_non_finite_step_of_one_point():
    c = dc.conv_case(65, True)
    tab = c["rec"]["tab"][:3].copy()
    base_U, base_info, base_defect = certified(65, tab, c["dt"], True, True)
    tab[2, 1, 0] = 0.0                                                       # h = 0 at step 2 of point 1
    U, info, defect = certified(65, tab, c["dt"], True, True)
    print(f"h = 0: info {info.tolist()} defect of the point {defect[1].tolist()}")
    assert info.tolist() == [0, 3, 0] and defect[1, 2] == np.inf
    for j in (0, 2):
        assert guarded.bits_equal(U[j], base_U[j]) and guarded.bits_equal(defect[j], base_defect[j])
    assert guarded.bits_equal(U[1, :2], base_U[1, :2]) and guarded.bits_equal(defect[1, :2], base_defect[1, :2])
    assert not base_info.any()


def test_argument_refusals_before_any_launch():
    from romtime_amd import _lib
    from romtime_amd._lib import Context

    ctx = Context.current()
    tab = torch.zeros((1, 1, 7), dtype=torch.float64, device="cuda")
    U = guarded.guarded_output((1, 9))
    defect = guarded.guarded_output((1, 1))
    info = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    desc = _lib.FomDesc(8, 1, 1, 0, 0.1, 0, 0, C.c_void_p(tab.data_ptr()), None)
    call = lambda tol, dp: ctx.lib.rt_p1_fom_bdf_sweep_certified(ctx.handle, C.byref(desc), C.c_void_p(U.t.data_ptr()), 9, 9, tol, dp,
                                                                 C.c_void_p(info.data_ptr()))
    dp = C.c_void_p(defect.t.data_ptr())
    assert call(1e-10, None) == -1 and call(-1.0, dp) == -1 and call(float("nan"), dp) == -1
    torch.cuda.synchronize()
    assert (guarded._as_bits(U.buf) == guarded.CANARY_BITS).all() and (guarded._as_bits(defect.buf) == guarded.CANARY_BITS).all()
    assert info.tolist() == [-77]


# ---- 6. independence ----------------------------------------------------------------------------------------------------------------
def test_chunked_horizon_and_batch_place():
    from romtime_amd import fom as dfom

    c, d = dc.conv_case(2050, True), device_run("nx2050-bdf2")
    whole, chunked = {}, {}
    (_, U), = dfom.fom_sweep(c["fom"], c["mus"], check="defect", report=whole)
    blocks = list(dfom.fom_sweep(c["fom"], c["mus"], chunk=5, check="defect", report=chunked))
    assert [b[0] for b in blocks] == [0, 5, 10]
    assert guarded.bits_equal(U.cpu().numpy(), d["U"]) and guarded.bits_equal(whole["defect"], d["defect"])
    assert guarded.bits_equal(torch.cat([b[1] for b in blocks], dim=1).cpu().numpy(), d["U"])
    assert guarded.bits_equal(chunked["defect"], d["defect"])
    for j in range(3):
        U1, info1, defect1 = certified(c["nx"], c["rec"]["tab"][:, j:j + 1], c["dt"], c["bdf2"], c["state_in_w"])
        assert guarded.bits_equal(U1[0], d["U"][j]) and guarded.bits_equal(defect1[0], d["defect"][j]) and info1.tolist() == [0]


# ---- 7. class surface -----------------------------------------------------------------------------------------------------------------
PISTON_BASIS = 40
PISTON_MUS = [dict(alpha_0=1e-6, delta=0.1, omega=6.0), dict(alpha_0=1e-6, delta=0.15, omega=4.0), dict(alpha_0=1e-6, delta=0.3, omega=9.0)]


def _build(where, check):
    from romtime_amd.conventions import RomParameters
    from romtime_amd.rom import RomConstructor

    fom = dc.make_fom(1000, 100, True, T=1.0)
    rom = RomConstructor(fom=fom, grid={k: [v] for k, v in PISTON_MUS[0].items()})
    rom.SNAPSHOTS_ON, rom.FOM_CHECK = where, check
    rom.setup(rnd=0)
    sols = rom.build_reduced_basis(mu_space=[dict(mu) for mu in PISTON_MUS], num_basis=PISTON_BASIS,
                                   tolerances={RomParameters.TOL_TIME: 1.0 - 1e-6})
    return fom, rom, sols


def test_build_reduced_basis_of_the_piston_sizes():
    """The test that shows the feature: "dominance" raises, "defect" builds.  40 modes, not the 8 of test_fom_gpu.py's
    diffusive models: the singular values of these convective snapshots fall from 53 to 4.7 over the first eight and to
    0.047 at the fortieth, so 8 modes leave a third of the set outside (projection error 20.9 of a norm of 66).  The
    two-level POD's basis is then not the optimal one, its projection error moves in first order with a rotation of
    the basis, and the bar e_dev <= e_host + 4 |dX|_F - a second-order statement about a converged basis - does not
    describe it: measured on the device with 8 modes, e_dev - e_host = 9.0e-11 against 4 |dX|_F = 2.0e-12 (on the host
    stand-ins 7.6e-11 against 1.3e-12; with 16 modes -9e-15, with 40 modes -5e-14).  40 modes capture the set to 1 %."""
    from romtime_amd import fom as dfom

    with pytest.raises(ArithmeticError, match="dominant"):
        _build("device", "dominance")
    fom, dev_rom, dev_sols = _build("device", "defect")
    _, host_rom, host_sols = _build("host", "dominance")
    assert sorted(dev_rom.fom_defects) == sorted(dev_sols) == [0, 1, 2] and host_rom.fom_defects == {}
    worst = max(float(v.max()) for v in dev_rom.fom_defects.values())
    print(f"piston sizes: worst defect {worst:.3e} = {worst / dc.omega_ref():.3f} OMEGA_REF")
    assert all(v.shape == (100,) for v in dev_rom.fom_defects.values()) and worst <= F * dc.omega_ref()
    for j in range(3):
        assert dev_sols[j].shape == host_sols[j].shape == (1001, 100)
        print(f"fom_solutions[{j}]: device - host {fc.rel(dev_sols[j], host_sols[j]):.3e}")
        assert fc.rel(dev_sols[j], host_sols[j]) <= 1e-12
    # the device-route basis spans the host snapshots as well as the host-route basis does (the bar of test_fom_gpu.py)
    host, _, _ = fc.host_solutions(fom, PISTON_MUS)
    (_, U), = dfom.fom_sweep(fom, PISTON_MUS, check="defect")
    X = np.hstack([host[j].T for j in range(3)])
    dX = np.linalg.norm(X - np.hstack([U[j].T.cpu().numpy() for j in range(3)]))
    err = lambda V: np.linalg.norm(X - V @ (V.T @ X))
    e_host, e_dev = err(host_rom.basis), err(dev_rom.basis)
    print(f"projection error: host basis {e_host:.6e}, device basis {e_dev:.6e}, |dX|_F {dX:.3e}")
    assert dev_rom.basis.shape == host_rom.basis.shape
    assert e_dev <= e_host + 4.0 * dX


def test_evaluate_takes_the_device_truth_of_a_convective_model(monkeypatch):
    from romtime_amd import fom as dfom
    from romtime_amd import online
    from romtime_amd.conventions import Errors, Stage
    from romtime_amd.rom import _HYPER_SLOTS
    from tests.test_surface import _fully_hyper_reduced_rom

    fom, srom, _ = _fully_hyper_reduced_rom()
    rom = srom.truncate(2)
    for which, slot in _HYPER_SLOTS.items():
        if getattr(srom, slot):
            rom.add_hyper_reductor(getattr(srom, slot), which)
    rom.project_reductors()
    mus = [dict(alpha_0=1e-6, delta=0.3, omega=9.0 + j) for j in range(2)]
    rec = dfom.recipe(fom, mus)
    _, margin, flags = fc.truth(int(fom.nx), rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"])
    assert margin < 0 and flags.all()
    seen = []
    real = dfom.fom_sweep
    monkeypatch.setattr(dfom, "fom_sweep", lambda *a, **kw: (seen.append(kw.get("check")), real(*a, **kw))[1])
    for model in (rom, srom):
        model.mu_space = dict(model.mu_space, **{Stage.ONLINE: []})
    with pytest.raises(ArithmeticError, match="dominant"):
        online.evaluate(rom, srom, mus, Stage.ONLINE)
    for model in (rom, srom):
        model.mu_space = dict(model.mu_space, **{Stage.ONLINE: []})
        model.FOM_CHECK = "defect"
    ev = online.evaluate(rom, srom, mus, Stage.ONLINE)
    assert seen == ["dominance", "defect"] and sorted(ev) == [0, 1]
    (_, U), = real(fom, mus, check="defect")
    for j in range(2):
        curve = ev[j][Errors.ROM]
        print(f"point {j}: ROM error against the certified device truth, max {np.max(curve):.3e}")
        assert curve.shape == (int(fom.domain["nt"]),) and np.isfinite(curve).all()
        assert np.isfinite(U[j].cpu().numpy()).all()
