"""rt_trajectory_residuals on the device (cases, truth and bars: tests/residual_cases.py).  Operands sit inside quiet NaNs
(the padding of every line, the rows between two trajectories, guard lines around), ``res`` and ``scale`` behind canaries.

1. the FOM's own trajectory (V = I, a = U of the certified sweep): res <= defect scale (1 + 4 N_h eps) step by step - the
   rows and the residual chain are the sweep's own - and res / scale <= DEFECT_TOL;
2. rows, 3. steps and flags, 4. k and strides, 6. size: ``dist(res)`` and ``dist(scale)`` from the long-double truth within
   ``8 d_np + 64 eps``; 5. determinism: batch place, CU count, horizon cut; 7. the classes.

Every test prints its figures before it asserts.  Measured on the MI355X over items 2 to 6: worst dist 4.4e-16 (2 eps),
worst dist / d_np 2.0 over the figures with d_np >= eps / 4; where NumPy's float64 value happens to be the truth's own
(d_np = 0, or 1.5e-17 in the two-row heat case) the device is half an ulp to two ulps away and the ratio says nothing
("Residuals of lifted trajectories").  The bar is the project's 8 d_np + 64 eps throughout."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import fom_cases as fc
from tests import fom_defect_cases as dc
from tests import guarded
from tests import residual_cases as rc

pytestmark = pytest.mark.gpu

GAP = 3                                     # NaN rows between two trajectories of A: stride_a = (nt + GAP) lda


def residuals(c, ldb_pad=0, lda_pad=0, want_scale=True, expect=0):
    """The C entry on guarded buffers for a case dict (nx, tab, dt, bdf2, state_in_w, V, a, a_init, first_step); (res,
    scale) as host arrays, every guard checked.  ``expect``: the return code the call must give (then None)."""
    from romtime_amd import _lib
    from romtime_amd._lib import Context

    nx, V, a = c["nx"], np.asarray(c["V"], dtype=np.float64), np.asarray(c["a"], dtype=np.float64)
    tab = np.ascontiguousarray(np.asarray(c["tab"], dtype=np.float64))
    n, nt, k = a.shape
    assert tab.shape == (nt, n, 7) and V.shape == (nx + 1, k)
    tab_host = tab.reshape(nt, n * 7)
    tab_d = guarded.guarded_operand(tab_host, misalign=True)
    V_d = guarded.guarded_operand(V, ld_pad=ldb_pad, misalign=bool(ldb_pad & 1))
    a_host = np.full((n, nt + GAP, k), np.nan)
    a_host[:, :nt] = a
    a_host = a_host.reshape(n * (nt + GAP), k)
    a_d = guarded.guarded_operand(a_host, ld_pad=lda_pad)
    init_host, init_d = None, None
    if c.get("a_init") is not None:
        init_host = np.ascontiguousarray(np.asarray(c["a_init"], dtype=np.float64)).reshape(n * 2, k)
        init_d = guarded.guarded_operand(init_host, guard=4, misalign=True)
    res, scale = guarded.guarded_output((n, nt)), guarded.guarded_output((n, nt), misalign=True)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ctx = Context.current()
    desc = _lib.FomDesc(nx, n, nt, int(c.get("first_step", 0)), float(c["dt"]), int(c["bdf2"]), int(c["state_in_w"]), P(tab_d), None)
    code = ctx.lib.rt_trajectory_residuals(ctx.handle, C.byref(desc), P(V_d), k + ldb_pad, k, P(a_d), k + lda_pad,
                                           (nt + GAP) * (k + lda_pad), P(init_d), P(res.t), P(scale.t) if want_scale else None)
    torch.cuda.synchronize()
    assert guarded.operand_intact(tab_d, tab_host) == [] and guarded.operand_intact(V_d, V) == []
    assert guarded.operand_intact(a_d, a_host) == []
    if init_d is not None:
        assert guarded.operand_intact(init_d, init_host) == []
    if expect != 0:
        assert code == expect, code
        for out in (res, scale):
            assert (guarded._as_bits(out.buf) == guarded.CANARY_BITS).all()
        return None
    ctx.check(code, "rt_trajectory_residuals")
    assert res.check() == [], res.check()
    if want_scale:
        assert scale.check() == [], scale.check()
    else:
        assert (guarded._as_bits(scale.buf) == guarded.CANARY_BITS).all()
    return res.t.cpu().numpy(), (scale.t.cpu().numpy() if want_scale else None)


def held_to_truth(name, c, got):
    """Prints the figures, then holds res and scale to the bar of the case."""
    res, scale = got
    d_res, d_scale = float(rc.dist(res, c["res"], c["scale"]).max()), float(rc.dist(scale, c["scale"], c["scale"]).max())
    ratio = lambda d, d_np: d / d_np if d_np > 0 else (0.0 if d == 0 else np.inf)
    print(f"{name}: res d_np {c['d_np_res']:.3e} dist {d_res:.3e} ratio {ratio(d_res, c['d_np_res']):.3f} bar {rc.bar(c['d_np_res']):.3e}; "
          f"scale d_np {c['d_np_scale']:.3e} dist {d_scale:.3e} ratio {ratio(d_scale, c['d_np_scale']):.3f} bar {rc.bar(c['d_np_scale']):.3e}; "
          f"res/scale {float(np.min(res / scale)):.3e} .. {float(np.max(res / scale)):.3e}")
    assert np.isfinite(res).all() and np.isfinite(scale).all()                  # no NaN from the basis' boundary rows
    assert d_res <= rc.bar(c["d_np_res"]) and d_scale <= rc.bar(c["d_np_scale"])


# ---- 1. the FOM's own trajectory ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["burgers", "heat"])
@pytest.mark.parametrize("nx", rc.OWN_NX)
def test_own_trajectory(kind, nx):
    from romtime_amd import ops

    fom = fc.make_fom(kind, nx, rc.OWN_NT)
    rec = fc.recipe(fom, fc.mus_of(kind, 3))
    U, info, defect = ops.p1_fom_bdf_sweep_certified(nx, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"])
    U, defect = U.cpu().numpy(), defect.cpu().numpy()
    c = dict(nx=nx, tab=rec["tab"], dt=fom.dt, bdf2=rec["bdf2"], state_in_w=rec["state_in_w"], V=np.eye(nx + 1), a=U)
    res, scale = residuals(c)
    bound = rc.own_bound(defect, scale, nx + 1)
    print(f"{kind} nx {nx}: worst defect {defect.max():.3e}, worst res/scale {np.max(res / scale):.3e}, "
          f"worst res / (defect scale) {np.max(res / np.where(defect > 0, defect * scale, 1.0)):.4f}")
    assert not info.cpu().numpy().any() and np.all(scale > 0)
    assert np.all(res <= bound), (res - bound).max()
    assert np.max(res / scale) <= dc.DEFECT_TOL


# ---- 2. truth, rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", rc.row_case_keys(), ids=lambda k: f"{k[0]}-n{k[1] - 1}")
def test_rows(key):
    c = rc.case(*key)
    held_to_truth(f"rows {key[0]} n = {key[1] - 1}", c, residuals(c))


# ---- 3. truth, steps and flags -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_run(key):
    return residuals(rc.case(*key))


@pytest.mark.parametrize("key", rc.step_case_keys(), ids=lambda k: f"nt{k[2]}-bdf{2 if k[5][0] else 1}-state{int(k[5][1])}")
def test_steps_and_flags(key):
    held_to_truth(f"steps nt = {key[2]} flags {key[5]}", rc.case(*key), step_run(key))


# ---- 4. truth, k and strides ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pads", [(0, 0), (1, 1), (3, 3), (1, 0), (0, 3)], ids=str)
@pytest.mark.parametrize("key", rc.k_case_keys(), ids=lambda k: f"k{k[3]}")
def test_k_and_strides(key, pads):
    c = rc.case(*key)
    got = residuals(c, ldb_pad=pads[0], lda_pad=pads[1])
    held_to_truth(f"k = {key[3]} pads {pads}", c, got)
    if pads != (0, 0):                                                              # strides and alignment do not change a bit
        plain = residuals(c)
        assert guarded.bits_equal(got[0], plain[0]) and guarded.bits_equal(got[1], plain[1])


def test_scale_may_be_absent():
    c = rc.case(*rc.k_case_keys()[3])
    res, none = residuals(c, want_scale=False)
    assert none is None and guarded.bits_equal(res, residuals(c)[0])


def test_refusals_leave_the_outputs_alone():
    rng = np.random.default_rng(5)
    c = dict(rc.case("burgers", rc.K_NX, 5, 128, 2, None, True))
    c["V"] = np.hstack([c["V"], rng.standard_normal((rc.K_NX + 1, 1))])
    c["a"] = np.concatenate([c["a"], rng.standard_normal((2, 5, 1))], axis=2)
    c["a_init"] = np.concatenate([c["a_init"], rng.standard_normal((2, 2, 1))], axis=2)
    assert residuals(c, expect=-3) is None                                          # k = 129
    d = dict(rc.case(*rc.k_case_keys()[3]))
    d["a_init"] = None                                                              # first_step = 7 without older states
    assert residuals(d, expect=-1) is None


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------------
DET_KEY = ("burgers", rc.STEP_NX, 130, 6, 3, (True, True))


def _single(c, j):
    return dict(c, tab=c["tab"][:, j:j + 1], a=c["a"][j:j + 1])


def test_batch_place():
    c, (res, scale) = rc.case(*DET_KEY), step_run(DET_KEY)
    alone = residuals(_single(c, 1))
    assert guarded.bits_equal(alone[0][0], res[1]) and guarded.bits_equal(alone[1][0], scale[1])
    for place in (0, 4):
        order = [1, 0, 2, 0, 2] if place == 0 else [0, 2, 0, 2, 1]
        batch = dict(c, tab=c["tab"][:, order], a=c["a"][order])
        r5, s5 = residuals(batch)
        assert guarded.bits_equal(r5[place], res[1]) and guarded.bits_equal(s5[place], scale[1]), place


def test_horizon_cut():
    """130 steps in one call and in calls of 64 + 1 + 65 steps through a_init / first_step."""
    c, (res, scale) = rc.case(*DET_KEY), step_run(DET_KEY)
    first, a_init = 0, None
    for steps in (64, 1, 65):
        part = dict(c, tab=c["tab"][first:first + steps], a=c["a"][:, first:first + steps], a_init=a_init, first_step=first)
        r, s = residuals(part)
        assert guarded.bits_equal(r, res[:, first:first + steps]), (first, guarded.mismatch(r, res[:, first:first + steps]))
        assert guarded.bits_equal(s, scale[:, first:first + steps]), first
        first += steps
        a_init = np.stack([c["a"][:, first - 1], c["a"][:, first - 2] if first >= 2 else 0 * c["a"][:, 0]], axis=1)
    assert first == 130


@functools.lru_cache(maxsize=None)
def size_run():
    return residuals(rc.case(*rc.SIZE_KEY))


def test_cu_limited_ctx():
    """A ctx confined to 64 CUs where the plan reports the same slicing: the same bits (through ops.trajectory_residuals)."""
    from romtime_amd import _lib, ops

    c, (res, scale) = rc.case(*rc.SIZE_KEY), size_run()
    full, masked_plan = rc.plan(c["nx"], c["k"], c["nt"], 2, 256), rc.plan(c["nx"], c["k"], c["nt"], 2, 64)
    print(f"plan on 256 CUs {full}, on 64 CUs {masked_plan}")
    assert full == masked_plan and full[1] > 1
    V = np.nan_to_num(c["V"], nan=7.0)                                             # the boundary rows are not looked at
    Vd, ad, tabd = ops.to_device(V), ops.to_device(c["a"]), ops.to_device(c["tab"])
    args = (c["nx"], tabd, c["dt"], c["bdf2"], c["state_in_w"])
    r0, s0 = ops.trajectory_residuals(Vd, ad, *args)
    assert guarded.bits_equal(r0.cpu().numpy(), res) and guarded.bits_equal(s0.cpu().numpy(), scale)
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rt_stream_create_cu_range(0, 0, 8, C.byref(h)) == 0 and h.value
    masked = _lib.Context(0)
    masked.set_option("cu_limit", 64)
    st = torch.cuda.ExternalStream(h.value)
    torch.cuda.synchronize()
    with masked.use(st):
        r1, s1 = ops.trajectory_residuals(Vd, ad, *args)
        info = masked.launch_info()
    st.synchronize()
    masked.set_option("cu_limit", 0)
    # (this stream stays: torch's allocator remembers the stream of every block handed out under it)
    assert (info["grid"], info["splits"]) == full[:2]
    assert guarded.bits_equal(r1.cpu().numpy(), res) and guarded.bits_equal(s1.cpu().numpy(), scale)


# ---- 6. size ---------------------------------------------------------------------------------------------------------------------------
def test_size():
    c = rc.case(*rc.SIZE_KEY)
    slices = rc.plan(c["nx"], c["k"], c["nt"], 2)[1]
    print(f"size: N_h {c['nx'] + 1}, {slices} slices per trajectory")
    assert slices >= 4
    held_to_truth("size", c, size_run())


# ---- 7. the classes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hyper_reduced_pair():
    """MockBurgers at nx = 200, nt = 24 with an (M)DEIM on every operator (the recipe of
    tests.test_surface._fully_hyper_reduced_rom at these sizes): the S-ROM with r = 8 and the ROM two modes short."""
    from scipy.stats.distributions import uniform

    from romtime_amd import (DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation,
                             MatrixDiscreteEmpiricalInterpolationNonlinear, RomConstructorNonlinear)
    from romtime_amd.conventions import OperatorType, RomParameters
    from romtime_amd.rom import _HYPER_SLOTS
    from tests.test_surface import _burgers

    fom = _burgers(True, nx=200, nt=24)
    mus = [dict(alpha_0=0.05 + 0.02 * i, delta=0.3, omega=9.0 + i) for i in range(3)]
    full = RomConstructorNonlinear(fom=fom, grid=None, name="srom")
    full.setup(rnd=0)
    full.build_reduced_basis(mu_space=mus, tolerances={RomParameters.TOL_TIME: None, RomParameters.TOL_MU: None})
    srom = full.truncate(full.N - 8) if full.N > 8 else full
    assert srom.N == 8
    grid = dict(alpha_0=uniform(0.04, 0.08), delta=uniform(0.29, 0.02), omega=uniform(8.5, 3.0))
    tw = {"ts": np.linspace(0.01, 0.5, 8), "num_snapshots": 4}
    rnd = lambda: np.random.RandomState(1)
    ops_m = dict(mass=(fom.assemble_mass, OperatorType.MASS), stiffness=(fom.assemble_stiffness, OperatorType.STIFFNESS),
                 convection=(fom.assemble_convection, OperatorType.CONVECTION),
                 nonlinear_lifting=(fom.assemble_nonlinear_lifting, OperatorType.NONLINEAR_LIFTING))
    for name, (assemble, which) in ops_m.items():
        md = MatrixDiscreteEmpiricalInterpolation(name=name, assemble=assemble, grid=grid, tree_walk_params=tw)
        md.setup(rnd=rnd())
        md.run()
        srom.add_hyper_reductor(md, which)
    nm = MatrixDiscreteEmpiricalInterpolationNonlinear(name="trilinear", assemble=fom.assemble_trilinear, grid=grid, tree_walk_params=tw)
    nm.setup(rnd=rnd(), u_n=np.linspace(0.0, 1.0, fom.Nh))
    nm.run(u_n=srom.basis)
    srom.add_hyper_reductor(nm, OperatorType.TRILINEAR)
    dl = DiscreteEmpiricalInterpolation(name="lifting", assemble=fom.assemble_lifting, grid=grid, tree_walk_params=tw)
    dl.setup(rnd=rnd())
    dl.run()
    srom.add_hyper_reductor(dl, OperatorType.LIFTING)
    srom.project_reductors()
    rom = srom.truncate(2)
    for which, slot in _HYPER_SLOTS.items():
        if getattr(srom, slot):
            rom.add_hyper_reductor(getattr(srom, slot), which)
    rom.project_reductors()
    for model in (rom, srom):
        model.ONLINE_ON = "device"
    return fom, rom, srom, mus


def _fresh(*models):
    from romtime_amd.conventions import Stage

    for model in models:
        model.mu_space = dict(model.mu_space, **{Stage.ONLINE: []})


def test_classes(monkeypatch):
    from romtime_amd import certify, online
    from romtime_amd import fom as dfom
    from romtime_amd.conventions import Errors, ProblemType, Stage

    fom, rom, srom, mus = hyper_reduced_pair()
    assert (int(fom.nx), int(fom.domain["nt"]), srom.N, rom.N) == (200, 24, 8, 6)
    # online.residuals = solve_many + certify.trajectory_residuals on its uN, bit for bit, and no full-order solve
    seen = []
    real = srom.solve_many
    monkeypatch.setattr(srom, "solve_many", lambda *a, **kw: (seen.append(real(*a, **kw)), seen[-1])[1], raising=False)
    monkeypatch.setattr(dfom, "fom_sweep", lambda *a, **kw: pytest.fail("a full-order sweep was made"))
    monkeypatch.setattr(fom, "solve", lambda *a, **kw: pytest.fail("a full-order solve was made"))
    _fresh(srom)
    curves = online.residuals(srom, mus, Stage.ONLINE)
    sol, = seen
    assert sorted(curves) == sol.idx == [0, 1, 2] and tuple(sol.uN.shape) == (3, 24, 8)
    by_hand = certify.trajectory_residuals(fom, sol._V, sol.uN, mus)
    chunked = certify.trajectory_residuals(fom, sol._V, sol.uN, mus, chunk=7)
    for j in range(3):
        assert curves[j].shape == (24,) and guarded.bits_equal(curves[j], by_hand[j]) and guarded.bits_equal(chunked[j], by_hand[j])
    # ... within the bar of the truth
    rec = dfom.recipe(fom, mus)
    c = dict(nx=200, tab=rec["tab"], dt=fom.dt, bdf2=rec["bdf2"], state_in_w=rec["state_in_w"], V=sol._V.cpu().numpy(),
             a=sol.uN.cpu().numpy())
    c.update(rc.reference(c))
    res, scale = certify.trajectory_residuals(fom, sol._V, sol.uN, mus, relative=False)
    held_to_truth("classes, S-ROM r = 8", c, (res, scale))
    assert guarded.bits_equal(res / scale, by_hand)
    monkeypatch.undo()
    # evaluate(residuals=True) carries the same curves, and every other payload is that of the default call
    _fresh(rom, srom)
    base = online.evaluate(rom, srom, mus, Stage.ONLINE)
    _fresh(rom, srom)
    ev = online.evaluate(rom, srom, mus, Stage.ONLINE, residuals=True)
    assert base.residuals == {} and sorted(ev.residuals) == sorted(ev) == sorted(base) == [0, 1, 2]
    assert base.mass == ev.mass == {} and base.probes == ev.probes == {}
    rom_uN = torch.cat([s.uN for s in ev.solutions[ProblemType.ROM]])
    rom_curves = certify.trajectory_residuals(fom, rom._V(), rom_uN, mus)
    for j in range(3):
        assert set(ev[j]) == set(base[j]) == {Errors.ESTIMATOR, Errors.ROM, Errors.SACRIFICIAL}
        for key in ev[j]:
            assert guarded.bits_equal(ev[j][key], base[j][key]), (j, key)
        assert set(ev.residuals[j]) == {ProblemType.ROM, ProblemType.SROM}
        assert guarded.bits_equal(ev.residuals[j][ProblemType.SROM], curves[j])
        assert guarded.bits_equal(ev.residuals[j][ProblemType.ROM], rom_curves[j])
        with np.printoptions(precision=3, linewidth=200):
            print(f"point {j}: residual ROM (r = 6)  {ev.residuals[j][ProblemType.ROM]}")
            print(f"point {j}: error    ROM          {ev[j][Errors.ROM]}")
            print(f"point {j}: residual S-ROM (r = 8) {ev.residuals[j][ProblemType.SROM]}")
            print(f"point {j}: error    S-ROM         {ev[j][Errors.SACRIFICIAL]}")
