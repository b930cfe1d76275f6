"""Premises and host side of the certified full-order sweep (rt_p1_fom_bdf_sweep_certified): the convective cases lose
diagonal dominance while the host loop and an unpivoted float64 elimination stay at rounding level, the flag cases are
regular systems that the unpivoted elimination solves badly, the plan twin and its refusals, the ABI, and the value
handling of ``fom.fom_sweep(check=...)`` and ``RomConstructor.FOM_CHECK`` on host stand-ins.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from romtime_amd import _lib
from tests import fom_cases as fc
from tests import fom_defect_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(REPO, *parts)) as fh:
        return fh.read()


# ---- premises ------------------------------------------------------------------------------------------------------------------
def test_convective_cases_lose_dominance_and_nothing_else():
    worst = 0.0
    for name, c in dc.all_conv_cases():
        om = float(c["seq_omega"].max())
        worst = max(worst, om)
        print(f"{name}: margin {c['margin']:.3e} flags {c['flags'].tolist()} d_host {c['d_host']:.3e} sequential omega {om:.3e}")
        if c["nx"] >= 65:
            assert c["margin"] < 0 and c["flags"].all(), name              # today's entry refuses every point
        assert c["d_host"] <= 1e-13 or c["nx"] >= 100_000, name               # mock.solve() at its usual distance
        assert np.isfinite(c["truth"].astype(np.float64)).all()
    big = dc.size_case()
    assert big["d_host"] <= 1e-9                                              # N_h = 1e5: the level test_fom_gpu.py records there
    ref = dc.omega_ref()
    print(f"OMEGA_REF {ref:.3e} = {ref / fc.EPS:.1f} eps")
    assert ref == worst and 0 < ref <= 1e-13


def test_flag_cases_are_regular_and_badly_solved_without_pivoting():
    from scipy.linalg import solve_banded

    for nx in dc.FLAG_NX:
        tab, dt = dc.flag_table(nx)
        _, margin, flags = fc.truth(nx, tab, dt, False, False)
        U, om = dc.sequential_sweep(nx, tab, dt, False, False)
        # the step's rows from the sequential states, solved with partial pivoting: a regular system
        lo, di, up, r = dc.step_rows(nx, tab[1], dt, False, False, U[:, 0], np.zeros_like(U[:, 0]))
        ab = np.zeros((3, nx - 1))
        ab[0, 1:], ab[1], ab[2, :-1] = up[0, :-1], di[0], lo[0, 1:]
        x = np.zeros((1, nx + 1))
        x[0, 1:-1] = solve_banded((1, 1), ab, r[0])
        om_piv = float(dc.omega_of(lo[:1], di[:1], up[:1], r[:1], x)[0])
        print(f"nx {nx}: |d| {np.abs(di[0]).max():.2e} |l|,|u| {np.abs(up[0]).min():.2e}..{np.abs(lo[0]).max():.2e} "
              f"omega unpivoted {om[0, 1]:.3e} pivoted {om_piv:.3e}, others {np.delete(om.ravel(), 1).max():.3e}")
        assert np.isfinite(U).all() and np.isfinite(x).all() and om_piv <= 64 * fc.EPS
        assert om[0, 1] >= 1e-7
        assert np.delete(om.ravel(), 1).max() <= 64 * fc.EPS                  # steps 0 and 2 of point 0, and point 1
        assert flags.tolist() == [2, 0]                                       # dominance is lost there and only there
        # every other (point, step) is strictly dominant
        for s, j in ((0, 0), (2, 0), (0, 1), (1, 1), (2, 1)):
            l, d, u, _ = dc.step_rows(nx, tab[s, j:j + 1], dt, False, False, np.zeros((1, nx + 1)), np.zeros((1, nx + 1)))
            assert (np.abs(d[:, 1:-1]) > np.abs(l[:, 1:-1]) + np.abs(u[:, 1:-1])).all()


def test_defect_of_a_solved_step_and_of_a_wrong_one():
    """omega_of itself: an exactly solvable integer system has defect 0, a perturbed entry of x shows at its size, 0/0
    counts as 0 and a non-finite value as +inf."""
    lo = np.array([[0.0, 1.0, 2.0]])
    di = np.array([[4.0, 4.0, 4.0]])
    up = np.array([[1.0, 1.0, 0.0]])
    x = np.array([[0.0, 1.0, 2.0, 3.0, 0.0]])
    r = np.array([[6.0, 12.0, 16.0]])
    assert dc.omega_of(lo, di, up, r, x)[0] == 0.0
    y = x.copy()
    y[0, 2] *= 1 + 1e-6
    assert 1e-7 < dc.omega_of(lo, di, up, r, y)[0] < 1e-6
    assert dc.omega_of(lo, di, up, 0 * r, 0 * x)[0] == 0.0
    y[0, 2] = np.nan
    assert dc.omega_of(lo, di, up, r, y)[0] == np.inf
    np.testing.assert_allclose(dc.thomas(lo, di, up, r), x[:, 1:-1], rtol=4 * fc.EPS)


# ---- plan twin -----------------------------------------------------------------------------------------------------------------------
def _plans(nx=64, n_mu=2, nt=3, first_step=0, tab=True, u_init=False, ld_step=None, stride_mu=None, num_cus=256):
    lib = _lib.load()
    Nh = nx + 1
    buf = (C.c_double * 7)()
    some = C.cast(buf, C.c_void_p)
    desc = _lib.FomDesc(nx, n_mu, nt, first_step, 0.1, 1, 1, some if tab else None, some if u_init else None)
    ld_step = Nh if ld_step is None else ld_step
    stride_mu = nt * ld_step if stride_mu is None else stride_mu
    info3, info4 = (C.c_int64 * 3)(), (C.c_int64 * 4)()
    rc3 = lib.rt_p1_fom_bdf_sweep_plan_info(num_cus, C.byref(desc), ld_step, stride_mu, info3)
    rc4 = lib.rt_p1_fom_bdf_sweep_certified_plan_info(num_cus, C.byref(desc), ld_step, stride_mu, info4)
    return rc3, [int(v) for v in info3], rc4, [int(v) for v in info4]


def test_certified_plan_is_the_plan_plus_the_scratch_the_header_states():
    header = _read("include", "romtime_hip.h")
    m = re.search(r"(\d+) KiB x ceil\(\(nx-1\)/1024\) per point of ctx leaf arena \(six arrays", header)
    assert m, "the header states the certified entry's scratch size"
    kib = int(m.group(1))
    assert kib == 6 * 1024 * 8 // 1024
    P = fc.partitions()
    for n in fc.row_counts(P) + [64, 999, 4 * P + 7, 99_999]:
        rc3, i3, rc4, i4 = _plans(nx=n + 1, n_mu=5)
        assert rc3 == rc4 == 0 and i4[:3] == i3
        assert i4[3] == kib * 1024 * -(-n // 1024)
    from romtime_amd import ops

    assert ops.p1_fom_plan_info_certified(2050, n_mu=3)[:3] == ops.p1_fom_plan(2050, n_mu=3)
    assert ops.p1_fom_plan_info_certified(2050)[3] == 3 * kib * 1024


def test_certified_plan_refuses_what_the_plan_refuses():
    lib = _lib.load()
    assert lib.rt_p1_fom_bdf_sweep_certified_plan_info(256, None, 65, 195, None) == -1
    m = re.search(r"nx <= 2\^(\d+)", _read("include", "romtime_hip.h"))
    limit = 1 << int(m.group(1))
    cases = [dict(), dict(num_cus=0), dict(tab=False), dict(nx=1), dict(n_mu=0), dict(nt=0), dict(first_step=-1),
             dict(first_step=2), dict(first_step=2, u_init=True), dict(ld_step=64), dict(stride_mu=2 * 65 + 64),
             dict(stride_mu=2 * 65 + 65), dict(ld_step=70, stride_mu=2 * 70 + 65), dict(ld_step=2 * 65, stride_mu=65),
             dict(n_mu=1, stride_mu=0), dict(nx=2), dict(nx=1 << 20), dict(nx=limit, n_mu=1), dict(nx=limit + 1, n_mu=1),
             dict(nx=limit, n_mu=1 << 20)]
    seen = set()
    for kw in cases:
        rc3, _, rc4, _ = _plans(**kw)
        assert rc3 == rc4, kw
        seen.add(rc4)
    assert seen == {0, -1, -3}
    # six arrays per point reach the 64 GiB limit of the arena before five do
    n_mu = (1 << 36) // (6 * 4096 * 1024 * 8) + 1
    rc3, _, rc4, _ = _plans(nx=limit, n_mu=n_mu)
    assert (rc3, rc4) == (0, -3)


def test_abi_entries():
    header = _read("include", "romtime_hip.h")
    assert "int rt_p1_fom_bdf_sweep_certified(rt_ctx* ctx, const rt_fom_desc* desc, double* U_out" in header
    assert "int rt_p1_fom_bdf_sweep_certified_plan_info(int num_cus" in header and "since version\n * 410" in header
    for name in ("rt_p1_fom_bdf_sweep_certified", "rt_p1_fom_bdf_sweep_certified_plan_info"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.SIGNATURES["rt_p1_fom_bdf_sweep_certified"][1][5] is C.c_double
    assert [f for f, _ in _lib.FomDesc._fields_] == ["nx", "n_mu", "nt", "first_step", "dt", "bdf2", "state_in_w", "tab", "u_init"]
    assert _lib.load().rt_version() >= 410
    assert int(re.search(r"int rt_version\(void\) \{ return (\d+); \}", _read("romtime_amd", "csrc", "api.hip")).group(1)) >= 410


# ---- fom_sweep(check=...) and FOM_CHECK on host stand-ins ----------------------------------------------------------------------------
def stub_certified(nx, tab, dt, bdf2, state_in_w, u_init=None, first_step=0, defect_tol=1e-10):
    """The certified entry on the host: the float64 sequential sweep of fom_cases.truth and every step's defect."""
    import torch

    tab = tab.numpy() if isinstance(tab, torch.Tensor) else np.asarray(tab)
    ui = None if u_init is None else (u_init.numpy() if isinstance(u_init, torch.Tensor) else np.asarray(u_init))
    U, _, _ = fc.truth(nx, tab, dt, bdf2, state_in_w, dtype=np.float64, u_init=ui, first_step=first_step)
    om = dc.step_defects(nx, tab, dt, bdf2, state_in_w, U, u_init=ui, first_step=first_step)
    bad = ~(om <= defect_tol)
    info = np.where(bad.any(axis=1), 1 + first_step + bad.argmax(axis=1), 0).astype(np.int32)
    return torch.from_numpy(U), torch.from_numpy(info), torch.from_numpy(om)


@pytest.fixture
def fom_ops(cpu_ops, monkeypatch):
    from romtime_amd import ops

    fc.install_stubs(monkeypatch)
    monkeypatch.setattr(ops, "p1_fom_bdf_sweep_certified", stub_certified)
    return cpu_ops


def test_fom_sweep_check_values(fom_ops):
    from romtime_amd import fom as dfom

    c = dc.conv_case(65, True)
    with pytest.raises(ValueError, match="check"):
        list(dfom.fom_sweep(c["fom"], c["mus"], check="pivot"))
    with pytest.raises(ValueError, match="defect_tol"):
        list(dfom.fom_sweep(c["fom"], c["mus"], check="defect", defect_tol=-1.0))
    with pytest.raises(ValueError, match="defect_tol"):
        list(dfom.fom_sweep(c["fom"], c["mus"], check="defect", defect_tol=float("nan")))
    with pytest.raises(ArithmeticError, match="dominant"):                    # the default is today's route
        list(dfom.fom_sweep(c["fom"], c["mus"]))
    report = {}
    (first, U), = dfom.fom_sweep(c["fom"], c["mus"], check="defect", report=report)
    assert first == 0 and fc.rel(U.numpy(), c["truth"]) <= fc.bar(c["d_host"])
    assert report["defect"].shape == (3, dc.NT) and report["defect"].max() <= 64 * fc.EPS
    chunked = {}
    blocks = list(dfom.fom_sweep(c["fom"], c["mus"], chunk=5, check="defect", report=chunked))
    assert [b[0] for b in blocks] == [0, 5, 10]
    np.testing.assert_array_equal(np.concatenate([b[1].numpy() for b in blocks], axis=1), U.numpy())
    np.testing.assert_array_equal(chunked["defect"], report["defect"])


def test_fom_sweep_defect_error_names_mu_step_and_defect(fom_ops):
    from romtime_amd import fom as dfom

    c = dc.conv_case(65, False)
    seen = {}
    list(dfom.fom_sweep(c["fom"], c["mus"], check="defect", report=seen))
    tol = float(np.median(seen["defect"]))
    over = seen["defect"] > tol
    j = int(np.flatnonzero(over.any(axis=1))[0])
    s = int(over[j].argmax())
    with pytest.raises(ArithmeticError) as err:
        list(dfom.fom_sweep(c["fom"], c["mus"], check="defect", defect_tol=tol))
    msg = str(err.value)
    assert str(c["mus"][j]) in msg and f"step {s}" in msg and f"{seen['defect'][j, s]:.3e}" in msg and "defect" in msg


def _rom(fom, check):
    from romtime_amd.rom import RomConstructor

    rom = RomConstructor(fom=fom, grid={k: [v] for k, v in dc.CONV_MUS[0].items()})
    rom.SNAPSHOTS_ON = "device"
    rom.FOM_CHECK = check
    rom.setup(rnd=0)
    return rom


def test_fom_check_of_the_constructor(fom_ops):
    from romtime_amd.rom import RomConstructor

    assert RomConstructor.FOM_CHECK == "dominance"
    mus = [dict(mu) for mu in dc.CONV_MUS]
    with pytest.raises(ValueError, match="FOM_CHECK"):
        _rom(dc.make_fom(65, dc.NT, True), "pivot").build_reduced_basis(mu_space=mus, num_basis=4)
    with pytest.raises(ArithmeticError, match="dominant"):
        _rom(dc.make_fom(65, dc.NT, True), "dominance").build_reduced_basis(mu_space=mus, num_basis=4)
    rom = _rom(dc.make_fom(65, dc.NT, True), "defect")
    sols = rom.build_reduced_basis(mu_space=mus, num_basis=4)
    assert sorted(sols) == sorted(rom.fom_defects) == [0, 1, 2]
    for k in sols:
        assert sols[k].shape == (66, dc.NT) and rom.fom_defects[k].shape == (dc.NT,)
        assert rom.fom_defects[k].max() <= 64 * fc.EPS
    assert rom.truncate(1).FOM_CHECK == "defect"
    plain = _rom(dc.make_fom(65, dc.NT, True), "dominance")
    assert plain.fom_defects == {}
