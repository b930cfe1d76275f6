"""Host side of the full-order sweep (rt_p1_fom_bdf_sweep): the recipe against ``mock.solve()``, strict dominance of every
GPU case, the plan query's checks, the ABI, and the Python layer (romtime_amd.fom, RomConstructor.SNAPSHOTS_ON) on host
stand-ins.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from romtime_amd import _lib
from tests import fom_cases as fc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(REPO, *parts)) as fh:
        return fh.read()


# ---- the recipe is the host loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bdf2,moving", [("burgers", True, True), ("burgers", True, False), ("burgers", False, True),
                                              ("burgers", False, False), ("heat", False, True), ("heat", False, False)])
def test_recipe_in_extended_precision_equals_mock_solve(kind, bdf2, moving):
    fom = fc.make_fom(kind, 40, 24, bdf2=bdf2, moving=moving)
    mus = fc.mus_of(kind, 3)
    rec = fc.recipe(fom, mus)
    assert rec["tab"].shape == (24, 3, 7) and rec["lift"].shape == (24, 3, 2)
    assert rec["bdf2"] == (kind == "burgers" and bdf2) and rec["state_in_w"] == (kind == "burgers")
    T, margin, info = fc.truth(40, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"])
    host, host_full, _ = fc.host_solutions(fom, mus)
    d = fc.rel(host, T)
    print(f"{kind} bdf2={bdf2} moving={moving}: host-truth {d:.3e}, dominance margin {margin:.3e}")
    assert d <= 1e-13
    assert margin > 0 and not info.any()
    # the lifting ramp of the recipe is the lifting function on the moved mesh
    ramp = np.arange(41) / 40.0
    lifted = T.astype(np.float64) + rec["lift"].transpose(1, 0, 2)[:, :, 0:1] + rec["lift"].transpose(1, 0, 2)[:, :, 1:2] * ramp
    assert fc.rel(lifted, host_full) <= 1e-13


def test_every_gpu_case_is_strictly_diagonally_dominant():
    keys = fc.row_case_keys() + fc.step_case_keys() + [("burgers", 64, 3, True, 3, None), ("heat", 64, 3, True, 3, None),
                                                         ("burgers", 200, 40, True, 3, None), ("heat", 200, 40, True, 3, None)]
    for key in keys:
        c = fc.case(*key)
        assert c["margin"] > 0 and not c["info"].any(), key
    # the rows of the size case (nx = 1e5) at their first step, where the state is zero: the later steps are held to
    # info = 0 on the device and to margin > 0 of the truth in test_fom_gpu.py
    for kind, nx, nt, bdf2, n_mu, _ in fc.size_case_keys():
        fom = fc.make_fom(kind, nx, 1, bdf2=bdf2)
        rec = fc.recipe(fom, fc.mus_of(kind, n_mu))
        tab = rec["tab"][0]
        h, alpha, c0, c1 = (tab[:, q][:, None] for q in range(4))
        w = c0 + c1 * (np.arange(nx + 1) / nx)[None, :]
        a, b = (2 * w[:, :-1] + w[:, 1:]) / 6, (w[:, :-1] + 2 * w[:, 1:]) / 6
        lo = h / 6 + fom.dt * (-alpha / h - b[:, :-1])
        di = 4 * h / 6 + fom.dt * (2 * alpha / h + b[:, :-1] - a[:, 1:])
        up = h / 6 + fom.dt * (-alpha / h + a[:, 1:])
        assert (np.abs(di) > np.abs(lo) + np.abs(up)).all()


def test_flag_case_loses_dominance_at_one_step_of_one_point_only():
    fom, mus, rec = fc.flag_table(64, 4, bad_step=2)
    _, _, info = fc.truth(64, rec["tab"], fom.dt, False, False)
    assert info.tolist() == [0, 3, 0]


# ---- plan query ------------------------------------------------------------------------------------------------------------
def _plan(nx=64, n_mu=2, nt=3, first_step=0, tab=True, u_init=False, ld_step=None, stride_mu=None, num_cus=256):
    lib = _lib.load()
    Nh = nx + 1
    buf = (C.c_double * 7)()
    some = C.cast(buf, C.c_void_p)
    desc = _lib.FomDesc(nx, n_mu, nt, first_step, 0.1, 1, 1, some if tab else None, some if u_init else None)
    ld_step = Nh if ld_step is None else ld_step
    stride_mu = nt * ld_step if stride_mu is None else stride_mu
    info3 = (C.c_int64 * 3)()
    rc = lib.rt_p1_fom_bdf_sweep_plan_info(num_cus, C.byref(desc), ld_step, stride_mu, info3)
    return rc, [int(v) for v in info3]


def test_plan_info_argument_checks():
    lib = _lib.load()
    assert _plan()[0] == 0
    assert lib.rt_p1_fom_bdf_sweep_plan_info(256, None, 65, 195, None) == -1
    assert _plan(num_cus=0)[0] == -1
    assert _plan(tab=False)[0] == -1
    assert _plan(nx=1)[0] == -1
    assert _plan(n_mu=0)[0] == -1
    assert _plan(nt=0)[0] == -1
    assert _plan(first_step=-1)[0] == -1
    assert _plan(first_step=2)[0] == -1                       # no initial states for a sweep that does not start at 0
    assert _plan(first_step=2, u_init=True)[0] == 0
    assert _plan(ld_step=64)[0] == -1                         # ld_step < N_h
    assert _plan(stride_mu=2 * 65 + 64)[0] == -1              # trajectories overlap
    assert _plan(stride_mu=2 * 65 + 65)[0] == 0
    assert _plan(ld_step=70, stride_mu=2 * 70 + 65)[0] == 0   # padded steps
    assert _plan(ld_step=2 * 65, stride_mu=65)[0] == -1       # interleaved trajectories are not taken
    assert _plan(n_mu=1, stride_mu=0)[0] == 0                 # one trajectory: its stride is not used
    assert _plan(nx=2)[0] == 0 and _plan(nx=1 << 20)[0] == 0  # the smallest system, and the size the header promises
    m = re.search(r"nx <= 2\^(\d+)", _read("include", "romtime_hip.h"))
    limit = 1 << int(m.group(1))
    assert limit >= 1 << 20
    assert _plan(nx=limit, n_mu=1)[0] == 0
    assert _plan(nx=limit + 1, n_mu=1)[0] == -3
    assert _plan(nx=limit, n_mu=1 << 20)[0] == -3             # states and factors beyond the arena's limit


def test_plan_info_partitions():
    P = fc.partitions()
    assert P >= 64
    for n in fc.row_counts(P) + [4 * P + 7, 99_999]:
        rc, (groups, parts, rows) = _plan(nx=n + 1, n_mu=5)
        assert rc == 0 and groups == 5
        assert rows == -(-n // P) and parts == -(-n // rows) and parts <= P and (parts - 1) * rows < n <= parts * rows
    # the plan does not depend on the batch, the horizon or the CU count
    assert _plan(nx=5000, n_mu=1, nt=1, num_cus=8)[1][1:] == _plan(nx=5000, n_mu=77, nt=500)[1][1:]


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_entries():
    header = _read("include", "romtime_hip.h")
    assert "int rt_p1_fom_bdf_sweep(rt_ctx*" in header and "int rt_p1_fom_bdf_sweep_plan_info(int num_cus" in header
    assert "} rt_fom_desc;" in header and "since version 390" in header
    for name in ("rt_p1_fom_bdf_sweep", "rt_p1_fom_bdf_sweep_plan_info"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert [f for f, _ in _lib.FomDesc._fields_] == ["nx", "n_mu", "nt", "first_step", "dt", "bdf2", "state_in_w", "tab", "u_init"]
    assert _lib.load().rt_version() >= 390
    assert int(re.search(r"int rt_version\(void\) \{ return (\d+); \}", _read("romtime_amd", "csrc", "api.hip")).group(1)) >= 390
    from romtime_amd import build

    assert "p1_fom.hip" in build.SOURCES


# ---- romtime_amd.fom on host stand-ins -------------------------------------------------------------------------------------
@pytest.fixture
def fom_ops(cpu_ops, monkeypatch):
    fc.install_stubs(monkeypatch)
    return cpu_ops


@pytest.mark.parametrize("kind", ["burgers", "heat"])
def test_fom_sweep_chunks_carry_the_two_last_states(fom_ops, kind):
    from romtime_amd import fom as dfom

    c = fc.case(kind, 40, 9, True, 3)
    (first, whole), = dfom.fom_sweep(c["fom"], c["mus"])
    assert first == 0 and tuple(whole.shape) == (3, 9, 41)
    assert fc.rel(whole.numpy(), c["truth"]) <= 1e-13
    for chunk in (1, 2, 4, 9, 50):
        blocks = list(dfom.fom_sweep(c["fom"], c["mus"], chunk=chunk))
        assert [b[0] for b in blocks] == list(range(0, 9, min(chunk, 9)))
        np.testing.assert_array_equal(np.concatenate([b[1].numpy() for b in blocks], axis=1), whole.numpy())
    with pytest.raises(ValueError, match="chunk"):
        list(dfom.fom_sweep(c["fom"], c["mus"], chunk=0))
    full = dfom.full_solution(whole, c["rec"]["lift"]).numpy()
    assert fc.rel(full, c["host_full"]) <= 1e-13


def test_fom_sweep_raises_for_a_flagged_point(fom_ops):
    from romtime_amd import fom as dfom

    fom, mus, rec = fc.flag_table(64, 4, bad_step=2)
    with pytest.raises(ArithmeticError) as err:
        list(dfom.fom_sweep(fom, mus, rec=rec))
    assert str(mus[1]) in str(err.value) and "step 2" in str(err.value)


def test_nonlinear_snapshots_are_the_host_sets(fom_ops):
    import torch

    from romtime_amd import fom as dfom

    for bdf2 in (True, False):
        c = fc.case("burgers", 40, 9, bdf2, 3)
        for j in range(3):
            got = dfom.nonlinear_snapshots(c["fom"], torch.from_numpy(c["host"][j].copy())).numpy()
            assert got.shape == c["host_nl"][j].shape == (3 * 39 + 2, 9)
            np.testing.assert_allclose(got, c["host_nl"][j], rtol=1e-13, atol=1e-14 * np.abs(c["host_nl"][j]).max())
            assert (got[0] == 0).all()


def _rom(fom, kind, where):
    from romtime_amd.rom import RomConstructor

    grid = {k: [v] for k, v in fc.mus_of(kind, 1)[0].items()}
    rom = RomConstructor(fom=fom, grid=grid)
    rom.SNAPSHOTS_ON = where
    rom.setup(rnd=0)
    return rom


@pytest.mark.parametrize("kind", ["burgers", "heat"])
def test_snapshots_on_device_feeds_the_same_sets_in_the_same_order(fom_ops, monkeypatch, kind):
    from romtime_amd import walks
    from romtime_amd.conventions import Stage, Treewalk

    seen = {}
    real = walks.pod_sequence

    def spy(sets, **kw):
        def tap():
            for X in sets:
                seen[where].append(X.numpy().copy())
                yield X
        return real(tap(), **kw)

    monkeypatch.setattr(walks, "pod_sequence", spy)
    roms, sols = {}, {}
    mus = fc.mus_of(kind, 3)
    for where in ("host", "device"):
        seen[where] = []
        rom = _rom(fc.make_fom(kind, 40, 12), kind, where)
        sols[where] = rom.build_reduced_basis(mu_space=[dict(mu) for mu in mus], num_basis=6)
        roms[where] = rom
    assert len(seen["host"]) == len(seen["device"]) == (6 if kind == "burgers" else 3)
    for a, b in zip(seen["host"], seen["device"]):
        assert a.shape == b.shape
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(a)
    assert sorted(sols["host"]) == sorted(sols["device"]) == [0, 1, 2]
    for k in sols["host"]:
        assert sols["host"][k].shape == sols["device"][k].shape == (41, 12)
        assert fc.rel(sols["device"][k], sols["host"][k]) <= 1e-13
    off_h, off_d = roms["host"].report[Stage.OFFLINE], roms["device"].report[Stage.OFFLINE]
    assert off_h[Treewalk.BASIS_TIME] == off_d[Treewalk.BASIS_TIME]
    assert off_h[Treewalk.BASIS_FINAL] == off_d[Treewalk.BASIS_FINAL] == 6
    assert roms["host"].mu_space[Stage.OFFLINE] == roms["device"].mu_space[Stage.OFFLINE]
    assert (roms["device"].basis_nonlinear is not None) == (kind == "burgers")


def test_snapshots_on_rejects_other_values_and_models_without_a_recipe(fom_ops):
    from romtime_amd.testing.mock import AffineBurgers

    rom = _rom(fc.make_fom("heat", 40, 4), "heat", "gpu")
    with pytest.raises(ValueError, match="SNAPSHOTS_ON"):
        rom.build_reduced_basis(mu_space=fc.mus_of("heat", 1), num_basis=2)
    rom = _rom(AffineBurgers(N=20, nt=4, dt=0.01), "heat", "device")
    with pytest.raises(NotImplementedError, match="p1_fom_recipe"):
        rom.build_reduced_basis(mu_space=[dict(alpha=1.0, beta=1.0, delta=0.1, omega=1.0)], num_basis=2)
    from romtime_amd.rom import RomConstructor

    assert RomConstructor.SNAPSHOTS_ON == "host"
