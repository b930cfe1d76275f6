"""rt_trajectory_residuals without a GPU: the plan query (argument checks and slicing, host logic only), the premises of
the cases of test_residual_gpu.py in NumPy, and the host logic of ``certify.trajectory_residuals``, ``online.residuals``
and ``online.evaluate(residuals=True)`` on a NumPy stand-in of the device operator (tests/residual_cases.py)."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import fom_cases as fc
from tests import residual_cases as rc

ROOT = Path(__file__).resolve().parent.parent
ARG, UNSUPPORTED = -1, -3


# ---- plan query ------------------------------------------------------------------------------------------------------------------
def _query(nx=70, n_mu=2, nt=5, first_step=0, k=5, ldb=None, lda=None, cus=256, desc=True, tab=True, u_init=False, B=True, A=True,
           a_init=False, res=True, want_info=True):
    from romtime_amd import _lib

    lib = _lib.load()
    some = (C.c_double * 8)()
    sp = lambda on: C.cast(some, C.c_void_p) if on else None
    d = _lib.FomDesc(nx, n_mu, nt, first_step, 0.1, 1, 1, sp(tab), sp(u_init))
    info3 = (C.c_int64 * 3)(-1, -1, -1)
    code = lib.rt_trajectory_residuals_plan_info(cus, C.byref(d) if desc else None, sp(B), k if ldb is None else ldb, k, sp(A),
                                                 k if lda is None else lda, nt * k, sp(a_init), sp(res), None,
                                                 info3 if want_info else None)
    return code, tuple(int(v) for v in info3)


def test_plan_query_accepts_the_plain_call():
    assert _query()[0] == 0 and _query(want_info=False)[0] == 0
    assert _query(first_step=3, a_init=True)[0] == 0 and _query(ldb=8, lda=6)[0] == 0


@pytest.mark.parametrize("kw", [dict(desc=False), dict(tab=False), dict(B=False), dict(A=False), dict(res=False), dict(u_init=True),
                                dict(nx=1), dict(nx=0), dict(n_mu=0), dict(nt=0), dict(k=0), dict(first_step=-1), dict(ldb=4),
                                dict(lda=4), dict(first_step=2), dict(cus=0)], ids=str)
def test_plan_query_refuses_bad_arguments(kw):
    code, info = _query(**kw)
    assert code == ARG and info == (-1, -1, -1)


def test_plan_query_limits():
    assert _query(k=128)[0] == 0 and _query(k=129)[0] == UNSUPPORTED
    assert _query(nx=1 << 22)[0] == 0 and _query(nx=(1 << 22) + 1)[0] == UNSUPPORTED       # the limit of rt_p1_fom_bdf_sweep
    assert _query(nx=1 << 22, n_mu=1 << 20, nt=1 << 20)[0] == UNSUPPORTED                  # more than 2^31 workgroups


def test_plan_info():
    """info3 = (workgroups, row slices, tile): the slices hold whole stages, at least ``slice_length()`` rows where the mesh
    allows and at most four workgroups per CU for one step block; they do not depend on nt or the number of
    trajectories."""
    e, b, s = rc.stage_rows(), rc.block_steps(), rc.slice_length()
    assert (e, b) == (30, 62) and s % e == 0
    cdiv = lambda p, q: -(-p // q)
    for nx in (2, 1024, 1025, s + 1, s + 2, 1 << 22):
        n = nx - 1
        for cus in (256, 8):
            slices = max(min(4 * cus, cdiv(n, s)), 1)
            slices = cdiv(n, cdiv(cdiv(n, slices), e) * e)
            for nt, n_traj in ((1, 1), (62, 1), (63, 3), (1000, 2)):
                code, info = _query(nx=nx, nt=nt, n_mu=n_traj, cus=cus)
                assert code == 0 and info == (cdiv(nt, b) * slices * n_traj, slices, 1000 * e + b), (nx, cus, nt, n_traj, info)
    assert _query(nx=2)[1][1] == 1 and _query(nx=1024)[1][1] == 2 and _query(nx=1025)[1][1] == 2
    assert _query(nx=s + 1)[1][1] == 1 and _query(nx=s + 2)[1][1] == 2
    # 1024 slices asked for, 137 stages of 30 rows each: 1021 slices cover the mesh
    assert _query(nx=1 << 22)[1][1] == 1021 and _query(nx=1 << 22, cus=8)[1][1] == 32


def test_abi_and_build_list():
    api = (ROOT / "romtime_amd" / "csrc" / "api.hip").read_text()
    assert int(re.search(r"int rt_version\(void\) \{ return (\d+); \}", api).group(1)) >= 420
    from romtime_amd import _lib, build

    assert "traj_residual.hip" in build.SOURCES
    assert {"rt_trajectory_residuals", "rt_trajectory_residuals_plan_info"} <= set(_lib.SIGNATURES)
    header = (ROOT / "include" / "romtime_hip.h").read_text()
    assert "since version 420" in header and "fom/base.py:693-831" in header.split("since version 420")[1][:200]


def test_rows_are_stated_once():
    """FomStep and the row functions live in p1_rows.h alone; both kernels include it."""
    csrc = ROOT / "romtime_amd" / "csrc"
    for name in ("p1_fom.hip", "traj_residual.hip"):
        text = (csrc / name).read_text()
        assert '#include "p1_rows.h"' in text
        assert not re.search(r"\bfom_(step|w|past|row)\s*\([^;{]*\)\s*\{", text) and "struct FomStep" not in text, name
    rows = (csrc / "p1_rows.h").read_text()
    assert all(re.search(rf"\b{f}\s*\(", rows) for f in ("fom_step", "fom_w", "fom_past", "fom_row")) and "struct FomStep" in rows
    # the contraction setting the rows compile under is the translation unit's default, in both files
    assert all("fp contract" not in (csrc / n).read_text() for n in ("p1_rows.h", "p1_fom.hip", "traj_residual.hip"))


# ---- premises of the GPU cases -------------------------------------------------------------------------------------------------------
def test_row_cases_reach_every_seam():
    e, s = rc.stage_rows(), rc.slice_length()
    counts = rc.row_counts()
    assert {1, 2, 31, 32, 33, 63, 64, 65, s - 1, s, s + 1, 2 * s + 1} <= set(counts)
    # one row short of a stage, a whole stage and one row more: at the first seam, at a later one and at the slice's end
    assert {e - 1, e, e + 1} <= set(counts) and {2 * e - 1, 2 * e, 2 * e + 1} <= set(counts) and s % e == 0
    slices = {n: rc.plan(n + 1)[1] for n in counts}
    assert slices[s] == 1 and slices[s + 1] == 2 and slices[2 * s + 1] == 3
    assert all((kind, n + 1, 3, 5, 1) in rc.row_case_keys() for kind in ("burgers", "heat") for n in counts)


def test_step_cases_straddle_a_block():
    b = rc.block_steps()
    assert {1, 2, 3, 63, 64, 65, 66, 130} <= set(rc.STEP_NTS)
    assert min(rc.STEP_NTS) == 1 and b + 1 in rc.STEP_NTS and b + 2 in rc.STEP_NTS and max(rc.STEP_NTS) > 2 * b
    keys = rc.step_case_keys()
    assert len(keys) == 4 * len(rc.STEP_NTS) and {k[5] for k in keys} == {(False, False), (False, True), (True, False), (True, True)}
    assert all(k[4] == 3 and k[1] == rc.STEP_NX for k in keys)


@pytest.mark.parametrize("kind", ["burgers", "heat"])
@pytest.mark.parametrize("nx", rc.OWN_NX)
def test_own_trajectory_bound_in_float64(kind, nx):
    """V = I, a = U: the float64 evaluation satisfies res <= omega scale (1 + 4 N_h eps), and the full-order trajectory's
    relative residual is rounding."""
    fom = fc.make_fom(kind, nx, rc.OWN_NT)
    rec = fc.recipe(fom, fc.mus_of(kind, 3))
    U, _, flags = fc.truth(nx, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"], dtype=np.float64)
    assert not flags.any()
    res, scale, omega = rc.truth(nx, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"], np.eye(nx + 1), U, dtype=np.float64)
    print(f"{kind} nx {nx}: worst res/scale {np.max(res / scale):.3e}, worst omega {omega.max():.3e}")
    assert np.all(res <= rc.own_bound(omega, scale, nx + 1)) and np.all(scale > 0)
    assert np.max(res / scale) <= 64 * rc.EPS


def test_truth_takes_the_older_states_from_a_init():
    """The horizon cut anywhere gives the truth of the whole: a_init = the two coefficient rows before the cut."""
    c = rc.case("burgers", 40, 7, 4, 2)
    whole = rc.truth(c["nx"], c["tab"], c["dt"], True, True, c["V"], c["a"])
    for cut in (1, 2, 5):
        older = np.stack([c["a"][:, cut - 1], c["a"][:, cut - 2] if cut >= 2 else 0 * c["a"][:, 0]], axis=1)
        part = rc.truth(c["nx"], c["tab"][cut:], c["dt"], True, True, c["V"], c["a"][:, cut:], a_init=older, first_step=cut)
        for w, p in zip(whole, part):
            assert np.array_equal(w[:, cut:], p)
    assert np.isfinite(np.asarray(whole[0], dtype=np.float64)).all()                      # no NaN from the basis' boundary rows


# ---- host logic -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def stubs(monkeypatch):
    rc.install_stubs(monkeypatch)


def _model(nx=24, nt=7, r=3, n_mu=2, seed=3):
    fom = fc.make_fom("burgers", nx, nt)
    mus = fc.mus_of("burgers", n_mu)
    rng = np.random.default_rng(seed)
    V = np.linalg.qr(rng.standard_normal((nx + 1, r)))[0]
    uN = rng.uniform(-1, 1, (n_mu, nt, r))
    return fom, mus, V, uN


def test_certify_shapes_and_chunk_carry(stubs):
    from romtime_amd import certify

    fom, mus, V, uN = _model()
    rec = fc.recipe(fom, mus)
    want_res, want_scale, _ = rc.truth(24, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"], V, uN, dtype=np.float64)
    curve = certify.trajectory_residuals(fom, V, uN, mus)
    assert isinstance(curve, np.ndarray) and curve.shape == (2, 7) and np.array_equal(curve, want_res / want_scale)
    res, scale = certify.trajectory_residuals(fom, V, uN, mus, rec=rec, relative=False)
    assert np.array_equal(res, want_res) and np.array_equal(scale, want_scale)
    for chunk in (1, 2, 3, 7, 50):                                                         # the carry: the result does not depend on it
        assert np.array_equal(certify.trajectory_residuals(fom, V, uN, mus, chunk=chunk), curve), chunk
    with pytest.raises(ValueError, match="chunk"):
        certify.trajectory_residuals(fom, V, uN, mus, chunk=0)
    with pytest.raises(ValueError, match="uN"):
        certify.trajectory_residuals(fom, V, uN[:1], mus)
    with pytest.raises(ValueError, match="uN"):
        certify.trajectory_residuals(fom, V, uN[:, :-1], mus)
    with pytest.raises(ValueError, match="basis"):
        certify.trajectory_residuals(fom, V[:-1], uN, mus)
    # scale == 0 gives 0, not NaN: zero coefficients in a problem without forcing have a zero system
    zero = dict(rec, tab=rec["tab"].copy())
    zero["tab"][:, :, 4:] = 0.0
    assert np.array_equal(certify.trajectory_residuals(fom, V, 0 * uN, mus, rec=zero), np.zeros((2, 7)))


def test_certify_names_the_missing_recipe(stubs):
    from romtime_amd import certify

    fom, mus, V, uN = _model()
    plain = SimpleNamespace(nx=fom.nx, dt=fom.dt, domain=fom.domain)
    with pytest.raises(NotImplementedError, match="p1_fom_recipe"):
        certify.trajectory_residuals(plain, V, uN, mus)


class _FakeRom:
    """What ``online.evaluate`` and ``online.residuals`` ask of a model: ``fom``, ``basis`` and ``solve_many``."""

    def __init__(self, fom, V, uN):
        self.fom, self.basis, self._uN, self.calls = fom, V, uN, 0

    def solve_many(self, mus, step=None):
        self.calls += 1
        lo = 10 * (self.calls - 1)
        n = len(mus)
        return SimpleNamespace(idx=list(range(lo, lo + n)), mus=list(mus), uN=torch.from_numpy(self._uN[:n].copy()),
                               _V=torch.from_numpy(np.ascontiguousarray(self.basis)))


def test_online_residuals(stubs):
    from romtime_amd import certify, online

    fom, mus, V, uN = _model()
    rom = _FakeRom(fom, V, uN)
    got = online.residuals(rom, mus, "online")
    want = certify.trajectory_residuals(fom, V, uN, mus)
    assert sorted(got) == [0, 1] and all(np.array_equal(got[j], want[j]) for j in range(2)) and rom.calls == 1
    with pytest.raises(NotImplementedError, match="p1_fom_recipe"):
        online.residuals(_FakeRom(SimpleNamespace(nx=fom.nx, dt=fom.dt, domain=fom.domain), V, uN), mus, "online")


def test_evaluate_residuals_and_unchanged_default(stubs, monkeypatch):
    from romtime_amd import certify, online
    from romtime_amd.conventions import ProblemType

    fom, mus, V, uN = _model(r=4)
    monkeypatch.setattr(certify, "evaluate", lambda Vr, ar, Vs, as_, U, lift=None: [dict(n=j, u=tuple(U[j].shape)) for j in range(len(U))])
    stored = {j: np.zeros((fom.nx + 1, 7)) for j in range(2)}

    def run(**kw):
        rom, srom = _FakeRom(fom, V[:, :3], uN[:, :, :3]), _FakeRom(fom, V, uN)
        return online.evaluate(rom, srom, mus, "online", fom_solutions=stored, **kw)

    base, with_res = run(), run(residuals=True)
    assert base.residuals == {} and dict(base) == dict(with_res) and base.mass == with_res.mass == {} and base.probes == with_res.probes == {}
    assert sorted(with_res.residuals) == [0, 1]
    want = {ProblemType.ROM: certify.trajectory_residuals(fom, V[:, :3], uN[:, :, :3], mus),
            ProblemType.SROM: certify.trajectory_residuals(fom, V, uN, mus)}
    for j in range(2):
        assert set(with_res.residuals[j]) == {ProblemType.ROM, ProblemType.SROM}
        for kind in want:
            assert np.array_equal(with_res.residuals[j][kind], want[kind][j])
    # a FOM without the recipe: the flag adds nothing and raises nothing
    bare = SimpleNamespace(nx=fom.nx, dt=fom.dt, domain=fom.domain, exact_solution=None, solve=None)
    rom, srom = _FakeRom(bare, V[:, :3], uN[:, :, :3]), _FakeRom(bare, V, uN)
    rom_grid = lambda j: (None, np.zeros((fom.nx + 1, 7)))
    real = rom.solve_many
    rom.solve_many = lambda mus, step=None: SimpleNamespace(**vars(real(mus, step)), grid=rom_grid)
    ev = online.evaluate(rom, srom, mus, "online", fom_solutions=stored, residuals=True)
    assert ev.residuals == {} and sorted(ev) == [0, 1]
