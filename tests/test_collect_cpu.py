"""Collecting the (M)DEIM snapshot sets on the device, host side: ``collect.resolve`` (which closed form stands behind a
reductor's callback, and the refusals - each before any bookkeeping), the ``SNAPSHOTS_ON`` attribute of the three classes,
the declaration / export / version / argument checks of rt_p1_snapshot_sets (its ``_plan_info`` twin runs the entry point's
own checks without a GPU), and the host logic of the device route on stand-ins: ``cpu_ops`` plus a NumPy restatement of
``ops.p1_snapshot_sets`` (tests/collect_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from romtime_amd import collect                      # noqa: F401  (without the feature nothing here can run)
from tests import collect_cases as cc
from tests import interp_cases as ic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG, RT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture
def host_sets(cpu_ops, monkeypatch):
    """The device route on the host: ``ops.p1_snapshot_sets`` restated in NumPy; ``host_sets.launches`` lists its calls."""
    from romtime_amd import ops

    launches = []

    def counted(kind, nx, rows, cols, h, **kw):
        out = cc.numpy_p1_snapshot_sets(kind, nx, rows, cols, h, **kw)
        launches.append((kind, tuple(out.shape)))
        return out

    monkeypatch.setattr(ops, "p1_snapshot_sets", counted, raising=False)
    monkeypatch.setattr(ops, "dense_solve_multi", ic.numpy_dense_solve_multi)          # what the device evaluate needs
    monkeypatch.setattr(ops, "interpolation_errors", ic.numpy_interpolation_errors)
    collect.launches = launches
    yield collect
    del collect.launches


# ---- resolve -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ("solver", "heat", "burgers"))
def test_resolve_every_callback_name(which):
    """Every ``assemble_*`` the FOM has: its own kind where p1_closed_form() carries the scalars (cc.CASES), a refusal
    that names the callback and the host route where it does not."""
    fom, mus = cc.make_fom(which), cc.mus_of(which)
    names = sorted(n for n in collect.CALLBACK_KINDS if hasattr(fom, n))
    assert len(names) >= 5
    seen = []
    for name in names:
        kind = collect.CALLBACK_KINDS[name]
        assert kind == ("rhs" if name == "assemble_rhs" else name[len("assemble_"):])
        red = cc.make_reductor(fom, kind, mus) if (which, kind) in cc.CASES else _bare(fom, kind)
        if (which, kind) in cc.CASES:
            assert collect.resolve(red, mus, cc.TS) == (fom, kind)
            assert collect.resolve(red) == (fom, kind)              # no parameter point, no grid: the name alone
            seen.append(kind)
        else:
            with pytest.raises(NotImplementedError, match=rf"{name}.*SNAPSHOTS_ON = 'host'"):
                collect.resolve(red, mus, cc.TS)
    assert seen == sorted(k for w, k in cc.CASES if w == which)


def _bare(fom, kind):
    from romtime_amd import DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation

    cls = DiscreteEmpiricalInterpolation if kind in cc.VECTOR_KINDS else MatrixDiscreteEmpiricalInterpolation
    return cls(assemble=getattr(fom, "assemble_" + kind), name=kind)


def test_resolve_override_grid_probe_and_class_fit():
    from scipy.stats.distributions import uniform

    from romtime_amd import DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation
    from romtime_amd.testing.walk_inputs import walk_rich_operator

    fom = cc.make_fom("burgers")
    red = MatrixDiscreteEmpiricalInterpolation(assemble=walk_rich_operator(fom), name="closure")
    with pytest.raises(NotImplementedError):
        collect.resolve(red)
    red.closed_form = (fom, "stiffness")                                # the instance attribute overrides the callback
    assert collect.resolve(red, cc.mus_of("burgers"), cc.TS) == (fom, "stiffness")
    assert red.copy().closed_form == (fom, "stiffness")
    red.closed_form = (fom, "stiff")
    with pytest.raises(NotImplementedError, match="unknown operator"):
        collect.resolve(red)
    # the kind has to fit the class: a load vector is no MDEIM snapshot, a matrix no DEIM snapshot
    red.closed_form = (fom, "lifting")
    with pytest.raises(NotImplementedError, match="does not take"):
        collect.resolve(red)
    with pytest.raises(NotImplementedError, match="does not take"):
        collect.resolve(DiscreteEmpiricalInterpolation(assemble=fom.assemble_mass, name="mass"))
    # without parameter points the scalars are asked of a point drawn from the grid, and no random state of the caller moves
    solver = cc.make_fom("solver")
    grid = dict(alpha_0=uniform(0.5, 1.0), gamma=uniform(0.1, 0.8))
    lifting = DiscreteEmpiricalInterpolation(assemble=solver.assemble_lifting, grid=grid, name="lifting")
    before = np.random.get_state()[1].copy()
    with pytest.raises(NotImplementedError, match="lacks the scalars"):
        collect.resolve(lifting)
    assert np.array_equal(np.random.get_state()[1], before)
    lifting.grid = None
    assert collect.resolve(lifting) == (solver, "lifting")              # nothing to ask: left to the first launch


def _refusals():
    """(label, reductor, run arguments) of the three refusals the issue names."""
    from romtime_amd import DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation
    from romtime_amd.base import Reductor
    from romtime_amd.testing.mock import AffineBurgers
    from romtime_amd.testing.walk_inputs import walk_rich_operator

    p = {"ts": cc.TS, "num_snapshots": 3}
    burgers, solver, affine = cc.make_fom("burgers"), cc.make_fom("solver"), AffineBurgers(N=40, nt=5, dt=0.01)
    out = []
    for label, cls, cb, mus in (("closure", MatrixDiscreteEmpiricalInterpolation, walk_rich_operator(burgers), cc.mus_of("burgers")),
                                ("no_closed_form", MatrixDiscreteEmpiricalInterpolation, affine.assemble_mass,
                                 [dict(alpha=1.0, beta=0.5, delta=0.2, omega=2.0)]),
                                ("no_scalars", DiscreteEmpiricalInterpolation, solver.assemble_lifting, cc.mus_of("solver"))):
        red = cls(assemble=cb, tree_walk_params=p, name=label)
        Reductor.setup(red, rnd=np.random.RandomState(0))
        red.rows, red.cols = [0, 1, 1], [0, 0, 1]
        out.append((label, red, mus))
    return out


def test_refusals_come_before_any_bookkeeping(host_sets):
    from copy import deepcopy

    from romtime_amd import interpolation
    from romtime_amd.conventions import Stage

    for label, red, mus in _refusals():
        assert not hasattr(getattr(red.assemble, "__self__", None), "p1_closed_form") or label == "no_scalars"
        red.SNAPSHOTS_ON = "device"
        report, space = deepcopy(dict(red.report)), deepcopy(red.mu_space)
        with pytest.raises(NotImplementedError, match="SNAPSHOTS_ON = 'host'") as info:
            red.run(mu_space=mus)
        assert label == "closure" or red.assemble.__name__ in str(info.value)             # the callback is named
        assert dict(red.report) == report and red.mu_space == space and red.mu is None, label
        assert dict(red.errors_rom) == {} and red.basis_fom is None
        # the device evaluate with device snapshots refuses at the same place: after the fold, before add_mu
        red.basis_fom = np.eye(3)[:, :2].copy()
        red.PT_U, red.dofs = red.basis_fom[:2].copy(), ([(0,), (1,)] if label == "no_scalars" else [(0, 0), (1, 0)])
        with pytest.raises(NotImplementedError, match="SNAPSHOTS_ON = 'host'"):
            interpolation.evaluate(red, cc.TS, mu_space=mus)
        assert red.mu_space[Stage.ONLINE] == [] and dict(red.errors_rom) == {}, label


# ---- the attribute ---------------------------------------------------------------------------------------------------------

def test_snapshots_on_default_override_copy_and_bad_value(host_sets):
    from romtime_amd import (DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation,
                             MatrixDiscreteEmpiricalInterpolationNonlinear)
    from romtime_amd import interpolation

    assert DiscreteEmpiricalInterpolation.SNAPSHOTS_ON == "host"
    fom = cc.make_fom("burgers")
    for cls, kind in ((DiscreteEmpiricalInterpolation, "lifting"), (MatrixDiscreteEmpiricalInterpolation, "mass"),
                      (MatrixDiscreteEmpiricalInterpolationNonlinear, "trilinear")):
        assert cls.SNAPSHOTS_ON == "host"
        red = cc.make_reductor(fom, kind, cc.mus_of("burgers"))
        assert type(red) is cls and red.SNAPSHOTS_ON == "host"
        assert "SNAPSHOTS_ON" not in red.copy().__dict__
        red.SNAPSHOTS_ON = "device"
        twin = red.copy()
        assert twin.SNAPSHOTS_ON == "device" and "SNAPSHOTS_ON" in twin.__dict__          # an instance override travels
        red.SNAPSHOTS_ON = "gpu"
        run = (lambda: red.run(u_n=cc.states(), mu_space=cc.mus_of("burgers"))) if kind == "trilinear" else \
            (lambda: red.run(mu_space=cc.mus_of("burgers")))
        with pytest.raises(ValueError, match="SNAPSHOTS_ON"):
            run()
        assert red.mu_space["offline"] == [] and red.basis_fom is None                  # before any bookkeeping
        with pytest.raises(ValueError, match="SNAPSHOTS_ON"):
            interpolation.evaluate(red, cc.TS, mu_space=cc.mus_of("burgers"))
        assert red.mu_space["online"] == []


# ---- the entry point's host side -------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entries():
    from romtime_amd import _lib, build

    text = open(os.path.join(REPO, "include", "romtime_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rt_p1_snapshot_sets", "rt_p1_snapshot_sets_plan_info"):
        assert re.search(rf"\bint\s+{name}\s*\(", code), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert _lib.load().rt_version() > 420
    api = open(os.path.join(REPO, "romtime_amd", "csrc", "api.hip")).read()
    assert int(re.search(r"int rt_version\(void\) \{ return (\d+); \}", api).group(1)) == _lib.load().rt_version()
    assert "p1_snapshots.hip" in build.SOURCES
    # one source for the entry formulas: both kernels include the header and neither restates a formula
    csrc = os.path.join(REPO, "romtime_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "p1_entry.h"))
    for src in ("p1_assembly.hip", "p1_snapshots.hip"):
        body = open(os.path.join(csrc, src)).read()
        body = re.sub(r"//.*", "", body)
        assert '#include "p1_entry.h"' in body and "p1_entry_value(" in body, src
        assert "/ 6.0" not in body and "/ 3.0" not in body, src


def _plan(lib, **a):
    info = (C.c_int64 * 2)(-7, -7)
    rc = lib.rt_p1_snapshot_sets_plan_info(a["cus"], a["kind"], a["nx"], a["rows"], a["cols"], a["m"], a["n_par"], a["h"], a["coef"],
                                           a["par_mode"], a["par"], a["n_fun"], a["fun"], a["zero_first"], a["beta"], a["out"], info)
    return rc, (int(info[0]), int(info[1]))


def test_argument_checks_and_plan_are_host_logic():
    """rt_p1_snapshot_sets_plan_info: the entry point's checks and return codes, {workgroups, launches}; no pointer read."""
    from romtime_amd import _lib
    from romtime_amd.ops import P1_KINDS as K

    lib = _lib.load()
    words = (C.c_double * 4)()
    ptr = C.cast(words, C.c_void_p)                                        # stands for every device array: never read
    good = dict(cus=256, kind=K["mass"], nx=100, rows=ptr, cols=ptr, m=298, n_par=4, h=ptr, coef=None, par_mode=0, par=None,
                n_fun=1, fun=None, zero_first=1, beta=0.0, out=ptr)
    call = lambda **change: _plan(lib, **dict(good, **change))
    tril = dict(kind=K["trilinear"])

    assert call() == (0, (5, 1))                                           # ceil(4 * 298 / 256) workgroups, one launch
    assert call(coef=ptr, beta=1.0, zero_first=0)[0] == 0
    assert call(n_par=500, m=6000, n_fun=40, fun=ptr, **tril) == (0, (256 * 32, 1))        # capped: the rest is the stride
    assert call(cus=64, n_par=500, m=6000, n_fun=40, fun=ptr, **tril) == (0, (64 * 32, 1))
    assert call(n_par=1, m=1) == (0, (1, 1)) and call(n_par=1, m=256) == (0, (1, 1)) and call(n_par=1, m=257) == (0, (2, 1))
    # every way of supplying the nodal function the kinds take
    assert call(par_mode=2, par=ptr, **tril)[0] == 0 and call(n_fun=7, fun=ptr, **tril)[0] == 0
    assert call(kind=K["load"], cols=None, par_mode=2, par=ptr)[0] == 0 and call(kind=K["load"], cols=None, fun=ptr, n_fun=3)[0] == 0
    assert call(kind=K["load_p2"], cols=None, par_mode=3, par=ptr)[0] == 0 and call(kind=K["load_p2"], cols=None, fun=ptr)[0] == 0
    assert call(kind=K["stiffness"], coef=ptr)[0] == 0 and call(kind=K["convection"])[0] == 0
    bads = (dict(rows=None), dict(h=None), dict(out=None), dict(cols=None), dict(m=0), dict(n_par=0), dict(n_fun=0), dict(m=-3),
            dict(nx=1), dict(nx=0), dict(kind=6), dict(kind=-1), dict(cus=0),
            dict(par_mode=1), dict(par_mode=4), dict(par_mode=2), dict(par=ptr),                # mode and pointer disagree
            dict(fun=ptr), dict(n_fun=2), dict(par_mode=2, par=ptr),                            # mass integrates no function
            dict(tril), dict(tril, par_mode=2, par=ptr, fun=ptr),                               # neither / both
            dict(tril, par_mode=3, par=ptr), dict(kind=K["load"], cols=None, par_mode=3, par=ptr),
            dict(kind=K["load_p2"], cols=None, par_mode=2, par=ptr),                            # a mode the kind does not take
            dict(tril, par_mode=2, par=ptr, n_fun=2),                                           # par goes with n_fun = 1
            dict(tril, fun=ptr, n_par=2 ** 31, n_fun=2 ** 31, m=1), dict(n_par=2 ** 40, m=2 ** 22),   # 2^62 words
            dict(tril, fun=ptr, n_par=2 ** 62, n_fun=2 ** 62, m=2 ** 62))                       # the product overflows
    for bad in bads:
        assert call(**bad) == (RT_ERR_ARG, (-7, -7)), bad
    assert call(fun=ptr, n_par=2 ** 31, n_fun=2 ** 31 - 1, m=1, **tril) == (0, (256 * 32, 1))   # any count below 2^62
    assert call(n_par=2 ** 40 - 1, m=2 ** 22)[0] == 0
    assert call(nx=2 ** 22)[0] == 0 and call(nx=2 ** 22 + 1)[0] == RT_ERR_UNSUPPORTED           # the family's limit
    assert call(nx=2 ** 22 + 1, rows=None)[0] == RT_ERR_ARG                                     # argument errors first
    assert lib.rt_p1_snapshot_sets(None, K["mass"], 100, ptr, ptr, 298, 4, ptr, None, 0, None, 1, None, 1, 0.0, ptr) == RT_ERR_ARG


# ---- host logic of the device route ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,kind", cc.CASES, ids=[f"{w}-{k}" for w, k in cc.CASES])
def test_sets_follow_the_kind_rules(host_sets, which, kind):
    """The kind rules, the column order and the zeroed entry: the sets of ``collect`` against the stacked
    ``assemble_snapshot`` columns (the bounds of tests/test_collect_gpu.py; here the closed forms are the NumPy ones)."""
    from romtime_amd.conventions import EmpiricalInterpolation as EI

    fom, mus = cc.make_fom(which), cc.mus_of(which)
    red = cc.make_reductor(fom, kind, mus)
    u_n = red.u_n if kind == "trilinear" else None
    ref = cc.callback_columns(red, mus, cc.TS, u_n)
    per_mu = ref.shape[1] // len(mus)
    for j, mu in enumerate(mus):
        want = ref[:, j * per_mu:(j + 1) * per_mu].copy()
        exact = host_sets.exact_snapshots(red, mu, cc.TS, funcs=u_n).numpy()
        atol = (2e-14 if kind == "rhs" else 1e-14) * np.abs(ref).max()
        np.testing.assert_allclose(exact, want, rtol=1e-12, atol=atol)
        if red.TYPE != EI.DEIM:
            assert np.all(want[0] == 1.0)
            want[0] = 0.0
        if kind == "trilinear":
            sets = host_sets.state_level_sets(red, mu, cc.TS, u_n)
            assert len(sets) == len(cc.TS) and all(tuple(S.shape) == (len(red.rows), cc.N_PSI) for S in sets)
            got = np.hstack([S.numpy() for S in sets])
        else:
            got = host_sets.time_level_set(red, mu, cc.TS).numpy()
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=atol)
        if red.TYPE != EI.DEIM:
            assert np.all(got[0] == 0.0)
    n_launch = len(host_sets.launches)
    assert n_launch == len(mus) * 2 * (2 if kind == "rhs" else 1)          # one launch per point and set (rhs: two kinds)


@pytest.mark.parametrize("which,kind", [("heat", "stiffness"), ("heat", "rhs"), ("burgers", "trilinear")])
def test_device_route_keeps_the_bookkeeping_and_makes_no_callback(host_sets, which, kind):
    from romtime_amd.conventions import Stage

    mus = cc.mus_of(which)
    tol = {"tol_mu": 1.0 - 1e-9, "tol_time": 1.0 - 1e-10}
    runs = {}
    for route in ("host", "device"):
        fom = cc.make_fom(which)
        red = cc.make_reductor(fom, kind, mus, params=tol)
        counter = cc.Counted(fom)
        red.assemble = getattr(fom, "assemble_" + kind)                   # the counted callback
        red.SNAPSHOTS_ON = route
        if kind == "trilinear":
            red.run(u_n=cc.states(), mu_space=[dict(m) for m in mus])
        else:
            red.run(mu_space=[dict(m) for m in mus])
        runs[route] = (red, counter.calls)
    (host, n_host), (dev, n_dev) = runs["host"], runs["device"]
    assert n_host == len(mus) * len(cc.TS) * (cc.N_PSI if kind == "trilinear" else 1) and n_dev == 0
    assert dev.mu_space == host.mu_space and dev.mu == host.mu
    a, b = host.report[Stage.OFFLINE], dev.report[Stage.OFFLINE]
    assert sorted(a) == sorted(b)
    ints = lambda off: {k: v for k, v in off.items() if isinstance(v, (int, dict)) and not isinstance(v, bool)
                        and (isinstance(v, int) or all(isinstance(x, int) for x in v.values()))}
    assert ints(a) == ints(b) and a["basis-shape-final"] == dev.N == host.N
    assert dev.dofs == host.dofs
