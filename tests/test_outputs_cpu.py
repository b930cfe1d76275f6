"""rt_trajectory_integrals' host side (declaration, export, version, argument checks and launch plan, none of which needs
a GPU) and the host logic of romtime_amd.outputs (quadrature rows and weights, lifting columns, layouts of ``length``,
payload keys, np.interp semantics of the probes, argument errors) with the device operators stubbed: ``cpu_ops`` plus a
NumPy restatement of ``ops.trajectory_integrals``.  The data are the reference driver's own run, tests/golden/hrom.npz;
truth and bar are those of tests/outputs_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import outputs_cases as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG, RT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture
def outputs(cpu_ops, monkeypatch):
    from romtime_amd import ops, outputs

    monkeypatch.setattr(ops, "trajectory_integrals", oc.numpy_trajectory_integrals)
    return outputs


@pytest.fixture(scope="module")
def golden_hrom():
    from tests.conftest import load_golden

    return load_golden("hrom.npz")


def test_header_declares_and_library_exports_the_entry():
    from romtime_amd import _lib

    text = open(os.path.join(REPO, "include", "romtime_hip.h")).read()
    assert re.search(r"#define\s+RT_FN_POWER\s+0\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rt_trajectory_integrals", "rt_trajectory_integrals_plan_info"):
        assert re.search(rf"\bint\s+{name}\s*\(", code), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert _lib.load().rt_version() >= 370


def test_argument_checks_and_plan_are_host_logic():
    """rt_trajectory_integrals_plan_info runs the entry point's own checks without a ctx and follows no pointer."""
    from romtime_amd import _lib

    lib = _lib.load()
    buf = (C.c_double * 4)()                                       # stands for every array: never read
    ptr = C.cast(buf, C.c_void_p)
    par = (C.c_double * 3)(1.0, -0.2, 5.000000000000001)
    good = dict(cus=256, E=ptr, lde=81, w=ptr, A=ptr, lda=81, stride_a=81 * 130, scale=ptr, n_pts=2200, k=81, nt=130,
                n_traj=2, fn=0, par=par, out=ptr)

    def call(**change):
        a = dict(good, **change)
        info = (C.c_int64 * 3)()
        rc = lib.rt_trajectory_integrals_plan_info(a["cus"], a["E"], a["lde"], a["w"], a["A"], a["lda"], a["stride_a"], a["scale"],
                                                   a["n_pts"], a["k"], a["nt"], a["n_traj"], a["fn"], a["par"], a["out"], info)
        return rc, dict(grid=int(info[0]), splits=int(info[1]), tile=(int(info[2]) // 1000, int(info[2]) % 1000))

    assert call() == (0, oc.trajectory_integrals_plan(2200, 130, 2, 256))
    assert call()[1]["splits"] == 3
    assert call(w=None, scale=None)[0] == 0                        # optional
    assert call(k=128, lde=128, lda=128)[0] == 0
    assert call(k=129, lde=129, lda=129)[0] == RT_ERR_UNSUPPORTED
    for bad in (dict(E=None), dict(A=None), dict(out=None), dict(par=None), dict(n_pts=0), dict(k=0), dict(nt=0),
                dict(n_traj=0), dict(n_pts=-5), dict(fn=1), dict(fn=-1), dict(lde=80), dict(lda=80)):
        assert call(**bad)[0] == RT_ERR_ARG, bad
    for n_pts, nt, n, cus in ((66, 1, 1, 256), (33, 63, 2, 256), (64, 65, 3, 304), (2049, 130, 1, 256), (200_000, 10_000, 32, 256),
                              (200_000, 10_000, 32, 64)):
        assert call(n_pts=n_pts, nt=nt, n_traj=n, cus=cus) == (0, oc.trajectory_integrals_plan(n_pts, nt, n, cus))
    assert lib.rt_trajectory_integrals(None, ptr, 81, ptr, ptr, 81, 81, ptr, 10, 81, 1, 1, 0, par, ptr) == RT_ERR_ARG   # no ctx


def test_two_points_integrate_a_cubic_of_a_p1_function_exactly(outputs):
    """(c0 + c1 u)^3 of a P1 u: per cell h (b1^4 - b0^4) / (4 c1 (u1 - u0)) with b = c0 + c1 u."""
    rng = np.random.default_rng(0)
    nx, c0, c1 = 40, 0.7, -0.3
    u = rng.uniform(-1.0, 1.0, nx + 1)
    u[5] = u[4] + 0.25                                             # no cell with u1 == u0 (the closed form divides by it)
    assert np.abs(np.diff(u)).min() > 1e-4
    b = (c0 + c1 * u).astype(np.longdouble)
    exact = np.sum((b[1:] ** 4 - b[:-1] ** 4) / (4 * c1 * np.diff(u).astype(np.longdouble))) / nx
    E, w = outputs.quadrature_basis(u[:, None], points=2)
    assert tuple(E.shape) == (2 * nx, 1) and tuple(w.shape) == (2 * nx,)
    got = np.sum(w.numpy() * (c0 + c1 * E.numpy()[:, 0]) ** 3)
    # rounding only: ten operations per term and a sum of 2 nx terms, each at most w max|b|^3 (sum w = 1)
    assert abs(got - exact) <= 2 * (nx + 13) * oc.U_ROUND * float(np.abs(b).max()) ** 3, (got, float(exact))
    E1, w1 = outputs.quadrature_basis(u[:, None], points=1)
    one = np.sum(w1.numpy() * (c0 + c1 * E1.numpy()[:, 0]) ** 3)
    assert abs(one - exact) > 1e-6                                 # one point does not: the rule is what is tested
    for points in (1, 2, 3, 4):
        E, w = outputs.quadrature_basis(u[:, None], points)
        Eh, wh = oc.host_quadrature(u[:, None], points)
        np.testing.assert_allclose(E.numpy(), Eh, rtol=0, atol=4 * oc.U_ROUND)
        np.testing.assert_allclose(w.numpy(), wh, rtol=4 * oc.U_ROUND)
        assert abs(w.numpy().sum() - 1.0) < 1e-14
    for points in (0, 5, 2.5):
        with pytest.raises(ValueError):
            outputs.quadrature_basis(u[:, None], points)


def test_density_and_pressure_are_the_references_functions(outputs):
    assert outputs.density(1.4) == ("power", 1.0, -(1.4 - 1.0) / 2.0, 2.0 / (1.4 - 1.0))
    assert outputs.pressure(1.4) == ("power", 1.0, -(1.4 - 1.0) / 2.0, 2.0 * (1.4 / (1.4 - 1.0)))
    assert outputs.density(1.4)[3] == 5.000000000000001            # not an integer: the pow route


def test_mass_conservation_on_the_piston_case(outputs, golden_hrom):
    from romtime_amd.conventions import MassConservation, ProbeLocations, ProblemType

    assert (MassConservation.WHICH, MassConservation.TIMESTEPS, MassConservation.MASS, MassConservation.MASS_CHANGE,
            MassConservation.OUTFLOW) == ("which", "timesteps", "mass", "mass_change", "outflow")
    assert (ProbeLocations.OUTFLOW, ProbeLocations.MIDDLE, ProbeLocations.PISTON) == ("outflow", "halfway", "piston")
    assert ProblemType.ROM == "rom"
    case = oc.piston_outputs_case(golden_hrom)
    payload = outputs.mass_conservation(case["Vr"], case["rom"], case["mus"], case["dt"], case["length"],
                                        lift=(case["ramp"], case["amp"]), ts=case["ts"])
    worst = oc.check_piston_mass(case, payload)
    print(f"mass_conservation (NumPy restatement) vs the long-double truth: worst |difference| / bar = {worst:.3f}")
    by_value = outputs.mass_conservation(case["Vr"], case["rom"], case["a0"], case["dt"], case["length"],
                                         lift=(case["ramp"], case["amp"]))           # a0 values, default time steps
    for a, b in zip(payload, by_value):
        np.testing.assert_array_equal(a["mass"], b["mass"])
        np.testing.assert_array_equal(a["outflow"], b["outflow"])
        np.testing.assert_array_equal(a["timesteps"], b["timesteps"])
    for points in (1, 3):                                          # other rules: the same truth at their own rows
        p = outputs.mass_conservation(case["Vr"], case["rom"], case["mus"], case["dt"], case["length"],
                                      lift=(case["ramp"], case["amp"]), ts=case["ts"], points=points)
        oc.check_piston_mass(case, p, points=points)
    one = outputs.mass_conservation(case["Vr"], case["rom"][1], [case["mus"][1]], case["dt"], case["length"][1],
                                    lift=(case["ramp"], case["amp"][1:2]))           # (nt, r) and (nt,) for one trajectory
    np.testing.assert_array_equal(one[0]["mass"], payload[1]["mass"])


def test_snapshot_mass_follows_the_same_quadrature(outputs, golden_hrom):
    case = oc.piston_outputs_case(golden_hrom)
    j = 1
    lifted = np.column_stack([case["Vr"], case["ramp"]]) @ np.column_stack([case["rom"][j], case["amp"][j]]).T
    fom = outputs.snapshot_mass_conservation(lifted, case["mus"][j], case["dt"], case["length"][j])
    rom = outputs.mass_conservation(case["Vr"], case["rom"][j], [case["mus"][j]], case["dt"], case["length"][j],
                                    lift=(case["ramp"], case["amp"][j:j + 1]))[0]
    assert fom["which"] == "fom" and set(fom) == set(rom)
    np.testing.assert_allclose(fom["mass"], rom["mass"], rtol=1e-13)
    np.testing.assert_allclose(fom["outflow"], rom["outflow"], rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(fom["mass_change"], np.gradient(fom["mass"], case["dt"], edge_order=2))


def test_probes_are_np_interp_on_the_moving_mesh(outputs, golden_hrom):
    case = oc.piston_outputs_case(golden_hrom)
    B = np.column_stack([case["Vr"], case["ramp"]])
    L = case["length"]
    x = np.array([0.0, 0.5, 0.3337, float(L.min()), float(L.max()) + 0.5, -0.25, np.inf])     # beyond L(t) and below 0: clamped
    got = outputs.probes(case["Vr"], case["rom"], x, L, lift=(case["ramp"], case["amp"]))
    assert got.shape == (5, 22, len(x))
    nodes = np.arange(61) / 60.0
    k = B.shape[1]
    for j in range(5):
        a = np.column_stack([case["rom"][j], case["amp"][j]])
        u = B @ a.T                                                # (61, nt)
        for t in range(22):
            want = np.interp(x, L[j, t] * nodes, u[:, t])
            # two dot products of k terms, and an interpolation weight that np.interp forms from x - x_i (error u x: nx u
            # of a cell) and the gather from x / L nx: twice [(k + 4) u 2 max |B||a| + 4 u nx max |u_i+1 - u_i|]
            mag = (np.abs(B) @ np.abs(a[t])).max()
            bar = 2.0 * ((k + 4) * oc.U_ROUND * 2 * mag + 4 * oc.U_ROUND * 60 * np.abs(np.diff(u[:, t])).max())
            assert np.all(np.abs(got[j, t] - want) <= bar), (j, t, np.abs(got[j, t] - want).max(), bar)
        np.testing.assert_allclose(got[j, :, 0], u[0], rtol=0, atol=bar)                        # x = 0: node 0
        np.testing.assert_array_equal(got[j, :, 4], got[j, :, 6])                               # past L(t): the piston's node
        np.testing.assert_allclose(got[j, :, 6], u[-1], rtol=0, atol=bar)
        np.testing.assert_array_equal(got[j, :, 5], got[j, :, 0])
    assert outputs.probes(case["Vr"], case["rom"][0], 0.5, L[0], lift=(case["ramp"], case["amp"][:1])).shape == (1, 22, 1)


def test_shape_errors(outputs, golden_hrom):
    case = oc.piston_outputs_case(golden_hrom)
    lift = (case["ramp"], case["amp"])
    fn = outputs.density(1.4)
    with pytest.raises(ValueError, match="n_mu, nt"):               # (nt, n_mu), as p1_closed_form()["h"] * nx comes
        outputs.trajectory_integrals(case["Vr"], case["rom"], fn, lift=lift, length=case["length"].T)
    with pytest.raises(ValueError):
        outputs.trajectory_integrals(case["Vr"], case["rom"], fn, lift=lift, length=case["length"][:, :21])
    with pytest.raises(ValueError):                                  # one row of lengths for five trajectories
        outputs.trajectory_integrals(case["Vr"], case["rom"], fn, lift=lift, length=case["length"][0])
    with pytest.raises(ValueError):
        outputs.probes(case["Vr"], case["rom"], [0.0], case["length"].T, lift=lift)
    with pytest.raises(ValueError):
        outputs.probes(case["Vr"], case["rom"], [0.0], None, lift=lift)
    with pytest.raises(ValueError):
        outputs.probes(case["Vr"], case["rom"], [[0.0, 1.0]], case["length"], lift=lift)
    with pytest.raises(ValueError):                                  # four parameter points for five trajectories
        outputs.mass_conservation(case["Vr"], case["rom"], case["mus"][:4], case["dt"], case["length"], lift=lift)
    with pytest.raises(ValueError):                                  # uN of the wrong width
        outputs.mass_conservation(case["Vs"], case["rom"], case["mus"], case["dt"], case["length"], lift=lift)
    with pytest.raises(ValueError):
        outputs.mass_conservation(case["Vr"], case["rom"], case["mus"], case["dt"], case["length"], lift=lift, ts=case["ts"][:5])
    with pytest.raises(ValueError):
        outputs.snapshot_mass_conservation(case["U"][1], case["mus"][1], case["dt"], case["length"][1][:21])
    with pytest.raises(ValueError):
        outputs.density(1.0)
    assert outputs.trajectory_integrals(case["Vr"], case["rom"], fn, lift=lift).shape == (5, 22)   # no length: the unit domain


def test_premise_of_the_nan_isolation_case():
    """In the truth of ``nan_case`` exactly one step is NaN (and the restatement agrees on which)."""
    import torch

    E, w, A, scale, fn = oc.nan_case()
    want = oc.longdouble_integrals(E, w, A[0], scale[0], fn)
    assert np.isnan(want.astype(np.float64)).sum() == 1 and np.isnan(want[7])
    got = oc.numpy_trajectory_integrals(torch.from_numpy(E), torch.from_numpy(A), torch.from_numpy(w), torch.from_numpy(scale), fn).numpy()
    assert np.array_equal(np.isnan(got[0]), np.isnan(want.astype(np.float64)))
    bar = oc.error_bar(E, w, A[0], scale[0], fn)
    ok, ratio = oc.within_bar(got[0], want, bar)
    assert ok and ratio < 0.5, ratio


def test_numpy_stays_far_inside_the_bar_on_rounded_data():
    """NumPy float64 on random cases with every exponent the GPU tests use: a bar that NumPy (correctly rounded sums aside,
    the same arithmetic) nearly touched would be too tight to hold a kernel to."""
    import torch

    for seed, (n_pts, k, nt) in enumerate(((97, 13, 70), (513, 128, 33))):
        E, w, A, scale = oc.rounded_case(seed, n_pts, k, nt)
        for p in oc.EXPONENTS:
            fn = ("power", 1.0, -0.6, p)
            want = oc.longdouble_integrals(E, w, A[0], scale[0], fn)
            bar = oc.error_bar(E, w, A[0], scale[0], fn)
            got = oc.numpy_trajectory_integrals(torch.from_numpy(E), torch.from_numpy(A), torch.from_numpy(w),
                                                torch.from_numpy(scale), fn).numpy()[0]
            ok, ratio = oc.within_bar(got, want, bar)
            rel = float((bar / np.abs(want).astype(np.float64)).max())
            assert ok and ratio < 0.25 and rel < 5e-13, (n_pts, p, ratio, rel)
