"""Shared pieces of the output tests (tests/test_outputs_cpu.py, tests/test_outputs_gpu.py): a NumPy restatement of
``ops.trajectory_integrals``, the same formula in extended precision, the derived error bar, the launch plan of
rt_trajectory_integrals restated, and the piston case of tests/golden/hrom.npz with a moving domain.  Plain module, not a
conftest."""
import warnings

import numpy as np
import torch

from tests.certify_cases import RUNS, _cdiv, piston_case

U_ROUND = 2.0 ** -53
POW_ULPS = 4.0        # rho of the bar: two ulps of the device pow.  Assumed: ROCm's accuracy table is not in this tree.
EXPONENTS = (5.000000000000001, -1.0, 7.000000000000001)


def numpy_trajectory_integrals(E, A, w=None, scale=None, fn=("power", 0.0, 1.0, 1.0)):
    """What ops.trajectory_integrals computes, with NumPy on CPU tensors (monkeypatched over it in the host-logic tests)."""
    kind, c0, c1, p = fn
    assert kind == "power"
    En = E.numpy()
    An = A.numpy() if A.dim() == 3 else A.numpy()[None]
    wn = np.ones(En.shape[0]) if w is None else w.numpy()
    out = np.empty(An.shape[:2])
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(An.shape[0]):
            out[j] = np.sum(wn[:, None] * (c0 + c1 * (En @ An[j].T)) ** p, axis=0)
    if scale is not None:
        out = out * scale.numpy().reshape(out.shape)
    return torch.from_numpy(out)


def longdouble_products(E, a):
    """z = E a^T (n_pts x nt) in np.longdouble: the part of the truth that does not depend on fn."""
    return E.astype(np.longdouble) @ a.T.astype(np.longdouble)


def longdouble_integrals(E, w, a, scale, fn, z=None):
    """out (nt) of one trajectory a (nt x k) in np.longdouble, on the float64 E, w, a and scale the device receives
    (``z``: longdouble_products(E, a) where several fn share it)."""
    _, c0, c1, p = fn
    ld = np.longdouble
    z = longdouble_products(E, a) if z is None else z
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = (ld(c0) + ld(c1) * z) ** ld(p)
    wl = np.ones(E.shape[0], dtype=ld) if w is None else w.astype(ld)
    s = np.sum(wl[:, None] * f, axis=0)
    return s if scale is None else s * np.asarray(scale).astype(ld)


def error_bar(E, w, a, scale, fn, rho=POW_ULPS):
    """Per step, with u = 2^-53, z = E a, b = c0 + c1 z:
        dz = (k + 2) u |E||a|                       a length-k dot product in any order
        db = |c1| dz + 2 u (|c0| + |c1 z|)          the base, fused or not
        df = |p| |b|^(p-1) db + rho u |b|^p         the power's condition, and rho / 2 ulps of pow itself
        bar = 2 [sum |w| df + (n_pts / 2 + 3) u sum |w| |b|^p] |scale|      a sum of n_pts terms in any order"""
    _, c0, c1, p = fn
    n_pts, k = E.shape
    z = E @ a.T
    dz = (k + 2) * U_ROUND * (np.abs(E) @ np.abs(a).T)
    b = c0 + c1 * z
    db = abs(c1) * dz + 2 * U_ROUND * (abs(c0) + np.abs(c1 * z))
    with np.errstate(invalid="ignore", divide="ignore"):
        fp = np.abs(b) ** p
        df = abs(p) * np.abs(b) ** (p - 1) * db + rho * U_ROUND * fp
    wa = np.ones(n_pts) if w is None else np.abs(w)
    bar = 2.0 * (wa @ df + (n_pts / 2 + 3) * U_ROUND * (wa @ fp))
    return bar if scale is None else bar * np.abs(scale)


def within_bar(got, want, bar):
    """(ok, worst ratio): every step within its bar, NaN steps of ``want`` excluded (they are compared by isnan)."""
    keep = ~np.isnan(np.asarray(want, dtype=np.float64))
    diff = np.abs(np.asarray(got, dtype=np.longdouble) - want).astype(np.float64)
    ratio = diff[keep] / bar[keep]
    return bool(np.all(diff[keep] <= bar[keep])), float(ratio.max()) if ratio.size else 0.0


def trajectory_integrals_plan(n_pts, nt, n_traj, cus):
    """launch_info of rt_trajectory_integrals (traj_output.hip): rt_trajectory_errors' slicing over the quadrature rows."""
    step_blocks = _cdiv(nt, 64)
    slices = max(min(_cdiv(4 * cus, step_blocks), _cdiv(n_pts, 1024)), 1)
    slice_rows = _cdiv(_cdiv(n_pts, slices), 32) * 32
    slices = _cdiv(n_pts, slice_rows)
    return dict(grid=step_blocks * slices * n_traj, splits=slices, tile=(32, 64))


def rounded_case(seed, n_pts, k, nt, n_traj=1):
    """E, w, A, scale with the base 1 + c1 z inside (0.4, 1.6): every exponent of EXPONENTS is well defined."""
    rng = np.random.default_rng(seed)
    E = rng.uniform(-1.0, 1.0, (n_pts, k))
    A = rng.uniform(-1.0, 1.0, (n_traj, nt, k)) / k
    w = rng.uniform(0.5, 1.5, n_pts) / n_pts
    scale = rng.uniform(0.8, 1.3, (n_traj, nt))
    return E, w, A, scale


def nan_case():
    """One step (the 8th of 70) whose base goes negative in some rows: p = 5.000000000000001 makes that step NaN."""
    E, w, A, scale = rounded_case(5, 97, 13, 70)
    A[0, 7] = 0.0
    A[0, 7, 0] = 3.0                                       # base 1 - 0.6 * 3 E[:, 0]: negative where E[:, 0] > 0.56
    return E, w, A, scale, ("power", 1.0, -0.6, EXPONENTS[0])


def piston_outputs_case(g):
    """``certify_cases.piston_case`` plus what the outputs need: a0 per run, the time step, and a moving domain
    L(mu, t) = 1 - delta (1 - cos(omega t)) / 2 - positive and different for every run and step (the fixture does not record
    the lengths its driver used; any positive L tests the same arithmetic)."""
    case = piston_case(g)
    mus = np.vstack([g["offline_mus"], g["online_mus"]])           # columns a0, omega, delta, alpha_0; rows in RUNS' order
    assert len(mus) == len(RUNS)
    nt = case["rom"].shape[1]
    dt = 0.25
    ts = dt * np.arange(nt)
    case["a0"] = mus[:, 0].copy()
    case["mus"] = [{"a0": float(m[0]), "omega": float(m[1]), "delta": float(m[2])} for m in mus]
    case["dt"], case["ts"] = dt, ts
    case["length"] = 1.0 - 0.5 * mus[:, 2:3] * (1.0 - np.cos(mus[:, 1:2] * ts[None, :]))
    assert case["length"].shape == (len(RUNS), nt) and case["length"].min() > 0.1
    return case


def host_quadrature(B, points):
    """quadrature_basis restated in NumPy."""
    x, gw = np.polynomial.legendre.leggauss(points)
    xi, gw = 0.5 * (x + 1.0), 0.5 * gw
    nx = B.shape[0] - 1
    E = np.vstack([(1.0 - q) * B[:-1] + q * B[1:] for q in xi])
    w = np.concatenate([np.full(nx, q / nx) for q in gw])
    return E, w


def check_piston_mass(case, payload, gamma=1.4, points=2):
    """mass_conservation's payload for ``piston_outputs_case`` against the extended-precision truth and the payload's own
    rules; returns the worst |difference| / bar of the mass."""
    from romtime_amd import outputs
    from romtime_amd.conventions import MassConservation as MC

    fn = outputs.density(gamma)
    B = np.column_stack([case["Vr"], case["ramp"]])
    E, w = host_quadrature(B, points)
    assert len(payload) == len(RUNS)
    worst = 0.0
    for j in range(len(RUNS)):
        a = np.column_stack([case["rom"][j], case["amp"][j]])
        entry = payload[j]
        assert set(entry) == {MC.WHICH, MC.TIMESTEPS, MC.MASS, MC.MASS_CHANGE, MC.OUTFLOW}
        assert entry[MC.WHICH] == "rom" and np.array_equal(entry[MC.TIMESTEPS], case["ts"])
        want = longdouble_integrals(E, w, a, case["length"][j], fn)
        bar = error_bar(E, w, a, case["length"][j], fn)
        ok, ratio = within_bar(entry[MC.MASS], want, bar)
        worst = max(worst, ratio)
        assert entry[MC.MASS].shape == (a.shape[0],) and ok, (j, ratio)
        assert 1e-14 < float((bar / np.abs(want).astype(np.float64)).max()) < 5e-13
        np.testing.assert_array_equal(entry[MC.MASS_CHANGE], np.gradient(entry[MC.MASS], case["dt"], edge_order=2))
        u0 = a @ B[0]
        np.testing.assert_allclose(entry[MC.OUTFLOW], case["a0"][j] * (fn[1] + fn[2] * u0) ** fn[3] * u0, rtol=1e-13)
    return worst

