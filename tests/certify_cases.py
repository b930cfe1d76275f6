"""Shared pieces of the certification tests (tests/test_certify_cpu.py, tests/test_traj_errors_gpu.py): a NumPy
restatement of ``ops.trajectory_errors``, an extended-precision reference, the derived error bar, the dispatch rule of
rt_trajectory_errors restated, and the piston case of tests/golden/hrom.npz.  Plain module, not a conftest."""
import numpy as np
import torch

U_ROUND = 2.0 ** -53
RUNS = [("validation", 0), ("validation", 1), ("validation", 2), ("online", 0), ("online", 1)]


def numpy_trajectory_errors(B, A, U=None, want_ref=False):
    """What ops.trajectory_errors computes, with NumPy on CPU tensors (monkeypatched over it in the host-logic tests)."""
    Bn = B.numpy()
    An = A.numpy() if A.dim() == 3 else A.numpy()[None]
    Un = None if U is None else (U.numpy() if U.dim() == 3 else U.numpy()[None])
    N = Bn.shape[0]
    err, ref = np.empty(An.shape[:2]), np.empty(An.shape[:2])
    for j in range(An.shape[0]):
        lifted = Bn @ An[j].T
        res = lifted if Un is None else Un[j] - lifted
        err[j] = np.sqrt(np.sum(res * res, axis=0)) / np.sqrt(N)
        if want_ref:
            ref[j] = np.sqrt(np.sum(Un[j] * Un[j], axis=0)) / np.sqrt(N)
    return (torch.from_numpy(err), torch.from_numpy(ref)) if want_ref else torch.from_numpy(err)


def longdouble_errors(B, a, U=None):
    """err (nt) of one trajectory a (nt x k) in np.longdouble."""
    lifted = B.astype(np.longdouble) @ a.T.astype(np.longdouble)
    res = lifted if U is None else U.astype(np.longdouble) - lifted
    return np.sqrt(np.sum(res * res, axis=0)) / np.sqrt(np.longdouble(B.shape[0]))


def error_bar(B, a, U, err):
    """Twice [(k + 2) u || |B| |a_t| ||_2 + u ||U_t||_2] / sqrt(N) + (N / 2 + 3) u err_t, per step: the standard bound
    for a length-k dot product in any order, one subtraction and a sum of N non-negative terms (u = 2^-53)."""
    N, k = B.shape
    mag = np.linalg.norm(np.abs(B) @ np.abs(a).T, axis=0)
    un = 0.0 if U is None else np.linalg.norm(U, axis=0)
    return 2.0 * (((k + 2) * U_ROUND * mag + U_ROUND * un) / np.sqrt(N) + (N / 2 + 3) * U_ROUND * np.asarray(err))


def _cdiv(a, b):
    return -(-a // b)


def trajectory_errors_plan(N, nt, n_traj, cus):
    """launch_info of rt_trajectory_errors (traj_error.hip): workgroups of 64 steps walking row slices in 32-row stages."""
    step_blocks = _cdiv(nt, 64)
    slices = max(min(_cdiv(4 * cus, step_blocks), _cdiv(N, 1024)), 1)
    slice_rows = _cdiv(_cdiv(N, slices), 32) * 32
    slices = _cdiv(N, slice_rows)
    return dict(grid=step_blocks * slices * n_traj, splits=slices, tile=(32, 64))


def piston_case(g):
    """The five runs of tests/golden/hrom.npz as ``certify.evaluate`` takes them: S-ROM basis (61 x 6), ROM basis = its
    first 4 columns, reduced trajectories (5, 22, r), the lifting as ramp x amplitude (the amplitude is the last row of
    rom_uh - V rom_uN: the homogeneous part vanishes at the piston), the one FOM trajectory the fixture holds."""
    Vs = g["srom_basis"]
    Vr = Vs[:, :4]
    ramp = np.arange(61) / 60.0
    rom, srom, amp = [], [], []
    for which, i in RUNS:
        uN = g[f"rom_uN__{which}__{i}"]                       # (r, nt), as solutions.rom stores it
        rom.append(uN.T)
        srom.append(g[f"srom_uN__{which}__{i}"].T)
        amp.append((g[f"rom_uh__{which}__{i}"] - Vr @ uN)[-1])
    U = [None, g["validation_solution_1"], None, None, None]
    return dict(Vs=Vs, Vr=Vr, ramp=ramp, rom=np.array(rom), srom=np.array(srom), amp=np.array(amp), U=U)


def check_piston_payload(g, payload):
    """certify.evaluate's payload for ``piston_case`` against the curves the reference's driver recorded."""
    from romtime_amd.conventions import Errors

    case = piston_case(g)
    Vs, Vr, ramp = case["Vs"], case["Vr"], case["ramp"]
    assert len(payload) == len(RUNS)
    worst = 0.0
    for j, (which, i) in enumerate(RUNS):
        d = case["srom"][j].copy()
        d[:, :4] -= case["rom"][j]
        want = g[f"errors__{which}__{i}__estimator"]
        got = payload[j][Errors.ESTIMATOR]
        bar = error_bar(Vs, d, None, want)
        worst = max(worst, float(np.max(np.abs(got - want) / bar)))
        assert got.shape == want.shape and np.all(np.abs(got - want) <= bar), (which, i, np.abs(got - want).max(), bar.min())
        if case["U"][j] is None:
            assert set(payload[j]) == {Errors.ESTIMATOR}
            continue
        assert set(payload[j]) == {Errors.ESTIMATOR, Errors.ROM, Errors.SACRIFICIAL}
        for key, V, a in ((Errors.ROM, Vr, case["rom"][j]), (Errors.SACRIFICIAL, Vs, case["srom"][j])):
            want = g[f"errors__{which}__{i}__{key}"]
            got = payload[j][key]
            bar = error_bar(np.column_stack([V, ramp]), np.column_stack([a, case["amp"][j]]), case["U"][j], want)
            worst = max(worst, float(np.max(np.abs(got - want) / bar)))
            assert got.shape == want.shape and np.all(np.abs(got - want) <= bar), (key, np.abs(got - want).max(), bar.min())
    return worst
