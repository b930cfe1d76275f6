"""Host logic of romtime_amd.certify (zero-padding to the S-ROM's size, lifting columns, layouts of uN, payload keys,
argument errors) with the device operators stubbed: ``cpu_ops`` plus a NumPy restatement of ``ops.trajectory_errors``.
The data are the reference driver's own run, tests/golden/hrom.npz; the bar is the derived one of
tests/certify_cases.py::error_bar."""
import numpy as np
import pytest

from tests import certify_cases as cc


@pytest.fixture
def certify(cpu_ops, monkeypatch):
    from romtime_amd import certify, ops

    monkeypatch.setattr(ops, "trajectory_errors", cc.numpy_trajectory_errors)
    return certify


@pytest.fixture(scope="module")
def golden_hrom():
    from tests.conftest import load_golden

    return load_golden("hrom.npz")


def test_evaluate_reproduces_the_reference_drivers_curves(certify, golden_hrom):
    case = cc.piston_case(golden_hrom)
    payload = certify.evaluate(case["Vr"], case["rom"], case["Vs"], case["srom"], case["U"], lift=(case["ramp"], case["amp"]))
    worst = cc.check_piston_payload(golden_hrom, payload)
    print(f"certify.evaluate vs the reference's curves: worst |difference| / bar = {worst:.3f}")


def test_layouts_of_uN_and_U_give_the_same_numbers(certify, golden_hrom):
    """(nt, r) and (n_mu, nt, r) coefficients, transposed views of (r, nt) storage, C- and F-ordered snapshots, tensors
    and arrays: one answer."""
    import torch

    case = cc.piston_case(golden_hrom)
    U, lift1 = case["U"][1], (case["ramp"], case["amp"][1:2])
    base = certify.trajectory_errors(case["Vr"], case["rom"][1], U, lift=lift1)
    assert base.shape == (1, 22)
    stored = np.ascontiguousarray(case["rom"][1].T)                      # (r, nt) as solutions.rom holds it
    for uN in (stored.T, case["rom"][1:2], torch.from_numpy(np.ascontiguousarray(case["rom"][1]))):
        for Uj in (np.ascontiguousarray(U), np.asfortranarray(U), [torch.from_numpy(np.ascontiguousarray(U))]):
            np.testing.assert_array_equal(certify.trajectory_errors(case["Vr"], uN, Uj, lift=lift1), base)
    lift3 = (case["ramp"][:, None], case["amp"][1:2, :, None])         # N x q shapes with n_mu x nt x q coefficients
    np.testing.assert_array_equal(certify.trajectory_errors(case["Vr"], case["rom"][1], U, lift=lift3), base)
    rel = certify.trajectory_errors(case["Vr"], case["rom"][1], U, lift=lift1, relative=True)
    ref = np.linalg.norm(U, axis=0) / np.sqrt(61)
    np.testing.assert_allclose(rel[0, 1:], base[0, 1:] / ref[1:], rtol=1e-14)
    est = certify.rom_difference(case["rom"], case["srom"], case["Vs"])
    assert est.shape == (5, 22)
    np.testing.assert_array_equal(est[1], certify.rom_difference(case["rom"][1], case["srom"][1], case["Vs"])[0])


def test_projection_errors_is_the_best_approximation(certify, golden_hrom):
    case = cc.piston_case(golden_hrom)
    Q, _ = np.linalg.qr(case["Vs"])
    U = case["U"][1]
    want = np.linalg.norm(U - Q @ (Q.T @ U), axis=0) / np.sqrt(61)
    got = certify.projection_errors(Q, U)
    assert got.shape == (22,)
    assert np.all(np.abs(got - want) <= cc.error_bar(Q, (Q.T @ U).T, U, want))
    assert certify.projection_errors(Q, [U, U]).shape == (2, 22)
    inside = certify.projection_errors(Q, Q @ (Q.T @ U))
    assert np.all(inside <= cc.error_bar(Q, (Q.T @ U).T, U, 0.0))


def test_argument_errors(certify, golden_hrom):
    case = cc.piston_case(golden_hrom)
    rng = np.random.RandomState(0)
    V = rng.standard_normal((61, 127))
    uN = rng.standard_normal((2, 22, 127))
    with pytest.raises(ValueError, match="at most 128"):               # r + q = 129
        certify.trajectory_errors(V, uN, lift=(rng.standard_normal((61, 2)), rng.standard_normal((2, 22, 2))))
    assert certify.trajectory_errors(V, uN, lift=(case["ramp"], rng.standard_normal((2, 22)))).shape == (2, 22)   # 128 is fine
    with pytest.raises(ValueError):                                     # snapshots with another nt
        certify.trajectory_errors(case["Vr"], case["rom"][1], case["U"][1][:, :21])
    with pytest.raises(ValueError):                                     # lifting coefficients with another nt
        certify.trajectory_errors(case["Vr"], case["rom"][1], case["U"][1], lift=(case["ramp"], case["amp"][1:2, :21]))
    with pytest.raises(ValueError):                                     # S-ROM trajectories with another nt
        certify.rom_difference(case["rom"], case["srom"][:, :21], case["Vs"])
    with pytest.raises(ValueError):                                     # one snapshot matrix for five trajectories
        certify.trajectory_errors(case["Vr"], case["rom"], case["U"][1])
    with pytest.raises(ValueError, match="relative"):
        certify.trajectory_errors(case["Vr"], case["rom"][1], relative=True)
    with pytest.raises(ValueError):                                     # uN of the wrong width
        certify.trajectory_errors(case["Vs"], case["rom"][1])
