"""rt_trajectory_errors and romtime_amd.certify on the device.

Exact cases: integer data (6-bit B and A, U below 2^17) whose residuals and column sums are exact below 2^53, operands
in NaN-poisoned guarded buffers, outputs in canary buffers (tests/guarded.py): err and ref equal
np.sqrt(S) / np.sqrt(N) bit for bit, each case asserts its route from rt_last_launch_info, and a trajectory's bits are
the same alone and in a batch.  Rounded data, the reference driver's recorded curves and the class-level flow are held to
the derived bar of tests/certify_cases.py::error_bar."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import certify_cases as cc
from tests import guarded as gd
from tests.guarded import exact_operands, guarded_operand, guarded_output

pytestmark = pytest.mark.gpu
LAY = {"C": 0, "F": 1}
GAP = 3            # poisoned lines between the trajectories of a batch


@pytest.fixture(scope="module")
def ctx():
    from romtime_amd._lib import Context

    return Context.current()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _stacked(blocks, axis):
    """The blocks of a batch in one matrix, GAP lines of NaN between them (a kernel that strays reads poison)."""
    rows, cols = blocks[0].shape
    n = len(blocks)
    shape = (n * (rows + GAP), cols) if axis == 0 else (rows, n * (cols + GAP))
    host = np.full(shape, np.nan)
    for j, b in enumerate(blocks):
        if axis == 0:
            host[j * (rows + GAP): j * (rows + GAP) + rows] = b
        else:
            host[:, j * (cols + GAP): j * (cols + GAP) + cols] = b
    return host


def _exact_sums(Bh, As, Us):
    """(S_err, S_ref) per trajectory, exact: every term an integer, every sum below 2^53."""
    se, sr = [], []
    for j, a in enumerate(As):
        lifted = Bh @ a.T
        res = lifted if Us is None else Us[j] - lifted
        se.append(np.sum(res * res, axis=0))
        sr.append(None if Us is None else np.sum(Us[j] * Us[j], axis=0))
        assert se[-1].max() < 2.0 ** 53 and np.abs(res).max() < 2.0 ** 26
    return se, sr


def _run_guarded(ctx, Bh, As, Us, layout, pads, misalign, want_ref=True):
    """One call on guarded operands; returns (err, ref) as host arrays (n_traj x nt) after checking guards and canaries."""
    N, k = Bh.shape
    nt, n = As[0].shape[0], len(As)
    pb, pa, pu = pads
    Bd = guarded_operand(Bh, "C", pb, misalign)
    Ah = _stacked(As, 0)
    Ad = guarded_operand(Ah, "C", pa, misalign)
    lda = k + pa
    Ud, Uh, ldu, su = None, None, 0, 0
    if Us is not None:
        if layout == "C":                                  # N x nt row-major blocks one under the other
            Uh = _stacked(Us, 0)
            Ud = guarded_operand(Uh, "C", pu, misalign)
            ldu = nt + pu
            su = (N + GAP) * ldu
        else:                                              # column-major: each snapshot contiguous, blocks side by side
            Uh = _stacked(Us, 1)
            Ud = guarded_operand(Uh, "F", pu, misalign)
            ldu = N + pu
            su = (nt + GAP) * ldu
    err = guarded_output((n, nt))
    ref = guarded_output((n, nt)) if (want_ref and Us is not None) else None
    rc = ctx.lib.rt_trajectory_errors(ctx.handle, P(Bd), k + pb, P(Ad), lda, (nt + GAP) * lda, P(Ud), ldu, LAY.get(layout, 0),
                                      su, N, k, nt, n, P(err.t), P(ref.t) if ref else None)
    ctx.check(rc, "rt_trajectory_errors")
    torch.cuda.synchronize()
    for o in (err, ref):
        if o is not None:
            assert o.check() == [], o.check()
    for v, h in ((Bd, Bh), (Ad, Ah), (Ud, Uh)):
        if v is not None:
            assert gd.operand_intact(v, h) == [], gd.operand_intact(v, h)
    return err.t.cpu().numpy(), (ref.t.cpu().numpy() if ref else None)


EXACT_CASES = [
    # id, N, nt, k, layout of U ("C" row-major, "F" column-major, None absent), (ldb, lda, ldu) padding, misaligned, n_traj
    ("one_step_one_column", 61, 1, 1, "F", (0, 0, 0), False, 1),
    ("piston_size_lifting_column", 61, 22, 5, "F", (0, 0, 0), False, 3),
    ("k4_rowmajor", 129, 65, 4, "C", (0, 0, 0), False, 1),
    ("k6_padded_rowmajor_batch", 129, 22, 6, "C", (1, 3, 5), False, 3),
    ("k17_odd_lds_misaligned", 1003, 130, 17, "F", (2, 2, 1), True, 1),
    ("k17_rowmajor_misaligned_batch", 129, 130, 17, "C", (0, 1, 2), True, 3),
    ("k80_sweep_width", 1003, 65, 80, "F", (0, 0, 0), False, 3),
    ("k80_rowmajor_padded", 1003, 22, 80, "C", (3, 0, 1), False, 1),
    ("k128_widest", 1003, 130, 128, "F", (0, 0, 3), False, 1),
    ("k128_rowmajor_misaligned", 129, 65, 128, "C", (1, 1, 1), True, 3),
    ("estimator_no_U", 1003, 130, 6, None, (0, 0, 0), False, 3),
    ("estimator_no_U_k80_misaligned", 129, 1, 80, None, (1, 1, 0), True, 1),
    ("estimator_no_U_k128", 61, 65, 128, None, (0, 2, 0), False, 1),
    ("row_slices_colmajor", 40_001, 70, 24, "F", (0, 0, 1), False, 1),
    ("row_slices_rowmajor_batch", 40_000, 70, 24, "C", (2, 0, 0), False, 3),
]


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_trajectory_errors_exact_guarded(ctx, cus, case):
    _, N, nt, k, layout, pads, misalign, n = case
    rng = np.random.default_rng(N * 1_000_003 + nt * 1009 + k * 31 + n)
    Bh = exact_operands(rng, (N, k), 6, k=k)
    As = [exact_operands(rng, (nt, k), 6, k=k) for _ in range(n)]
    Us = None if layout is None else [exact_operands(rng, (N, nt), 16) for _ in range(n)]
    se, sr = _exact_sums(Bh, As, Us)
    err, ref = _run_guarded(ctx, Bh, As, Us, layout, pads, misalign)
    plan = cc.trajectory_errors_plan(N, nt, n, cus)
    assert ctx.launch_info() == plan, (ctx.launch_info(), plan)
    assert (plan["splits"] > 1) == (N >= 40_000)
    for j in range(n):
        want = np.sqrt(se[j]) / np.sqrt(float(N))
        assert gd.bits_equal(err[j], want), (j, gd.mismatch(err[j], want))
        if Us is not None:
            want = np.sqrt(sr[j]) / np.sqrt(float(N))
            assert gd.bits_equal(ref[j], want), (j, gd.mismatch(ref[j], want))
    if n > 1:                                              # the last trajectory alone: the same bits as in the batch
        alone, alone_ref = _run_guarded(ctx, Bh, As[-1:], None if Us is None else Us[-1:], layout, pads, misalign)
        assert ctx.launch_info() == cc.trajectory_errors_plan(N, nt, 1, cus)
        assert gd.bits_equal(alone[0], err[-1])
        assert Us is None or gd.bits_equal(alone_ref[0], ref[-1])
        only_err, none = _run_guarded(ctx, Bh, As, Us, layout, pads, misalign, want_ref=False)   # ref == NULL
        assert none is None and gd.bits_equal(only_err, err)


def test_return_codes(ctx):
    B = torch.zeros((64, 129), dtype=torch.float64, device="cuda")
    A = torch.zeros((8, 129), dtype=torch.float64, device="cuda")
    U = torch.zeros((64, 8), dtype=torch.float64, device="cuda")
    out, ref = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
    call = lambda N, k, nt, n, u, r: ctx.lib.rt_trajectory_errors(ctx.handle, P(B), 129, P(A), 129, 8 * 129, P(u), 8, 0, 64 * 8,
                                                                  N, k, nt, n, P(out), P(r))
    assert call(64, 129, 8, 1, U, ref) == -3               # RT_ERR_UNSUPPORTED
    assert call(64, 128, 8, 1, U, ref) == 0
    assert call(64, 128, 8, 1, None, None) == 0
    assert call(64, 128, 8, 1, None, ref) == -1            # ref without U
    for bad in ((0, 4, 8, 1), (64, 0, 8, 1), (64, 4, 0, 1), (64, 4, 8, 0), (-1, 4, 8, 1)):
        assert call(*bad, U, ref) == -1, bad
    torch.cuda.synchronize()
    from romtime_amd import ops
    from romtime_amd._lib import RomtimeHipError

    with pytest.raises(RomtimeHipError):
        ops.trajectory_errors(B, A, U)                     # k = 129 through the wrapper: an error, no other route


def test_rounded_data_within_the_derived_bar(ctx):
    """U = B a + 1e-9 noise: an error far below ||U||, so the cancellation in U - B a is what is measured."""
    from romtime_amd import ops

    N, nt, k = 1003, 65, 80
    rng = np.random.default_rng(7)
    Bh = rng.standard_normal((N, k))
    a = rng.standard_normal((nt, k))
    for layout in ("C", "F"):
        Uh = Bh @ a.T + 1e-9 * rng.standard_normal((N, nt))
        Ud = ops.to_device(np.asfortranarray(Uh) if layout == "F" else Uh)
        err, ref = ops.trajectory_errors(ops.to_device(Bh), ops.to_device(a), Ud, want_ref=True)
        err, ref = err.cpu().numpy()[0], ref.cpu().numpy()[0]
        want = cc.longdouble_errors(Bh, a, Uh)
        bar = cc.error_bar(Bh, a, Uh, want.astype(np.float64))
        diff = np.abs(err.astype(np.longdouble) - want).astype(np.float64)
        print(f"rounded data, U {layout}: err ~ {float(want.mean()):.2e}, worst |difference| / bar = {float((diff / bar).max()):.2e}")
        assert np.all(diff <= bar), (layout, float((diff / bar).max()))
        want_ref = np.linalg.norm(Uh.astype(np.longdouble), axis=0) / np.sqrt(np.longdouble(N))
        assert np.all(np.abs(ref - want_ref) <= 2 * (N / 2 + 3) * cc.U_ROUND * want_ref.astype(np.float64))


@pytest.fixture(scope="module")
def golden_hrom():
    from tests.conftest import load_golden

    return load_golden("hrom.npz")


def test_evaluate_reproduces_the_reference_drivers_curves_on_the_device(ctx, cus, golden_hrom):
    from romtime_amd import certify

    case = cc.piston_case(golden_hrom)
    payload = certify.evaluate(case["Vr"], case["rom"], case["Vs"], case["srom"], case["U"], lift=(case["ramp"], case["amp"]))
    assert ctx.launch_info() == cc.trajectory_errors_plan(61, 22, 1, cus)      # the last call: S-ROM against the FOM run
    worst = cc.check_piston_payload(golden_hrom, payload)
    print(f"certify.evaluate on the device vs the reference's curves: worst |difference| / bar = {worst:.3f}")
    rel = certify.trajectory_errors(case["Vr"], case["rom"][1], case["U"][1], lift=(case["ramp"], case["amp"][1:2]), relative=True)
    ref = np.linalg.norm(case["U"][1], axis=0) / np.sqrt(61)
    np.testing.assert_allclose(rel[0, 1:] * ref[1:], payload[1]["rom"][1:], rtol=1e-13)


@pytest.fixture(scope="module")
def swept_pair():
    """ROM (r = 20) and S-ROM (r = 24) trajectories of the device sweep on a small hyper-reduced model, and FOM-space
    trajectories lifted on the host."""
    from romtime_amd.sweep import hrom_bdf_sweep
    from romtime_amd.testing.workloads import c5_hyper_reduced

    out = {}
    for name, r in (("rom", 20), ("srom", 24)):
        terms, _, V, _ = c5_hyper_reduced(N=3000, nt=40, n_mu=3, r=r)
        uN = hrom_bdf_sweep(terms["mass"], terms["lin"], terms["nl"], terms["rhs"], terms["dt"], bdf2=True)
        out[name] = (V, uN)
    rng = np.random.default_rng(3)
    Vs, uNs = out["srom"]
    out["U"] = [Vs @ uNs[j].cpu().numpy().T + 1e-7 * rng.standard_normal((3000, 40)) for j in range(3)]
    return out


def test_evaluate_on_sweep_output_matches_the_host_loop(swept_pair):
    """certify.evaluate takes the sweeps' (n_mu, nt, r) device tensors as they are; the host loop of
    utils.compute_error / compute_rom_difference (tests/test_hrom_flow.py's evaluate) is the reference."""
    from romtime_amd import certify
    from romtime_amd.conventions import Errors
    from romtime_amd.utils import compute_error, compute_rom_difference

    (Vr, uNr), (Vs, uNs), U = swept_pair["rom"], swept_pair["srom"], swept_pair["U"]
    assert uNr.is_cuda and tuple(uNr.shape) == (3, 40, 20) and tuple(uNs.shape) == (3, 40, 24)
    payload = certify.evaluate(Vr, uNr, Vs, uNs, [U[0], np.asfortranarray(U[1]), torch.from_numpy(U[2]).cuda()])
    hr, hs = uNr.cpu().numpy(), uNs.cpu().numpy()
    for j in range(3):
        d = hs[j].copy()
        d[:, :20] -= hr[j]
        host = {Errors.ESTIMATOR: np.array([compute_rom_difference(hr[j, t], hs[j, t], Vs) for t in range(40)]),
                Errors.ROM: np.array([compute_error(U[j][:, t], Vr @ hr[j, t]) for t in range(40)]),
                Errors.SACRIFICIAL: np.array([compute_error(U[j][:, t], Vs @ hs[j, t]) for t in range(40)])}
        bars = {Errors.ESTIMATOR: cc.error_bar(Vs, d, None, host[Errors.ESTIMATOR]),
                Errors.ROM: cc.error_bar(Vr, hr[j], U[j], host[Errors.ROM]),
                Errors.SACRIFICIAL: cc.error_bar(Vs, hs[j], U[j], host[Errors.SACRIFICIAL])}
        assert set(payload[j]) == set(host)
        for key in host:
            diff = np.abs(payload[j][key] - host[key])
            assert np.all(diff <= bars[key]), (j, key, float((diff / bars[key]).max()))
        assert host[Errors.ESTIMATOR].max() > 0 and host[Errors.ROM].max() > host[Errors.SACRIFICIAL].max() > 0


def test_projection_of_a_vector_in_the_span_is_zero_to_the_bar(swept_pair):
    from romtime_amd import certify

    Vs, uNs = swept_pair["srom"]
    c = uNs[0].cpu().numpy()                               # (nt, r)
    inside = Vs @ c.T
    got = certify.projection_errors(Vs, inside)
    assert got.shape == (40,)
    bar = cc.error_bar(Vs, c, inside, 0.0)
    print(f"projection of vectors in the span: worst err / bar = {float((got[1:] / bar[1:]).max()):.3f}")
    assert np.all(got <= bar), float(got.max())
    U = swept_pair["U"][1]
    want = np.linalg.norm(U - Vs @ (Vs.T @ U), axis=0) / np.sqrt(3000)
    assert np.all(np.abs(certify.projection_errors(Vs, U) - want) <= cc.error_bar(Vs, (Vs.T @ U).T, U, want))
