"""rt_interpolation_errors and romtime_amd.interpolation on the device.

Exact cases (tests/interp_cases.py::EXACT_CASES): integer Psi and F whose interpolants, residuals and column sums are exact
below 2^53, operands in NaN-poisoned guarded buffers, outputs in canary buffers (tests/guarded.py): err and ref equal NumPy
bit for bit, and each case asserts its launch plan.  Random data are held to the bar of tests/interp_cases.py against the
long-double truth; a snapshot's bits are the same alone, in a block, at another place, in chunks and under grouping.  The
premises of every fixture are checked on the CPU (tests/test_interpolation_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from romtime_amd import interpolation as _feature  # noqa: F401  (without the feature nothing here can run)
from tests import guarded as gd
from tests import interp_cases as ic
from tests.guarded import guarded_operand, guarded_output

pytestmark = pytest.mark.gpu
LAY = {"C": 0, "F": 1}
RT_ERR_ARG, RT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def ctx():
    from romtime_amd._lib import Context

    return Context.current()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _idx(idx):
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    return idx, idx.ctypes.data_as(C.POINTER(C.c_int64))


def _run_guarded(ctx, Psi, idx, F, layout="F", pads=(0, 0), misalign=False, pin=None, group=1, want_ref=True):
    """One call on guarded operands; (err, ref) as host arrays after checking guards and canaries."""
    N, m = Psi.shape
    S = F.shape[1]
    assert all(0 <= int(i) < N for i in idx)                       # no out-of-range index ever reaches a launch
    Pd = guarded_operand(Psi, "C", pads[0], misalign)
    Fd = guarded_operand(F, layout, pads[1], misalign)
    ldf = (S if layout == "C" else N) + pads[1]
    err = guarded_output((S // group,))
    ref = guarded_output((S // group,)) if want_ref else None
    keep, ip = _idx(idx)
    pin_row, pin_value = (-1, 0.0) if pin is None else pin
    rc = ctx.lib.rt_interpolation_errors(ctx.handle, P(Pd), m + pads[0], ip, m, P(Fd), ldf, LAY[layout], N, S, group, pin_row,
                                         float(pin_value), P(err.t), P(ref.t) if ref else None)
    ctx.check(rc, "rt_interpolation_errors")
    torch.cuda.synchronize()
    for o in (err, ref):
        if o is not None:
            assert o.check() == [], o.check()
    for v, h in ((Pd, Psi), (Fd, F)):
        assert gd.operand_intact(v, h) == [], gd.operand_intact(v, h)
    return err.t.cpu().numpy(), (ref.t.cpu().numpy() if ref else None)


@pytest.mark.parametrize("case", ic.EXACT_CASES, ids=[c[0] for c in ic.EXACT_CASES])
def test_exact_data_gives_numpys_bits(ctx, cus, case):
    _, N, S, m, layout, pads, misalign, pin_row, pin_value, group, want_ref = case
    Psi, idx, F = ic.exact_case(case)
    want, want_r = ic.exact_expected(case, Psi, idx, F)
    pin = None if pin_row < 0 else (pin_row, pin_value)
    for lay in (layout, "C" if layout == "F" else "F"):             # the case's layout, then the other one
        err, ref = _run_guarded(ctx, Psi, idx, F, lay, pads, misalign, pin, group, want_ref)
        plan = ic.interpolation_errors_plan(N, S, cus)
        assert ctx.launch_info() == plan, (ctx.launch_info(), plan)
        assert gd.bits_equal(err, want), (lay, gd.mismatch(err, want))
        if want_ref:
            assert gd.bits_equal(ref, want_r), (lay, gd.mismatch(ref, want_r))
    assert (plan["splits"] > 1) == (N > 1024)


def test_ops_wrapper_detects_the_memory_order(ctx):
    from romtime_amd import ops

    case = ic.EXACT_CASES[8]
    _, N, S, m, _, _, _, pin_row, pin_value, group, _ = case
    Psi, idx, F = ic.exact_case(case)
    want, want_r = ic.exact_expected(case, Psi, idx, F)
    Pd = ops.to_device(Psi)
    for Fd in (ops.to_device(F), ops.to_device(np.asfortranarray(F)), guarded_operand(F, "F", 3, True), guarded_operand(F, "C", 1, True)):
        err, ref = ops.interpolation_errors(Pd, idx, Fd, group=group, pin=(pin_row, pin_value), want_ref=True)
        assert gd.bits_equal(err.cpu().numpy(), want) and gd.bits_equal(ref.cpu().numpy(), want_r)
    only = ops.interpolation_errors(guarded_operand(Psi, "C", 5, True), list(idx), ops.to_device(F), group=group, pin=(pin_row, pin_value))
    assert gd.bits_equal(only.cpu().numpy(), want)
    with pytest.raises(ops.RomtimeHipError):
        ops.interpolation_errors(Pd, idx[:-1], ops.to_device(F))
    with pytest.raises(ops.RomtimeHipError):
        ops.interpolation_errors(Pd, idx, ops.to_device(F), group=7)
    with pytest.raises(ops.RomtimeHipError):
        ops.interpolation_errors(Pd, idx, ops.to_device(F), pin=(N, 1.0))
    bad = idx.copy()
    bad[3] = N
    with pytest.raises(ops.RomtimeHipError, match="bad argument"):
        ops.interpolation_errors(Pd, bad, ops.to_device(F))


@pytest.mark.parametrize("case", ic.RANDOM_CASES, ids=[c[0] for c in ic.RANDOM_CASES])
def test_random_data_within_the_bar_of_the_truth(ctx, case):
    c = ic.random_case(case)
    worst = 0.0
    for layout, pads, misalign in (("F", (0, 0), False), ("C", (1, 3), True)):
        err, ref = _run_guarded(ctx, c["Psi"], c["idx"], c["F"], layout, pads, misalign, c["pin"], c["group"], True)
        diff = np.abs(err.astype(np.longdouble) - c["truth"]).astype(np.float64)
        worst = max(worst, float((diff / c["bar"]).max()))
        print(f"{case[0]} {layout}: worst |device - truth| / bar = {float((diff / c['bar']).max()):.3e}")
        assert np.all(diff <= c["bar"]), (layout, float((diff / c["bar"]).max()))
        want_ref = ic.group_mean(np.linalg.norm(c["F"], axis=0) / np.sqrt(float(c["F"].shape[0])), c["group"])
        np.testing.assert_allclose(ref, want_ref, rtol=64 * ic.EPS)


def test_a_snapshots_bits_do_not_depend_on_its_company(ctx):
    """Alone, inside a block of 130, at another place, in two chunks, under grouping, and again."""
    c = ic.random_case(ic.RANDOM_CASES[0])
    Psi, idx, F = c["Psi"], c["idx"], c["F"]
    assert F.shape[1] == 130
    for layout in ("F", "C"):
        run = lambda cols, group=1, pin=(7, 0.25): _run_guarded(ctx, Psi, idx, np.ascontiguousarray(cols), layout, (1, 1), True, pin, group, True)
        whole, whole_ref = run(F)
        again, again_ref = run(F)
        assert gd.bits_equal(whole, again) and gd.bits_equal(whole_ref, again_ref)
        for s in (0, 63, 64, 129):
            alone, alone_ref = run(F[:, s:s + 1])
            assert gd.bits_equal(alone, whole[s:s + 1]) and gd.bits_equal(alone_ref, whole_ref[s:s + 1]), s
        moved, moved_ref = run(np.roll(F, 37, axis=1))
        assert gd.bits_equal(np.roll(whole, 37), moved) and gd.bits_equal(np.roll(whole_ref, 37), moved_ref)
        first, first_ref = run(F[:, :65])
        second, second_ref = run(F[:, 65:])
        assert gd.bits_equal(np.concatenate([first, second]), whole)
        assert gd.bits_equal(np.concatenate([first_ref, second_ref]), whole_ref)
        for g in (5, 130):
            grouped, grouped_ref = run(F, group=g)
            assert gd.bits_equal(grouped, ic.group_mean(whole, g)), g
            assert gd.bits_equal(grouped_ref, ic.group_mean(whole_ref, g)), g
        unpinned, unpinned_ref = run(F, pin=None)
        assert not np.array_equal(unpinned, whole) and gd.bits_equal(unpinned_ref, whole_ref)      # ref never sees the pin


def test_argument_errors_leave_the_output_untouched(ctx):
    """Every refusal comes before any launch: its code is returned and err keeps its canary."""
    N, m, S = 200, 6, 10
    rng = np.random.default_rng(11)
    Pd = guarded_operand(rng.standard_normal((N, m)), "C")
    Fd = guarded_operand(rng.standard_normal((N, S)), "F")
    err, ref = guarded_output((S,)), guarded_output((S,))
    good = dict(Psi=P(Pd), ldpsi=m, idx=[0, 5, 199, 7, 7, 100], m=m, F=P(Fd), ldf=N, layout=1, N=N, S=S, group=1, pin_row=0,
                pin_value=1.0, err=P(err.t), ref=P(ref.t))

    def call(**change):
        a = dict(good, **change)
        ip = None if a["idx"] is None else _idx(a["idx"])
        rc = ctx.lib.rt_interpolation_errors(ctx.handle, a["Psi"], a["ldpsi"], ip[1] if ip else None, a["m"], a["F"], a["ldf"],
                                             a["layout"], a["N"], a["S"], a["group"], a["pin_row"], a["pin_value"], a["err"], a["ref"])
        torch.cuda.synchronize()
        return rc

    canary = lambda o: bool((o.buf.view(torch.int64) == gd.CANARY_BITS).all())
    for bad in (dict(idx=[0, 5, 200, 7, 7, 100]), dict(idx=[0, 5, -1, 7, 7, 100]), dict(idx=[0, 5, 199, 7, 7, 2 ** 33]),
                dict(idx=None), dict(Psi=None), dict(F=None), dict(group=3), dict(group=0), dict(pin_row=N), dict(pin_row=-2),
                dict(S=0), dict(N=0), dict(m=0), dict(ldpsi=m - 1), dict(ldf=N - 1), dict(layout=0, ldf=S - 1), dict(layout=5)):
        assert call(**bad) == RT_ERR_ARG, bad
        assert canary(err) and canary(ref), bad
    assert call(err=None) == RT_ERR_ARG and canary(ref)
    assert call(m=129, ldpsi=129, idx=list(range(129))) == RT_ERR_UNSUPPORTED and canary(err) and canary(ref)
    assert call() == 0
    assert err.check() == [] and ref.check() == []


# ---- class level -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ic.MOCK_CASES)
def test_classes_evaluate_on_the_device(which):
    from romtime_amd import interpolation

    red, _ = ic.mock_reductor(which)
    red.EVALUATE_ON = "device"
    red.evaluate(ic.MOCK_TS, mu_space=ic.MOCK_MUS)
    idx = interpolation.flat_indices(red)
    assert sorted(red.errors_rom) == [0, 1]
    for k, mu in enumerate(ic.MOCK_MUS):
        F, group = ic.mock_samples(red, mu, ic.MOCK_TS)
        want = ic.oracle_errors(red.basis_fom, red.PT_U, idx, F, (0, 1.0), group)
        bar = ic.error_bar(red.PT_U, F, group)
        got = red.errors_rom[k]
        assert type(got) is np.ndarray and got.shape == (len(ic.MOCK_TS),)
        print(f"{which} mu {k}: worst |device - oracle| / bar = {float((np.abs(got - want) / bar).max()):.3e}")
        assert np.all(np.abs(got - want) <= bar), (which, k, np.abs(got - want), bar)


def test_the_pinned_entry_is_visible():
    """MDEIM's interpolant has entry 0 pinned to 1: moving entry 0 of one snapshot by delta moves that snapshot's squared
    error by exactly the pinned entry's share, and no other snapshot's."""
    from romtime_amd import interpolation

    red, _ = ic.mock_reductor("mass")
    F, _ = ic.mock_samples(red, ic.MOCK_MUS[0], ic.MOCK_TS)
    base = interpolation.snapshot_errors(red, F)
    moved = F.copy()
    moved[0, 2] = 1.0 + 0.5
    got = interpolation.snapshot_errors(red, np.asfortranarray(moved))
    N = F.shape[0]
    keep = [0, 1, 3]
    assert gd.bits_equal(got[keep], base[keep])
    want = np.sqrt(base[2] ** 2 + 0.5 ** 2 / N)                     # entry 0 is no interpolation entry: only (f_0 - 1)^2 changes
    assert 0 not in interpolation.flat_indices(red)
    assert abs(got[2] - want) <= ic.error_bar(red.PT_U, moved)[2] + 4 * ic.EPS * want


def test_closed_form_snapshots_on_the_device():
    """evaluate_closed_form (no FOM callback) against interpolation.evaluate on the same reductor: nx = 100, 3 mu, 4 instants."""
    from romtime_amd import interpolation

    mus = ic.MOCK_MUS + [dict(alpha_0=1.1, delta=0.55, omega=9.7)]
    for which, kind in (("mass", "mass"), ("stiffness_ale", "stiffness")):
        red, solver = ic.mock_reductor(which, nx=100)
        got = interpolation.evaluate_closed_form(red, kind, solver, mus, ic.MOCK_TS, max_columns=6)
        assert got.shape == (3, 4)
        interpolation.evaluate(red, ic.MOCK_TS, mu_space=mus)
        for k, mu in enumerate(mus):
            F, _ = ic.mock_samples(red, mu, ic.MOCK_TS)
            bar = ic.error_bar(red.PT_U, F)
            print(f"{which} mu {k}: worst |closed form - callbacks| / bar = {float((np.abs(got[k] - red.errors_rom[k]) / bar).max()):.3e}")
            assert np.all(np.abs(got[k] - red.errors_rom[k]) <= bar), (which, k)
