"""rt_trajectory_integrals and romtime_amd.outputs on the device.

Exact cases: 4-bit integer E and A, small integer c0 and c1, p = 2, power-of-two weights and scales - every base, square,
weighted term and column sum is exact below 2^53, so NumPy's float64 result is the exact answer whatever the order of the
sums.  Operands sit in NaN-poisoned guarded buffers, the output in a canary buffer (tests/guarded.py); each case asserts
its launch plan from rt_last_launch_info.  Rounded data, the padding hazard, NaN isolation, the piston case and the sweep
output are held to the derived bar of tests/outputs_cases.py::error_bar against the extended-precision truth."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guarded as gd
from tests import outputs_cases as oc
from tests.guarded import exact_operands, guarded_operand, guarded_output

pytestmark = pytest.mark.gpu
GAP = 3            # poisoned lines between the trajectories of a batch: a padded stride_a


@pytest.fixture(scope="module")
def ctx():
    from romtime_amd._lib import Context

    return Context.current()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _dev(*arrays):
    from romtime_amd import ops

    return [None if a is None else ops.to_device(a) for a in arrays]


SHAPES = [(66, 1, 1, 1), (33, 3, 63, 2), (64, 81, 65, 3), (2200, 128, 130, 2)]      # n_pts, k, nt, n_traj
VARIANTS = [
    # id, (lde, lda) padding, misaligned, w given, scale given
    ("plain", (0, 0), False, True, True),
    ("padded_misaligned_null_w_scale", (3, 1), True, False, False),
    ("padded_w_only", (1, 2), False, True, False),
    ("misaligned_scale_only", (0, 3), True, False, True),
]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_trajectory_integrals_exact_guarded(ctx, cus, shape, variant):
    n_pts, k, nt, n = shape
    _, (pe, pa), misalign, with_w, with_scale = variant
    rng = np.random.default_rng(n_pts * 1_000_003 + nt * 1009 + k * 31 + n + 7 * pe + pa)
    Eh = exact_operands(rng, (n_pts, k), 4, k=k)
    As = [exact_operands(rng, (nt, k), 4, k=k) for _ in range(n)]
    c0, c1 = 3.0, -2.0
    wh = np.ldexp(1.0, rng.integers(-2, 3, size=n_pts)) if with_w else None
    sh = np.ldexp(1.0, rng.integers(-3, 4, size=(n, nt))) if with_scale else None
    want = np.empty((n, nt))
    for j, a in enumerate(As):
        b = c0 + c1 * (Eh @ a.T)
        terms = b * b if wh is None else wh[:, None] * (b * b)
        assert np.abs(b).max() < 2.0 ** 18 and np.sum(np.abs(terms), axis=0).max() < 2.0 ** 50      # exact in float64
        want[j] = np.sum(terms, axis=0) * (1.0 if sh is None else sh[j])
    Ed = guarded_operand(Eh, "C", pe, misalign)
    Ah = np.full((n * (nt + GAP), k), np.nan)
    for j, a in enumerate(As):
        Ah[j * (nt + GAP): j * (nt + GAP) + nt] = a
    Ad = guarded_operand(Ah, "C", pa, misalign)
    wd = guarded_operand(wh[None, :], "C", 0, misalign) if with_w else None
    sd = guarded_operand(sh, "C", 0, False) if with_scale else None
    out = guarded_output((n, nt))
    lda = k + pa
    par = (C.c_double * 3)(c0, c1, 2.0)
    rc = ctx.lib.rt_trajectory_integrals(ctx.handle, P(Ed), k + pe, P(wd), P(Ad), lda, (nt + GAP) * lda, P(sd), n_pts, k, nt, n,
                                         0, par, P(out.t))
    ctx.check(rc, "rt_trajectory_integrals")
    torch.cuda.synchronize()
    plan = oc.trajectory_integrals_plan(n_pts, nt, n, cus)
    assert ctx.launch_info() == plan, (ctx.launch_info(), plan)
    assert (plan["splits"] > 1) == (n_pts == 2200)
    assert out.check() == [], out.check()
    for v, h in ((Ed, Eh), (Ad, Ah), (wd, None if wh is None else wh[None, :]), (sd, sh)):
        if v is not None:
            assert gd.operand_intact(v, h) == [], gd.operand_intact(v, h)
    got = out.t.cpu().numpy()
    assert gd.bits_equal(got, want), gd.mismatch(got, want)


def test_return_codes(ctx):
    E = torch.zeros((64, 129), dtype=torch.float64, device="cuda")
    A = torch.zeros((8, 129), dtype=torch.float64, device="cuda")
    w = torch.ones(64, dtype=torch.float64, device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    par = (C.c_double * 3)(1.0, 1.0, 2.0)

    def call(n_pts=64, k=128, nt=8, n=1, fn=0, E=E, A=A, out=out, par=par, lde=129, lda=129):
        return ctx.lib.rt_trajectory_integrals(ctx.handle, P(E), lde, P(w), P(A), lda, 8 * 129, None, n_pts, k, nt, n, fn, par,
                                               P(out))

    assert call() == 0
    assert call(k=129) == -3                               # RT_ERR_UNSUPPORTED
    for bad in (dict(n_pts=0), dict(k=0), dict(nt=0), dict(n=0), dict(nt=-1), dict(fn=1), dict(E=None), dict(A=None),
                dict(out=None), dict(par=None), dict(lde=127), dict(lda=127)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 64.0))    # (1 + 0)^2 summed over 64 rows of weight 1
    from romtime_amd import ops
    from romtime_amd._lib import RomtimeHipError

    with pytest.raises(RomtimeHipError):
        ops.trajectory_integrals(E, A)                     # k = 129 through the wrapper: an error, no other route
    with pytest.raises(RomtimeHipError):
        ops.trajectory_integrals(E[:, :4], A[:, :4], fn=("exp", 1.0, 1.0, 1.0))


@pytest.fixture(scope="module", params=[(97, 13, 70), (2049, 128, 130)], ids=["97x13x70", "2049x128x130"])
def rounded(request):
    """One rounded case per shape with its products in extended precision, shared by the exponents."""
    n_pts, k, nt = request.param
    E, w, A, scale = oc.rounded_case(n_pts, n_pts, k, nt)
    return E, w, A, scale, oc.longdouble_products(E, A[0])


@pytest.mark.parametrize("p", oc.EXPONENTS)
def test_rounded_data_within_the_derived_bar(rounded, p):
    from romtime_amd import ops

    E, w, A, scale, z = rounded
    fn = ("power", 1.0, -0.6, p)
    got = ops.trajectory_integrals(*_dev(E, A, w, scale), fn=fn).cpu().numpy()[0]
    want = oc.longdouble_integrals(E, w, A[0], scale[0], fn, z=z)
    bar = oc.error_bar(E, w, A[0], scale[0], fn)
    ok, ratio = oc.within_bar(got, want, bar)
    rel = float((bar / np.abs(want).astype(np.float64)).max())
    print(f"rounded data {E.shape} x {A.shape[1]} steps, p = {p!r}: worst |difference| / bar = {ratio:.3f}, bar / |truth| <= {rel:.2e}")
    assert ok and rel < 5e-13, (ratio, rel)


def test_rows_past_the_end_are_predicated_out_not_weighted_by_zero():
    """c0 = 0, p = -1, positive data, 33 rows: the 31 padded rows of the second stage evaluate 1 / 0."""
    from romtime_amd import ops

    rng = np.random.default_rng(33)
    E = rng.uniform(0.5, 1.5, (33, 5))
    A = rng.uniform(0.5, 1.5, (2, 70, 5))
    w = rng.uniform(0.5, 1.5, 33)
    fn = ("power", 0.0, 1.0, -1.0)
    for wh in (w, None):
        got = ops.trajectory_integrals(*_dev(E, A, wh), fn=fn).cpu().numpy()
        assert np.all(np.isfinite(got))
        for j in range(2):
            want = oc.longdouble_integrals(E, wh, A[j], None, fn)
            ok, ratio = oc.within_bar(got[j], want, oc.error_bar(E, wh, A[j], None, fn))
            assert ok, (j, ratio)


def test_a_negative_base_is_nan_in_its_own_step_only():
    from romtime_amd import ops

    E, w, A, scale, fn = oc.nan_case()
    got = ops.trajectory_integrals(*_dev(E, A, w, scale), fn=fn).cpu().numpy()[0]
    want = oc.longdouble_integrals(E, w, A[0], scale[0], fn)
    assert np.isnan(want.astype(np.float64)).sum() == 1
    assert np.array_equal(np.isnan(got), np.isnan(want.astype(np.float64)))
    ok, ratio = oc.within_bar(got, want, oc.error_bar(E, w, A[0], scale[0], fn))
    assert ok, ratio


@pytest.mark.parametrize("n_pts", [97, 2049])
def test_a_trajectory_has_the_same_bits_alone_and_in_a_batch(n_pts):
    from romtime_amd import ops

    E, w, A, scale = oc.rounded_case(11, n_pts, 13, 70, n_traj=3)
    fn = ("power", 1.0, -0.6, oc.EXPONENTS[0])
    Ed, Ad, wd, sd = _dev(E, A, w, scale)
    batch = ops.trajectory_integrals(Ed, Ad, wd, sd, fn=fn).cpu().numpy()
    for j in range(3):
        alone = ops.trajectory_integrals(Ed, Ad[j], wd, sd[j], fn=fn).cpu().numpy()
        assert gd.bits_equal(alone[0], batch[j]), (j, gd.mismatch(alone[0], batch[j]))


@pytest.fixture(scope="module")
def golden_hrom():
    from tests.conftest import load_golden

    return load_golden("hrom.npz")


def test_mass_conservation_and_probes_of_the_piston_case_on_the_device(ctx, cus, golden_hrom):
    from romtime_amd import outputs

    case = oc.piston_outputs_case(golden_hrom)
    lift = (case["ramp"], case["amp"])
    payload = outputs.mass_conservation(case["Vr"], case["rom"], case["mus"], case["dt"], case["length"], lift=lift, ts=case["ts"])
    assert ctx.launch_info() == oc.trajectory_integrals_plan(120, 22, 5, cus)
    worst = oc.check_piston_mass(case, payload)
    print(f"mass_conservation on the device vs the long-double truth: worst |difference| / bar = {worst:.3f}")
    B = np.column_stack([case["Vr"], case["ramp"]])
    x = np.array([0.0, 0.5, 0.3337, np.inf])
    got = outputs.probes(case["Vr"], case["rom"], x, case["length"], lift=lift)
    assert got.shape == (5, 22, 4)
    nodes, k = np.arange(61) / 60.0, B.shape[1]
    for j in range(5):
        a = np.column_stack([case["rom"][j], case["amp"][j]])
        u = B @ a.T
        for t in range(22):
            want = np.interp(x, case["length"][j, t] * nodes, u[:, t])
            bar = 2.0 * ((k + 4) * oc.U_ROUND * 2 * (np.abs(B) @ np.abs(a[t])).max() + 4 * oc.U_ROUND * 60 * np.abs(np.diff(u[:, t])).max())
            assert np.all(np.abs(got[j, t] - want) <= bar), (j, t)
    fom = outputs.snapshot_mass_conservation(B @ np.column_stack([case["rom"][1], case["amp"][1]]).T, case["mus"][1], case["dt"],
                                             case["length"][1])
    np.testing.assert_allclose(fom["mass"], payload[1]["mass"], rtol=1e-13)


def test_integrals_of_sweep_output_match_the_host_loop():
    """outputs.trajectory_integrals takes the sweep's (n_mu, nt, r) device tensor as it is; the reference is the host loop
    over lifted steps (u = V u_N[j, t], then the same quadrature in NumPy).  c1 is scaled to the trajectories so that the
    base stays within (0.5, 1.5)."""
    from romtime_amd import outputs
    from romtime_amd.sweep import hrom_bdf_sweep
    from romtime_amd.testing.workloads import c5_hyper_reduced

    terms, _, V, _ = c5_hyper_reduced(N=3000, nt=40, n_mu=3, r=20)
    uN = hrom_bdf_sweep(terms["mass"], terms["lin"], terms["nl"], terms["rhs"], terms["dt"], bdf2=True)
    assert uN.is_cuda and tuple(uN.shape) == (3, 40, 20)
    h = uN.cpu().numpy()
    lifted = [V @ h[j].T for j in range(3)]
    umax = max(float(np.abs(u).max()) for u in lifted)
    assert umax > 0
    fn = ("power", 1.0, -0.5 / umax, 5.000000000000001)
    L = 1.0 + 0.1 * np.sin(np.arange(3)[:, None] + 0.2 * np.arange(40)[None, :])
    got = outputs.trajectory_integrals(V, uN, fn, length=L)
    assert got.shape == (3, 40)
    E, w = oc.host_quadrature(V, 2)
    xi, gw = outputs.gauss_unit_interval(2)

    def host_mass(u, length):                              # one lifted step
        return length * sum(np.sum(g / 2999 * (fn[1] + fn[2] * ((1 - q) * u[:-1] + q * u[1:])) ** fn[3]) for q, g in zip(xi, gw))

    for j in range(3):
        host = np.array([host_mass(lifted[j][:, t], L[j, t]) for t in range(40)])
        bar = oc.error_bar(E, w, h[j], L[j], fn)
        diff = np.abs(got[j] - host)
        assert np.all(diff <= bar), (j, float((diff / bar).max()))
        assert np.ptp(host) > 0
