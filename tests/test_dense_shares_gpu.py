"""The dense products, bit-exact on every GEMM tile shape and on the CU shares production runs them on.

A ctx with the option "cu_limit" sizes its grids for a share of the chip on the ordinary stream: 224 and 32 CUs are the two
streams of the POD pipeline, 8 the smallest share the option takes, 0 the whole chip.  Every launch rule of the dense routes
depends on that count - the tile narrowing and the split count of the strided GEMM, the thresholds of the tall-skinny
product, the grids of the rank update, of rt_skinny_tn and of the sparse product - and at 8 CUs small outputs reach every
instantiation of the GEMM and make the grid-stride loops turn over (tests/gemm_cases.py; the conditions are held on the CPU
by tests/test_gemm_cases_cpu.py).

Every case asserts its route (Context.launch_info against the rules restated in tests/guarded.py), then the exact answer bit
for bit - integers scaled by powers of two, every partial sum below 2^53, so NumPy's product is the answer in whatever order
a kernel adds - inside NaN-poisoned operands and canary-guarded outputs.  The existing tables of
tests/test_guarded_kernels_gpu.py and tests/test_tallskinny_blocks_gpu.py run through the same bodies on each share."""
import numpy as np
import pytest
import torch

from tests import gemm_cases as gc
from tests import guarded as gd
from tests import test_guarded_kernels_gpu as gk
from tests import test_tallskinny_blocks_gpu as ts
from tests.guarded import exact_operands, guarded_operand, guarded_output
from tests.test_guarded_kernels_gpu import LAY, P, _bits_for, _clean, _defaults_only, _exact, _host  # noqa: F401

pytestmark = pytest.mark.gpu
LIMITED = tuple(s for s in gc.SHARES if s)


@pytest.fixture(scope="module")
def shares():
    """{share: (a ctx of its own with "cu_limit" at the share, the CUs it sizes its grids for)}."""
    from romtime_amd._lib import Context

    device_cus = torch.cuda.get_device_properties(0).multi_processor_count
    made = {}
    try:
        for share in gc.SHARES:
            ctx = Context(0)
            made[share] = (ctx, gc.share_cus(share, device_cus))
            ctx.set_option("cu_limit", share)
        yield made
    finally:
        torch.cuda.synchronize()
        for ctx, _ in made.values():
            ctx.set_option("cu_limit", 0)
            ctx.destroy()


def _ids(cases):
    return [c[0] for c in cases]


# ---- every GEMM case ----------------------------------------------------------------------------------------------------

def _run_gemm_case(ctx, cus, case):
    ops = gc.gemm_operands(case)
    _, _, _, _, lda, ldb = gc.case_strides(case)
    if case.entry == "tn":
        A, B = ops["A"], ops["B"]
        Ad = guarded_operand(A, case.la, case.pa, case.mis_a)
        Bd = Ad if case.sym else guarded_operand(B, case.lb, case.pb, case.mis_b)
        out = guarded_output((case.M, case.Nn), ld=case.Nn + case.pc)
        operands = [(Ad, A)] + ([] if case.sym else [(Bd, B)])
        call = lambda: ctx.lib.rt_gemm_tn(ctx.handle, P(Ad), lda, LAY[case.la], P(Bd), ldb, LAY[case.lb], case.K, case.M, case.Nn,
                                          P(out.t), out.ld)
    else:
        X, T = ops["X"], ops["T"]
        Ad, Bd = guarded_operand(X, case.la, case.pa, case.mis_a), guarded_operand(T, "C", case.pb, case.mis_b)
        out = guarded_output((case.M, case.Nn), ld=(case.Nn if case.lc == "C" else case.M) + case.pc, layout=case.lc)
        if case.beta != 0.0:
            out.fill(ops["Y0"])
        operands = [(Ad, X), (Bd, T)]
        call = lambda: ctx.lib.rt_gemm_nn_axpby(ctx.handle, P(Ad), lda, LAY[case.la], P(Bd), ldb, case.M, case.K, case.Nn,
                                                case.alpha, case.beta, P(out.t), out.ld, LAY[case.lc])
    # the buffers are what the table says they are: the vector-load premise of the case rests on it
    assert (Ad.data_ptr() % 16 != 0) == case.mis_a and (Bd.data_ptr() % 16 != 0) == case.mis_b
    ctx.check(call(), f"rt_gemm_{case.entry}")
    assert ctx.launch_info() == gc.case_plan(case, cus), (ctx.launch_info(), gc.case_plan(case, cus))
    got = _host(out.t)
    _exact(got, ops["ref"])
    _clean([out], operands)
    return got


@pytest.mark.parametrize("case", gc.GEMM_CASES, ids=[c.id for c in gc.GEMM_CASES])
def test_gemm_case(shares, case):
    ctx, cus = shares[case.share]
    assert case.share == 0 or cus == case.share
    _run_gemm_case(ctx, cus, case)


# ---- the existing tables at every share -----------------------------------------------------------------------------------

@pytest.mark.parametrize("share", LIMITED)
@pytest.mark.parametrize("case", gk.GEMM_TN_CASES, ids=_ids(gk.GEMM_TN_CASES))
def test_gemm_tn_table(shares, share, case):
    gk._gemm_tn_case(*shares[share], case)


@pytest.mark.parametrize("share", LIMITED)
@pytest.mark.parametrize("case", gk.GEMM_NN_CASES, ids=_ids(gk.GEMM_NN_CASES))
def test_gemm_nn_table(shares, share, case):
    gk._gemm_nn_case(*shares[share], case)


RANK_UPDATE_TABLE = gk.RANK_UPDATE_CASES + gc.RANK_UPDATE_TRIP_CASES


@pytest.mark.parametrize("share", LIMITED)
@pytest.mark.parametrize("case", RANK_UPDATE_TABLE, ids=_ids(RANK_UPDATE_TABLE))
def test_rank_update_table(shares, share, case):
    ctx, cus = shares[share]
    if share == 8 and case in gc.RANK_UPDATE_TRIP_CASES:          # the rows are walked in several uneven trips
        trips, stages, gx = gc.rank_update_trips(case[1], case[2], cus)
        assert trips >= 3 and stages % gx != 0, (trips, stages, gx)
    gk._rank_update_case(ctx, cus, case)


SPMM_TABLE = [c + (500,) for c in gk.CSR_SPMM_CASES] + [c + (gc.SPMM_TRIP_ROWS,) for c in gc.SPMM_TRIP_CASES]


@pytest.mark.parametrize("share", LIMITED)
@pytest.mark.parametrize("r,pv,py,mis,N", SPMM_TABLE)
def test_csr_spmm_table(shares, share, r, pv, py, mis, N):
    ctx, cus = shares[share]
    if share == 8 and N == gc.SPMM_TRIP_ROWS:
        passes, last = gc.spmm_passes(N, cus)
        assert passes >= 3 and last < 4 * 8 * cus
    gk._csr_spmm_case(ctx, r, pv, py, mis, N=N)


PROJECT_TABLE = gk.PROJECT_CASES + [gc.PROJECT_TRIP_CASE]


@pytest.mark.parametrize("share", LIMITED)
@pytest.mark.parametrize("case", PROJECT_TABLE, ids=_ids(PROJECT_TABLE))
def test_project_table(shares, share, case):
    gk._project_case(*shares[share], *case[1:])


# ---- the tall-skinny product ----------------------------------------------------------------------------------------------

TALLSKINNY = gc.tallskinny_cases()


@pytest.mark.parametrize("case", TALLSKINNY, ids=_ids(TALLSKINNY))
def test_tallskinny_every_k(shares, case):
    _, share, N, n, k = case
    ctx, cus = shares[share]
    ts._run(ctx, cus, N, n, k, 64 * gc.tallskinny_variant(N, k, cus)[2])


@pytest.mark.parametrize("case", ts.GENERAL, ids=_ids(ts.GENERAL))
def test_tallskinny_general_loop_share224(shares, case):
    _, n, k, px, mis, pt = case
    ctx, cus = shares[224]
    ts._run(ctx, cus, 64 * cus + 37, n, k, 64, px=px, mis=mis, pt=pt)


# ---- rt_skinny_tn ---------------------------------------------------------------------------------------------------------

_SKINNY_B = {}


def _skinny_b(N, n):
    """The tall operand of (N, n), drawn once and left unchanged."""
    if (N, n) not in _SKINNY_B:
        rng = np.random.default_rng(N + n)
        _SKINNY_B[N, n] = exact_operands(rng, (N, n), _bits_for(N), gd.graded_exponents(rng, n), k=N)
    return _SKINNY_B[N, n]


def _run_skinny_tn(ctx, cus, case):
    _, _, N, m, n, pb, mis_b, pa = case
    rng = np.random.default_rng(1000 * n + m)
    B = _skinny_b(N, n)
    A = exact_operands(rng, (N, m), _bits_for(N), gd.graded_exponents(rng, m), k=N)
    Ad, Bd = guarded_operand(A, "C", pa, False), guarded_operand(B, "C", pb, mis_b)
    Cm = guarded_output((m, n), ld=n + 3)
    ctx.check(ctx.lib.rt_gemm_tn(ctx.handle, P(Ad), m + pa, LAY["C"], P(Bd), n + pb, LAY["C"], N, m, n, P(Cm.t), Cm.ld), "rt_gemm_tn")
    plan = gd.skinny_tn_plan(N, m, n, cus)
    assert plan is not None and plan["tile"][0] == m and ctx.launch_info() == plan, (ctx.launch_info(), plan)
    got = _host(Cm.t)
    _exact(got, A.T @ B)
    _clean([Cm], [(Ad, A), (Bd, B)])
    return got


@pytest.mark.parametrize("case", gc.SKINNY_TN_CASES, ids=_ids(gc.SKINNY_TN_CASES))
def test_skinny_tn_every_m(shares, case):
    _run_skinny_tn(*shares[case[1]], case)


# ---- the same bits on every share -----------------------------------------------------------------------------------------

def _by_id(cases, cid):
    return next(c for c in cases if c[0] == cid)


ACROSS_SHARES = {
    "gemm_split": lambda ctx, cus: _run_gemm_case(ctx, cus, _by_id(gc.GEMM_CASES, "lift_shape_share32")),
    "gemm_symmetric": lambda ctx, cus: _run_gemm_case(ctx, cus, _by_id(gc.GEMM_CASES, "sym128_diag_and_off_C_m129_K300")),
    "gemm_direct_store": lambda ctx, cus: _run_gemm_case(ctx, cus, _by_id(gc.GEMM_CASES, "nn_128x96_lift")),
    "tallskinny": lambda ctx, cus: ts._run(ctx, cus, 64 * 256 + 37, 96, 40, 64 if cus > 32 else 128),
    "skinny_tn": lambda ctx, cus: _run_skinny_tn(ctx, cus, _by_id(gc.SKINNY_TN_CASES, "m9_odd_n_misaligned_share8")),
    "rank_update": lambda ctx, cus: gk._rank_update_case(ctx, cus, _by_id(gc.RANK_UPDATE_TRIP_CASES, "trips_vector")),
    "csr_spmm": lambda ctx, cus: gk._csr_spmm_case(ctx, 130, 5, 1, False, N=gc.SPMM_TRIP_ROWS),
}


@pytest.mark.parametrize("kernel", sorted(ACROSS_SHARES))
def test_bits_do_not_depend_on_the_share(shares, kernel):
    """The data is exact, so each share equals NumPy and hence the others; stated once, so that a later test on inexact data
    does not assume it silently: where a share changes only the grid (and the order of exact additions), it changes no bit."""
    got = {share: ACROSS_SHARES[kernel](ctx, cus) for share, (ctx, cus) in shares.items()}
    first = got[gc.SHARES[0]]
    for share in gc.SHARES[1:]:
        assert gd.bits_equal(got[share], first), (kernel, share, gd.mismatch(got[share], first))
