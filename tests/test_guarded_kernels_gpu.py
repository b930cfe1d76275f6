"""Every kernel route, bit-exact, inside NaN-poisoned operands and canary-guarded outputs (tests/guarded.py).

Each case names the route it expects and asserts it (launch_info / rt_gram_plan_info against the dispatch rules restated
in tests/guarded.py), then requires: the exact answer bit for bit (integer data scaled by powers of two, every partial
sum below 2^53), no word of the output buffer written outside the output, every output word written, and operands and
their poison unchanged.  The entry points without an exact answer (rt_gram_scale, rt_pod_backproject_weights) are held
to a few ulps of an np.longdouble reference per entry."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import guarded as gd
from tests.guarded import guarded_operand, guarded_output, exact_operands

pytestmark = pytest.mark.gpu
LAY = {"C": 0, "F": 1}
ULP = 2.0 ** -52


@pytest.fixture(scope="module", autouse=True)
def _defaults_only():
    try:
        gd.require_clean_env()
    except RuntimeError as exc:
        pytest.fail(str(exc))


@pytest.fixture(scope="module")
def ctx():
    from romtime_amd._lib import Context

    return Context.current()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _host(t):
    return t.cpu().numpy()


def _clean(outs=(), operands=()):
    torch.cuda.synchronize()
    for o in outs:
        assert o.check() == [], o.check()
    for v, h in operands:
        assert gd.operand_intact(v, h) == [], gd.operand_intact(v, h)


def _exact(got, want):
    assert gd.bits_equal(got, want), gd.mismatch(np.asarray(got), np.asarray(want))


def _bits_for(k, partner_bits=None, cap=18):
    """Largest integer width (<= cap) whose k-term contraction stays exact."""
    b = cap
    while k * 2.0 ** (b + (b if partner_bits is None else partner_bits)) >= 2.0 ** 53:
        b -= 1
    return b


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- rt_gram ----------------------------------------------------------------------------------------------------------

GRAM_CASES = [
    # id, N, n, layout, ld_pad, misalign, form (0 generic symmetric GEMM, 1 gram128 two launches, 2 gram128 one launch)
    ("generic_n64", 5000, 64, "C", 1, False, 0),
    ("generic_short_K", 6000, 200, "F", 3, True, 0),
    ("two_launch_full_tiles", 100_000, 128, "C", 0, False, 1),
    ("two_launch_shifted_panel", 100_000, 250, "C", 2, False, 1),
    ("two_launch_predicated_odd_n", 100_000, 255, "C", 1, False, 1),
    ("two_launch_predicated_misaligned", 100_000, 250, "F", 0, True, 1),
    ("one_launch_512", 40_000, 512, "C", 0, False, 2),
    ("one_launch_384_misaligned", 60_000, 384, "F", 1, True, 2),
    ("one_launch_1000_shifted", 30_000, 1000, "F", 0, False, 2),
    ("one_launch_odd_n", 100_000, 301, "C", 1, False, 2),
]


def _gram_form(ctx, cus, N, n):
    out = (C.c_int * 5)()
    assert ctx.lib.rt_gram_plan_info(cus, N, n, out) == 0
    return list(out)


def _assert_gram_route(ctx, cus, N, n, form):
    plan = _gram_form(ctx, cus, N, n)
    assert plan[0] == form, (N, n, plan)
    info = ctx.launch_info()
    if form == 0:
        assert info == gd.gemm_plan(n, n, N, True, True, cus), info
    elif form == 1:
        tiles1 = -(-n // 128)
        n_off = tiles1 * (tiles1 - 1) // 2
        assert info == dict(grid=8 * (n_off * plan[3] + tiles1 * plan[4]), splits=8 * plan[3], tile=(128, 128)), (info, plan)
    else:
        assert info["grid"] == 2 * cus and info["tile"] == (128, 128), info


def _run_gram(ctx, Xd, N, n):
    ld, lay = gd.leading_dim(Xd)
    G = guarded_output((n, n))
    ctx.check(ctx.lib.rt_gram(ctx.handle, P(Xd), N, n, ld, LAY[lay], P(G.t)), "rt_gram")
    return G


@pytest.mark.parametrize("case", GRAM_CASES, ids=[c[0] for c in GRAM_CASES])
def test_gram_guarded(ctx, cus, case):
    _, N, n, layout, ld_pad, misalign, form = case
    rng = np.random.default_rng(N + n)
    X = exact_operands(rng, (N, n), _bits_for(N), gd.graded_exponents(rng, n), k=N)
    Xd = guarded_operand(X, layout, ld_pad, misalign)
    G = _run_gram(ctx, Xd, N, n)
    _assert_gram_route(ctx, cus, N, n, form)
    _exact(_host(G.t), X.T @ X)
    ctx.set_option("gram_pace", 0)            # the pacing of the gram128 workgroups must not change a bit
    try:
        G0 = _run_gram(ctx, Xd, N, n)
    finally:
        ctx.set_option("gram_pace", 1)
    assert torch.equal(G0.t.view(torch.int64), G.t.view(torch.int64))
    _clean([G, G0], [(Xd, X)])


@pytest.mark.parametrize("ld", [4_194_302, 4_194_304], ids=["vector_loads", "past_32bit_offsets"])
def test_gram_column_stride_at_the_32bit_offset_switch(ctx, cus, ld):
    """Column-major X whose column stride puts 64 columns ms*64*8 bytes apart just below / at 2^31: the gram128 loader
    switches from 32-bit per-thread offsets to the predicated loader there.  ~4.3 GB, nearly all of it poison."""
    N, n = 98_304, 128
    rng = np.random.default_rng(ld)
    X = exact_operands(rng, (N, n), _bits_for(N), gd.graded_exponents(rng, n), k=N)
    Xd = guarded_operand(X, "F", ld - N, False, guard=1)
    assert gd.leading_dim(Xd) == (ld, "F")
    try:
        G = _run_gram(ctx, Xd, N, n)
        _assert_gram_route(ctx, cus, N, n, 1)
        _exact(_host(G.t), X.T @ X)
        _clean([G], [(Xd, X)])
    finally:
        del Xd
        _free()


# ---- rt_gemm_tn ------------------------------------------------------------------------------------------------------

GEMM_TN_CASES = [
    # id, N, m, n, layout A, layout B, ld_pad A, ld_pad B, misalign A, ldc pad, symmetric
    ("skinny_one_strip", 20_000, 8, 300, "C", "C", 1, 3, True, 5, False),
    ("skinny_two_strips", 20_000, 16, 700, "C", "C", 0, 0, False, 1, False),
    ("generic_no_split", 100, 300, 200, "F", "C", 0, 1, False, 3, False),
    ("generic_split_k", 50_000, 100, 90, "F", "F", 1, 0, True, 2, False),
    ("generic_row_major_m17", 30_000, 17, 50, "C", "C", 0, 2, False, 7, False),
    ("symmetric", 40_000, 150, 150, "C", "C", 1, 1, False, 4, True),
]


def _gemm_tn_case(ctx, cus, case):
    """The body of test_gemm_tn_guarded on a ctx that sizes its grids for ``cus`` CUs; returns C."""
    _, N, m, n, la, lb, pa, pb, mis, pc, sym = case
    rng = np.random.default_rng(N + m + n)
    b = _bits_for(N)
    A = exact_operands(rng, (N, m), b, gd.graded_exponents(rng, m), k=N)
    Ad = guarded_operand(A, la, pa, mis)
    if sym:
        B, Bd = A, Ad
    else:
        B = exact_operands(rng, (N, n), b, gd.graded_exponents(rng, n), k=N)
        Bd = guarded_operand(B, lb, pb, False)
    lda, la_ = gd.leading_dim(Ad)
    ldb, lb_ = gd.leading_dim(Bd)
    Cm = guarded_output((m, n), ld=n + pc)
    ctx.check(ctx.lib.rt_gemm_tn(ctx.handle, P(Ad), lda, LAY[la_], P(Bd), ldb, LAY[lb_], N, m, n, P(Cm.t), n + pc), "rt_gemm_tn")
    skinny = None if (sym or la != "C" or lb != "C") else gd.skinny_tn_plan(N, m, n, cus)
    want = skinny or gd.gemm_plan(m, n, N, sym, True, cus)
    assert ctx.launch_info() == want
    assert (skinny is not None) == case[0].startswith("skinny")
    assert (want["splits"] == 1) == (case[0] == "generic_no_split")
    got = _host(Cm.t)
    _exact(got, A.T @ B)
    _clean([Cm], [(Ad, A)] + ([] if sym else [(Bd, B)]))
    return got


@pytest.mark.parametrize("case", GEMM_TN_CASES, ids=[c[0] for c in GEMM_TN_CASES])
def test_gemm_tn_guarded(ctx, cus, case):
    _gemm_tn_case(ctx, cus, case)


# ---- rt_gemm_nn_axpby ------------------------------------------------------------------------------------------------

GEMM_NN_CASES = [
    # id, N, n, k, X layout, X ld_pad, X misalign, T ld_pad, Y layout, Y ld_pad, alpha, beta, route
    ("tallskinny_fast", 140_000, 96, 16, "C", 0, False, 0, "C", 3, 1.0, 0.0, "tallskinny"),
    ("tallskinny_slow", 20_001, 70, 15, "C", 1, True, 1, "C", 1, 1.0, 0.0, "tallskinny"),
    ("expansion", 48, 288, 16_384, "C", 0, False, 0, "C", 2, 1.0, 0.0, "expansion"),
    ("expansion_declined_misaligned", 48, 288, 16_384, "C", 0, True, 0, "C", 2, 1.0, 0.0, "generic"),
    ("generic_axpby_col_major_y", 3000, 100, 40, "F", 1, False, 2, "F", 3, 0.5, -2.0, "generic"),
    ("generic_row_major_y", 5000, 64, 70, "C", 2, False, 0, "C", 5, -1.0, 0.0, "generic"),
    ("generic_skinny_output", 9000, 33, 20, "F", 0, True, 1, "C", 1, 2.0, 0.25, "generic"),
]


def _gemm_nn_case(ctx, cus, case):
    """The body of test_gemm_nn_axpby_guarded on a ctx that sizes its grids for ``cus`` CUs; returns Y."""
    _, N, n, k, lx, px, mis, pt, ly, py, alpha, beta, route = case
    rng = np.random.default_rng(N + n + k)
    b = _bits_for(2 * n + 2)
    g, f = gd.graded_exponents(rng, N, 60), gd.graded_exponents(rng, k, 60)
    X = exact_operands(rng, (n, N), b, g).T                 # rows of X graded
    T = exact_operands(rng, (n, k), b, f, k=n + 1)          # columns of T graded
    Y0 = np.ldexp(rng.integers(-1024, 1025, size=(N, k)).astype(np.float64), g[:, None] + f[None, :])
    Xd, Td = guarded_operand(X, lx, px, mis), guarded_operand(T, "C", pt, False)
    ldx, lx_ = gd.leading_dim(Xd)
    Y = guarded_output((N, k), ld=(k if ly == "C" else N) + py, layout=ly)
    if beta != 0.0:
        Y.fill(Y0)
    ctx.check(ctx.lib.rt_gemm_nn_axpby(ctx.handle, P(Xd), ldx, LAY[lx_], P(Td), k + pt, N, n, k, alpha, beta, P(Y.t), Y.ld,
                                       LAY[ly]), "rt_gemm_nn_axpby")
    info = ctx.launch_info()
    if route == "tallskinny":
        assert info == gd.tallskinny_plan(N, n, k, cus)
    elif route == "expansion":
        assert info == gd.expansion_plan(k) != gd.gemm_plan(N, k, n, False, False, cus)
    else:
        assert info == gd.gemm_plan(N, k, n, False, False, cus)
    ref = alpha * (X @ T) + (beta * Y0 if beta != 0.0 else 0.0)
    got = _host(Y.t)
    _exact(got, ref)
    _clean([Y], [(Xd, X), (Td, T)])
    return got


@pytest.mark.parametrize("case", GEMM_NN_CASES, ids=[c[0] for c in GEMM_NN_CASES])
def test_gemm_nn_axpby_guarded(ctx, cus, case):
    _gemm_nn_case(ctx, cus, case)


# ---- rt_rank_update ----------------------------------------------------------------------------------------------------

RANK_UPDATE_CASES = [
    # id, N, n, k, colscale, Ysrc ld_pad, Ydst ld_pad, misalign src, misalign dst, in place, alpha
    ("k1_vector_scaled", 5000, 200, 1, True, 0, 2, False, False, False, -1.0),
    ("k63_scalar_odd_ld", 3001, 131, 63, False, 0, 2, False, False, False, 0.5),
    ("k64_scalar_misaligned", 4099, 256, 64, True, 2, 4, True, False, False, -1.0),
    ("k64_in_place_vector", 5000, 300, 64, True, 2, 2, False, False, True, -1.0),
    ("k1_in_place_scalar", 2001, 77, 1, False, 0, 0, True, True, True, 2.0),
]


def _rank_update_case(ctx, cus, case):
    """The body of test_rank_update_guarded on a ctx that sizes its grids for ``cus`` CUs; returns the updated matrix."""
    _, N, n, k, use_cs, ps, pd, ms, md, in_place, alpha = case
    rng = np.random.default_rng(N + n + k)
    g, f = gd.graded_exponents(rng, N, 60), gd.graded_exponents(rng, n, 60)
    c = rng.integers(-3, 4, size=n) if use_cs else np.zeros(n, dtype=np.int64)
    X = exact_operands(rng, (k, N), 16, g).T
    T = exact_operands(rng, (k, n), 16, f, k=k + 1)
    Ys = np.ldexp(rng.integers(-(1 << 16), (1 << 16) + 1, size=(N, n)).astype(np.float64), g[:, None] + f[None, :] - c[None, :])
    cs = np.ldexp(1.0, c)
    Xd, Td = guarded_operand(X, "C", 1, False), guarded_operand(T, "C", 3, False)
    Ysd = guarded_operand(Ys, "C", ps, ms)
    csd = guarded_operand(cs[None, :], "C", 0, True) if use_cs else None
    ref = Ys * cs[None, :] + alpha * (X @ T)
    if in_place:
        dst, ldd = Ysd, Ysd.stride(0)
    else:
        Yd = guarded_output((N, n), ld=n + pd, misalign=md)
        dst, ldd = Yd.t, n + pd
    ctx.check(ctx.lib.rt_rank_update(ctx.handle, P(Ysd), Ysd.stride(0), P(csd), P(Xd), Xd.stride(0), P(Td), Td.stride(0),
                                     N, k, n, alpha, P(dst), ldd), "rt_rank_update")
    assert ctx.launch_info() == gd.rank_update_plan(N, n, cus)
    got = _host(dst)
    _exact(got, ref)
    ops = [(Xd, X), (Td, T)] + ([(csd, cs[None, :])] if use_cs else [])
    if in_place:
        _clean([], ops + [(Ysd, ref)])          # the poison around the updated matrix is untouched
    else:
        _clean([Yd], ops + [(Ysd, Ys)])
    return got


@pytest.mark.parametrize("case", RANK_UPDATE_CASES, ids=[c[0] for c in RANK_UPDATE_CASES])
def test_rank_update_guarded(ctx, cus, case):
    _rank_update_case(ctx, cus, case)


# ---- rt_transpose ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,ps,pd,mis", [(45, 77, 3, 5, False), (1, 100, 0, 1, True), (100, 1, 2, 0, False),
                                                (64, 96, 1, 1, True), (33, 1000, 0, 7, False)])
def test_transpose_guarded(ctx, rows, cols, ps, pd, mis):
    rng = np.random.default_rng(rows * cols)
    S = exact_operands(rng, (rows, cols), 30, gd.graded_exponents(rng, cols, 200))
    Sd = guarded_operand(S, "C", ps, mis)
    D = guarded_output((cols, rows), ld=rows + pd, misalign=not mis)
    ctx.check(ctx.lib.rt_transpose(ctx.handle, P(Sd), rows, cols, cols + ps, P(D.t), rows + pd), "rt_transpose")
    _exact(_host(D.t), S.T)
    _clean([D], [(Sd, S)])


# ---- rt_csr_spmm -------------------------------------------------------------------------------------------------------

def _csr(rng, N, ncols, per_row=6, empty_every=7):
    indptr, indices = [0], []
    for i in range(N):
        cnt = 0 if i % empty_every == 3 else int(rng.integers(1, per_row + 1))
        cols = set(rng.choice(ncols, size=min(cnt, ncols), replace=False).tolist())
        if i == N - 2:
            cols.add(ncols - 1)                      # the last column, and in the second last row
        indices += sorted(cols)
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64)


CSR_SPMM_CASES = [(7, 1, 2, True), (64, 0, 3, False), (130, 5, 1, False)]       # r, V ld_pad, Y ld_pad, V misaligned


def _csr_spmm_case(ctx, r, pv, py, mis, N=500):
    """The body of test_csr_spmm_guarded for N rows; returns Y."""
    ncols = 300
    rng = np.random.default_rng(r)
    indptr, indices = _csr(rng, N, ncols)
    data = exact_operands(rng, (1, len(indices)), 10)[0]
    V = exact_operands(rng, (ncols, r), 16, gd.graded_exponents(rng, r), k=8, partner_bits=10)
    Vd = guarded_operand(V, "C", pv, mis)
    dd = guarded_operand(data[None, :], "C", 0, not mis)
    Y = guarded_output((N, r), ld=r + py)
    ip, ix = torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda()
    ctx.check(ctx.lib.rt_csr_spmm(ctx.handle, P(ip), P(ix), P(dd), N, P(Vd), r + pv, r, P(Y.t), r + py), "rt_csr_spmm")
    A = sp.csr_matrix((data, indices, indptr), shape=(N, ncols))
    got = _host(Y.t)
    _exact(got, A @ V)
    _clean([Y], [(Vd, V), (dd, data[None, :])])
    return got


@pytest.mark.parametrize("r,pv,py,mis", CSR_SPMM_CASES)
def test_csr_spmm_guarded(ctx, r, pv, py, mis):
    _csr_spmm_case(ctx, r, pv, py, mis)


# ---- rt_project_csr_batched --------------------------------------------------------------------------------------------

def _banded_pattern(rng, N, extra=2):
    rows = []
    for i in range(N):
        cols = {c for c in (i - 1, i, i + 1) if 0 <= c < N} | set(rng.integers(0, N, size=extra).tolist())
        rows.append(sorted(cols))
    indptr = np.cumsum([0] + [len(c) for c in rows]).astype(np.int64)
    return indptr, np.concatenate([np.array(c, dtype=np.int64) for c in rows])


def _project_case(ctx, cus, N, r, B, dlay, dpad, vpad, vmis, route, extra=2, vguard=gd.GUARD):
    rng = np.random.default_rng(N + r + B)
    indptr, indices = _banded_pattern(rng, N, extra)
    nnz = len(indices)
    bv = 12 if nnz < (1 << 15) else 10
    assert nnz * 2.0 ** (2 * bv + 10) < 2.0 ** 53
    data = exact_operands(rng, (nnz, B), 10)
    V = exact_operands(rng, (N, r), bv, gd.graded_exponents(rng, r, 60))
    # guarded operands and output; written, bounded and intact are asserted in there (tests/guarded.py)
    got, info, Vd = gd.project_guarded(ctx, (indptr, indices), data, V, dlay, dpad, vpad, vmis, vguard)
    if route == "fused":
        rp = 16 * (-(-r // 16))
        assert info["tile"] == (rp, rp) and info["grid"] == B * info["splits"], info
    else:
        chunk = max(min(B, (2 << 30) // (8 * N * r)), 1)
        assert info == gd.gemm_plan(r, (r if chunk == 1 else chunk * r), N, False, True, cus), info
    for b in range(B):
        A = sp.csr_matrix((data[:, b], indices, indptr), shape=(N, N))
        _exact(got[b], V.T @ (A @ V))
    return Vd


PROJECT_CASES = [
    # id, N, r, B, data layout, data ld_pad, V ld_pad, V misalign, route
    ("fused_vec2", 3000, 32, 3, "C", 0, 0, False, "fused"),
    ("fused_odd_ldv", 3000, 32, 2, "F", 1, 1, False, "fused"),
    ("fused_misaligned_v", 2500, 24, 4, "C", 2, 0, True, "fused"),
    ("fused_odd_r", 2000, 17, 2, "F", 0, 1, False, "fused"),
    ("unfused_r_above_128", 2000, 130, 2, "C", 1, 0, False, "unfused"),
]


@pytest.mark.parametrize("case", PROJECT_CASES, ids=[c[0] for c in PROJECT_CASES])
def test_project_csr_batched_guarded(ctx, cus, case):
    _project_case(ctx, cus, *case[1:])


@pytest.mark.parametrize("ldv,route", [(4094, "fused"), (4096, "unfused")], ids=["fused_below_2_32", "unfused_at_2_32"])
def test_project_at_the_32bit_offset_limit(ctx, cus, ldv, route):
    """N * ldv * 8 bytes of V just below / exactly 2^32: the fused kernel's 32-bit offsets end there."""
    N, r = 131_072, 8
    try:
        Vd = _project_case(ctx, cus, N, r, 1, "F", 0, ldv - r, False, route, extra=0, vguard=1)
        del Vd
    finally:
        _free()


# ---- rt_deim_greedy ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,m,layout,pad,mis", [(3000, 40, "C", 0, False), (3000, 40, "C", 0, True), (2999, 37, "F", 1, False),
                                                (2000, 64, "F", 0, True), (1500, 20, "C", 3, False)])
def test_deim_greedy_guarded(ctx, N, m, layout, pad, mis):
    from romtime_amd import ops

    rng = np.random.default_rng(N + m)
    Phi = rng.standard_normal((N, m)) * np.ldexp(1.0, rng.integers(-30, 31, size=m))[None, :]
    tight = ops.to_device(np.asfortranarray(Phi) if layout == "F" else Phi)
    idx0, PT0, mg0 = ops.deim_greedy(tight)
    Pd = guarded_operand(Phi, layout, pad, mis)
    ld, lay = gd.leading_dim(Pd)
    idx = torch.empty(m, dtype=torch.int64, device="cuda")
    PT, mg = guarded_output((m, m)), guarded_output((m,))
    ctx.check(ctx.lib.rt_deim_greedy(ctx.handle, P(Pd), N, m, ld, LAY[lay], P(idx), P(PT.t), P(mg.t)), "rt_deim_greedy")
    assert torch.equal(idx, idx0)
    _exact(_host(PT.t), _host(PT0))
    _exact(_host(mg.t), _host(mg0))
    _exact(_host(PT.t), Phi[_host(idx)])
    _clean([PT, mg], [(Pd, Phi)])


# ---- rt_sym_eig_values_part / rt_sym_eig_vectors -----------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 200, 513, 1024])
def test_sym_eig_parts_guarded(ctx, n):
    """Slices of the spectrum (count 1, the last index, a middle block) are the full call's values bit for bit, within
    the bound of test_sym_eig_device, and nothing outside the slice is written; the eigenvectors of a slice that starts
    at first > 0 span the slice's invariant subspace (to the bound of test_sym_eig_device; see below why not bitwise)."""
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam_true = np.sort(10.0 ** (-16.0 * np.arange(n) / max(n - 1, 1)))[::-1]
    G = (Q * lam_true) @ Q.T
    G = 0.5 * (G + G.T)
    Gd = guarded_operand(G, "C", 0, n % 2 == 1)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lam_full = torch.empty(n, dtype=torch.float64, device="cuda")
    ctx.check(ctx.lib.rt_sym_eig_values(ctx.handle, P(Gd), n, P(lam_full), P(status)), "rt_sym_eig_values")
    W_full = guarded_output((n, n))
    ctx.check(ctx.lib.rt_sym_eig_vectors(ctx.handle, n, n, P(lam_full), P(W_full.t)), "rt_sym_eig_vectors")
    assert int(status.item()) == 0
    ref = np.linalg.eigvalsh(G)[::-1]
    full = _host(lam_full)
    assert np.abs(full - ref).max() <= 20 * n * 2.2e-16 * abs(ref[0])
    _clean([W_full])
    slices = sorted({(0, 1), (n - 1, 1), (n // 3, max(1, n // 4)), (1, n - 1)})
    for first, count in slices:
        lam = guarded_output((n,))
        ctx.check(ctx.lib.rt_sym_eig_values_part(ctx.handle, P(Gd), n, first, count, P(lam.t), P(status)),
                  "rt_sym_eig_values_part")
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        part = lam.t[first:first + count].cpu().numpy()
        _exact(part, full[first:first + count])
        # only [first, first + count) written: the rest of lam still holds the canary
        bits = lam.t.view(torch.int64).cpu().numpy()
        outside = np.r_[bits[:first], bits[first + count:]]
        assert np.all(outside == gd.CANARY_BITS), (first, count)
        lam.prefilled = True
        assert lam.check() == []
        if first > 0 and first + count == n:
            W = guarded_output((n, count))
            ctx.check(ctx.lib.rt_sym_eig_vectors(ctx.handle, n, count, P(lam.t[first:]), P(W.t)), "rt_sym_eig_vectors")
            # Not bitwise: inverse iteration seeds the start vector of column t from t itself (symeig.hip), so a slice
            # that starts at first > 0 starts its vectors elsewhere - signs differ, and so do the vectors of the
            # eigenvalues at the rounding floor.  The bound of test_sym_eig_device (an invariant subspace of the
            # slice's eigenvalues) holds instead.
            Wh = _host(W.t)
            Qs, _ = np.linalg.qr(Wh)
            H = Qs.T @ G @ Qs
            assert np.abs(G @ Qs - Qs @ H).max() <= 1e-10 * abs(ref[0])
            np.testing.assert_allclose(np.sort(np.linalg.eigvalsh(H))[::-1], ref[first:], rtol=0, atol=1e-11 * abs(ref[0]))
            _clean([W])
    _clean([], [(Gd, G)])


# ---- rt_pod_backproject_weights, rt_gram_scale (no exact answer: a few ulps per entry) --------------------------------

def _within_ulps(got, ref, ulps):
    ref = np.asarray(ref, dtype=np.longdouble)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref)
    bound = ulps * ULP * np.abs(ref)
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, f"{len(bad)} entries beyond {ulps} ulps, first {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("n,k,with_norms,mis", [(200, 40, True, False), (513, 513, True, True), (3, 1, False, True),
                                                (100, 64, False, False)])
def test_backproject_weights_guarded(ctx, n, k, with_norms, mis):
    rng = np.random.default_rng(n + k)
    Z = rng.uniform(-1, 1, (n, k)) * np.ldexp(1.0, rng.integers(-100, 101, size=k))[None, :]
    lam = rng.uniform(1, 2, n) * np.ldexp(1.0, rng.integers(-100, 101, size=n))
    lam[n // 2:: 7] = 0.0
    lam[n - 1] = -lam[0] if n > 1 else lam[0]
    cn = rng.uniform(1, 2, n) * np.ldexp(1.0, rng.integers(-50, 51, size=n))
    Zd = guarded_operand(Z, "C", 0, mis)
    lamd = guarded_operand(lam[None, :], "C", 0, not mis)
    cnd = guarded_operand(cn[None, :], "C", 0, mis) if with_norms else None
    out = guarded_output((n, k), misalign=not mis)
    ctx.check(ctx.lib.rt_pod_backproject_weights(ctx.handle, P(Zd), n, k, P(cnd), P(lamd), P(out.t)),
              "rt_pod_backproject_weights")
    L = lam[:k].astype(np.longdouble)
    inv = np.where(L > 0, 1 / np.sqrt(np.where(L > 0, L, 1)), 0)
    ref = Z.astype(np.longdouble) / (cn.astype(np.longdouble)[:, None] if with_norms else 1) * inv[None, :]
    got = _host(out.t)
    assert np.all(got[:, lam[:k] <= 0] == 0)
    _within_ulps(got, ref, 4)
    _clean([out], [(Zd, Z), (lamd, lam[None, :])] + ([(cnd, cn[None, :])] if with_norms else []))


@pytest.mark.parametrize("n,normalize", [(3, 1), (200, 1), (777, 1), (200, 0)])
def test_gram_scale_guarded(ctx, n, normalize):
    rng = np.random.default_rng(n + normalize)
    X = exact_operands(rng, (500, n), 16, gd.graded_exponents(rng, n, 60), k=500)
    G0 = X.T @ X
    G = guarded_output((n, n), misalign=bool(n % 2)).fill(G0)
    cn = guarded_output((n,), misalign=not n % 2)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.check(ctx.lib.rt_gram_scale(ctx.handle, P(G.t), n, P(cn.t), normalize, P(flag)), "rt_gram_scale")
    d = np.sqrt(np.diag(G0).astype(np.longdouble))
    _within_ulps(_host(cn.t), d, 1)
    got = _host(G.t)
    if normalize:
        ref = G0.astype(np.longdouble) / (d[:, None] * d[None, :])
        np.fill_diagonal(ref, 1)
        _within_ulps(got, ref, 4)
    else:
        _exact(got, G0)
    assert int(flag.item()) == 0
    _clean([G, cn])
