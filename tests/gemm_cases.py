"""The dense products on every GEMM tile shape and CU share: the cases, and the launch rules they rest on, in NumPy.

gemm_mfma.hip instantiates gemm_f64_mfma_kernel<MT, NT, KCA, KCB, SKINNY> 80 times (4 x 4 tile shapes x 4 operand layouts,
and 4 skinny widths x 4 layouts).  Which one a call takes depends on the output's extents, the operands' strides and the CUs
the ctx sizes its grids for: a product with fewer output tiles than CUs narrows its tile, so on the whole chip (256 CUs)
everything below about 30 000 output columns runs NT = 1.  With the ctx option "cu_limit" at 8 the narrowing stops at 8
tiles and outputs below 130 x 1030 reach every instantiation; tests/test_gemm_cases_cpu.py holds that as a condition.

``gemm_variant``, ``tallskinny_variant``, ``rank_update_trips`` and ``spmm_passes`` restate rt_gemm_strided, rt_tallskinny,
rt_rank_update and spmm_launch; tile and split counts come from tests/guarded.py (gemm_plan), which the GPU tests compare
with Context.launch_info.  One case table per kernel; each GEMM case names its CU share, its entry point (rt_gemm_tn: any
m x n output, both layouts of both operands, symmetric when A is B, split contraction; rt_gemm_nn_axpby: the direct store
with alpha and beta, both layouts of Y), its operand layouts, leading-dimension padding and 8-byte misalignment, and its
contraction length.  tests/test_dense_shares_gpu.py runs them."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import guarded as gd
from tests.guarded import _cdiv, exact_operands, graded_exponents

SHARES = (0, 224, 32, 8)          # "cu_limit": the whole chip, the POD pipeline's two streams, the smallest the option takes
CHIP_CUS = 256                    # the MI355X; what share 0 stands for wherever a rule is evaluated without a device
KB = 16                           # contraction depth of one LDS stage (gemm_panel.h)


def share_cus(share, device_cus=CHIP_CUS):
    return share or device_cus


# ---- the launch rules, restated -------------------------------------------------------------------------------------------

def gemm_variant(M, Nn, symmetric, a_ks, a_ms, b_ks, b_ns, aligned_a, aligned_b, cus):
    """(MT, NT, KCA, KCB, SKINNY, vecA, vecB) of rt_gemm_strided (gemm_mfma.hip) for an M x Nn output of operands with
    contraction strides a_ks / b_ks and tile strides a_ms / b_ns whose base pointers are 16-byte aligned or not.  The skinny
    form has MT = 2 (four waves x 32 rows) and NT = 16-column tiles; the tile itself is gemm_plan's."""
    kca = a_ks == 1 and not (a_ms == 1 and M > 1)
    kcb = b_ks == 1 and not (b_ns == 1 and Nn > 1)
    BM, BN = gd.gemm_plan(M, Nn, 1, symmetric, False, cus)["tile"]
    skinny = not symmetric and Nn <= 64 and M >= 256       # the rule launch_info cannot show: (128, 32) exists in both forms
    mt, nt = (2, BN // 16) if skinny else (BM // 32, BN // 32)

    def vec(aligned, ks, ms, kc):                          # 16-byte loads: the pair contiguous and aligned for every (k, m)
        contiguous, other = (ks, ms) if kc else (ms, ks)
        return int(bool(aligned) and other % 2 == 0 and contiguous == 1)

    return mt, nt, kca, kcb, skinny, vec(aligned_a, a_ks, a_ms, kca), vec(aligned_b, b_ks, b_ns, kcb)


def tallskinny_variant(N, k, cus):
    """(KF, G, RB) of rt_tallskinny (tallskinny.hip): whole 16-column tiles, groups of four remainder columns, 16-row blocks
    per wave.  A remainder of 13 .. 15 columns stays a padded tile."""
    nt, c = _cdiv(k, 16), k % 16
    whole = c == 0 or c >= 13
    return (nt if whole else nt - 1), (0 if whole else _cdiv(c, 4)), (2 if nt <= 4 and N >= 512 * cus else 1)


def tallskinny_dispatchable():
    """Every instantiation behind rt_tallskinny's switch: KF = 0 with 1 .. 3 groups, KF = 1 .. 7 with 0 .. 3, KF = 8 alone,
    each with one row block per wave, and with two where the accumulators fit (KF + (G > 0) <= 4)."""
    one = [(0, g) for g in (1, 2, 3)] + [(kf, g) for kf in range(1, 8) for g in range(4)] + [(8, 0)]
    return {(kf, g, 1) for kf, g in one} | {(kf, g, 2) for kf, g in one if kf + (g > 0) <= 4}


def rank_update_trips(N, n, cus):
    """(trips of the busiest workgroup through rank_update_kernel's row loop, stages, gx) - rt_rank_update."""
    stages, gy = _cdiv(N, 32), _cdiv(n, 128)
    gx = min(max(8 * cus // gy, 1), stages)
    return _cdiv(stages, gx), stages, gx


def spmm_passes(N, cus):
    """(passes of csr_spmm_kernel's row loop, rows of the last pass) - spmm_launch (sparse.hip): one wave per row, four per
    block, at most 8 blocks per CU."""
    rows = 4 * max(min(_cdiv(N, 4), 8 * cus), 1)
    return _cdiv(N, rows), N - (_cdiv(N, rows) - 1) * rows


# ---- the GEMM table -------------------------------------------------------------------------------------------------------

GemmCase = namedtuple("GemmCase", "id entry share K M Nn la lb pa pb mis_a mis_b lc pc sym alpha beta")
GemmCase.__doc__ = """entry "tn": C (M x Nn, row-major, ld = Nn + pc) = A^T B through rt_gemm_tn, A (K x M) and B (K x Nn) in
layouts la / lb with ld padding pa / pb, 8 bytes off a 16-byte boundary with mis_a / mis_b; sym: B is A.
entry "nn": Y (M x Nn, layout lc, ld padding pc) = alpha X T + beta Y through rt_gemm_nn_axpby, X (M x K) in layout la, T
(K x Nn) row-major: the contraction of X is contiguous where X is row-major."""

_ALIGN = ("vec", "odd", "mis", "vec2")


def _pad(width, mode):
    """(ld padding, misaligned) that make 16-byte loads possible ("vec", "vec2": even ld, aligned base) or not ("odd": odd
    ld; "mis": even ld, base 8 bytes off).  A line of one element gets ld = 3, not 1: with both strides 1 the library could
    not tell the layouts apart."""
    even = width % 2
    return {"vec": (even, False), "vec2": (even + 2, False), "odd": (2 if width == 1 else 1 - even, False),
            "mis": (even, True)}[mode]


def _tn(cid, share, K, M, Nn, la, lb, va, vb, pc, sym=False):
    pa, mis_a = _pad(M if la == "C" else K, va)
    pb, mis_b = (pa, mis_a) if sym else _pad(Nn if lb == "C" else K, vb)
    return GemmCase(cid, "tn", share, K, M, Nn, la, la if sym else lb, pa, pb, mis_a, mis_b, "C", pc, sym, 1.0, 0.0)


def _nn(cid, share, K, M, Nn, lx, vx, vt, ly, py, alpha, beta):
    pa, mis_a = _pad(K if lx == "C" else M, vx)
    pb, mis_b = _pad(Nn, vt)
    return GemmCase(cid, "nn", share, K, M, Nn, lx, "C", pa, pb, mis_a, mis_b, ly, py, False, alpha, beta)


_LAYOUTS = (("C", "C"), ("C", "F"), ("F", "C"), ("F", "F"))
_SMALL_K = (1, 15, 16, 17, 33, 45)                  # one stage and its edges; odd K: a k-contiguous pair straddles kend
_SPLIT_K = (133, 300, 1285)                         # 2 x 128 with a last split of 5 rows; 2 x 160 (140); 8 x 176 (53)
# extents one below, at and one above the edges of the tiles.  MT follows from M alone (1 .. 32 -> 1, ..., 97 and up -> 4),
# so only BM = 128 has a second row of tiles; at 8 CUs a row of tiles keeps NT while it has 8 tiles and NT + 1 would not.
_M = {1: (1, 31, 32, 17), 2: (33, 63, 64, 50), 3: (65, 95, 96, 80), 4: (97, 127, 128, 129)}
_N_ONE_ROW = {1: (31, 32, 33, 447), 2: (449, 511, 512, 513), 3: (673, 767, 768, 769), 4: (897, 1023, 1024, 1025)}
_N_TWO_ROWS = {1: 192, 2: 257, 3: 289, 4: 513}      # under M = 129
_M_SKINNY = (256, 257, 383, 385)
_N_SKINNY = {1: (1, 15, 16, 9), 2: (17, 31, 32, 24), 3: (33, 47, 48, 40), 4: (49, 63, 64, 56)}


def _gemm_cases():
    cases = []
    # every generic instantiation at 8 CUs, the contraction inside one or a few stages, no split
    for mt in (1, 2, 3, 4):
        for nt in (1, 2, 3, 4):
            for i, (la, lb) in enumerate(_LAYOUTS):
                M = _M[mt][i]
                Nn = _N_TWO_ROWS[nt] if M == 129 else _N_ONE_ROW[nt][i]
                K = _SMALL_K[(4 * mt + nt + i) % len(_SMALL_K)]
                cases.append(_tn(f"tile{32 * mt}x{32 * nt}_{la}{lb}_M{M}_N{Nn}_K{K}", 8, K, M, Nn, la, lb,
                                 _ALIGN[(mt + i) % 4], _ALIGN[(nt + 2 * i + 1) % 4], 1 + (mt + nt + i) % 5))
    # every generic tile with a split contraction: 8 tiles (2 of 32 columns) leave 2 (8) slots each at 8 CUs; two splits
    # pad the grid to eight per tile, six of which return at once
    for mt in (1, 2, 3, 4):
        for nt in (1, 2, 3, 4):
            la, lb = _LAYOUTS[(mt + 2 * nt) % 4]
            M, Nn = _M[mt][2 if nt > 1 else 1], (_N_ONE_ROW[nt][1] if nt > 1 else 33)
            K = _SPLIT_K[(mt + nt) % 3]
            cases.append(_tn(f"split{32 * mt}x{32 * nt}_{la}{lb}_M{M}_N{Nn}_K{K}", 8, K, M, Nn, la, lb,
                             _ALIGN[(mt + nt) % 4], _ALIGN[(mt + 2 * nt) % 4], 2 + (mt + nt) % 3))
    # symmetric (A is B): MT = NT, never narrowed, always through the slab and the mirrored reduction
    for cid, share, K, m, lay, va in [("sym32", 8, 17, 20, "C", "vec"), ("sym64", 8, 133, 64, "F", "vec"),
                                      ("sym96", 8, 1, 95, "C", "odd"), ("sym128_one_tile", 8, 300, 127, "F", "mis"),
                                      ("sym128_diag_and_off", 8, 300, 129, "C", "vec2"),
                                      ("sym128_three_rows_share32", 32, 1285, 300, "F", "odd"),
                                      ("sym128_share224", 224, 2000, 150, "C", "mis"),
                                      ("sym64_chip", 0, 1285, 40, "F", "vec")]:
        cases.append(_tn(f"{cid}_{lay}_m{m}_K{K}", share, K, m, m, lay, lay, va, va, 3, sym=True))
    # every skinny instantiation (M >= 256, at most 64 columns: the rule knows no CU count), one split per width
    for snt in (1, 2, 3, 4):
        for i, (la, lb) in enumerate(_LAYOUTS):
            M, Nn, share = _M_SKINNY[(snt + i) % 4], _N_SKINNY[snt][i], (8, 32, 224, 8)[i]
            K = (_SMALL_K + _SPLIT_K[:2])[(2 * snt + 3 * i) % 8]
            cases.append(_tn(f"skinny128x{16 * snt}_{la}{lb}_M{M}_N{Nn}_K{K}_share{share}", share, K, M, Nn, la, lb,
                             _ALIGN[(snt + i + 1) % 4], _ALIGN[(snt + 3 * i) % 4], 1 + i))
    # a split count that is no multiple of 8 and above it: 11 splits in a grid padded to 16, the last 5 rows long
    cases.append(_tn("split11_of_16_share32", 32, 1285, 20, 20, "C", "F", "vec", "vec", 4))
    cases.append(_tn("split5_of_8_share32", 32, 517, 100, 90, "F", "C", "mis", "odd", 2))
    # the production shares and the whole chip: the narrowing goes all the way to 32 columns, the splits are many
    cases.append(_tn("lift_shape_share224", 224, 300, 129, 200, "C", "C", "vec", "vec", 5))
    cases.append(_tn("lift_shape_chip", 0, 300, 129, 200, "F", "F", "vec", "mis", 5))
    cases.append(_tn("lift_shape_share32", 32, 300, 129, 300, "C", "F", "odd", "vec", 1))
    cases.append(_tn("wide_share32", 32, 45, 65, 700, "F", "C", "vec", "vec", 3))
    # one row short of the skinny form: two rows of generic 128 x 32 tiles
    cases.append(_tn("below_skinny_M255", 8, 17, 255, 40, "F", "C", "vec", "odd", 2))
    # rt_gemm_nn_axpby: the direct store with c_alpha and c_beta into both layouts of Y, never split; T is row-major, so
    # KCB is false unless T is a single contiguous column
    for cid, share, K, M, Nn, lx, vx, vt, ly, py, alpha, beta in [
            ("nn_64x32_colmajor_y", 8, 15, 33, 1, "F", "vec", "odd", "F", 3, 0.5, -2.0),
            ("nn_one_column_contiguous_t", 8, 17, 50, 1, "C", "vec", "vec", "C", 2, -2.0, 0.5),
            ("nn_96x96_rowmajor_y", 8, 16, 65, 700, "F", "mis", "vec", "C", 5, -1.0, 0.0),
            ("nn_96x96_x_rowmajor", 8, 45, 96, 768, "C", "vec", "mis", "F", 1, 2.0, 0.25),
            ("nn_128x96_lift", 8, 70, 129, 289, "C", "odd", "vec", "C", 3, 0.5, 1.0),
            ("nn_128x64_lift_plain", 8, 100, 129, 257, "F", "vec", "vec2", "C", 0, 1.0, 0.0),
            ("nn_32x128", 8, 1, 31, 900, "F", "odd", "odd", "F", 2, -0.5, -1.0),
            ("nn_skinny128x48", 8, 33, 300, 40, "C", "vec", "vec", "C", 1, 2.0, -0.5),
            ("nn_skinny128x16_colmajor", 32, 17, 257, 9, "F", "vec", "odd", "F", 4, -1.0, 2.0),
            ("nn_share224", 224, 64, 300, 130, "C", "vec", "vec", "F", 1, 0.25, 1.0),
            ("nn_chip", 0, 40, 300, 100, "F", "odd", "vec", "C", 3, 0.5, -2.0)]:
        cases.append(_nn(cid, share, K, M, Nn, lx, vx, vt, ly, py, alpha, beta))
    assert len({c.id for c in cases}) == len(cases)
    return cases


GEMM_CASES = _gemm_cases()


def case_strides(case):
    """(a_ks, a_ms, b_ks, b_ns, lda, ldb) as the entry point hands them to rt_gemm_strided."""
    if case.entry == "tn":
        lda = (case.M if case.la == "C" else case.K) + case.pa
        ldb = (case.Nn if case.lb == "C" else case.K) + case.pb
        a = (lda, 1) if case.la == "C" else (1, lda)
        b = (ldb, 1) if case.lb == "C" else (1, ldb)
    else:
        lda = (case.K if case.la == "C" else case.M) + case.pa
        ldb = case.Nn + case.pb
        a = (1, lda) if case.la == "C" else (lda, 1)
        b = (ldb, 1)
    return a + b + (lda, ldb)


def case_variant(case, cus=None):
    a_ks, a_ms, b_ks, b_ns, _, _ = case_strides(case)
    cus = share_cus(case.share) if cus is None else cus
    return gemm_variant(case.M, case.Nn, case.sym, a_ks, a_ms, b_ks, b_ns, not case.mis_a, not case.mis_b, cus)


def case_plan(case, cus=None):
    """launch_info of the case: rt_gemm_tn may split the contraction, rt_gemm_nn_axpby never does."""
    cus = share_cus(case.share) if cus is None else cus
    return gd.gemm_plan(case.M, case.Nn, case.K, case.sym, case.entry == "tn", cus)


def split_lengths(case, cus=None):
    """Rows of the contraction each split takes (rt_gemm_strided: at least 128 per split, whole stages)."""
    cus = share_cus(case.share) if cus is None else cus
    plan = case_plan(case, cus)
    if plan["splits"] == 1:
        return [case.K]
    tm, tn = _cdiv(case.M, plan["tile"][0]), _cdiv(case.Nn, plan["tile"][1])
    s0 = 2 * cus // (tm * (tm + 1) // 2 if case.sym else tm * tn)
    if s0 >= 8:
        s0 &= ~7
    kps = _cdiv(max(_cdiv(case.K, s0), 128), KB) * KB
    assert _cdiv(case.K, kps) == plan["splits"]
    return [min(kps, case.K - s * kps) for s in range(plan["splits"])]


def exact_bits(k, cap=18):
    """Largest integer width (<= cap) at which k products of two such integers sum below 2^53."""
    b = cap
    while k * 2.0 ** (2 * b) >= 2.0 ** 53:
        b -= 1
    return b


def gemm_operands(case):
    """Host operands and the exact answer of a case: dict(A, B, ref) for "tn", dict(X, T, Y0, ref) for "nn".  Integers scaled
    by powers of two (tests/guarded.py); exact_operands refuses a contraction whose partial sums could reach 2^53, and the
    "nn" cases also need alpha * (X T) + beta * Y0 inside 53 bits from the smaller of the two units."""
    rng = np.random.default_rng(sum(map(ord, case.id)))
    K, M, Nn = case.K, case.M, case.Nn
    if case.entry == "tn":
        b = exact_bits(K)
        A = exact_operands(rng, (K, M), b, graded_exponents(rng, M), k=K)
        B = A if case.sym else exact_operands(rng, (K, Nn), b, graded_exponents(rng, Nn), k=K)
        return dict(A=A, B=B, ref=A.T @ B)
    b = exact_bits(2 * K + 2)
    unit = min(abs(case.alpha), abs(case.beta)) if case.beta != 0.0 else abs(case.alpha)
    assert (abs(case.alpha) * K * 2.0 ** (2 * b) + abs(case.beta) * 1024) / unit < 2.0 ** 53, case.id
    for s in (case.alpha, case.beta):
        assert s == 0.0 or np.frexp(abs(s))[0] == 0.5, f"{case.id}: {s} is no power of two"
    g, f = graded_exponents(rng, M, 60), graded_exponents(rng, Nn, 60)
    X = exact_operands(rng, (K, M), b, g).T                   # rows of X graded
    T = exact_operands(rng, (K, Nn), b, f, k=K + 1)           # columns of T graded
    Y0 = np.ldexp(rng.integers(-1024, 1025, size=(M, Nn)).astype(np.float64), g[:, None] + f[None, :])
    ref = case.alpha * (X @ T) + (case.beta * Y0 if case.beta != 0.0 else 0.0)
    return dict(X=X, T=T, Y0=Y0, ref=ref)


# ---- the other dense routes -----------------------------------------------------------------------------------------------

# rt_tallskinny: (id, share, rows beyond the threshold: N = factor * cus + extra, n, the k to run).  Three stages of the
# contraction (n = 96) at every k the kernel takes; a ragged stage (n = 70) at one k per group count G = 0 .. 3.
TALLSKINNY_SWEEPS = [
    ("one_row_block", 8, (64, 37), 96, tuple(range(1, 129))),
    ("two_row_blocks", 8, (512, 129), 96, tuple(range(1, 65))),
    ("one_row_block_ragged_stage", 8, (64, 37), 70, (32, 20, 8, 44, 109)),
    ("two_row_blocks_ragged_stage", 8, (512, 129), 70, (64, 36, 24, 12)),
]


def tallskinny_cases():
    """(id, share, N, n, k) of every run of the sweeps."""
    return [(f"{sid}_k{k}", share, f * share_cus(share) + extra, n, k)
            for sid, share, (f, extra), n, ks in TALLSKINNY_SWEEPS for k in ks]


# rt_skinny_tn (C/C operands, m <= 16, N >= 16384, N n >= 2^22): id, share, N, m, n, B ld padding, B misaligned, A ld padding
SKINNY_TN_CASES = [(f"m{m}", 0, 16_384, m, 256, 0, False, m % 3) for m in range(1, 17)] + \
                  [(f"m{m}_odd_n_misaligned_share8", 8, 16_384, m, 257, 1, True, 1) for m in (1, 9, 16)]

# rt_rank_update, the row loop turning over: 102 stages on 32 workgroups per strip at 8 CUs, four trips for six of them.
# Fields as RANK_UPDATE_CASES of tests/test_guarded_kernels_gpu.py:
# id, N, n, k, colscale, Ysrc ld_pad, Ydst ld_pad, misalign src, misalign dst, in place, alpha
RANK_UPDATE_TRIP_CASES = [
    ("trips_vector", 3239, 130, 5, True, 0, 2, False, False, False, -1.0),
    ("trips_scalar_odd_ld", 3239, 130, 5, False, 1, 2, False, False, False, 0.5),
    ("trips_in_place_vector", 3239, 130, 64, True, 2, 2, False, False, True, -1.0),
    ("trips_in_place_scalar_misaligned", 3239, 131, 3, False, 0, 0, True, True, True, 2.0),
]

# rt_csr_spmm and the unfused projection, the row loop turning over: 1100 rows are 4 passes of 256 and one of 76 at 8 CUs
SPMM_TRIP_ROWS = 1100
SPMM_TRIP_CASES = [(7, 1, 2, True), (130, 5, 1, False)]                 # r, V ld_pad, Y ld_pad, V misaligned
PROJECT_TRIP_CASE = ("unfused_r_above_128_row_passes", SPMM_TRIP_ROWS, 130, 3, "C", 1, 0, False, "unfused")
