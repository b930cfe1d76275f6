"""The premises of tests/test_dense_shares_gpu.py, as conditions on the case tables (tests/gemm_cases.py): every
instantiation of the strided GEMM, of the tall-skinny product and of rt_skinny_tn is reached, the stride loops turn over, and
every case's data is exact.  A table that loses coverage, or a launch rule that moves, fails here without a GPU."""
import numpy as np
import pytest

from tests import gemm_cases as gc
from tests import guarded as gd

GENERIC = {(mt, nt, a, b, False) for mt in (1, 2, 3, 4) for nt in (1, 2, 3, 4) for a in (False, True) for b in (False, True)}
SKINNY = {(2, nt, a, b, True) for nt in (1, 2, 3, 4) for a in (False, True) for b in (False, True)}


def _variants(cus=None):
    return {gc.case_variant(c, cus)[:5] for c in gc.GEMM_CASES}


def test_every_gemm_instantiation_is_reached_at_the_chosen_shares():
    got = _variants()
    print(f"GEMM instantiations reached at the cases' shares: {len(got)} of {len(GENERIC | SKINNY)}")
    assert len(GENERIC | SKINNY) == 80 and got == GENERIC | SKINNY, sorted((GENERIC | SKINNY) - got)
    assert {c.share for c in gc.GEMM_CASES} == set(gc.SHARES)
    assert {(c.entry, c.lc) for c in gc.GEMM_CASES} == {("tn", "C"), ("nn", "C"), ("nn", "F")}
    assert {c.la for c in gc.GEMM_CASES if c.entry == "nn"} == {"C", "F"}


def test_the_whole_chip_alone_reaches_a_strict_subset():
    """Why the cases run on shares: at 256 CUs the narrowing rule sends every output of the table to 32-column tiles, so only
    NT = 1, the symmetric MT = NT tiles and the skinny form are left."""
    got = _variants(gc.CHIP_CUS)
    print(f"GEMM instantiations the same table reaches on {gc.CHIP_CUS} CUs alone: {len(got)} of 80")
    assert len(got) == 36 and got < GENERIC | SKINNY
    assert SKINNY <= got                                             # the skinny rule knows no CU count
    wide = {v for v in got if not v[4] and v[1] != 1}
    assert {v[:2] for v in wide} == {(2, 2), (3, 3), (4, 4)} and all(v[2] == v[3] for v in wide)   # the symmetric cases


def test_every_generic_tile_occurs_split_and_every_square_one_symmetric():
    split = {gc.case_variant(c)[:2] for c in gc.GEMM_CASES
             if not c.sym and not gc.case_variant(c)[4] and gc.case_plan(c)["splits"] > 1}
    assert split == {(mt, nt) for mt in (1, 2, 3, 4) for nt in (1, 2, 3, 4)}
    assert {gc.case_variant(c)[3:5] for c in gc.GEMM_CASES if gc.case_plan(c)["splits"] > 1} >= {(False, True), (True, True)}
    sym = [c for c in gc.GEMM_CASES if c.sym]
    assert {gc.case_variant(c)[:2] for c in sym} == {(mt, mt) for mt in (1, 2, 3, 4)}
    assert all(c.entry == "tn" and c.M == c.Nn and (c.la, c.pa, c.mis_a) == (c.lb, c.pb, c.mis_b) for c in sym)
    # both the diagonal tiles (B panel never loaded) and the off-diagonal ones, whose mirror the reduction reads
    assert any(gd._cdiv(c.M, gc.case_plan(c)["tile"][0]) >= 2 for c in sym)
    # no split at all on the direct-store entry, whatever the share
    assert all(gc.case_plan(c)["splits"] == 1 for c in gc.GEMM_CASES if c.entry == "nn")
    assert {(c.alpha != 1.0, c.beta != 0.0) for c in gc.GEMM_CASES if c.entry == "nn"} == {(True, True), (True, False), (False, False)}


def test_vector_and_scalar_loads_in_both_panel_forms():
    seen = set()
    for c in gc.GEMM_CASES:
        _, _, kca, kcb, _, va, vb = gc.case_variant(c)
        seen |= {("A", kca, va), ("B", kcb, vb)}
    assert seen == {(op, kc, v) for op in "AB" for kc in (False, True) for v in (0, 1)}
    # each way of losing the vector loads: an odd leading dimension, a base 8 bytes off
    assert {(c.mis_a, gc.case_strides(c)[4] % 2) for c in gc.GEMM_CASES} == {(False, 0), (False, 1), (True, 0)}


def test_contraction_lengths():
    by_k = {}
    for c in gc.GEMM_CASES:
        by_k.setdefault(c.K, []).append(c)
    assert {1, 15, 16, 17} <= set(by_k)
    # an odd K on a k-contiguous operand: the last pair of a line straddles kend, with and without vector loads
    odd = {gc.case_variant(c)[5] for c in gc.GEMM_CASES if c.K % 2 and c.K > 1 and gc.case_variant(c)[2]}
    assert odd == {0, 1}
    lengths = [gc.split_lengths(c) for c in gc.GEMM_CASES if gc.case_plan(c)["splits"] > 1]
    assert all(sum(ls) == c.K and min(ls) >= 1 for c, ls in
               ((c, gc.split_lengths(c)) for c in gc.GEMM_CASES))
    assert any(ls[-1] < gc.KB for ls in lengths)                    # a last split shorter than one stage
    assert any(gc.KB < ls[-1] < ls[0] and ls[-1] % gc.KB for ls in lengths)
    counts = {len(ls) for ls in lengths}
    # padded grids: splits % 8 != 0 leaves workgroups that return at s >= splits, below and above eight
    assert any(n < 8 for n in counts) and any(n > 8 and n % 8 for n in counts) and any(n % 8 == 0 for n in counts)
    for c in gc.GEMM_CASES:
        plan = gc.case_plan(c)
        assert plan["grid"] % 8 == 0 or plan["splits"] == 1


def test_extents_sit_on_both_sides_of_every_tile_edge():
    rows = {bm: set() for bm in (32, 64, 96, 128)}
    cols = {bn: set() for bn in (32, 64, 96, 128)}
    srows, scols = set(), {bn: set() for bn in (16, 32, 48, 64)}
    for c in gc.GEMM_CASES:
        (bm, bn), skinny = gc.case_plan(c)["tile"], gc.case_variant(c)[4]
        if skinny:
            srows.add(c.M)
            scols[bn].add(c.Nn)
        else:
            rows[bm].add(c.M)
            cols[bn].add(c.Nn)
    for bm in (32, 64, 96):                                           # M picks MT, so M = BM + 1 is the next tile shape
        assert {bm - 1, bm} <= rows[bm] and bm - 31 in rows[bm]
    assert {127, 128, 129, 255} <= rows[128] and {256, 257, 383, 385} <= srows     # 256 rows: the skinny form begins
    for bn in (32, 64, 96, 128):
        assert any({t * bn - 1, t * bn, t * bn + 1} <= cols[bn] for t in range(1, 9)), (bn, sorted(cols[bn]))
    for bn in (16, 32, 48, 64):
        assert {bn - 15, bn - 1, bn} <= scols[bn], (bn, sorted(scols[bn]))
    assert max(c.M for c in gc.GEMM_CASES) <= 385 and max(c.Nn for c in gc.GEMM_CASES) <= 1025
    assert max(c.K for c in gc.GEMM_CASES) <= 2000


def test_no_gemm_case_is_taken_by_another_kernel():
    for c in gc.GEMM_CASES:
        for share in gc.SHARES:
            cus = gc.share_cus(share)
            if c.entry == "tn":
                assert gd.skinny_tn_plan(c.K, c.M, c.Nn, cus) is None
            elif (c.la, c.lc, c.alpha, c.beta) == ("C", "C", 1.0, 0.0):
                assert gd.tallskinny_plan(c.M, c.K, c.Nn, cus) is None and not (c.M <= 64 and c.Nn >= 256)


def test_every_case_is_exact():
    """exact_operands refuses a contraction whose partial sums could reach 2^53: called with each case's real K."""
    for c in gc.GEMM_CASES:
        ops = gc.gemm_operands(c)
        assert ops["ref"].shape == (c.M, c.Nn) and np.isfinite(ops["ref"]).all(), c.id
    rng = np.random.default_rng(0)
    with pytest.raises(AssertionError):
        gd.exact_operands(rng, (2, 2), 18, k=1 << 17)
    for _, _, N, n, k in gc.tallskinny_cases():
        gd.exact_operands(rng, (1, 1), gc.exact_bits(2 * n + 2), k=n + 1)
    for _, _, N, m, n, *_ in gc.SKINNY_TN_CASES:
        gd.exact_operands(rng, (1, 1), gc.exact_bits(N), k=N)
    for case in gc.RANK_UPDATE_TRIP_CASES:
        gd.exact_operands(rng, (1, 1), 16, k=case[3] + 1)


def test_every_tallskinny_instantiation_is_reached():
    want = gc.tallskinny_dispatchable()
    got = {gc.tallskinny_variant(N, k, gc.share_cus(share)) for _, share, N, n, k in gc.tallskinny_cases()}
    print(f"tall-skinny instantiations reached: {len(got)} of {len(want)}")
    assert len(want) == 32 + 16 and got == want
    for _, share, N, n, k in gc.tallskinny_cases():
        cus = gc.share_cus(share)
        plan = gd.tallskinny_plan(N, n, k, cus)
        assert plan is not None and plan["tile"] == (64 * gc.tallskinny_variant(N, k, cus)[2], 16 * gd._cdiv(k, 16))
    ragged = {(gc.tallskinny_variant(N, k, gc.share_cus(s))[1:]) for _, s, N, n, k in gc.tallskinny_cases() if n % 32}
    assert ragged == {(g, rb) for g in range(4) for rb in (1, 2)}


def test_every_skinny_tn_row_count_is_reached():
    assert {c[3] for c in gc.SKINNY_TN_CASES if c[1] == 0} == set(range(1, 17))
    small = [c for c in gc.SKINNY_TN_CASES if c[1] == 8]
    assert {c[3] for c in small} == {1, 9, 16} and all(c[4] % 2 and c[6] for c in small)      # odd n, misaligned B
    for _, share, N, m, n, *_ in gc.SKINNY_TN_CASES:
        assert gd.skinny_tn_plan(N, m, n, gc.share_cus(share)) is not None
        assert gd.skinny_tn_plan(N - 1, m, n, gc.share_cus(share)) is None                      # the smallest N it accepts


def test_the_stride_loops_turn_over_at_share_8():
    trips = {c[0]: gc.rank_update_trips(c[1], c[2], 8) for c in gc.RANK_UPDATE_TRIP_CASES}
    print("rank-update (trips, stages, workgroups per strip) at 8 CUs:", trips)
    assert all(t >= 3 and stages % gx != 0 for t, stages, gx in trips.values())
    assert all(gc.rank_update_trips(c[1], c[2], gc.CHIP_CUS)[0] == 1 for c in gc.RANK_UPDATE_TRIP_CASES)
    assert {(c[9], (c[5] | c[6]) % 2 == 0 and not (c[7] or c[8])) for c in gc.RANK_UPDATE_TRIP_CASES} == \
        {(ip, vec) for ip in (False, True) for vec in (False, True)}    # in place or not, vector or scalar stores
    passes, last = gc.spmm_passes(gc.SPMM_TRIP_ROWS, 8)
    print(f"spmm passes over {gc.SPMM_TRIP_ROWS} rows at 8 CUs: {passes}, the last of {last} rows")
    assert passes >= 3 and last < 4 * 8 * 8 and gc.spmm_passes(gc.SPMM_TRIP_ROWS, gc.CHIP_CUS)[0] == 1
    assert {c[0] for c in gc.SPMM_TRIP_CASES} == {7, 130} and gc.PROJECT_TRIP_CASE[1:4] == (gc.SPMM_TRIP_ROWS, 130, 3)


def test_the_existing_ids_name_the_route_taken_at_every_share():
    """tests/test_dense_shares_gpu.py runs the tables of tests/test_guarded_kernels_gpu.py on every share through the bodies
    that assert the route each id names: no id needs another route on a share (none is listed as an exception)."""
    from tests import test_guarded_kernels_gpu as gk

    for cus in map(gc.share_cus, gc.SHARES):
        for cid, N, m, n, la, lb, _, _, _, _, sym in gk.GEMM_TN_CASES:
            skinny = None if (sym or la != "C" or lb != "C") else gd.skinny_tn_plan(N, m, n, cus)
            want = skinny or gd.gemm_plan(m, n, N, sym, True, cus)
            assert (skinny is not None) == cid.startswith("skinny") and (want["splits"] == 1) == (cid == "generic_no_split")
        for cid, N, n, k, lx, _, _, _, ly, _, alpha, beta, route in gk.GEMM_NN_CASES:
            streaming = (lx, ly, alpha, beta) == ("C", "C", 1.0, 0.0)
            assert (streaming and gd.tallskinny_plan(N, n, k, cus) is not None) == (route == "tallskinny"), (cid, cus)
