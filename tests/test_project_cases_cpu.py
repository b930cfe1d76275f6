"""The premises of tests/test_project_truth_gpu.py, checked without a device: every pattern has the property it is named
for under the restated stage rule, the device runs together reach every tile layout, loader, row-sum path and chunk
remainder, the exact cases are exact, and the componentwise bar of the rounded cases holds for NumPy's own float64
product - so the bar asks nothing a correct implementation cannot give."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import project_cases as pc
from tests.project_cases import PATTERNS, PK, WROWS, EMAX


def _kinds(name, r=16, pad=0, aligned=True):
    p = PATTERNS[name]
    rec, any_unwindowed = pc.stage_records(*p.csr, p.N)
    return pc.stage_kinds(rec, p.N, r, r + pad, aligned), any_unwindowed


def _unit_exponent(col):
    """e with 2^e the largest power of two that divides every nonzero entry of ``col``."""
    m, ex = np.frexp(np.abs(col[col != 0]))
    mi = np.ldexp(m, 53).astype(np.int64)
    return int((ex - 53 + np.log2((mi & -mi).astype(np.float64)).astype(np.int64)).min())


def test_restated_rules_on_hand_made_stages():
    # one stage, three rows: window = rows 0 .. 2 although row 2 has no entry
    rec, any_u = pc.stage_records(np.array([0, 1, 3, 3]), np.array([1, 0, 2]), 3)
    assert rec.tolist() == [[0, 0, 3, 3, 2, 0]] and not any_u
    # 32 rows of one entry each, all in column 47: the window ends there (48 rows); column 48 is one too many
    for col, want in ((47, [0, 0, 32, 48, 1, 1]), (48, [0, 0, 0, 0, 0, 0])):
        rec, any_u = pc.stage_records(np.arange(101).clip(max=32), np.full(32, col), 100)
        assert rec[0].tolist() == want and any_u == (col == 48)
        assert rec[1:].tolist() == [[32, 32, 0, 32, 0, 1], [32, 64, 0, 32, 0, 1], [32, 96, 0, 4, 0, 0]]
    assert [pc.window_margin(tr) for tr in range(1, 9)] == [64, 64, 63, 48, 48, 50, 54, 48]
    assert [pc.chunk_width(tr) for tr in range(1, 9)] == [6, 6, 3, 3, 2, 2, 2, 2]
    assert [pc.fused_splits(N) for N in (3, 255, 256, 512, 647, 1030, 2100)] == [1, 1, 1, 2, 2, 4, 8]
    win = (0, 100, 160, 36, 5, 1)
    assert pc.loader(win, 102, 1030, 64, 64, True) == "descriptor"
    assert [pc.loader(win, 102, 1030, *a) for a in ((63, 64, True), (64, 65, True), (64, 64, False))] == ["predicated"] * 3
    assert pc.loader(win, 102, 148, 64, 64, True) == "predicated" and pc.loader(win, 102, 149, 64, 64, True) == "descriptor"
    assert pc.loader(win, 102, 133, 64, 64, True) == "predicated"          # 31 rows left
    assert pc.loader((0, 96, 0, 0, 0, 0), 96, 1030, 64, 64, True) == "gather"


@pytest.mark.parametrize("name", list(PATTERNS))
def test_pattern_is_sorted_csr_within_the_size_limits_and_has_its_kind(name):
    p = PATTERNS[name]
    indptr, indices = p.csr
    assert indptr.dtype == np.int64 and indices.dtype == np.int64 and indptr[0] == 0 and np.all(np.diff(indptr) >= 0)
    assert (600 <= p.N <= 2100 or name.startswith("ends_")) and p.nnz <= 40_000
    if p.nnz:
        assert indices.min() >= 0 and indices.max() < p.N
        rows = np.repeat(np.arange(p.N), np.diff(indptr))
        assert np.all(np.diff(rows * p.N + indices) > 0), "columns of a row must be sorted and distinct"
    for r, pad in ((16, 0), (64, 2), (110, 0)):
        kinds, _ = _kinds(name, r, pad)
        assert p.has_kind(kinds), name


def test_named_edges_of_the_stage_table():
    k, any_u = _kinds("banded_8_8")
    assert not any_u and any(s.windowed and s.nrow == WROWS for s in k)
    k, any_u = _kinds("banded_8_9")
    assert any_u and not any(s.windowed for s in k[2:-2])
    assert {s.shift for s in _kinds("banded_0_16")[0]} == {0} and 16 in {s.shift for s in _kinds("banded_16_0")[0]}
    k, any_u = _kinds("entries_512")
    assert max(s.ne for s in k) == EMAX and not any_u
    k, any_u = _kinds("entries_513")
    assert any_u and sum(not s.windowed for s in k) == 1
    for mr in range(1, 14):
        k, any_u = _kinds(f"row_length_{mr}")
        assert not any_u and sum(s.uni and s.mr == mr for s in k) >= 10
        p = PATTERNS[f"row_length_ragged_{mr}"]
        k, any_u = _kinds(p.name)
        assert not any_u and any(s.windowed and not s.uni and s.mr == mr and pc.last_row_is_short(p, s.st) for s in k)
        assert any(s.uni and s.mr == mr for s in k)
    k, _ = _kinds("skewed")
    lens = np.diff(PATTERNS["skewed"].csr[0])[pc.SKEWED_STAGE * PK:(pc.SKEWED_STAGE + 1) * PK]
    assert sorted(lens.tolist()) == [1] * 31 + [40] and lens[-1] == 1
    assert PATTERNS["empty_all"].nnz == 0
    k, any_u = _kinds("far_entry")
    assert any_u and sum(not s.windowed for s in k) == 1 and sum(s.windowed for s in k) == len(k) - 1
    assert [PATTERNS[f"ends_{N}"].N for N in pc.ENDS_N] == [3, 31, 32, 33, 64, 65, 641]
    assert [len(_kinds(f"ends_{N}")[0]) for N in pc.ENDS_N] == [1, 1, 1, 2, 2, 3, 21]
    assert _kinds("ends_33")[0][-1].rows == 1 and _kinds("ends_641")[0][-1].rows == 1


@pytest.fixture(scope="module")
def coverage():
    """What the device runs reach: (TR, MIXED), (TR, loader), (U, uni, mr mod U), and per TR the side of the
    lo + NWP RPP < N switch on which full windowed stages of descriptor-capable runs fall."""
    pairs, loaders, chunks, sides = set(), set(), set(), set()
    for name, r, ldv, aligned in pc.gpu_runs():
        p = PATTERNS[name]
        rec, any_u = p.records
        tr = pc.tile_rows(r)
        pairs.add((tr, any_u))
        for s in pc.stage_kinds(rec, p.N, r, ldv, aligned):
            if not s.windowed:
                continue
            loaders.add((tr, s.loader))
            chunks.add((pc.chunk_width(tr), s.uni, s.mr % pc.chunk_width(tr)))
            if s.rows == PK and ldv % 2 == 0 and aligned and r % 2 == 0:
                sides.add((tr, s.lo + pc.window_margin(tr) < p.N))
    return pairs, loaders, chunks, sides


def test_device_runs_reach_every_layout_loader_and_chunk_remainder(coverage):
    pairs, loaders, chunks, sides = coverage
    assert pairs == {(tr, mixed) for tr in range(1, 9) for mixed in (False, True)}
    assert loaders == {(tr, how) for tr in range(1, 9) for how in ("descriptor", "predicated")}
    assert chunks >= {(U, uni, rest) for U in (6, 3, 2) for uni in (False, True) for rest in range(U)}
    assert sides == {(tr, side) for tr in range(1, 9) for side in (False, True)}


def test_layout_sizes_are_the_ones_named():
    assert {50, 63, 64, 98, 111, 112} <= set(pc.LAYOUT_R) and len(pc.LAYOUT_R) == 24
    assert {pc.tile_rows(r) for r in pc.LAYOUT_R} == set(range(1, 9))
    assert [pc.tile_rows(r) for r in pc.EDGE_R] == [1, 1, 3, 4, 5, 6, 7]
    for name in pc.LAYOUT_PATTERNS:
        assert PATTERNS[name].N == 1030 and pc.fused_splits(1030, pc.LAYOUT_B) == 4
    assert [PATTERNS[n].records[1] for n in pc.LAYOUT_PATTERNS] == [False, True]


def test_exactness_premise_of_every_exact_case():
    """nnz products of a 10-bit value and two bv-bit V entries: every partial sum of an output entry stays below 2^53
    units of its column pair's scale, and the drawn operands are such integers."""
    for name, p in PATTERNS.items():
        bv = pc.exact_bits(p.nnz)
        assert 8 <= bv <= 14 and p.nnz * 2.0 ** (2 * bv + 10) < 2.0 ** 53
    # the premise itself, from the drawn numbers alone: with u_j the largest power of two that divides column j of V,
    # every term of entry (i, j) is a multiple of u_i u_j and the sum of their magnitudes stays below 2^53 u_i u_j
    for name, r in [(n, 14) for n in pc.EDGE_PATTERNS] + [(n, 112) for n in pc.LAYOUT_PATTERNS]:
        c = pc.exact_case(name, r, 3)
        assert np.all(np.abs(c.data) <= 2 ** 10) and np.all(c.data == np.rint(c.data))
        u = np.array([_unit_exponent(c.V[:, j]) for j in range(r)])
        assert u.max() - u.min() >= 100
        for b in range(c.B):
            mag = pc.project(*c.pattern.csr, np.abs(c.data[:, b]), np.abs(c.V))
            assert np.all(np.ldexp(mag, -(u[:, None] + u[None, :])) < 2.0 ** 53), (name, r)
    # the float64 product in another order (scipy's row loop and BLAS) gives the same bits: the answer is exact
    c = pc.exact_case("entries_513", 14, 3)
    indptr, indices = c.pattern.csr
    for b in range(c.B):
        A = sp.csr_matrix((c.data[:, b], indices, indptr), shape=(c.pattern.N, c.pattern.N))
        assert np.array_equal((c.V.T @ (A @ c.V)).view(np.int64), c.want[b].view(np.int64))
        ld = pc.project(indptr, indices, c.data[:, b], c.V.astype(pc.LD))
        assert np.array_equal(ld.astype(np.float64).view(np.int64), c.want[b].view(np.int64)) and np.all(ld.astype(np.float64) == ld)


@pytest.mark.parametrize("name", pc.ROUNDED_PATTERNS)
@pytest.mark.parametrize("r", pc.ROUNDED_R)
def test_numpy_float64_product_is_within_the_componentwise_bar(name, r):
    c = pc.rounded_case(name, r)
    indptr, indices = c.pattern.csr
    got = np.stack([c.V.T @ (sp.csr_matrix((c.data[:, b], indices, indptr), shape=(c.pattern.N,) * 2) @ c.V) for b in range(c.B)])
    ok, worst = pc.within_bar(got, c)
    assert ok and worst < 1.0, worst
    # and the bar bites: one dropped entry of A, or an error of 1e-12 relative in one small entry, is outside it
    e = int(indptr[c.pattern.N // 2])
    data = c.data[:, 0].copy()
    data[e] = 0.0
    dropped = c.V.T @ (sp.csr_matrix((data, indices, indptr), shape=(c.pattern.N,) * 2) @ c.V)
    assert not pc.within_bar(np.stack([dropped, got[1]]), c)[0]
    small = got.copy()
    small[0, 0, 0] *= 1.0 + 1e-10
    assert not pc.within_bar(small, c)[0]
