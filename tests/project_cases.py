"""Cases of the fused-projection truth tests (tests/test_project_cases_cpu.py, tests/test_project_truth_gpu.py) and the
rules of csrc/project_fused.hip restated in NumPy.  Plain host module, not a conftest; nothing here needs a GPU.

The kernel  A_N[b] = V^T (A_b V)  picks its code paths from facts the caller never names.  It walks the N rows in stages
of 32; the stage table (project_stages_kernel) decides per stage whether the V rows its entries touch are copied into an
LDS window (at most WROWS = 48 rows, at most EMAX = 512 entries) or gathered from global memory; a pattern with any
stage of the second kind runs the MIXED kernel.  A windowed stage is loaded through buffer descriptors or through
predicated loads, its rows are summed without or with a per-row mask (uni), U = 6, 3 or 2 entries at a time, and
ceil(r / 16) = TR selects one of eight compile-time tile layouts.  ``stage_records``, ``loader``, ``chunk_width`` and
``fused_splits`` restate those rules; the pattern builders below each sit on one of their edges and carry a predicate
(``Pattern.has_kind``) that says so, checked on the CPU against the restated rules and on the device against the table
the kernel reads (rt_project_stage_info)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from tests import guarded as gd

PK = 32          # rows per stage
PT = 512         # threads of a workgroup
WROWS = 48       # V rows of an LDS window
EMAX = 512       # entries of a windowed stage
LD = np.longdouble
U_ROUND = 2.0 ** -53


def _cdiv(a, b):
    return -(-a // b)


# ---- the rules of project_fused.hip, restated ---------------------------------------------------------------------------
def tile_rows(r):
    return _cdiv(r, 16)


def stage_records(indptr, indices, N):
    """(records [stages][6] int64 = (e0, lo, ne, nrow, mr, uni), any_unwindowed) as project_stages_kernel writes them:
    lo = min(k0, columns), hi = max(k1 - 1, columns); windowed iff hi - lo + 1 <= WROWS and ne <= EMAX; mr the longest
    row; uni iff all 32 rows exist and have mr entries; an unwindowed stage is (e0, k0, 0, 0, 0, 0)."""
    stages = _cdiv(N, PK)
    rec = np.zeros((stages, 6), dtype=np.int64)
    rowlen = np.diff(indptr)
    any_unwindowed = False
    for st in range(stages):
        k0, k1 = st * PK, min(st * PK + PK, N)
        e0, e1 = int(indptr[k0]), int(indptr[k1])
        cols = indices[e0:e1]
        lo = min(k0, int(cols.min())) if e1 > e0 else k0
        hi = max(k1 - 1, int(cols.max())) if e1 > e0 else k1 - 1
        if hi - lo + 1 <= WROWS and e1 - e0 <= EMAX:
            lens = rowlen[k0:k1]
            mr = int(lens.max())
            rec[st] = (e0, lo, e1 - e0, hi - lo + 1, mr, int(k1 - k0 == PK and int(lens.min()) == mr))
        else:
            rec[st] = (e0, k0, 0, 0, 0, 0)
            any_unwindowed = True
    return rec, any_unwindowed


def window_margin(tr):
    """NWP * RPP: the window copy of a workgroup reads that many V rows from lo on, whatever the window holds."""
    pairs = 8 * tr
    rpp = PT // pairs
    return _cdiv(WROWS, rpp) * rpp


def loader(rec, k0, N, r, ldv, aligned):
    """How the kernel's fetch() loads the stage with record ``rec`` that starts at row k0: "descriptor" (buffer
    descriptors: even ldv, 16-byte aligned V, even r, a windowed stage of 32 rows whose window copy stays inside V),
    "predicated" for every other windowed stage, "gather" for a stage that is not windowed."""
    e0, lo, ne, nrow, mr, uni = (int(x) for x in rec)
    if nrow == 0:
        return "gather"
    if ldv % 2 == 0 and aligned and r % 2 == 0 and min(N - k0, PK) == PK and lo + window_margin(tile_rows(r)) < N:
        return "descriptor"
    return "predicated"


def chunk_width(tr):
    return 6 if tr <= 2 else (3 if tr <= 4 else 2)


def fused_splits(N, B=1):
    """DoF ranges S per value vector, for B so small that B * (stages // 8) <= 256: every candidate count then lies below
    one round of resident workgroups on any occupancy, and the count with at least 8 stages per workgroup is taken."""
    stages = _cdiv(N, PK)
    cand = max(stages // 8, 1)
    assert B * cand <= 256
    per = _cdiv(_cdiv(N, cand), PK) * PK
    return _cdiv(N, per)


def stage_kinds(records, N, r, ldv, aligned):
    """One namespace per stage: the record's fields, k0, rows, shift = k0 - lo and the loader."""
    out = []
    for st, rec in enumerate(np.asarray(records)):
        e0, lo, ne, nrow, mr, uni = (int(x) for x in rec)
        k0 = st * PK
        out.append(SimpleNamespace(st=st, k0=k0, rows=min(N - k0, PK), e0=e0, lo=lo, ne=ne, nrow=nrow, mr=mr, uni=bool(uni),
                                   windowed=nrow > 0, shift=k0 - lo, loader=loader(rec, k0, N, r, ldv, aligned)))
    return out


# ---- pattern builders (sorted CSR, vectorised) --------------------------------------------------------------------------
def _csr(N, rows, cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    ok = (cols >= 0) & (cols < N)
    key = np.unique(rows[ok] * N + cols[ok])
    rows, cols = key // N, key % N
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int64)
    return indptr, cols.astype(np.int64)


def _offsets(N, offs, keep=None):
    i = np.arange(N)
    rows = np.repeat(i, len(offs))
    cols = (i[:, None] + np.asarray(offs)[None, :]).reshape(-1)
    if keep is not None:
        sel = keep(rows, cols)
        rows, cols = rows[sel], cols[sel]
    return rows, cols


PENTA = (-2, -1, 0, 1, 2)


def banded(h_left, h_right, N=647):
    """Row i holds the columns i - h_left, i, i + h_right and its nearest neighbours on the sides that have any: an
    interior stage spans exactly 32 + h_left + h_right rows with few entries; (2, 2) is the pentadiagonal pattern."""
    offs = {-h_left, 0, h_right} | ({-1} if h_left else set()) | ({1} if h_right else set())
    return _csr(N, *_offsets(N, sorted(offs)))


def entries_512(N=647):
    """Interior rows of 16 entries (columns i - 8 .. i + 7): a 47-row window holds exactly EMAX entries."""
    return _csr(N, *_offsets(N, range(-8, 8)))


ENTRIES_513_ROW = 5 * PK + 10


def entries_513(N=647):
    """entries_512 with one row of 17 entries: that stage alone has 513 entries and is not windowed."""
    rows, cols = _offsets(N, range(-8, 8))
    return _csr(N, np.append(rows, ENTRIES_513_ROW), np.append(cols, ENTRIES_513_ROW + 8))


def _run_start(N, mr):
    return np.clip(np.arange(N) - mr // 2, 0, N - mr)


def row_length(mr, N=647):
    """Every row has exactly mr contiguous entries around the diagonal (shifted inwards at the two ends, not cut): every
    full stage is uni, the short last one is masked."""
    start = _run_start(N, mr)
    return _csr(N, np.repeat(np.arange(N), mr), (start[:, None] + np.arange(mr)[None, :]).reshape(-1))


def ragged_lengths(mr, N):
    """Row lengths of row_length_ragged: in the odd stages the LAST row loses one entry (none left for mr = 1), in every
    fourth stage rows 3 and 17 keep only ceil(mr / 2); the even stages stay uni."""
    i = np.arange(N)
    st, k = i // PK, i % PK
    lens = np.full(N, mr, dtype=np.int64)
    lens[(st % 2 == 1) & (k == PK - 1)] = mr - 1
    lens[(st % 4 == 1) & ((k == 3) | (k == 17))] = _cdiv(mr, 2)
    return lens


def row_length_ragged(mr, N=647):
    start, lens = _run_start(N, mr), ragged_lengths(mr, N)
    rows = np.repeat(np.arange(N), mr)
    j = np.tile(np.arange(mr), N)
    sel = j < lens[rows]
    return _csr(N, rows[sel], (start[rows] + j)[sel])


SKEWED_STAGE, SKEWED_ROW, SKEWED_LEN = 3, 5, 40


def skewed(N=647):
    """One entry per row (the diagonal), but row 5 of stage 3 has 40: columns k0 - 4 .. k0 + 35.  The masked sum of the
    31 rows after it, the stage's last row included, reads 39 entries past each row's own."""
    k0 = SKEWED_STAGE * PK
    i = np.arange(N)
    return _csr(N, np.concatenate([i, np.full(SKEWED_LEN, k0 + SKEWED_ROW)]), np.concatenate([i, k0 - 4 + np.arange(SKEWED_LEN)]))


EMPTY_RUN = (60, 71)          # rows 60 .. 70: across the boundary of stages 1 and 2
EMPTY_STAGE = 3


def empty(which, N=647):
    """The pentadiagonal pattern with rows removed: "rows" = rows 0, N - 1 and 60 .. 70, "stage" = all of stage 3,
    "last_stage" = the whole (short) last stage, "all" = every row (nnz = 0)."""
    gone = {"rows": lambda r: (r == 0) | (r == N - 1) | ((r >= EMPTY_RUN[0]) & (r < EMPTY_RUN[1])),
            "stage": lambda r: r // PK == EMPTY_STAGE,
            "last_stage": lambda r: r // PK == (N - 1) // PK,
            "all": lambda r: np.ones_like(r, dtype=bool)}[which]
    return _csr(N, *_offsets(N, PENTA, keep=lambda r, c: ~gone(r)))


def ends(N):
    """The pentadiagonal pattern at the sizes where the stage loop begins and ends differently."""
    return _csr(N, *_offsets(N, PENTA))


ENDS_N = (3, 31, 32, 33, 64, 65, 32 * 20 + 1)
FAR_STAGE = 7


def far_entry(N=1030):
    """Pentadiagonal plus one entry (i, (i + N // 2) % N) in stage 7: one stage that is not windowed among windowed ones."""
    rows, cols = _offsets(N, PENTA)
    i = FAR_STAGE * PK + 13
    return _csr(N, np.append(rows, i), np.append(cols, (i + N // 2) % N))


class Pattern:
    """A named CSR pattern and the predicate over ``stage_kinds`` that says what it exists for."""

    def __init__(self, name, build, has_kind, N):
        self.name, self._build, self.has_kind, self.N = name, build, has_kind, N

    @functools.cached_property
    def csr(self):
        indptr, indices = self._build()
        assert indptr.shape == (self.N + 1,) and indptr[-1] == indices.size and indices.size <= 40_000
        return indptr, indices

    @property
    def nnz(self):
        return int(self.csr[1].size)

    @functools.cached_property
    def records(self):
        return stage_records(*self.csr, self.N)


def _interior(kinds):
    return [s for s in kinds[1:-1] if s.rows == PK]


def _mk_patterns():
    P = {}

    def add(name, build, has_kind, N=647):
        P[name] = Pattern(name, build, has_kind, N)

    full = lambda s: s.rows == PK
    add("banded_2_2", lambda: banded(2, 2, 1030), lambda k: all(s.windowed for s in k) and any(s.uni for s in k), 1030)
    add("banded_8_8", lambda: banded(8, 8), lambda k: all(s.windowed and s.nrow == WROWS and s.shift == 8 for s in _interior(k)[1:-1]))
    add("banded_8_9", lambda: banded(8, 9), lambda k: not any(s.windowed for s in _interior(k)[1:-1]) and k[0].windowed)
    add("banded_0_16", lambda: banded(0, 16), lambda k: all(s.windowed and s.nrow == WROWS and s.shift == 0 for s in _interior(k)[:-1]))
    add("banded_16_0", lambda: banded(16, 0), lambda k: all(s.windowed and s.nrow == WROWS and s.shift == 16 for s in _interior(k)[1:]))
    add("entries_512", entries_512, lambda k: all(s.windowed for s in k) and max(s.ne for s in k) == EMAX
        and any(s.ne == EMAX and s.uni and s.mr == 16 for s in k))
    add("entries_513", entries_513, lambda k: [s.st for s in k if not s.windowed] == [ENTRIES_513_ROW // PK]
        and any(s.ne == EMAX for s in k))
    for mr in range(1, 14):
        add(f"row_length_{mr}", functools.partial(row_length, mr),
            lambda k, mr=mr: all(s.windowed and s.mr == mr for s in k) and all(s.uni for s in k if full(s)) and not k[-1].uni)
        add(f"row_length_ragged_{mr}", functools.partial(row_length_ragged, mr),
            lambda k, mr=mr: all(s.windowed and s.mr == mr for s in k) and all(s.uni == (s.st % 2 == 0) for s in k if full(s))
            and sum(not s.uni for s in k if full(s)) >= 5)
    add("skewed", skewed, lambda k: (lambda s: s.windowed and not s.uni and s.mr == SKEWED_LEN and s.ne == SKEWED_LEN + PK - 1
                                     and s.shift == 4)(k[SKEWED_STAGE]))
    add("empty_rows", lambda: empty("rows"), lambda k: all(s.windowed for s in k) and not k[0].uni and not k[1].uni and not k[2].uni
        and k[3].uni and k[1].ne < k[3].ne)
    add("empty_stage", lambda: empty("stage"), lambda k: (lambda s: s.windowed and s.ne == 0 and s.mr == 0 and s.uni and s.nrow == PK)(k[EMPTY_STAGE])
        and k[EMPTY_STAGE + 1].ne > 0)
    add("empty_last_stage", lambda: empty("last_stage"), lambda k: k[-1].windowed and k[-1].ne == 0 and k[-1].rows < PK and k[-2].ne > 0)
    add("empty_all", lambda: empty("all"), lambda k: all(s.windowed and s.ne == 0 and s.e0 == 0 for s in k))
    for N in ENDS_N:
        q, rest = divmod(N, PK)
        add(f"ends_{N}", functools.partial(ends, N),
            lambda k, q=q, rest=rest, N=N: len(k) == q + (rest > 0) and all(s.windowed for s in k) and k[-1].rows == (rest or PK)
            and (N > WROWS or not any(s.loader == "descriptor" for s in k)), N)   # no window copy fits below 48 rows
    add("far_entry", far_entry, lambda k: [s.st for s in k if not s.windowed] == [FAR_STAGE], 1030)
    add("far_entry_647", lambda: far_entry(647), lambda k: [s.st for s in k if not s.windowed] == [FAR_STAGE])
    return P


PATTERNS = _mk_patterns()
# the patterns of test_stage_edges_exact: every builder (far_entry at the size of its neighbours)
EDGE_PATTERNS = [n for n in PATTERNS if n not in ("banded_2_2", "far_entry")] + ["banded_2_2"]


def last_row_is_short(pattern, st):
    """Row 31 of stage st has fewer entries than the stage's longest row."""
    lens = np.diff(pattern.csr[0])[st * PK:(st + 1) * PK]
    return lens.size == PK and lens[-1] < lens.max()


# ---- the runs of the GPU tests --------------------------------------------------------------------------------------------
LAYOUT_R = sorted({x for tr in range(1, 9) for x in (16 * tr, 16 * tr - 1, 16 * (tr - 1) + 2)})
LAYOUT_PATTERNS = ("banded_2_2", "far_entry")
LAYOUT_B = 3
# V placements: (id, ld_pad, misalign).  The even pad keeps the descriptor loads for even r: the 16 TR-wide window copy
# then carries the NaN pad into the LDS columns >= r.
V_PLACEMENTS = (("tight", 0, False), ("even_pad", 2, False), ("odd_pad", 1, False), ("misaligned", 0, True))
EDGE_R = (16, 14, 40, 64, 80, 96, 110)
# (B, data order, data ld_pad, V ld_pad)
EDGE_RUNS = ((1, "C", 1, 2), (1, "F", 2, 0), (3, "C", 2, 0), (3, "F", 1, 2))
ENDS_RUNS = ((9, "C", 1, 2), (9, "F", 1, 0))
REPEAT_CASES = (("far_entry", 64), ("banded_8_8", 112), ("row_length_ragged_7", 33), ("skewed", 50))
ROUNDED_PATTERNS = ("banded_8_8", "row_length_ragged_7", "far_entry", "skewed")
ROUNDED_R = (33, 64, 80, 112)
ROUNDED_B = 2


def gpu_runs():
    """Every (pattern name, r, ldv, V aligned) the device tests launch."""
    for name in LAYOUT_PATTERNS:
        for r in LAYOUT_R:
            for _, pad, mis in V_PLACEMENTS:
                yield name, r, r + pad, not mis
    for name in EDGE_PATTERNS:
        for r in EDGE_R:
            runs = EDGE_RUNS + (ENDS_RUNS if name.startswith("ends_") else ())
            for vpad in sorted({run[3] for run in runs}):
                yield name, r, r + vpad, True
    for name, r in REPEAT_CASES:
        yield name, r, r, True
    for name in ROUNDED_PATTERNS:
        for r in ROUNDED_R:
            yield name, r, r, True


# ---- operands ---------------------------------------------------------------------------------------------------------------
def exact_bits(nnz):
    """Widest V integers (<= 14 bits) for which nnz products of a 10-bit value and two V entries stay below 2^53."""
    b = 14
    while nnz * 2.0 ** (2 * b + 10) >= 2.0 ** 53:
        b -= 1
    return b


def _seed(*parts):
    return sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(str(p) for p in parts))) % 1000003


def csr_mm(indptr, indices, vals, X):
    """A X for the CSR matrix with values ``vals``, in the dtype of X."""
    N = indptr.size - 1
    out = np.zeros((N, X.shape[1]), dtype=X.dtype)
    np.add.at(out, np.repeat(np.arange(N), np.diff(indptr)), np.asarray(vals, dtype=X.dtype)[:, None] * X[indices])
    return out


def project(indptr, indices, vals, V):
    return V.T @ csr_mm(indptr, indices, vals, V)


@functools.lru_cache(maxsize=None)
def exact_case(name, r, B):
    """V (N x r), data (nnz x B) and the exact A_N (B x r x r) on pattern ``name``: integers scaled by powers of two, every
    partial sum of every entry below 2^53 units, so the float64 NumPy product is the answer whatever the order."""
    p = PATTERNS[name]
    indptr, indices = p.csr
    rng = np.random.default_rng(_seed(name, r, B))
    bv = exact_bits(p.nnz)
    assert p.nnz * 2.0 ** (2 * bv + 10) < 2.0 ** 53
    data = gd.exact_operands(rng, (p.nnz, B), 10)
    V = gd.exact_operands(rng, (p.N, r), bv, gd.graded_exponents(rng, r, 60))
    want = np.stack([project(indptr, indices, data[:, b], V) for b in range(B)])
    want.setflags(write=False)
    return SimpleNamespace(pattern=p, r=r, B=B, bv=bv, V=V, data=data, want=want)


def rounded_bar(pattern, S):
    """Terms of the componentwise forward bound: one rounding per gathered entry of the longest row, one per contraction
    row, one per slab, two for the products."""
    return int(np.diff(pattern.csr[0]).max(initial=0)) + pattern.N + S + 2


@functools.lru_cache(maxsize=None)
def rounded_case(name, r, B=ROUNDED_B):
    """Gaussian V with columns scaled by 2^graded_exponents(.., 30), Gaussian data; ``ref`` the np.longdouble product,
    ``bound`` = rounded_bar * 2^-53 * |V|^T |A| |V| per entry."""
    p = PATTERNS[name]
    indptr, indices = p.csr
    rng = np.random.default_rng(_seed("rounded", name, r))
    V = rng.standard_normal((p.N, r)) * np.ldexp(1.0, gd.graded_exponents(rng, r, 30))[None, :]
    data = rng.standard_normal((p.nnz, B))
    Vl = V.astype(LD)
    ref = np.stack([project(indptr, indices, data[:, b], Vl) for b in range(B)])
    mag = np.stack([project(indptr, indices, np.abs(data[:, b]), np.abs(Vl)) for b in range(B)])
    bound = LD(rounded_bar(p, fused_splits(p.N, B))) * LD(U_ROUND) * mag
    for a in (ref, bound):
        a.setflags(write=False)
    return SimpleNamespace(pattern=p, r=r, B=B, V=V, data=data, ref=ref, bound=bound)


def within_bar(got, case):
    """(ok, worst |got - ref| / bound) per entry against the componentwise bar of a rounded case."""
    err = np.abs(np.asarray(got, dtype=LD) - case.ref)
    ok = bool(np.all(err <= case.bound))
    worst = float(np.max(err / np.maximum(case.bound, np.finfo(np.float64).tiny)))
    return ok, worst
