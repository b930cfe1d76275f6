"""rt_deim_oversample_step alone (helpers in tests/oversample_cases.py; the host half is tests/test_oversample_cpu.py).

``Phi``, ``w`` and ``taken`` lie inside poisoned guards (quiet NaNs; bytes that say "taken"), ``pick`` and ``top2`` inside
canary buffers (tests/guarded.py).  The pick is held to the long-double scores of the (w, g) the kernel was handed: its score
is at least (1 - 1e-9) of the top, it IS the true argmax wherever the true margin exceeds 1e-9, and ``top2`` are the two
largest true scores to 1e-10 relative (float64 moves a score by (2 m + 10) eps |u| . |w| / |c|, below 1e-11 on these data).
Shapes: N = 2 and 3, the kernel's rows per workgroup (read from its plan) - 1, exactly that and + 1, several workgroups with
a ragged tail; m on both sides of every lanes-per-row choice and of the 64-lane wave; tight and padded leading dimensions,
aligned and 8 bytes off, in both layouts.  Exact ties are bitwise statements."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guarded as gd
from tests import oversample_cases as oc

pytestmark = pytest.mark.gpu

ROWS = None     # rows per workgroup, from the plan


@pytest.fixture(scope="module")
def ops():
    from romtime_amd import ops as _ops

    global ROWS
    ROWS = _ops.deim_oversample_step_plan(1000, 8)[1]
    assert ROWS == _ops.deim_oversample_step_plan(1000, 8, layout=1)[1] == 512
    return _ops


def _basis(N, m, seed=0):
    """N x m with rows of comparable norm and no structure (orthonormal columns where N >= m)."""
    rng = oc.dc._rng("step", N, m, seed)
    B = rng.standard_normal((N, m))
    return np.linalg.qr(B)[0] if N >= m else B / np.sqrt(m)


def _direction(B, seed=0):
    """(w, g) as the loop would hand them over: from the SVD of m + 3 rows of the size of B's (rows of B itself where it
    has enough of them to leave a gap)."""
    N, m = B.shape
    rng = oc.dc._rng("step-rows", N, m, seed)
    rows = B[rng.choice(N, m + 3, replace=False)] if N >= 4 * m else rng.standard_normal((m + 3, m)) / np.sqrt(max(N, m))
    w, g, _ = oc.direction(rows)
    assert g > 0
    return w, g


def _taken_view(mask):
    """uint8[N] inside a buffer whose guard bytes all say "taken"."""
    N = mask.size
    buf = torch.full((N + 2 * gd.GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    view = buf[gd.GUARD:gd.GUARD + N]
    view.copy_(torch.from_numpy(mask.astype(np.uint8)))
    return buf, view


def _step(ops, B, w, g, mask, layout="C", ld_pad=0, misalign=False):
    """One guarded call: (pick, top2) on the host, with every guard and canary checked."""
    N, m = B.shape
    Phi = gd.guarded_operand(B, layout, ld_pad, misalign)
    wv = gd.guarded_operand(w[None, :], "C", 0, False)
    wd = wv[0]
    tbuf, taken = _taken_view(mask)
    pick, top2 = gd.guarded_output((1,), dtype=torch.int64), gd.guarded_output((2,))
    ops.deim_oversample_step(Phi, wd, g, taken, pick=pick.t, top2=top2.t)
    torch.cuda.synchronize()
    assert pick.check() == [] and top2.check() == [], (pick.check(), top2.check())
    assert gd.operand_intact(Phi, B) == [] and gd.operand_intact(wv, w[None, :]) == []
    tb = tbuf.cpu().numpy()
    assert np.all(tb[:gd.GUARD] == 0xFF) and np.all(tb[gd.GUARD + N:] == 0xFF) and np.array_equal(tb[gd.GUARD:gd.GUARD + N] != 0, mask)
    return int(pick.t.cpu()[0]), top2.t.cpu().numpy().copy()


def _held_to_the_truth(B, w, g, mask, pick, top2, label):
    sc, i, top, second = oc.step_truth(B, w, g, mask)
    free = int((~mask).sum())
    if free == 0:
        assert pick == -1 and top2[0] == -1.0 and top2[1] == -1.0, (label, pick, top2)
        return
    assert 0 <= pick < B.shape[0] and not mask[pick], (label, pick)
    margin = float((top - max(second, 0)) / top) if top > 0 else 0.0
    short = float((top - sc[pick]) / top) if top > 0 else 0.0
    print(f"OVERSAMPLE-STEP {label} pick={pick} argmax={i} shortfall/top={short:.3g} margin={margin:.3g} "
          f"top2 rel err={abs(top2[0] - float(sc[pick])) / float(top):.3g}")
    assert sc[pick] >= (1 - oc.LD(oc.NEAR_TIE)) * top, (label, pick, i, short)
    if margin > oc.NEAR_TIE:
        assert pick == i, (label, pick, i)
    assert abs(top2[0] - float(sc[pick])) <= 1e-10 * float(top), (label, top2, float(top))
    if free == 1:
        assert top2[1] == -1.0, (label, top2)
    else:
        assert abs(top2[1] - float(second)) <= 1e-9 * float(top), (label, top2, float(second))


def _both_layouts(ops, B, w, g, mask, label, **place):
    out = []
    for layout in ("C", "F"):
        pick, top2 = _step(ops, B, w, g, mask, layout=layout, **place)
        _held_to_the_truth(B, w, g, mask, pick, top2, f"{label}-{layout}")
        out.append((pick, top2))
    return out


def _patterns(B, w, g):
    """The four ``taken`` patterns: empty, the true argmax taken, all but one taken, all taken."""
    N = B.shape[0]
    none = np.zeros(N, dtype=bool)
    argmax = oc.step_truth(B, w, g, none)[1]
    one_taken = none.copy()
    one_taken[argmax] = True
    but_one = np.ones(N, dtype=bool)
    but_one[(7 * N) // 11] = False
    return dict(empty=none, argmax_taken=one_taken, all_but_one=but_one, all=np.ones(N, dtype=bool))


def _edge_sizes():
    return [2, 3, ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 77]


@pytest.mark.parametrize("which", range(6), ids=["N2", "N3", "rows-1", "rows", "rows+1", "ragged"])
@pytest.mark.parametrize("m", [2, 3, 5, 17, 33, 64, 65, 128])
def test_every_edge_every_pattern(ops, which, m):
    N = _edge_sizes()[which]
    B = _basis(N, m)
    w, g = _direction(B)
    for name, mask in _patterns(B, w, g).items():
        (pc, tc), (pf, tf) = _both_layouts(ops, B, w, g, mask, f"{N}x{m}-{name}")
        if name in ("all", "all_but_one"):
            assert pc == pf


@pytest.mark.parametrize("m", [2, 5, 17, 64, 65])
@pytest.mark.parametrize("ld_pad,misalign", [(1, False), (3, True), (0, True), (6, False)])
def test_the_basis_where_it_lies(ops, m, ld_pad, misalign):
    """ld > m (odd and even), the base 16-byte aligned and 8 bytes off: the 16-byte loads of the column-major kernel only
    where they are legal, the same bits either way."""
    N = ROWS + 131
    B = _basis(N, m, seed=1)
    w, g = _direction(B, seed=1)
    mask = np.zeros(N, dtype=bool)
    mask[::7] = True
    placed = _both_layouts(ops, B, w, g, mask, f"{N}x{m}-pad{ld_pad}-mis{int(misalign)}", ld_pad=ld_pad, misalign=misalign)
    tight = _both_layouts(ops, B, w, g, mask, f"{N}x{m}-tight")
    for (p, t), (p0, t0) in zip(placed, tight):
        assert p == p0 and gd.bits_equal(t, t0)


@pytest.mark.parametrize("m", [3, 17, 64])
def test_exact_ties_go_to_the_lowest_index(ops, m):
    """Duplicated rows get the same fma sequence, so their scores are equal bits: the lower row wins inside a thread's
    pair, inside a workgroup and across workgroups, and top2 holds the same value twice."""
    N = 2 * ROWS + 40
    B = _basis(N, m, seed=2)
    w, g = _direction(B, seed=2)
    best = oc.step_truth(B, w, g, np.zeros(N, dtype=bool))[1]
    for low, high in ((10, 11), (11, 10 + ROWS // 2), (5, N - 3), (ROWS - 1, ROWS)):
        D = B.copy()
        D[low] = D[high] = B[best] * 1.5                       # the unique maximum, twice
        mask = np.zeros(N, dtype=bool)
        for pick, top2 in _both_layouts(ops, D, w, g, mask, f"tie-{low}-{high}-m{m}"):
            assert pick == low and top2[0] == top2[1] > 0, (low, high, pick, top2)
        mask[low] = True
        for pick, top2 in _both_layouts(ops, D, w, g, mask, f"tie-{low}-{high}-m{m}-low-taken"):
            assert pick == high and top2[0] > top2[1], (low, high, pick, top2)


def test_g_zero_returns_the_lowest_free_index(ops):
    N, m = ROWS + 9, 5
    B = _basis(N, m)
    w, _ = _direction(B)
    mask = np.zeros(N, dtype=bool)
    mask[:3] = True
    for layout in ("C", "F"):
        pick, top2 = _step(ops, B, w, 0.0, mask, layout=layout)
        assert pick == 3 and top2[0] == 0.0 and top2[1] == 0.0


def test_same_bits_on_eight_compute_units(ops):
    """A ctx confined to one CU of every XCD ("cu_limit" 8): pick and top2 bit for bit those of the whole chip."""
    from romtime_amd import _lib

    cases = []
    for N, m in ((3 * ROWS + 77, 17), (9 * ROWS + 1, 64), (ROWS - 1, 5)):
        B = _basis(N, m, seed=3)
        w, g = _direction(B, seed=3)
        mask = np.zeros(N, dtype=bool)
        mask[::5] = True
        cases.append((B, w, g, mask))
    whole = [[_step(ops, *c, layout=lay) for lay in ("C", "F")] for c in cases]
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rt_stream_create_cu_range(0, 0, 1, C.byref(h)) == 0 and h.value
    masked = _lib.Context(0)
    masked.set_option("cu_limit", 8)
    st = torch.cuda.ExternalStream(h.value)
    torch.cuda.synchronize()
    with masked.use(st):
        part = [[_step(ops, *c, layout=lay) for lay in ("C", "F")] for c in cases]
    st.synchronize()
    masked.set_option("cu_limit", 0)
    # (this stream stays: torch's allocator remembers the stream of every block handed out under it)
    for a, b in zip(whole, part):
        for (p0, t0), (p1, t1) in zip(a, b):
            assert p0 == p1 and gd.bits_equal(t0, t1), (p0, p1, t0, t1)


@pytest.mark.parametrize("change", [dict(m=1), dict(g=-1.0), dict(g=float("nan")), dict(ld=3), dict(layout=2), dict(N=0),
                                    dict(m=1025, ld=1025)],
                         ids=["m1", "g_negative", "g_nan", "short_ld", "layout", "N0", "m1025"])
def test_bad_arguments_raise_and_write_nothing(change):
    from romtime_amd._lib import Context, RomtimeHipError

    a = dict(N=40, m=8, ld=8, layout=0, g=0.5)
    a.update(change)
    ctx = Context.current()
    Phi = torch.randn(40 * 1025 + 8, dtype=torch.float64, device="cuda")
    w = torch.randn(1025, dtype=torch.float64, device="cuda")
    taken = torch.zeros(64, dtype=torch.uint8, device="cuda")
    pick = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    top2 = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx.lib.rt_deim_oversample_step(ctx.handle, P(Phi), a["N"], a["m"], a["ld"], a["layout"], P(w), a["g"], P(taken), P(pick),
                                         P(top2))
    with pytest.raises(RomtimeHipError):
        ctx.check(rc, "rt_deim_oversample_step")
    torch.cuda.synchronize()
    assert int(pick[0]) == -7 and bool((top2 == -7.0).all())
