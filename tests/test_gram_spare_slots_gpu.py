"""Two-launch Gram with spare workgroup slots: every stage of every tile summed exactly once, whatever the grouping.

Where a launch of the two-launch form leaves slots of an XCD without a workgroup, they take the tails of the tiles'
stage ranges (gram_spare_plan in csrc/gram_mfma.hip).  The operands are the exact integers of tests/guarded.py inside
NaN-poisoned buffers, so G must equal X.T @ X bit for bit - a stage taken twice or not at all, by a regular or a spare
slot, changes it - and the guard buffers must be intact.  A ctx with "cu_limit" sizes the grids for a share of the
chip on the ordinary stream.  Two calls, and the two settings of "gram_pace", must give identical bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guarded as gd
from tests.guarded import exact_operands, guarded_operand, guarded_output

pytestmark = pytest.mark.gpu
LAY = {"C": 0, "F": 1}

CASES = [
    # id, cu_limit (0: the whole chip), N, n, layout, misalign,
    # (tiles, regular slots per tile, spare slots, most tails per spare slot) of the off-diagonal / the diagonal launch
    ("share224_2x3_tails", 224, 90_112, 512, "C", False, (6, 9, 2, 3), (4, 14, 0, 0)),
    ("share224_short_last_range", 224, 90_112 + 37, 512, "C", False, (6, 9, 2, 3), (4, 14, 0, 0)),
    ("share224_column_major_misaligned", 224, 90_112, 512, "F", True, (6, 9, 2, 3), (4, 14, 0, 0)),
    ("chip_640_uneven_tails", 0, 73_728, 640, "C", False, (10, 6, 4, 3), (5, 12, 0, 0)),
    ("share96_640_both_launches", 96, 73_728, 640, "C", False, (10, 2, 4, 3), (5, 4, 4, 2)),
    ("cap_bound_plain", 0, 100_000, 250, "C", False, (1, 16, 0, 0), (2, 16, 0, 0)),
]


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
def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_HOST = {}


def _operands(N, n):
    """X (exact integers, graded column scales) and X.T @ X, computed once per shape and never changed."""
    if (N, n) not in _HOST:
        rng = np.random.default_rng(N + n)
        bits = 18
        while N * 2.0 ** (2 * bits) >= 2.0 ** 53:
            bits -= 1
        X = exact_operands(rng, (N, n), bits, gd.graded_exponents(rng, n), k=N)
        G = X.T @ X
        G.setflags(write=False)                                    # (torch warns about wrapping a read-only X)
        _HOST[(N, n)] = (X, G)
    return _HOST[(N, n)]


def _P(t):
    return C.c_void_p(t.data_ptr())


def _run(ctx, Xd, N, n):
    ld, lay = gd.leading_dim(Xd)
    G = guarded_output((n, n))
    ctx.check(ctx.lib.rt_gram(ctx.handle, _P(Xd), N, n, ld, LAY[lay], _P(G.t)), "rt_gram")
    return G


def _spare_plan(ctx, cus, N, n, launch):
    out = (C.c_int * 6)()
    assert ctx.lib.rt_gram_spare_plan_info(cus, N, n, launch, 0, out) == 0
    return tuple(out)[:4]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gram_spare_slots_exact(ctx, device_cus, case):
    _, cu_limit, N, n, layout, misalign, want_off, want_diag = case
    cus = cu_limit or device_cus                                   # (the whole-chip plans are stated for 256 CUs)
    X, want = _operands(N, n)
    Xd = guarded_operand(X, layout, 0, misalign)
    ctx.set_option("cu_limit", cu_limit)
    try:
        choice = (C.c_int * 5)()
        assert ctx.lib.rt_gram_plan_info(cus, N, n, choice) == 0
        assert choice[0] == 1, tuple(choice)                       # two launches
        assert _spare_plan(ctx, cus, N, n, 0) == want_off and _spare_plan(ctx, cus, N, n, 1) == want_diag
        G = _run(ctx, Xd, N, n)
        info = ctx.launch_info()
        # the workgroups really launched: regular and spare slots of both launches on the 8 XCDs
        grid = 8 * sum(t * s + spare for t, s, spare, _ in (want_off, want_diag))
        assert info == dict(grid=grid, splits=8 * want_off[1], tile=(128, 128)), info
        if case[0].startswith("share224"):
            assert tuple(choice) == (1, 6, 4, 9, 14) and info["grid"] == 8 * (56 + 56)
        if case[0] == "cap_bound_plain":                           # exactly the grid of the plain plan
            assert info["grid"] == 8 * (1 * choice[3] + 2 * choice[4])
        got = G.t.cpu().numpy()
        assert gd.bits_equal(got, want), gd.mismatch(got, want)
        G1 = _run(ctx, Xd, N, n)                                   # a second call: the same bits
        assert torch.equal(G1.t.view(torch.int64), G.t.view(torch.int64))
        ctx.set_option("gram_pace", 0)                             # pacing must not change a bit
        try:
            G0 = _run(ctx, Xd, N, n)
        finally:
            ctx.set_option("gram_pace", 1)
        assert torch.equal(G0.t.view(torch.int64), G.t.view(torch.int64))
        torch.cuda.synchronize()
        for out in (G, G1, G0):
            assert out.check() == [], out.check()
        assert gd.operand_intact(Xd, X) == [], gd.operand_intact(Xd, X)
    finally:
        ctx.set_option("cu_limit", 0)
        del Xd
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
