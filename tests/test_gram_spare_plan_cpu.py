"""The slot plan of the two-launch Gram with spare slots (rt_gram_spare_plan_info: host logic, no GPU needed).

For one launch with n_t tiles and s regular slots per tile the windows are rebuilt here from what the entry point
reports: regular slot (t, q) takes the stages q, q + s, ... below n_main, spare slot j the stages [n_main, nst) of its
consecutive tiles.  Every stage of every tile must be taken exactly once, and no slot may carry more than the balanced
load plus what rounding costs."""
import ctypes as C
import math

import pytest

from romtime_amd import _lib


def _choice(cus, K, n):
    out = (C.c_int * 5)()
    assert _lib.load().rt_gram_plan_info(cus, K, n, out) == 0
    return tuple(out)


def _plan(cus, K, n, launch, xcd):
    out = (C.c_int * 6)()
    rc = _lib.load().rt_gram_spare_plan_info(cus, K, n, launch, xcd, out)
    assert rc == 0, rc
    return tuple(out)


def _slot_loads(plan):
    """(loads of all slots, times each stage of each tile is taken) of one launch on one XCD."""
    n_t, s, spare, m, n_main, nst = plan
    taken = [[0] * nst for _ in range(n_t)]
    loads = []
    for t in range(n_t):
        for q in range(s):
            stages = range(q, n_main, s)
            loads.append(len(stages))
            for k in stages:
                taken[t][k] += 1
    t0 = 0
    for j in range(spare):
        cnt = n_t // spare + (1 if j < n_t % spare else 0)
        assert 1 <= cnt <= m
        for t in range(t0, t0 + cnt):
            for k in range(n_main, nst):
                taken[t][k] += 1
        loads.append(cnt * (nst - n_main))
        t0 += cnt
    assert spare == 0 or t0 == n_t
    return loads, taken


SHAPES = [
    # cus, K, n: the pipeline's share and the whole chip, long and short sets, a last range that ends in a partial stage
    (224, 1_000_000, 512),
    (224, 90_112, 512),
    (224, 90_112 + 37, 512),
    (256, 73_728, 640),
    (256, 600_000, 640),
    (256, 1_000_000, 768),
    (96, 73_728, 640),
    (144, 73_728, 640),
    (256, 100_000, 250),
]


@pytest.mark.parametrize("cus,K,n", SHAPES)
def test_windows_cover_every_stage_once_and_slots_are_balanced(cus, K, n):
    form, _, _, s_off, s_diag = _choice(cus, K, n)
    assert form == 1
    tiles1 = -(-n // 128)
    slots_max = 2 * cus // 8
    for launch, n_t, s in ((0, tiles1 * (tiles1 - 1) // 2, s_off), (1, tiles1, s_diag)):
        for xcd in range(8):
            plan = _plan(cus, K, n, launch, xcd)
            assert plan[:2] == (n_t, s)
            _, _, spare, m, n_main, nst = plan
            assert n_t * s + spare <= slots_max and spare <= n_t
            loads, taken = _slot_loads(plan)
            assert all(c == 1 for row in taken for c in row)
            if spare == 0:
                assert n_main == nst and m == 0
                continue
            assert m == -(-n_t // spare)
            # balanced level of a full spare slot and a regular one: nst m / (1 + m s); n_main is rounded to a stage
            # (half a stage, felt m-fold by a spare slot) and a regular slot's share of it to a whole number
            level = nst * m / (1 + m * s)
            assert max(loads) <= level + 1 + m / 2, (plan, max(loads), level)
            if n_t % spare == 0:          # all spare slots full: the level is the mean
                assert abs(level - sum(loads) / len(loads)) < 1e-9 * level


def test_pipeline_shape_takes_two_spare_slots_of_three_tails():
    """bench shape on the pipeline's 224 CUs: 6 off-diagonal tiles x 9 slots leave 2 of 56; n_main = 27/28 of the range."""
    assert _choice(224, 1_000_000, 512) == (1, 6, 4, 9, 14)
    for xcd in range(8):
        n_t, s, spare, m, n_main, nst = _plan(224, 1_000_000, 512, 0, xcd)
        assert (n_t, s, spare, m) == (6, 9, 2, 3)
        assert n_main == math.floor(nst * 27 / 28 + 0.5)
        loads, _ = _slot_loads((n_t, s, spare, m, n_main, nst))
        assert max(loads) - sum(loads) / len(loads) <= 1.0
        assert _plan(224, 1_000_000, 512, 1, xcd)[2] == 0          # 4 x 14 = 56: no slot spare
    assert [_plan(224, 1_000_000, 512, 0, x)[5] for x in (0, 7)] == [7813, 7809]


def test_short_sets_and_short_tails_keep_the_plain_launch():
    # the cap binds (at least 48 stages per workgroup): exactly the plain plan
    for launch in (0, 1):
        assert _plan(256, 100_000, 250, launch, 0)[2:4] == (0, 0)
    # 5 diagonal tiles, 4 spare slots: the slots with a single tail of 23 stages would fall below the floor
    assert _plan(256, 73_728, 640, 1, 0)[2] == 0
    assert _plan(256, 73_728, 640, 0, 0)[:4] == (10, 6, 4, 3)
    assert _plan(256, 600_000, 640, 1, 0)[:4] == (5, 12, 4, 2)


def test_refusals_and_abi():
    lib = _lib.load()
    out = (C.c_int * 6)()
    assert lib.rt_version() >= 430
    assert lib.rt_gram_spare_plan_info(256, 40_000, 512, 0, 0, out) < 0       # the one-launch form
    assert lib.rt_gram_spare_plan_info(256, 100_000, 128, 0, 0, out) < 0      # no off-diagonal tile
    assert lib.rt_gram_spare_plan_info(256, 100_000, 128, 1, 0, out) == 0
    assert lib.rt_gram_spare_plan_info(256, 100_000, 250, 2, 0, out) < 0
    assert lib.rt_gram_spare_plan_info(256, 100_000, 250, 0, 8, out) < 0
    assert lib.rt_gram_spare_plan_info(256, 100_000, 250, 0, 0, None) < 0
