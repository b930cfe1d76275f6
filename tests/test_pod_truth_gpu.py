"""POD modes against an extended-precision SVD on every route, on the device (helpers, cases and bars in
tests/svd_cases.py; the premises are proved on the host by tests/test_pod_truth_cpu.py).

Every kept column of Q (and of VT where returned), all of s, the energy curve, the kept-mode count and Q^T Q - I of
``orth`` (passes None, "deflate", 2) and of ``rt_pod_orth``, on C- and F-ordered snapshots, against the long-double truth
of the case.  The shape rows are the smallest that reach each kernel on a 256-CU part; each asserts its Gram form from
``rt_gram_plan_info`` and each deflated run its level count.  The ratios are printed before they are asserted."""
import ctypes as C

import pytest
import torch

from tests import svd_cases as sc

pytestmark = pytest.mark.gpu


def _gram_form(N, n):
    from romtime_amd import _lib

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = (C.c_int * 5)()
    assert _lib.load().rt_gram_plan_info(cus, N, n, out) == 0
    return list(out)


def _one_launch_cases():
    """The smallest N = N0 4^m <= 262144 at n = 136 for which rt_gram takes the one-launch form on this part."""
    for N, N0, p in sorted((N0 * p, N0, p) for N0 in (1536, 2048, 2880, 4096) for p in (16, 64)):
        if N <= 262144 and _gram_form(N, 136)[0] == 2:
            return [sc.Case("stairs", N0, 136, p, num=136)]
    raise AssertionError("no N0 4^m <= 262144 takes the one-launch Gram at n = 136 on this part")


def _check_row(case, form, route, order):
    plan = _gram_form(case.N0 * case.p, case.n)
    assert plan[0] == form, (case.label, plan)
    if form == 1 and case.n == 128:
        assert plan[3] == 0 and plan[4] >= 1, plan       # the diagonal tile only
    if form == 1 and case.n == 136:
        assert plan[3] >= 1, plan                        # an off-diagonal tile (and the shifted last panel)
    sc.check_pod_against_truth(case, (route,), order=order)


# every route on C-ordered snapshots; the two entry points that read the caller's array also on F-ordered ones
ROUTES = [("auto", "C"), ("deflate", "C"), ("two_pass", "C"), ("composite", "C"), ("auto", "F"), ("composite", "F")]
_ids = dict(ids=lambda v: v.label if isinstance(v, sc.Case) else "-".join(v))


@pytest.mark.parametrize("route", ROUTES, **_ids)
@pytest.mark.parametrize("case", sc.SMALL_CASES, **_ids)
def test_small(case, route):
    """600 x 32 and 1536 x 64: the generic GEMM everywhere, and rt_pod_orth's own level loop."""
    _check_row(case, 0, *route)


@pytest.mark.parametrize("route", ROUTES, **_ids)
@pytest.mark.parametrize("case", sc.STREAM_128, **_ids)
def test_stream_128(case, route):
    """98304 x 128 (1536 rows stacked 64 times): gram128_kernel with the diagonal tile only, tallskinny's fast loop and
    its odd-k path, skinny_tn (levels of <= 16 modes) and rank_update (<= 64) beside the generic kernels (``stairs``:
    levels of 17, 65, 16, 8 and 22 modes)."""
    _check_row(case, 1, *route)


@pytest.mark.parametrize("route", ROUTES, **_ids)
@pytest.mark.parametrize("case", sc.STREAM_136, **_ids)
def test_stream_136(case, route):
    """98304 x 136: an off-diagonal Gram tile, the shifted last panel, tallskinny's general loader."""
    _check_row(case, 1, *route)


@pytest.mark.parametrize("route", [("auto", "C"), ("composite", "C"), ("composite", "F")], **_ids)
def test_one_launch(route):
    """gram128_merged_kernel with pacing on: ``stairs`` at the smallest stacked size that takes the one-launch form."""
    for case in _one_launch_cases():
        _check_row(case, 2, *route)


@pytest.mark.parametrize("case", [sc.Case("graded", 1536, 128, 64, num=64), sc.Case("stairs", 1536, 128, 64, num=128)],
                         ids=lambda c: c.label)
def test_forced_one_pass_fails_the_bar(case):
    """Misuse on purpose: passes=1 on a deep case must miss the column bar by more than ten times."""
    X, blocks = sc.snapshots(case)
    m = sc.measure(case, "one_pass", sc.run_route(case, "one_pass", X), blocks)
    print("POD-TRUTH forced one pass", m)
    assert max(m["col"], m["vt"]) > 10.0 * sc.F_COL, m       # the column bar holds Q's columns and VT's
    with pytest.raises(AssertionError):
        sc.assert_within(m, case, "one_pass")
