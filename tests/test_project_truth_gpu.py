"""The fused projection A_N[b] = V^T (A_b V) (csrc/project_fused.hip) held to exact answers on every tile layout and at
every edge of its stage table, inside NaN-poisoned operands and a canary-guarded output (tests/guarded.py).

The cases, the restated rules and their premises live in tests/project_cases.py and tests/test_project_cases_cpu.py.
Every run goes through rt_project_csr_batched or rt_project_csr and requires: the exact product bit for bit (integer
data scaled by powers of two, every partial sum below 2^53 units), every output word written, nothing written outside
the output, operands and their poison intact, and the launch the restated rules predict.  The stage table the kernel
reads is compared field for field with the restated one (rt_project_stage_info), so a case cannot quietly stop reaching
the path it is named for.  Rounded data is held to a componentwise forward bound without a measured constant."""
import numpy as np
import pytest
import torch

from tests import guarded as gd
from tests import project_cases as pc
from tests.project_cases import PATTERNS

pytestmark = pytest.mark.gpu


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
def ops():
    from romtime_amd import ops

    return ops


_DEVICE_PATTERNS = {}


def _device(name):
    if name not in _DEVICE_PATTERNS:
        _DEVICE_PATTERNS[name] = gd.device_pattern(*PATTERNS[name].csr)
    return _DEVICE_PATTERNS[name]


def _exact(got, want, what):
    assert gd.bits_equal(got, want), f"{what}: {gd.mismatch(np.asarray(got), np.asarray(want))}"


def _assert_launch(info, N, r, B):
    rp = 16 * pc.tile_rows(r)
    assert info["tile"] == (rp, rp) and info["grid"] == B * info["splits"] and info["splits"] == pc.fused_splits(N, B), info


def _run_exact(ctx, name, r, B, dlay, dpad, vpad, vmis=False):
    c = pc.exact_case(name, r, B)
    got, info, _ = gd.project_guarded(ctx, _device(name), c.data, c.V, dlay, dpad, vpad, vmis)
    _assert_launch(info, c.pattern.N, r, B)
    for b in range(B):
        _exact(got[b], c.want[b], f"{name} r={r} B={B} b={b} data {dlay}+{dpad} V pad {vpad}{' misaligned' if vmis else ''}")
    if c.pattern.nnz == 0:
        assert not got.any() and not np.signbit(got).any()
    return got


@pytest.mark.parametrize("name", list(PATTERNS))
def test_stage_table_is_the_restated_one(ops, name):
    p = PATTERNS[name]
    rec, any_unwindowed = ops.project_stage_info(*_device(name))
    want, want_any = pc.stage_records(*p.csr, p.N)
    assert rec.shape == want.shape and any_unwindowed == want_any
    for st, (g, w) in enumerate(zip(rec.tolist(), want.tolist())):
        if w[3] == 0:   # not windowed: e0, lo = k0 and nrow = 0
            assert (g[0], g[1], g[3]) == (w[0], st * pc.PK, 0), (st, g, w)
        else:
            assert g == w, (st, g, w)


@pytest.mark.parametrize("r", pc.LAYOUT_R)
@pytest.mark.parametrize("name", pc.LAYOUT_PATTERNS)
def test_every_tile_layout_exact(ctx, ops, name, r):
    p = PATTERNS[name]
    rec, any_unwindowed = ops.project_stage_info(*_device(name))
    assert any_unwindowed == (name == "far_entry") and pc.fused_splits(p.N, pc.LAYOUT_B) > 1
    for k, (_, vpad, vmis) in enumerate(pc.V_PLACEMENTS):
        kinds = pc.stage_kinds(rec, p.N, r, r + vpad, not vmis)
        assert p.has_kind(kinds)
        assert any(s.loader == "descriptor" for s in kinds) == (r % 2 == 0 and vpad % 2 == 0 and not vmis)
        assert any(s.loader == "predicated" and s.rows == pc.PK for s in kinds)
        _run_exact(ctx, name, r, pc.LAYOUT_B, "CF"[k % 2], (0, 1, 2, 0)[k], vpad, vmis)


@pytest.mark.parametrize("r", pc.EDGE_R)
@pytest.mark.parametrize("name", pc.EDGE_PATTERNS)
def test_stage_edges_exact(ctx, ops, name, r):
    p = PATTERNS[name]
    rec, _ = ops.project_stage_info(*_device(name))
    runs = pc.EDGE_RUNS + (pc.ENDS_RUNS if name.startswith("ends_") else ())
    for B, dlay, dpad, vpad in runs:
        assert p.has_kind(pc.stage_kinds(rec, p.N, r, r + vpad, True)), f"{name} lost the stage kind it is named for"
        _run_exact(ctx, name, r, B, dlay, dpad, vpad)


@pytest.mark.parametrize("name,r", pc.REPEAT_CASES)
def test_batch_and_repeat_bits(ctx, name, r):
    """Exact data: any summation order gives the same bits, so a vector's result may depend neither on its place in a
    batch nor on the call."""
    c = pc.exact_case(name, r, 3)
    first = _run_exact(ctx, name, r, 3, "C", 1, 0)
    again = _run_exact(ctx, name, r, 3, "C", 1, 0)
    _exact(again, first, "two identical calls")
    for b in range(3):
        alone, info, _ = gd.project_guarded(ctx, _device(name), c.data[:, b:b + 1], c.V, "F", 3, 0, single=True)
        _assert_launch(info, c.pattern.N, r, 1)
        _exact(alone[0], first[b], f"vector {b} alone and in the batch")


@pytest.mark.parametrize("r", pc.ROUNDED_R)
@pytest.mark.parametrize("name", pc.ROUNDED_PATTERNS)
def test_rounded_data_within_the_componentwise_bar(ctx, name, r):
    """|got - ref| <= (longest row + N + S + 2) 2^-53 (|V|^T |A| |V|) per entry against the np.longdouble product: the
    forward bound of a sum of that many roundings in any order, so a column scaled by 2^-30 is held as tightly as one
    scaled by 2^30."""
    c = pc.rounded_case(name, r)
    for dlay, dpad, vpad, vmis in (("C", 1, 0, False), ("F", 0, 1, True)):
        got, info, _ = gd.project_guarded(ctx, _device(name), c.data, c.V, dlay, dpad, vpad, vmis)
        _assert_launch(info, c.pattern.N, r, c.B)
        ok, worst = pc.within_bar(got, c)
        print(f"{name} r={r} data {dlay}: worst |err| / bound = {worst:.3g}")
        assert ok, worst
