"""rt_dense_lstsq_multi against the defining properties of its two modes, in long double, inside guard buffers.

* ``trans = 0`` (X minimises ||A X - B|| column by column): the optimality defect d = A^T (B - A X), per column
      ratio = |d|_inf / floor,   floor = EPS max_i (|A|^T (|B| + |A| |X|))_i .
* ``trans = 1`` (X the minimum-norm solution of A^T X = B): the defect d = A^T X - B with floor = EPS max_i (|A|^T |X| + |B|)_i,
  and the part of X outside the range of A, p = X - Q (Q^T X) with Q from a long-double Householder QR written here,
  with floor = EPS max_i (|X| + |Q| (|Q|^T |X|))_i .
Every measure is taken of the device's X and of NumPy's (``np.linalg.lstsq``; ``np.linalg.pinv(A).T @ B``) on the same data,
and the bar is  ratio <= F max(ratio_numpy, 1):  rounding differs between summation orders, so F is measured on the
MI355X as the worst observed ratio / max(ratio_numpy, 1) times 10 ("Oversampled (M)DEIM") and never derived
from the code under test on the CPU.

Shapes: the smallest, both sides of the 64-lane wave in rows and columns, the LDS limit in three proportions; right-hand
sides 1 and both sides of the 256 a workgroup takes (read from the plan)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guarded as gd
from tests.svd_cases import _need_extended

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
# measured on the MI355X over every case below: worst ratio / max(ratio_numpy, 1) = 8.875 (optimality defect of the fit, at
# 2 x 1, where the residual is nearly orthogonal to the one column and the floor is small), 3.151 (defect of the
# minimum-norm solve) and 2.329 (its part outside the range of A); times 10
F_DEFECT_LS = 89.0
F_DEFECT_MN = 32.0
F_RANGE = 24.0
SHAPES = [(2, 1), (2, 2), (3, 2), (16, 8), (17, 16), (33, 32), (65, 64), (128, 64), (256, 64), (128, 128)]
KINDS = ("normal", "graded")
WARN_SINGULAR = 2
_cache = {}


@pytest.fixture(scope="module")
def ops():
    from romtime_amd import ops as _ops

    return _ops


def _nrhs_list(ops, rows, cols):
    per = ops.dense_lstsq_plan(rows, cols)[1]
    assert per == 256
    return [1, 63, 65, per - 1, per, per + 1, 2 * per + 1]


def _matrix(rows, cols, kind):
    rng = np.random.default_rng(1000 * rows + cols + (7 if kind == "graded" else 0))
    A = rng.standard_normal((rows, cols))
    if kind == "graded":
        A *= 10.0 ** (-4.0 * np.arange(cols) / max(cols - 1, 1))[None, :]
    return A


def householder_q(A):
    """Thin Q (rows x cols, long double) of A = Q R by Householder reflections, all arithmetic in long double."""
    _need_extended()
    R = np.array(A, dtype=LD)
    rows, cols = R.shape
    vs = []
    for k in range(cols):
        x = R[k:, k].copy()
        nrm = np.sqrt((x * x).sum())
        v = x
        if nrm > 0:
            v[0] += nrm if x[0] >= 0 else -nrm
            R[k:, k:] -= np.outer(v, (2 / (v * v).sum()) * (v @ R[k:, k:]))
        vs.append(v)
    Q = np.zeros((rows, cols), dtype=LD)
    Q[np.arange(cols), np.arange(cols)] = 1
    for k in range(cols - 1, -1, -1):
        v = vs[k]
        vv = (v * v).sum()
        if vv > 0:
            Q[k:, :] -= np.outer(v, (2 / vv) * (v @ Q[k:, :]))
    return Q


def _data(rows, cols, kind, trans):
    key = (rows, cols, kind, trans)
    if key not in _cache:
        A = _matrix(rows, cols, kind)
        rng = np.random.default_rng(17 + rows * cols)
        B = rng.standard_normal((cols if trans else rows, 2 * 256 + 1))
        ref = np.linalg.pinv(A).T @ B if trans else np.linalg.lstsq(A, B, rcond=None)[0]
        Q = householder_q(A) if trans else None
        _cache[key] = dict(A=A, B=B, Q=Q, numpy=measures(A, B, ref, trans, Q))
    return _cache[key]


def measures(A, B, X, trans, Q=None):
    """Per column: dict of ratio arrays (``defect``; with ``trans`` also ``range``)."""
    Al, Bl, Xl = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD), np.asarray(X, dtype=LD)
    aA = np.abs(Al)
    tiny = LD(np.finfo(np.float64).tiny)
    if not trans:
        d = Al.T @ (Bl - Al @ Xl)
        floor = EPS * (aA.T @ (np.abs(Bl) + aA @ np.abs(Xl))).max(axis=0)
        return dict(defect=(np.abs(d).max(axis=0) / np.maximum(floor, tiny)).astype(np.float64))
    d = Al.T @ Xl - Bl
    floor = EPS * (aA.T @ np.abs(Xl) + np.abs(Bl)).max(axis=0)
    p = Xl - Q @ (Q.T @ Xl)
    pfloor = EPS * (np.abs(Xl) + np.abs(Q) @ (np.abs(Q).T @ np.abs(Xl))).max(axis=0)
    return dict(defect=(np.abs(d).max(axis=0) / np.maximum(floor, tiny)).astype(np.float64),
                range=(np.abs(p).max(axis=0) / np.maximum(pfloor, tiny)).astype(np.float64))


def _solve(A, B, trans, want_info=0):
    """rt_dense_lstsq_multi with A and B as guarded operands and X in a guarded output; returns X on the host."""
    from romtime_amd._lib import Context

    ctx = Context.current()
    rows, cols = A.shape
    nrhs = B.shape[1]
    Ad, Bd = gd.guarded_operand(A, "C"), gd.guarded_operand(B, "C")
    X = gd.guarded_output((rows if trans else cols, nrhs))
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    ctx.check(ctx.lib.rt_dense_lstsq_multi(ctx.handle, P(Ad), rows, cols, int(trans), P(Bd), P(X.t), nrhs, P(info)),
              "rt_dense_lstsq_multi")
    torch.cuda.synchronize()
    assert X.check() == [], X.check()
    assert gd.operand_intact(Ad, A) == [] and gd.operand_intact(Bd, B) == []
    assert int(info[0]) == want_info, int(info[0])
    return X.t.cpu().numpy().copy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("trans", [0, 1], ids=["fit", "min_norm"])
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_defining_properties(ops, rows, cols, trans, kind):
    c = _data(rows, cols, kind, trans)
    results = {}
    for nrhs in _nrhs_list(ops, rows, cols):
        X = _solve(c["A"], np.ascontiguousarray(c["B"][:, :nrhs]), trans)
        got = measures(c["A"], c["B"][:, :nrhs], X, trans, c["Q"])
        for name, ratio in got.items():
            base = np.maximum(c["numpy"][name][:nrhs], 1.0)
            F = F_RANGE if name == "range" else (F_DEFECT_MN if trans else F_DEFECT_LS)
            print(f"LSTSQ {rows}x{cols} {kind} trans={trans} nrhs={nrhs} {name}: ratio max={ratio.max():.3g} numpy max="
                  f"{c['numpy'][name][:nrhs].max():.3g} worst ratio/max(numpy,1)={np.max(ratio / base):.3g}")
            assert np.all(ratio <= F * base), (name, nrhs, float(np.max(ratio / base)))
        results[nrhs] = X
    full = results[max(results)]
    for nrhs, X in results.items():                               # a column's bits depend neither on nrhs nor on its place
        assert gd.bits_equal(X, full[:, :nrhs]), (nrhs, gd.mismatch(X, np.ascontiguousarray(full[:, :nrhs])))
    last = _solve(c["A"], np.ascontiguousarray(c["B"][:, full.shape[1] - 1:full.shape[1]]), trans)
    assert gd.bits_equal(last[:, 0], full[:, -1])                 # the last column alone, first in its own batch


@pytest.mark.parametrize("n", [1, 2, 17, 64, 65, 128])
def test_square_agrees_with_the_pivoted_lu(ops, n):
    """rows == cols: both modes against ``ops.dense_solve_multi`` - two backward-stable solves of one system differ by at
    most a modest multiple of eps cond(A) |x|; 100 n covers the growth constants of both."""
    A = _matrix(n, n, "normal")
    B = np.random.default_rng(n).standard_normal((n, 300))
    cond = np.linalg.cond(A)
    lu, info = ops.dense_solve_multi(ops.to_device(A), ops.to_device(B))
    lut, _ = ops.dense_solve_multi(ops.to_device(np.ascontiguousarray(A.T)), ops.to_device(B))
    assert int(info.item()) == 0
    for trans, ref in ((0, lu.cpu().numpy()), (1, lut.cpu().numpy())):
        X = _solve(A, B, trans)
        err = np.abs(X - ref).max(axis=0) / np.abs(ref).max(axis=0)
        print(f"LSTSQ square n={n} trans={trans} cond={cond:.3g} worst rel difference={err.max():.3g}")
        assert np.all(err <= 100 * n * EPS * cond), (trans, err.max(), cond)


@pytest.mark.parametrize("rows,cols,first,again", [(3, 2, 0, 1), (17, 16, 3, 9), (65, 64, 0, 63), (128, 64, 31, 32), (128, 128, 5, 100)])
def test_a_repeated_column_is_flagged(ops, rows, cols, first, again):
    A = _matrix(rows, cols, "normal")
    B = np.random.default_rng(3).standard_normal((rows, 5))
    _solve(A, B, 0, want_info=0)
    A[:, again] = A[:, first]
    for trans in (0, 1):
        _solve(A, np.ascontiguousarray(B[:cols] if trans else B), trans, want_info=WARN_SINGULAR)


def test_ops_wrapper_and_limits(ops):
    from romtime_amd._lib import RomtimeHipError

    A = _matrix(48, 32, "normal")
    B = np.random.default_rng(5).standard_normal((48, 40))
    X, info = ops.dense_lstsq_multi(ops.to_device(A), ops.to_device(B))
    assert int(info.item()) == 0 and tuple(X.shape) == (32, 40)
    np.testing.assert_allclose(X.cpu().numpy(), np.linalg.lstsq(A, B, rcond=None)[0], rtol=0, atol=1e-12)
    Xt, _ = ops.dense_lstsq_multi(ops.to_device(A), ops.to_device(B[:32]), trans=True)
    np.testing.assert_allclose(Xt.cpu().numpy(), np.linalg.pinv(A).T @ B[:32], rtol=0, atol=1e-12)
    for rows, cols in ((257, 8), (200, 100), (130, 129)):
        with pytest.raises(RomtimeHipError):
            ops.dense_lstsq_multi(torch.zeros((rows, cols), dtype=torch.float64, device="cuda"),
                                  torch.zeros((rows, 3), dtype=torch.float64, device="cuda"))
