"""The three reduced-solve entry points of solve.hip - rt_dense_solve_batched, rt_dense_solve_multi and
rt_tracked_solve_batched (newton_solve_kernel, also the solve of both online sweeps) - where a subtly wrong kernel
used to pass:

* systems whose pivoted LU is exact in float64 (tests/solve_cases.py; premise proved on the host by
  tests/test_reduced_solves_cpu.py): the device answer must equal the known solution bit for bit, at both sides of
  every change of the thread mapping, with pivots in every wave, under growth (Wilkinson's matrix), and with two
  equal pivot candidates in different waves, of which only the documented (|value| desc, row asc) choice stays exact;
* every operand inside NaN-poisoned / canary buffers, aligned and 8 bytes off;
* accuracy on systems of condition number 1 .. 1e10 against the solution in 50-digit arithmetic, as a ratio to
  LAPACK's error on the same system instead of a fixed tolerance;
* every route of the tracked solve's state machine, asserted by the device counters (Context.sweep_stats) and by the
  bits of the carried inverse;
* both sweeps at the sizes the solve kernels branch on.

Not covered, for want of inputs that reach them: the route where the refinement has solved but the refresh of the
inverse then fails, and the NaN exits of the refinement and of the Newton-Schulz loop.

The ratio bar: error <= F * max(LAPACK's error on the same system, r * 2.2e-16), for the forward error against the
50-digit solution and for the normwise backward error.  F is ten times the worst ratio measured on an MI355X over the
cases of this module (never more than 100); the measured figures are in the docstrings of the tests that assert it.
"""
import ctypes as C

import mpmath  # noqa: F401  (the 50-digit reference of tests/solve_cases.py: its absence is an error, not a skip)
import numpy as np
import pytest
import torch

from oracle import romtime_oracle as oracle
from tests import guarded as gd
from tests import solve_cases as sc

pytestmark = pytest.mark.gpu

F_BATCHED, F_MULTI, F_TRACKED = sc.F_BATCHED, sc.F_MULTI, sc.F_TRACKED


def P(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def ops():
    from romtime_amd import ops

    gd.require_clean_env()
    return ops


def _ctx():
    from romtime_amd._lib import Context

    gd.require_clean_env()
    return Context.current()


def _exact_batch(r, B=3, tiny_last=False, tied=False):
    """B different exact systems of size r (the seeds the host test proves the premise for)."""
    sys_ = [sc.exact_lu_system(r, np.random.RandomState(r + 1000 * i), tiny_last, tied) for i in range(B)]
    return tuple(np.stack([s[k] for s in sys_]) for k in range(3))


def _wilkinson_batch(r, B=3):
    sys_ = [sc.wilkinson_system(r, np.random.RandomState(r + 1000 * i)) for i in range(B)]
    return tuple(np.stack([s[k] for s in sys_]) for k in range(3))


def _assert_bar(ratios, F, what):
    print(f"ratio to LAPACK {what}: forward {ratios[0]:.3g} backward {ratios[1]:.3g}")
    assert ratios[0] <= F[0] and ratios[1] <= F[1], (what, ratios, F)


# ---- rt_dense_solve_batched / rt_dense_solve_multi: exact answers ------------------------------------------------------
@pytest.mark.parametrize("r", sc.LU_SIZES)
def test_batched_lu_exact_family_bitwise(ops, r):
    """Three different systems per launch (a kernel that solves system 0 three times fails), pivots in every wave."""
    K, b, x = _exact_batch(r)
    got, info = ops.dense_solve(ops.to_device(K), ops.to_device(b))
    assert gd.bits_equal(got.cpu().numpy(), x), gd.mismatch(got.cpu().numpy(), x)
    assert info.cpu().tolist() == [0, 0, 0]


@pytest.mark.parametrize("r", sc.WILKINSON_SIZES)
def test_batched_lu_wilkinson_bitwise(ops, r):
    """Wilkinson's growth matrix: the last column doubles at every step up to 2^(r-1), all of it exact integers."""
    K, b, x = _wilkinson_batch(r)
    got, info = ops.dense_solve(ops.to_device(K), ops.to_device(b))
    assert gd.bits_equal(got.cpu().numpy(), x), gd.mismatch(got.cpu().numpy(), x)
    assert info.cpu().tolist() == [0, 0, 0]


@pytest.mark.parametrize("r", sc.TIED_SIZES)
def test_lu_tie_break_across_waves_bitwise(ops, r):
    """Two equal candidates in column 0, in row 0 (wave 0) and in the last row (the last wave that owns rows): the
    cross-wave merge must take (|value| desc, row asc).  Under that order the factorisation is the exact one; the other
    tied row leads to pivots that are no powers of two and a rounded answer (host proof:
    test_tied_exact_family_is_exact_only_under_the_documented_order).  Both LU kernels, 256 threads."""
    K, b, x = _exact_batch(r, tied=True)
    got, info = ops.dense_solve(ops.to_device(K), ops.to_device(b))
    assert gd.bits_equal(got.cpu().numpy(), x), gd.mismatch(got.cpu().numpy(), x)
    assert info.cpu().tolist() == [0, 0, 0]
    X = sc.small_integers(np.random.RandomState(r), (r, 300))
    got, info = ops.dense_solve_multi(ops.to_device(K[0]), ops.to_device(K[0] @ X))
    assert gd.bits_equal(got.cpu().numpy(), X), gd.mismatch(got.cpu().numpy(), X)
    assert int(info.item()) == 0


@pytest.mark.parametrize("r", sc.LU_SIZES + sc.WILKINSON_SIZES)
def test_multi_lu_exact_family_bitwise(ops, r):
    """The same matrices with the columns of a small-integer X as right-hand sides, at the workgroup edges of the
    right-hand-side index (256 per workgroup)."""
    rng = np.random.RandomState(r)
    K = sc.wilkinson_system(r, rng)[0] if r in sc.WILKINSON_SIZES else sc.exact_lu_system(r, rng)[0]
    Kd = ops.to_device(K)
    for nrhs in (1, 255, 256, 257, 513):
        X = sc.small_integers(rng, (r, nrhs))
        got, info = ops.dense_solve_multi(Kd, ops.to_device(K @ X))
        assert gd.bits_equal(got.cpu().numpy(), X), (nrhs, gd.mismatch(got.cpu().numpy(), X))
        assert int(info.item()) == 0


@pytest.mark.parametrize("r", [33, 65])
def test_batched_lu_info_is_per_system(ops, r):
    """A regular system, an exactly singular one (a zero column) and another regular one in one launch."""
    K, b, x = _exact_batch(r)
    K[1][:, r // 2] = 0.0
    got, info = ops.dense_solve(ops.to_device(K), ops.to_device(b))
    assert info.cpu().tolist() == [0, sc.WARN_SINGULAR, 0]
    got = got.cpu().numpy()
    assert gd.bits_equal(got[0], x[0]) and gd.bits_equal(got[2], x[2])


# ---- ... inside guard buffers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("r", [33, 64, 65, 128])
def test_lu_kernels_inside_guard_buffers(r, misalign):
    """K (and B) inside NaN-poisoned buffers, rhs / X / info inside canaries, base pointers aligned or 8 bytes off:
    nothing read or written outside, every output word written, the exact answers."""
    ctx = _ctx()
    B = 3
    K, b, x = _exact_batch(r, B)
    Kg = gd.guarded_operand(K.reshape(B * r, r), "C", 0, misalign=misalign)
    xo = gd.guarded_output((B, r), misalign=misalign).fill(b)
    io = sc.GuardedInt32(B)
    assert ctx.lib.rt_dense_solve_batched(ctx.handle, P(Kg), P(xo.t), r, B, P(io.t)) == 0
    torch.cuda.synchronize()
    assert xo.check() == [] and io.check() == [], (xo.check(), io.check())
    assert gd.operand_intact(Kg, K.reshape(B * r, r)) == []
    assert gd.bits_equal(xo.t.cpu().numpy(), x), gd.mismatch(xo.t.cpu().numpy(), x)
    assert io.t.cpu().tolist() == [0] * B

    nrhs = 257                                           # odd: every other row of B and X starts 8 bytes off
    X = sc.small_integers(np.random.RandomState(r), (r, nrhs))
    K1g = gd.guarded_operand(K[0], "C", 0, misalign=misalign)
    Bg = gd.guarded_operand(K[0] @ X, "C", 0, misalign=misalign)
    Xo = gd.guarded_output((r, nrhs), misalign=misalign)
    i1 = sc.GuardedInt32(1)
    assert ctx.lib.rt_dense_solve_multi(ctx.handle, P(K1g), r, P(Bg), P(Xo.t), nrhs, P(i1.t)) == 0
    torch.cuda.synchronize()
    assert Xo.check() == [] and i1.check() == [], (Xo.check(), i1.check())
    assert gd.operand_intact(K1g, K[0]) == [] and gd.operand_intact(Bg, K[0] @ X) == []
    assert gd.bits_equal(Xo.t.cpu().numpy(), X), gd.mismatch(Xo.t.cpu().numpy(), X)
    assert i1.t.cpu().tolist() == [0]


# ---- ... accuracy against the 50-digit solution ------------------------------------------------------------------------
_CONDITIONED = {}


def _conditioned(r, e):
    """K of condition number 10^e, right-hand sides (three columns for the sizes rt_dense_solve_multi runs) and their
    50-digit solutions; computed once per (r, e): twelve systems with twenty-eight right-hand sides.  (The tracked-solve
    tests compare every one of their answers with such a solution as well: a few hundred more, r^2 multi-precision
    operations per refinement pass each.)"""
    if (r, e) not in _CONDITIONED:
        rng = np.random.RandomState(100 * r + e)
        K, b = sc.conditioned_system(r, e, rng)
        Bm = np.column_stack([b] + [rng.standard_normal(r) for _ in range(2 if r <= 80 else 0)])
        _CONDITIONED[(r, e)] = (K, Bm, sc.reference_solve(K, Bm))
    return _CONDITIONED[(r, e)]


@pytest.mark.parametrize("e", [0, 4, 8, 10])
@pytest.mark.parametrize("r", [40, 80, 128])
def test_batched_lu_accuracy_against_50_digits(ops, r, e):
    """Measured on an MI355X: worst forward ratio 1.25 (r = 40, e = 4), worst backward ratio 0.054 (r = 40, e = 0) over
    these twelve cases; 1.34 and 0.079 over the cases of tests/test_kernels_gpu.py::test_dense_solve, which shares the
    bar: F_BATCHED = (13.4, 0.79).  The backward error sits at 0.05 r eps, well under the floor of the bar."""
    K, Bm, Xref = _conditioned(r, e)
    got, info = ops.dense_solve(ops.to_device(K), ops.to_device(Bm[:, 0]))
    assert int(info.item()) == 0
    _assert_bar(sc.error_ratios(K, Bm[:, 0], got.cpu().numpy(), Xref[:, 0]), F_BATCHED, f"batched r={r} e={e}")


@pytest.mark.parametrize("e", [0, 4, 8, 10])
@pytest.mark.parametrize("r", [40, 80])
def test_multi_lu_accuracy_against_50_digits(ops, r, e):
    """Measured on an MI355X: worst forward ratio 1.25 (r = 40, e = 4), worst backward ratio 0.060 (r = 40, e = 0) over
    these eight cases (the worst of the three columns of each): F_MULTI = (12.5, 0.6)."""
    K, Bm, Xref = _conditioned(r, e)
    got, info = ops.dense_solve_multi(ops.to_device(K), ops.to_device(Bm))
    assert int(info.item()) == 0
    got = got.cpu().numpy()
    ratios = [sc.error_ratios(K, Bm[:, j], got[:, j], Xref[:, j]) for j in range(Bm.shape[1])]
    _assert_bar(tuple(max(c) for c in zip(*ratios)), F_MULTI, f"multi r={r} e={e}")


# ---- rt_tracked_solve_batched: every route, asserted by the counters -------------------------------------------------------
def _tracked(K, b, Xinv=None, have_prev=None, misalign=False):
    """One call of the C entry point on operands placed at a 16-byte aligned base or 8 bytes past one.  ``Xinv``: the
    carried inverse, or what the buffer holds before a first call.  Returns x, info, Xinv after the call, and the
    differences of the four device counters."""
    ctx = _ctx()
    B, r, _ = K.shape
    have_prev = (Xinv is not None) if have_prev is None else have_prev
    Kd, bd = sc.place(K, misalign), sc.place(b, misalign)
    Xd = sc.place(np.zeros_like(K) if Xinv is None else Xinv, misalign)
    info = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    before = ctx.sweep_stats()
    assert ctx.lib.rt_tracked_solve_batched(ctx.handle, P(Kd), P(Xd), P(bd), r, B, int(have_prev), P(info)) == 0
    after = ctx.sweep_stats()
    assert gd.bits_equal(Kd.cpu().numpy(), K)
    return bd.cpu().numpy(), info.cpu().numpy(), Xd.cpu().numpy(), {k: after[k] - before[k] for k in after}


_LADDER_REF = {}


def _ladder_reference(r, i, K, b):
    if (r, i) not in _LADDER_REF:
        _LADDER_REF[(r, i)] = np.stack([sc.reference_solve(K[s], b[s]) for s in range(K.shape[0])])
    return _LADDER_REF[(r, i)]


def _ladder_bar(r, i, K, b, x, what):
    ref = _ladder_reference(r, i, K, b)
    ratios = [sc.error_ratios(K[s], b[s], x[s], ref[s]) for s in range(K.shape[0])]
    _assert_bar(tuple(max(c) for c in zip(*ratios)), F_TRACKED, what)


@pytest.mark.parametrize("r,misalign", [(r, False) for r in sc.LADDER_SIZES] + [(16, True), (64, True), (80, True)])
def test_tracked_solve_route_ladder(r, misalign):
    """A first call with K0 = randn / sqrt(r) + 2 I, then K0 + d dK from the inverse that call left, four different
    systems per launch.  The route of every rung is asserted by the counters and by the bits of Xinv:

      first call            safe start, Newton-Schulz              newton_iterations > 0, restarts 0
      d = 0 .. 1e-3         refinement alone (<= 4 steps)          newton_iterations +0, solves +B, Xinv bitwise unchanged
      d = 2e-2              solved by refinement, then refreshed   newton_iterations > 0, restarts 0, Xinv changed
      d = 0.1               out of steps, Newton-Schulz from X     newton_iterations > 0, restarts 0, Xinv changed
      d = 1, 3              |I - K X| >= 0.7: restart              restarts +B

    d = 2e-2: the host restatement (solve_cases.tracked_model) solves these systems at refinement step 7 or 8 at every
    size, at least two steps past NS_REFRESH_AFTER = 5 (at 1e-2 it took 6); tests/test_reduced_solves_cpu.py holds the
    ladder's inputs to that and to the margins of the other rungs.  r = 5 .. 80 run all five tile layouts (50: layout 4
    on the scalar path, 64: layout 4 on the 16-byte path); the misaligned runs take the scalar path with r == rp.
    Every answer against the 50-digit solution under the ratio bar.  Measured on an MI355X over all rungs and sizes
    (and the other tracked-solve tests of this module): worst forward ratio 2.7 (r = 5, d = 3), worst backward ratio 0.275
    (r = 5, d = 2e-2): F_TRACKED = (27, 2.75)."""
    calls = sc.ladder_calls(r)
    K0, b0, _ = calls[0]
    B = K0.shape[0]
    x, info, X0, dc = _tracked(K0, b0, misalign=misalign)
    assert info.tolist() == [0] * B
    assert dc["newton_iterations"] >= B and dc["restarts"] == 0 and dc["lu_fallbacks"] == 0 and dc["solves"] == B, dc
    _ladder_bar(r, 0, K0, b0, x, f"tracked r={r} first call")
    for i, (K, b, route) in enumerate(calls[1:], start=1):
        x, info, X1, dc = _tracked(K, b, X0, misalign=misalign)
        what = f"tracked r={r} d={sc.LADDER[i - 1][0]} ({route})"
        assert info.tolist() == [0] * B, what
        assert dc["lu_fallbacks"] == 0 and dc["solves"] == B, (what, dc)
        if route == "refine":
            assert dc["newton_iterations"] == 0 and dc["restarts"] == 0, (what, dc)
            assert gd.bits_equal(X1, X0), (what, gd.mismatch(X1, X0))
        else:
            assert dc["newton_iterations"] >= B, (what, dc)
            assert dc["restarts"] == (B if route == "restart" else 0), (what, dc)
            assert all(not gd.bits_equal(X1[s], X0[s]) for s in range(B)), what
            # the refreshed inverse is one: |I - K X|_F after the last update is far below the 1e-6 it was stopped at
            assert max(np.linalg.norm(np.eye(r) - K[s] @ X1[s]) for s in range(B)) <= 1e-9, what
        _ladder_bar(r, i, K, b, x, what)


@pytest.mark.parametrize("r,misalign", [(r, False) for r in sc.LADDER_SIZES] + [(16, True), (64, True), (80, True)])
def test_tracked_solve_scaled_permutations_bitwise(r, misalign):
    """One nonzero per row and column: every entry of every Newton-Schulz iterate is a chain of single correctly
    rounded operations, repeated on the host (solve_cases.scaled_permutation_first_call).  The inverse the kernel
    leaves, its answer and its iteration count are known exactly; the nonzeros of X and X T lie in every full tile of
    every layout, so a tile computed by no wave, by two, or scaled by 1 + 2^-40 changes the bits of Xinv (the answer
    alone would hide it: its refinement step squares the error of X away)."""
    B = 4
    sys_ = [sc.scaled_permutation_system(r, np.random.RandomState(r + 1000 * i)) for i in range(B)]
    K, b = np.stack([s[0] for s in sys_]), np.stack([s[1] for s in sys_])
    want = [sc.scaled_permutation_first_call(K[i], b[i]) for i in range(B)]
    got, info, X1, dc = _tracked(K, b, misalign=misalign)
    assert info.tolist() == [0] * B
    assert dc == dict(newton_iterations=sum(w[2] for w in want), restarts=0, lu_fallbacks=0, solves=B), dc
    for i in range(B):
        assert gd.bits_equal(X1[i], want[i][1]), (i, gd.mismatch(X1[i], want[i][1]))
        assert gd.bits_equal(got[i], want[i][0]), (i, gd.mismatch(got[i], want[i][0]))


@pytest.mark.parametrize("r", sc.FALLBACK_SIZES)
def test_tracked_solve_fallback_then_recovery(r):
    """Condition number 2^60: Newton-Schulz runs out of iterations, the pivoted LU inside the kernel (512 threads,
    lu_parts = min(8, 512 / r)) gives the exact answer and zeroes Xinv - which held ones before, so the zeros are the
    kernel's.  The next call, tracked from that zeroed inverse with a regular matrix, restarts and does not fall back:
    "the next call starts afresh"."""
    B = 2
    K, b, x = _exact_batch(r, B, tiny_last=True)
    got, info, X1, dc = _tracked(K, b, np.ones_like(K), have_prev=False)
    assert info.tolist() == [0] * B
    assert dc["lu_fallbacks"] == B and dc["solves"] == B and dc["newton_iterations"] == B * sc.NS_MAX_ITER, dc
    assert gd.bits_equal(got, x), gd.mismatch(got, x)
    assert gd.bits_equal(X1, np.zeros_like(K))
    K0, _, rng = sc.ladder_systems(r, B)
    b0 = rng.standard_normal((B, r))
    got, info, X2, dc = _tracked(K0, b0, X1, have_prev=True)
    assert info.tolist() == [0] * B
    assert dc["restarts"] == B and dc["lu_fallbacks"] == 0 and dc["solves"] == B, dc
    ref = np.stack([sc.reference_solve(K0[s], b0[s]) for s in range(B)])
    ratios = [sc.error_ratios(K0[s], b0[s], got[s], ref[s]) for s in range(B)]
    _assert_bar(tuple(max(c) for c in zip(*ratios)), F_TRACKED, f"tracked r={r} after a fallback")
    assert max(np.linalg.norm(np.eye(r) - K0[s] @ X2[s]) for s in range(B)) <= 1e-9


@pytest.mark.parametrize("r", sc.FALLBACK_SIZES)
def test_tracked_solve_fallback_tie_break_across_waves_bitwise(r):
    """The tied exact family with condition number 2^60: the fallback LU (512 threads, eight waves) meets the two equal
    candidates of column 0 in its first and in its last wave that owns rows, and only the documented order is exact."""
    B = 2
    K, b, x = _exact_batch(r, B, tiny_last=True, tied=True)
    got, info, X1, dc = _tracked(K, b)
    assert info.tolist() == [0] * B and dc["lu_fallbacks"] == B and dc["solves"] == B, (info, dc)
    assert gd.bits_equal(got, x), gd.mismatch(got, x)
    assert not X1.any()


@pytest.mark.parametrize("r", [16, 50])
def test_tracked_solve_four_routes_in_one_launch(r):
    """Refinement alone, restart, fallback and exactly singular side by side: per-system info, every non-singular
    answer, and counters equal to the sums of the same four systems solved one launch each."""
    K0, dK, rng = sc.ladder_systems(r, 2)
    Kt, bt, xt = sc.exact_lu_system(r, np.random.RandomState(r), tiny_last=True)
    Ks = sc.exact_lu_system(r, np.random.RandomState(r + 1))[0]
    Ks[:, r // 3] = 0.0
    _, _, X0, _ = _tracked(K0, rng.standard_normal((2, r)))
    K = np.stack([K0[0] + 1e-4 * dK[0], K0[1] + 3.0 * dK[1], Kt, Ks])
    b = np.stack([rng.standard_normal(r), rng.standard_normal(r), bt, rng.standard_normal(r)])
    X = np.stack([X0[0], X0[1], X0[0], X0[1]])
    single = [_tracked(K[s:s + 1], b[s:s + 1], X[s:s + 1]) for s in range(4)]
    routes = [dict(newton_iterations=0, restarts=0, lu_fallbacks=0), dict(restarts=1, lu_fallbacks=0),
              dict(restarts=1, lu_fallbacks=1), dict(lu_fallbacks=1)]
    for (_, _, _, dc), want in zip(single, routes):
        assert dc["solves"] == 1 and all(dc[k] == v for k, v in want.items()), (dc, want)
    got, info, X1, dc = _tracked(K, b, X)
    assert info.tolist() == [0, 0, 0, sc.WARN_SINGULAR]
    assert dc == {k: sum(s[3][k] for s in single) for k in dc}, (dc, [s[3] for s in single])
    for s in range(3):
        assert gd.bits_equal(got[s], single[s][0][0])
        assert gd.bits_equal(X1[s], single[s][2][0])
    assert gd.bits_equal(got[2], xt), gd.mismatch(got[2], xt)
    assert gd.bits_equal(X1[0], X0[0]) and not X1[2].any() and not X1[3].any()
    for s in (0, 1):
        ref = sc.reference_solve(K[s], b[s])
        _assert_bar(sc.error_ratios(K[s], b[s], got[s], ref), F_TRACKED, f"tracked r={r} mixed launch, system {s}")


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("r", [16, 50, 80])
def test_tracked_solve_inside_guard_buffers(r, misalign):
    """A first call (Xinv an output: every word written, none outside) and a refinement-alone call (Xinv an operand:
    intact bit for bit, poison untouched), K poisoned around, rhs and info in canaries; the bits of the plain calls."""
    ctx = _ctx()
    B = 3
    K0, dK, rng = sc.ladder_systems(r, B)
    b0, b1 = rng.standard_normal((B, r)), rng.standard_normal((B, r))
    K1 = K0 + 1e-4 * dK
    x0, _, X0, _ = _tracked(K0, b0, misalign=misalign)
    x1, _, _, _ = _tracked(K1, b1, X0, misalign=misalign)

    Kg = gd.guarded_operand(K0.reshape(B * r, r), "C", 0, misalign=misalign)
    Xo = gd.guarded_output((B * r, r), misalign=misalign)
    xo = gd.guarded_output((B, r), misalign=misalign).fill(b0)
    io = sc.GuardedInt32(B)
    assert ctx.lib.rt_tracked_solve_batched(ctx.handle, P(Kg), P(Xo.t), P(xo.t), r, B, 0, P(io.t)) == 0
    torch.cuda.synchronize()
    assert Xo.check() == [] and xo.check() == [] and io.check() == [], (Xo.check(), xo.check(), io.check())
    assert gd.operand_intact(Kg, K0.reshape(B * r, r)) == []
    assert gd.bits_equal(xo.t.cpu().numpy(), x0) and gd.bits_equal(Xo.t.cpu().numpy().reshape(B, r, r), X0)
    assert io.t.cpu().tolist() == [0] * B

    Kg = gd.guarded_operand(K1.reshape(B * r, r), "C", 0, misalign=misalign)
    Xg = gd.guarded_operand(X0.reshape(B * r, r), "C", 0, misalign=misalign)
    xo = gd.guarded_output((B, r), misalign=misalign).fill(b1)
    io = sc.GuardedInt32(B)
    before = ctx.sweep_stats()
    assert ctx.lib.rt_tracked_solve_batched(ctx.handle, P(Kg), P(Xg), P(xo.t), r, B, 1, P(io.t)) == 0
    after = ctx.sweep_stats()
    assert after["newton_iterations"] == before["newton_iterations"] and after["solves"] - before["solves"] == B
    assert xo.check() == [] and io.check() == [], (xo.check(), io.check())
    assert gd.operand_intact(Kg, K1.reshape(B * r, r)) == []
    assert gd.operand_intact(Xg, X0.reshape(B * r, r)) == []
    assert gd.bits_equal(xo.t.cpu().numpy(), x1)
    assert io.t.cpu().tolist() == [0] * B


# ---- the sweeps at the sizes the solve kernels branch on -------------------------------------------------------------------
@pytest.mark.parametrize("bdf2", [True, False])
@pytest.mark.parametrize("r", [16, 50, 64, 80, 81, 128])
def test_hyper_reduced_sweep_at_the_solve_kernels_sizes(ops, r, bdf2):
    """rt_hrom_bdf_sweep against oracle.hrom_solve under the 1e-10 rel-L2 bar: r a multiple of 16 (M_N comes in by
    16-byte loads), tile layout 4 (50, 64), the largest tracked size (80), the first size of the three-launch route
    (81) and the largest size (128).  Up to 80 the regular systems must not ride on the LU fallback, and the sweep
    replayed as a graph gives the same bits."""
    from romtime_amd.sweep import hrom_bdf_sweep

    nt, n_mu, dt = 6, 3, 1e-2
    rng = np.random.RandomState(40 + r)
    mass, lin, nl, rhs = sc.synthetic_hrom_terms(rng, r, nt, n_mu, 4, [(3, "spd"), (5, "general")], 6, 4, wobble_tables=True)
    uN = hrom_bdf_sweep(mass, lin, nl, rhs, dt, bdf2=bdf2).cpu().numpy()
    stats = _ctx().sweep_stats()
    for b in range(n_mu):
        ref = oracle.hrom_solve(mass, lin, nl, rhs, b, r, nt, dt, bdf2)
        rel = np.linalg.norm(uN[b].T - ref) / np.linalg.norm(ref)
        assert rel <= 1e-10, (b, rel)
    if r <= 80:
        assert stats["lu_fallbacks"] == 0 and stats["solves"] == nt * n_mu, stats
        ctx = _ctx()
        ctx.set_option("sweep_graph", 1)
        try:
            uG = hrom_bdf_sweep(mass, lin, nl, rhs, dt, bdf2=bdf2).cpu().numpy()
        finally:
            ctx.set_option("sweep_graph", 0)
        np.testing.assert_array_equal(uG, uN)


@pytest.mark.parametrize("bdf2", [True, False])
@pytest.mark.parametrize("r", [16, 64, 81])
def test_rom_sweep_at_the_solve_kernels_sizes(ops, r, bdf2):
    """rt_rom_bdf_sweep against oracle.rom_solve_nonlinear (exact dense solver) under the 1e-10 rel-L2 bar."""
    from romtime_amd.sweep import rom_bdf_sweep
    from romtime_amd.testing.mock import AffineBurgers

    fom = AffineBurgers(N=1500, nt=6, dt=2e-3, bdf2=bdf2, seed=3)
    rng = np.random.RandomState(r)
    xs = (np.arange(fom.Nh) + 0.5) / fom.Nh
    V, _ = np.linalg.qr(np.stack([np.sin((k + 1) * np.pi * xs) for k in range(r)], axis=1)
                        + 1e-3 * rng.standard_normal((fom.Nh, r)))
    mus = [dict(alpha=0.5 + 0.2 * i, beta=1.0 - 0.1 * i, delta=0.3 + 0.05 * i, omega=7.0 + i) for i in range(3)]
    d = fom.descriptor(mus)
    uN = rom_bdf_sweep(V, d["indptr"], d["indices"], d["mass"], d["terms"], d["term_coef"], d["tril"], d["rhs_terms"],
                       d["rhs_coef"], d["dt"], bdf2=bdf2).cpu().numpy()
    stats = _ctx().sweep_stats()
    for i, mu in enumerate(mus):
        ref, _ = oracle.rom_solve_nonlinear(fom, V, mu, solver=np.linalg.solve)
        rel = np.linalg.norm(uN[i].T - ref) / np.linalg.norm(ref)
        assert rel <= 1e-10, (i, rel)
        assert np.abs(ref).max() > 1e-4
    if r <= 80:
        assert stats["lu_fallbacks"] == 0 and stats["solves"] == 6 * len(mus), stats
