"""The premises of tests/test_reduced_solves_gpu.py, proved on the host for every size that module uses: the exact
family's answer is exact (so a device answer that differs in one bit is wrong), every pivot is strictly unique, the
pivot sequence visits every wave of the kernel's thread mapping, the ladder's inputs take the routes the GPU test
asserts with a margin, and the 50-digit reference is what it says."""
import mpmath
import numpy as np
import pytest

from tests import guarded as gd
from tests import solve_cases as sc

EXACT_SIZES = sorted(set(sc.LU_SIZES + sc.FALLBACK_SIZES))


def _waves_visited(piv, r):
    """For both thread mappings of lu_solve_lds (256 threads: the LU kernels, 512: the tracked solve's fallback):
    the pivot rows' waves must be all the waves that own a row, wherever there is more than one."""
    for threads in (sc.SOLVE_THREADS, sc.NS_THREADS):
        if threads == sc.NS_THREADS and r > 80:
            continue
        owned = set(sc.lu_waves(np.arange(r), r, threads).tolist())
        if len(owned) > 1:
            assert set(sc.lu_waves(piv, r, threads).tolist()) == owned, (r, threads)
            # ... and the winner changes wave from one column to the next: the merge is not a constant
            assert np.count_nonzero(np.diff(sc.lu_waves(piv, r, threads))) >= 1


@pytest.mark.parametrize("r,tiny_last", [(r, False) for r in EXACT_SIZES] + [(r, True) for r in sc.FALLBACK_SIZES])
def test_exact_family_is_exact_with_unique_pivots_in_every_wave(r, tiny_last):
    for seed in range(3):                                  # the GPU tests draw one system per batch entry: seeds r + 1000 i
        K, b, x = sc.exact_lu_system(r, np.random.RandomState(r + 1000 * seed), tiny_last)
        assert gd.bits_equal(K @ x, b)
        xh, piv, margins = sc.retiring_lu_solve(K, b)
        assert gd.bits_equal(xh, x), gd.mismatch(xh, x)
        assert gd.bits_equal(np.linalg.solve(K, b), x)
        assert all(best > second for best, second in margins)
        assert sorted(piv.tolist()) == list(range(r))
        _waves_visited(piv, r)
        if tiny_last and r > 1:
            assert np.linalg.cond(K) > 2.0 ** 55
            last = K[:, r - 1]
            assert np.count_nonzero(last) == 1 and np.abs(last).max() == 2.0 ** -60


@pytest.mark.parametrize("r", sc.WILKINSON_SIZES)
def test_wilkinson_is_exact_with_growth(r):
    """Growth 2^(r-1) in the last column with every intermediate an integer float64 holds.  Every column ties, but this
    matrix does not test the order of equals: whichever tied row is taken, the arithmetic stays exact (the tied exact
    family below does)."""
    K, b, x = sc.wilkinson_system(r, np.random.RandomState(r))
    xh, piv, margins = sc.retiring_lu_solve(K, b)
    assert gd.bits_equal(xh, x) and gd.bits_equal(np.linalg.solve(K, b), x)
    assert piv.tolist() == list(range(r))                  # no exchanges ...
    assert all(best == second == 1.0 for best, second in margins[:-1])   # ... and every column but the last a tie
    assert len(set(sc.lu_waves(piv, r).tolist())) > 1
    assert 2.0 ** (r - 1) < 2.0 ** 53


TIED_CASES = [(r, False, sc.SOLVE_THREADS) for r in sc.TIED_SIZES] + [(r, True, sc.NS_THREADS) for r in sc.FALLBACK_SIZES]


@pytest.mark.parametrize("r,tiny_last,threads", TIED_CASES)
def test_tied_exact_family_is_exact_only_under_the_documented_order(r, tiny_last, threads):
    """Two equal candidates in column 0, in the first and the last wave that owns a row (256 threads: the LU kernels;
    512 with tiny_last: the tracked solve's fallback).  Lowest row first - the kernel's order and LAPACK's - gives x bit
    for bit with unique pivots from column 1 on; the other order of equals takes the last row and loses the exact
    answer.  Plain exact systems and Wilkinson's matrix cannot tell the two orders apart: there any choice stays exact."""
    for seed in range(3):
        K, b, x = sc.exact_lu_system(r, np.random.RandomState(r + 1000 * seed), tiny_last, tied=True)
        assert gd.bits_equal(K @ x, b)
        xh, piv, margins = sc.retiring_lu_solve(K, b)
        assert gd.bits_equal(xh, x) and gd.bits_equal(np.linalg.solve(K, b), x)
        assert piv[0] == 0 and margins[0][0] == margins[0][1] == abs(K[0, 0]) == abs(K[r - 1, 0])
        assert all(best > second for best, second in margins[1:])
        assert sc.lu_waves(r - 1, r, threads) > sc.lu_waves(0, r, threads)
        _waves_visited(piv, r)
        xo, pivo, _ = sc.retiring_lu_solve(K, b, other_tie_order=True, threads=threads)
        assert pivo[0] == r - 1 and not gd.bits_equal(xo, x)
    K, b, x = sc.wilkinson_system(20, np.random.RandomState(20))
    assert gd.bits_equal(sc.retiring_lu_solve(K, b, other_tie_order=True)[0], x)     # blind to the order


def test_multi_right_hand_sides_are_exact():
    """rt_dense_solve_multi's cases: K X for small-integer X is exact, so X is the answer bit for bit."""
    for r in sc.LU_SIZES:
        rng = np.random.RandomState(r)
        K, _, _ = sc.exact_lu_system(r, rng)
        X = sc.small_integers(rng, (r, 7))
        B = K @ X
        assert gd.bits_equal(np.linalg.solve(K, B), X)
        assert np.abs(B * 4 - np.round(B * 4)).max() == 0.0 and np.abs(B).max() < 2.0 ** 20


@pytest.mark.parametrize("r", sc.LADDER_SIZES)
def test_ladder_inputs_take_their_routes_with_a_margin(r):
    """The restatement of newton_solve_kernel's decisions on the ladder's own inputs: every rung takes the route the
    GPU test asserts, and not narrowly -
    * refinement alone: at most 4 steps, where 6 would change the route;
    * refinement that then refreshes: at least 7 steps (two past NS_REFRESH_AFTER = 5) - this is the margin that chose
      REFRESH_D = 2e-2: at 1e-2 the model takes 6 steps at every size, at 1.5e-2 six or seven;
    * Newton-Schulz from the carried inverse: |I - K X|_F <= 0.6 against the restart test at 0.7;
    * restart: |I - K X|_F >= 1.0."""
    calls = sc.ladder_calls(r)
    K0, b0, _ = calls[0]
    B = K0.shape[0]
    X0 = []
    for s in range(B):
        m = sc.tracked_model(K0[s], b0[s])
        assert m["route"] == "first" and m["restarts"] == 0 and m["newton_iterations"] > 0
        X0.append(m["X"])
    for K, b, route in calls[1:]:
        for s in range(B):
            m = sc.tracked_model(K[s], b[s], X0[s])
            assert m["route"] == route, (route, s, m["route"], m["refine_steps"], m["ns_res"][:2])
            if route == "refine":
                assert m["refine_steps"] <= 4 and m["newton_iterations"] == 0
            elif route == "refine_refresh":
                assert m["refine_steps"] >= 7 and m["restarts"] == 0
            elif route == "newton":
                assert m["ns_res"][0] <= 0.6 and m["restarts"] == 0 and m["refine_steps"] is None
            else:
                assert m["ns_res"][0] >= 1.0 and m["restarts"] == 1


@pytest.mark.parametrize("r", sc.FALLBACK_SIZES)
def test_tiny_last_defeats_newton_schulz_and_a_regular_matrix_recovers(r):
    K, b, _ = sc.exact_lu_system(r, np.random.RandomState(r), tiny_last=True)
    m = sc.tracked_model(K, b)
    assert m["route"] == "fallback" and m["newton_iterations"] == sc.NS_MAX_ITER and m["ns_res"][-1] > 0.5
    assert not m["X"].any()
    K0, _, rng = sc.ladder_systems(r, 1)
    again = sc.tracked_model(K0[0], rng.standard_normal(r), m["X"])      # from the zeroed inverse: |I - 0| = sqrt(r) >= 0.7
    assert again["route"] == "restart" and again["lu_fallbacks"] == 0


@pytest.mark.parametrize("r", sc.LADDER_SIZES)
def test_scaled_permutation_restatement_agrees_with_the_dense_model(r):
    """The entry-by-entry restatement and the dense NumPy model take the same number of iterations and agree to
    rounding; the nonzeros cover every full tile; no tested residual is within a factor ten of the threshold."""
    for i in range(4):
        K, b, s = sc.scaled_permutation_system(r, np.random.RandomState(r + 1000 * i))
        x, X, n, res = sc.scaled_permutation_first_call(K, b)
        m = sc.tracked_model(K, b)
        assert m["route"] == "first" and m["newton_iterations"] == n
        assert np.abs(X - m["X"]).max() <= 4 * sc.EPS and np.abs(x - np.linalg.solve(K, b)).max() <= 8 * sc.EPS * np.abs(x).max()
        assert all(v < 1e-7 or v > 1e-5 for v in res) and res[-1] < 1e-7
        tiles = {(int(j) // 16, c // 16) for c, j in enumerate(s)}
        assert all((a, c) in tiles for a in range(r // 16) for c in range(r // 16))
        assert np.count_nonzero(X) == r and np.array_equal(np.nonzero(X.T), np.nonzero(K))


def test_reference_solve_is_a_50_digit_solution():
    """Against mpmath's own LU at a size where that is affordable, and by its residual in 60 digits at cond 1e10."""
    rng = np.random.RandomState(0)
    K, b = sc.conditioned_system(12, 10, rng)
    x = sc.reference_solve(K, b)
    with mpmath.workdps(50):
        xm = mpmath.lu_solve(mpmath.matrix(K.tolist()), mpmath.matrix(b.tolist()))
        want = np.array([float(v) for v in xm])
    assert gd.bits_equal(x, want), gd.mismatch(x, want)
    K, b = sc.conditioned_system(40, 10, rng)
    x = sc.reference_solve(K, b)
    fwd, bwd = sc.solve_errors(K, b, x, x)
    assert bwd <= 2.0 ** -52                                # a correctly rounded solution: backward error of one rounding
    fl, bl = sc.solve_errors(K, b, np.linalg.solve(K, b), x)
    assert 1e-12 < fl < 1e-4 and bl < 40 * sc.EPS           # LAPACK: forward error ~ cond eps, backward stable
    assert sc.error_ratios(K, b, np.linalg.solve(K, b), x)[0] == 1.0


def test_synthetic_terms_are_reproducible():
    a = sc.synthetic_hrom_terms(np.random.RandomState(5), 6, 4, 2, 3, [(3, "spd"), (4, "general")], 5, 3)
    b = sc.synthetic_hrom_terms(np.random.RandomState(5), 6, 4, 2, 3, [(3, "spd"), (4, "general")], 5, 3)
    assert all(np.array_equal(x["F"], y["F"]) for x, y in zip([a[0]] + a[1], [b[0]] + b[1]))
    assert a[0]["basis_rom"].shape == (36, 3) and a[2]["W"].shape == (5, 6) and a[3][0]["F"].shape == (4, 2, 3)
