"""The premises of the POD-against-the-truth tests, on the host (helpers in tests/svd_cases.py; the device half is
tests/test_pod_truth_gpu.py): the long-double SVD against 50-digit arithmetic, the stacked matrices' exact truth, dgesvd
inside the model bars on every case, a one-pass Gram POD far outside them, and ``pod.py``'s level logic through the
host stand-ins (``cpu_ops``) held to the same bars as the device."""
import mpmath
import numpy as np
import pytest

from oracle import romtime_oracle as oracle
from tests import svd_cases as sc

LD = np.longdouble
ALL_CASES = sc.SMALL_CASES + sc.STREAM_128 + sc.STREAM_136

def test_longdouble_svd_against_50_digits():
    """40 x 8 graded (s8 / s1 = 1e-8): singular values to 2e-18 s1 - a backward stable SVD in long double resolves them
    to a few eps_ld s1 (measured: 6.5e-19 s1) and no better, so the bound is relative to s1 - and vectors to
    1e-16 (s1 / s_i) / relgap of mpmath.svd_r."""
    rng = np.random.RandomState(5)
    X = (sc._orthonormal(rng, 40, 8) * 10.0 ** (-8.0 * np.arange(8) / 7.0)) @ sc._orthonormal(rng, 8, 8).T
    U, s, V = sc.longdouble_svd(X)
    with mpmath.workdps(50):
        Um, sm, Vm = mpmath.svd_r(mpmath.matrix(X.tolist()), full_matrices=False, compute_uv=True)
        to_ld = lambda M: np.array([[LD(mpmath.nstr(M[i, j], 25)) for j in range(M.cols)] for i in range(M.rows)])
        Ur, sr, Vr = to_ld(Um), to_ld(sm)[:, 0], to_ld(Vm).T
    assert np.all(np.abs(s - sr) <= 2e-18 * sr[0]), np.abs(s - sr) / sr[0]
    bar = 1e-16 * float(sr[0]) / (sr.astype(float) * sc.relgaps(sr))
    for mine, ref in ((U, Ur), (V, Vr)):
        sign = np.sign(np.sum(mine * ref, axis=0))
        err = np.sqrt(np.sum((mine * sign - ref) ** 2, axis=0)).astype(float)
        assert np.all(err <= bar), (err, bar)


@pytest.mark.parametrize("family,N0,n", [("graded", 600, 32), ("stairs", 1536, 128)])
def test_longdouble_svd_reconstructs(family, N0, n):
    X0 = sc.generator(family, N0, n, 1, 0)
    U, s, V = sc._generator_svd(family, N0, n, 1, 0, False)
    assert U.dtype == LD and U.shape == (N0, n) and np.all(np.diff(s) <= 0)
    assert np.abs((U * s) @ V.T - X0).max() < 1e-17 * s[0]
    assert np.abs(U.T @ U - np.eye(n)).max() < 1e-17
    assert np.abs(V.T @ V - np.eye(n)).max() < 1e-17


def test_longdouble_svd_needs_extended_precision(monkeypatch):
    monkeypatch.setattr(sc, "LD", np.float64)
    with pytest.raises(RuntimeError):
        sc.longdouble_svd(np.eye(3))


@pytest.mark.parametrize("p", [4, 64])
def test_stacked_truth_is_exact(p):
    """max |U S V^T - X| < 1e-17 s1 for the stacked matrix, with U and S lifted from the generator's truth."""
    case = sc.Case("graded", 1536, 128, p, num=64)
    t = sc.truth(case)
    X, blocks = sc.snapshots(case)
    assert X.shape == (1536 * p, 128)
    U = sc.lift(t.U0, blocks)
    W = t.V * t.s
    # the long-double product has no BLAS behind it: every row at p = 4; at p = 64 a different random 192 of the 1536
    # rows of each block (12288 rows in all), so that no block and no row position is left out by design
    if p == 4:
        rows = np.arange(X.shape[0])
    else:
        pick = np.random.RandomState(p)
        rows = np.concatenate([j * 1536 + pick.choice(1536, size=192, replace=False) for j in range(p)])
    worst = np.abs(U[rows] @ W.T - X[rows]).max()
    print("POD-TRUTH stacked", p, float(worst / t.s[0]))
    assert worst < 1e-17 * t.s[0], float(worst)
    # every block is a different permutation: a wrong row index changes the matrix
    assert len({tuple(perm[:8]) for perm, _ in blocks}) == p


def _dgesvd_result(case, X):
    Q, s, energy, VT = oracle.orth(X, return_VT=True, **case.kwargs)
    return Q, s, energy, VT, None


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.label)
def test_dgesvd_stays_inside_the_bars(case):
    """oracle.orth (dgesvd) on the matrix of every case, the stacked ones included: below twice the model for the columns
    of Q and VT, within the singular-value bar (the levels' one, the stricter).  Measured: columns 0.09 ... 1.4, singular
    values 1.6 ... 7.3, and 11.3 on ``scaled_columns`` stacked 64 times (the float64 column norms of 98304 rows).  The
    ratio depends on the draw (``family_cases`` says how the draws were taken), and the 65-mode block of ``stairs`` is
    the second one: as the first, dgesvd sat at 2.1 ... 4.6 there."""
    X, blocks = sc.snapshots(case)
    m = sc.measure(case, "deflate", _dgesvd_result(case, X), blocks)   # the levels' bar: the stricter one
    print("POD-TRUTH dgesvd", m)
    assert m["r"] == m["r_true"]
    assert m["col"] < sc.DGESVD_BAR and m["vt"] < sc.DGESVD_BAR and m.get("span4", 0.0) < sc.DGESVD_BAR, m
    assert m["s"] <= sc.F_S and m["energy"] <= 1e-10, m


def _one_pass_gram(X, r):
    lam, W = np.linalg.eigh(X.T @ X)
    lam, W = lam[::-1], W[:, ::-1]
    s = np.sqrt(np.clip(lam, 0.0, None))
    return X @ (W[:, :r] / s[:r]), s, np.cumsum(s * s) / np.sum(s * s), W[:, :r].T.copy(), None


def test_one_pass_gram_pod_is_told_apart():
    """eigh(X^T X) and a back-projection on ``graded``: more than ten times the model at some kept mode."""
    case = sc.Case("graded", 1536, 128, 1, num=64)
    X, blocks = sc.snapshots(case)
    m = sc.measure(case, "one_pass", _one_pass_gram(X, 64), blocks)
    print("POD-TRUTH one-pass NumPy", m)
    assert max(m["col"], m["vt"]) > 10.0 * sc.HOST_FACTORS[0], m


@pytest.mark.parametrize("case", sc.SMALL_CASES, ids=lambda c: c.label)
def test_level_logic_meets_the_bars_hostlogic(cpu_ops, case):
    """pod.py's routes with the oracle's arithmetic in place of the kernels: the same check as on the device."""
    sc.check_pod_against_truth(case, ("auto", "deflate", "two_pass"), order="C", factors=sc.HOST_FACTORS)
    sc.check_pod_against_truth(case, ("auto",), order="F", factors=sc.HOST_FACTORS)


@pytest.mark.parametrize("N0,n", [(600, 32), (1536, 64)])
def test_forced_one_pass_fails_the_bar_hostlogic(cpu_ops, N0, n):
    """orth(..., passes=1) on ``graded`` with num = n / 2 misses the column bar by more than ten times."""
    case = sc.Case("graded", N0, n, 1, num=n // 2)
    X, blocks = sc.snapshots(case)
    m = sc.measure(case, "one_pass", sc.run_route(case, "one_pass", X), blocks)
    print("POD-TRUTH forced one pass", m)
    assert max(m["col"], m["vt"]) > 10.0 * sc.HOST_FACTORS[0], m       # the column bar holds Q's columns and VT's
    with pytest.raises(AssertionError):
        sc.assert_within(m, case, "one_pass", sc.HOST_FACTORS)
