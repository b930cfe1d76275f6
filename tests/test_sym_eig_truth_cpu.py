"""The premises of tests/test_sym_eig_truth_gpu.py (the tridiagonal eigensolver of csrc/symeig.hip against exact and
extended-precision truth), as far as a host without a GPU can prove them.  Helpers: tests/eig_cases.py.

* The exact family is exact: P^2 G is the integer matrix (P I - 2 v v^T) D (P I - 2 v v^T) in Python integers,
  (P I - 2 v v^T)^2 = P^2 I, G times P^2 gives those integers back in float64, with ``fractions`` H D H = G entry by
  entry on the small sizes; G is exactly symmetric and a float64 Householder reduction of it leaves no zero off-diagonal
  and no zero tau (the solver sees n - 2 real reflectors).
* LAPACK's figures (``np.linalg.eigh``, the reference's library) on every matrix are recorded in
  tests/golden/eig_lapack.json; those of the sizes up to 257 are recomputed and printed here.  Measured: eigenvalues
  0.001 ... 0.42 n eps lam_1, residuals 0.002 ... 0.52, gap-scaled orthogonality 0.000 ... 0.25, gap-scaled distance from
  the exact eigenvectors 0.001 ... 0.47 (all below 1: every such bar of the device is 4), norms 0.8 ... 9.4 eps (the
  device's bar: four times that, at most 20).
* The measuring functions tell a broken answer apart.  Starting from LAPACK's answer: one vector moved by 1e-11
  towards its neighbour fails ``res``, ``orth`` and ``vec`` (a wrong vector is a wrong residual: the three figures are
  one statement there) while ``lam`` and ``norm`` pass; one eigenvalue moved by 100 n eps lam_1 fails ``lam`` and that
  column's ``res`` (the residual is taken with the returned eigenvalue) while ``norm``, ``orth`` and ``vec`` pass; one
  reflector block's cross products zeroed in the NumPy restatement of the blocked back-transformation fails ``res``
  and ``vec`` while ``lam`` passes.  The same restatement equals reflector-by-reflector application for every
  (n - 2) % 4, four and two at a time.
"""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import eig_cases as ec
from tests import jacobi_cases as jc

SMALL = tuple(n for n in ec.EXACT_SIZES if n <= 130)
_ids = dict(ids=lambda c: str(c))


# ---- the exact family -----------------------------------------------------------------------------------------------------
def test_fill_reaches_a_power_of_two_at_every_size_but_three():
    """Every size of the tests but n = 3 has a power of two P >= n with P - n = 3 a + 8 b + 15 c; only n = 6 needs a
    +-4; n = 3 has none (and cannot: see eig_cases)."""
    for n in ec.EXACT_SIZES:
        found = ec.fill(n)
        if n == 3:
            assert found is None
            continue
        P, (a, b, c) = found
        assert P >= n and P & (P - 1) == 0 and n + 3 * a + 8 * b + 15 * c == P and a + b + c <= n - 1
        assert c == (1 if n == 6 else 0), (n, found)
    sums = {x * x + y * y + z * z for x in range(1, 64) for y in range(1, 64) for z in range(1, 64)}
    assert not any(1 << m in sums for m in range(1, 13))


@pytest.mark.parametrize("spectrum,n", ec.exact_cases(SMALL), **_ids)
def test_exact_family_is_exact(spectrum, n):
    """Python integers: P^2 G = (P I - 2 v v^T) D (P I - 2 v v^T) entry by entry, (P I - 2 v v^T)^2 = P^2 I, and the
    float64 matrix holds exactly those integers over P^2.  n <= 10 also in ``fractions``: H D H = G and H^T H = I."""
    ex = ec.exact(spectrum, n)
    P, v, D = ex.P, [int(x) for x in ex.v], [int(x) for x in ex.D]
    K = np.array([[(P if i == j else 0) - 2 * v[i] * v[j] for j in range(n)] for i in range(n)], dtype=object)
    Dm = np.array([[D[i] if i == j else 0 for j in range(n)] for i in range(n)], dtype=object)
    M = K.dot(Dm).dot(K)
    assert all(int(M[i, j]) == int(ex.M[i, j]) for i in range(n) for j in range(n))
    KK = K.dot(K)
    assert all(int(KK[i, j]) == (P * P if i == j else 0) for i in range(n) for j in range(n))
    assert np.array_equal(ex.G, ex.G.T)
    if ex.factor == 1:
        assert P & (P - 1) == 0
        back = ex.G * float(P * P)                       # a power of two: exact
    else:
        assert n == 3 and ex.factor == P * P == 9
        back = ex.G
    assert np.array_equal(back, ex.M.astype(np.float64)) and np.all(back == np.rint(back))
    assert all(int(back[i, j]) == int(M[i, j]) for i in range(n) for j in range(n))
    assert sorted(D, reverse=True) == [int(t) // ex.factor for t in ex.truth] and len(set(D)) == n
    if n <= 10:
        H = [[Fraction(int(i == j)) - Fraction(2 * v[i] * v[j], P) for j in range(n)] for i in range(n)]
        for i in range(n):
            for j in range(n):
                assert sum(H[k][i] * H[k][j] for k in range(n)) == int(i == j)
                assert sum(H[i][k] * D[k] * H[k][j] for k in range(n)) * ex.factor == Fraction(ex.G[i, j])
        Hl = ex.vectors(np.arange(n))
        for q in range(n):
            for i in range(n):
                want = H[i][int(ex.order[q])]
                if ex.factor == 1:
                    assert Fraction(float(Hl[i, q])) == want          # exact in float64, too
                else:
                    assert abs(Fraction(float(Hl[i, q])) - want) <= Fraction(1, 1 << 52)


@pytest.mark.parametrize("n", [4, 130, 2047, 2048])
def test_exact_family_at_the_large_sizes(n):
    """The same bound and symmetry at the sizes that are too large for Python integers entry by entry: the int64
    products are below 2^53 (asserted by the builder), G is symmetric, G v-products reproduce D: G h_i = D_i h_i exactly
    in long double on a few columns (every operand a dyadic rational of few bits)."""
    for spectrum in ec.SPECTRA:
        ex = ec.exact(spectrum, n)
        assert int(np.abs(ex.M).max()) < (1 << 53) and np.array_equal(ex.G, ex.G.T)
        cols = np.array([0, 1, n // 2, n - 1])
        Hc = ex.vectors(cols)
        R = ex.G.astype(jc.LD) @ Hc - Hc * ex.truth[cols]
        assert float(np.abs(R).max()) == 0.0
        assert float(np.abs(ex.apply(Hc) - Hc * ex.truth[cols]).max()) == 0.0
        assert float(np.abs(Hc.T @ Hc - np.eye(len(cols))).max()) == 0.0


@pytest.mark.parametrize("spectrum,n", ec.exact_cases(ec.CPU_SIZES + (512, 513)) + [("spread", 1025)], **_ids)
def test_exact_family_is_irreducible(spectrum, n):
    """A float64 Householder reduction from row 0 (the recurrences of the kernel) leaves no zero off-diagonal and no
    zero tau: the solver sees n - 2 real reflectors, and its tridiagonal matrix has the eigenvalues of G."""
    ex = ec.exact(spectrum, n)
    d, e, V, tau = ec.tridiagonalise(ex.G)
    assert np.all(e[:n - 1] != 0.0) and np.all(tau[:n - 2] != 0.0)
    assert np.all(V[np.arange(n - 2), np.arange(1, n - 1)] == 1.0)
    if n <= 130:
        T = np.diag(d) + np.diag(e[:n - 1], 1) + np.diag(e[:n - 1], -1)
        err = np.abs(np.linalg.eigvalsh(T)[::-1] - ex.truth.astype(np.float64)).max()
        assert err <= 20 * n * ec.EPS * float(ex.truth[0])


# ---- LAPACK's figures -----------------------------------------------------------------------------------------------------
SANITY = dict(lam=ec.BAR_CAP / ec.BAR_FACTOR, res=ec.BAR_CAP / ec.BAR_FACTOR, orth=ec.BAR_CAP / ec.BAR_FACTOR,
              vec=ec.BAR_CAP / ec.BAR_FACTOR, norm=ec.BAR_CAP)     # norm is in units of eps, not n eps


def test_record_holds_every_case_within_the_sanity_bounds():
    """Every case of the GPU test has LAPACK's figures on record, each below the cap over the factor (the bars then
    mean something); the norms, in units of eps, below the cap."""
    for label in ec.all_labels():
        ref = ec.lapack_reference(label)
        print(ec.format_line("EIG-LAPACK-RECORD", label, ref, ref))
        assert set(ref) == set(ec.FIGURES) - (set() if label.startswith("exact") else {"vec"}), label
        for key, value in ref.items():
            assert 0.0 <= value <= SANITY[key], (label, key, value)


CPU_LABELS = [ec.exact_label(s, n) for s, n in ec.exact_cases(ec.CPU_SIZES)] + \
             [ec.recorded_label(k, n) for k, n in jc.cases(jc.CPU_SIZES + (257,))]


@pytest.mark.parametrize("label", CPU_LABELS)
def test_lapack_figures_recomputed(label):
    """np.linalg.eigh on the matrix of the case, measured as the device will be, next to the record: a library that
    rounds differently moves a figure by about two, so each is held to twice the larger of 1 and the other."""
    got, rec = ec.compute_lapack_reference(label), ec.lapack_reference(label)
    print(ec.format_line("EIG-LAPACK", label, got, rec))
    for key in rec:
        assert got[key] <= SANITY[key], (key, got[key])
        assert got[key] <= 2 * max(1.0, rec[key]) and rec[key] <= 2 * max(1.0, got[key]), (key, got[key], rec[key])
    if label.startswith("exact"):
        _, spectrum, n = label.split("-")
        ex = ec.exact(spectrum, int(n))
        k = ec.separated_prefix(ex.truth)
        if k:
            # information, no bar: LAPACK's own distance where pod_rules.separated holds is 5.7e-16 ... 2.84e-12 (the
            # largest on ``spread`` at n = 130, k = n, smallest gap 1.01e-4 lam_1: eps / gap alone is 2.2e-12)
            print(f"EIG-LAPACK {label} separated k={k}: worst distance {got['vec_abs'][:k].max():.2e}")


# ---- broken answers ---------------------------------------------------------------------------------------------------------
def _verdict(ex, lam, W):
    n = ex.n
    got = ec.measure(ex.truth, np.arange(n), lam, np.arange(n), W, ex.apply, H=ex.vectors(np.arange(n)))
    ref = ec.lapack_reference(ec.exact_label(ex.spectrum, n))
    return {key: got[key] <= ec.bar(ref[key]) for key in ec.FIGURES}, got


def test_a_vector_moved_towards_its_neighbour_is_rejected():
    """w_0 + 1e-11 w_1 on ``graded`` at n = 66 (gap 0.19 lam_1): 1e-11 x 0.19 / (66 eps) = 130 on ``res``, ``orth`` and
    ``vec``; ``lam`` and ``norm`` do not move."""
    ex = ec.exact("graded", 66)
    lam, W = ec.lapack_eigh(ex.G)
    ok, got = _verdict(ex, lam, W)
    assert all(ok.values()), got
    Wb = W.copy()
    Wb[:, 0] += 1e-11 * W[:, 1]
    ok, got = _verdict(ex, lam, Wb)
    print("EIG-BROKEN vector", {k: round(got[k], 3) for k in ec.FIGURES})
    assert ok == dict(lam=True, res=False, norm=True, orth=False, vec=False), (ok, got)
    assert got["vec_abs"][0] > ec.SEPARATED_BOUND


def test_an_eigenvalue_moved_is_rejected():
    """lam_5 + 100 n eps lam_1: ``lam`` and the residual taken with it; the vectors' own figures do not move."""
    ex = ec.exact("spread", 66)
    lam, W = ec.lapack_eigh(ex.G)
    lb = lam.copy()
    lb[5] += 100 * ex.n * ec.EPS * float(ex.truth[0])
    ok, got = _verdict(ex, lb, W)
    print("EIG-BROKEN eigenvalue", {k: round(got[k], 3) for k in ec.FIGURES})
    assert ok == dict(lam=False, res=False, norm=True, orth=True, vec=True), (ok, got)
    assert 99 <= got["lam"] <= 101


@pytest.mark.parametrize("n", [63, 64, 65, 66])
def test_blocked_back_transformation_and_a_block_without_cross_products(n):
    """(n - 2) % 4 = 1, 2, 3, 0.  The restated reduction, LAPACK on its tridiagonal matrix and the restated blocked
    back-transformation meet every bar; four and two reflectors at a time equal one at a time to rounding; the last,
    partial block with its cross products zeroed fails ``res`` and ``vec`` - but for (n - 2) % 4 = 1, where that block
    holds one reflector and has no cross product in use: there nothing changes, and the first block is zeroed."""
    ex = ec.exact("spread", n)
    d, e, V, tau = ec.tridiagonalise(ex.G)
    T = np.diag(d) + np.diag(e[:n - 1], 1) + np.diag(e[:n - 1], -1)
    lam, Z = ec.lapack_eigh(T)
    one = ec.back_transform(V, tau, Z, rb=1)
    four = ec.back_transform(V, tau, Z, rb=4)
    two = ec.back_transform(V, tau, Z, rb=2)
    assert np.abs(four - one).max() <= 4 * n * ec.EPS and np.abs(two - one).max() <= 4 * n * ec.EPS
    for W in (one, two, four):
        ok, got = _verdict(ex, lam, W)
        assert all(ok.values()), got
    last = (n - 2 + 3) // 4 - 1
    broken = ec.back_transform(V, tau, Z, rb=4, zero_block=last)
    if (n - 2) % 4 == 1:
        assert np.array_equal(broken, four)
        broken = ec.back_transform(V, tau, Z, rb=4, zero_block=0)
    ok, got = _verdict(ex, lam, broken)
    print(f"EIG-BROKEN block n={n}", {k: round(got[k], 3) for k in ec.FIGURES})
    assert ok["lam"] and not ok["res"] and not ok["vec"], (ok, got)
    # the pair form reads the first or the last of a block's six products: zeroing a pair's product is caught as well
    pair = ec.back_transform(V, tau, Z, rb=2, zero_block=0)
    ok, got = _verdict(ex, lam, pair)
    assert ok["lam"] and not ok["res"] and not ok["vec"], (ok, got)


def test_golden_record_is_committed_next_to_its_writer():
    here = os.path.dirname(os.path.abspath(ec.GOLDEN))
    assert os.path.exists(ec.GOLDEN) and os.path.exists(os.path.join(here, "make_eig_lapack.py"))
