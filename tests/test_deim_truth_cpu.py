"""The premises of the greedy-against-the-truth tests, on the host (helpers in tests/deim_cases.py; the device half is
tests/test_deim_truth_gpu.py): the long-double certificate against 50-digit arithmetic, the oracle's picks inside it on
every case of the device's table, the condition on the inputs that keeps the 1e-9 rule a hundred times above float64
rounding, and the proof that the certificate is not vacuous: it rejects a pick swapped for the runner-up and the output of
two deliberately broken greedies, and the tie assertion rejects the higher index of a duplicated pair."""
import functools
import os

import mpmath
import numpy as np
import pytest

from tests import deim_cases as dc

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


# ---- host greedies: a right one with hooks, and two broken ones --------------------------------------------------------
def host_greedy(B, forced=None, fault=None):
    """float64 greedy in the device's form (residual columns, coefficients at the pivots).  ``forced``: {step: index} in
    place of the argmax.  ``fault``: "drop" leaves column k - 8 out of the residual of every step k >= 8 (past the first
    block); "stale" applies the coefficients of step 11 again at step 12."""
    N, m = B.shape
    forced = forced or {}
    R, idx, prev = [], [], []
    for k in range(m):
        t = B[:, k].copy()
        coef = []
        for j in range(k):
            if fault == "drop" and k >= 8 and j == k - 8:
                coef.append(0.0)
                continue
            c = prev[j] if (fault == "stale" and k == 12 and j < k - 1) else t[idx[j]] / R[j][idx[j]]
            coef.append(c)
            t -= R[j] * c
        prev = coef
        R.append(t)
        idx.append(forced.get(k, int(np.argmax(np.abs(t)))))
    return np.array(idx, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _oracle_case(case):
    """(basis, the oracle's picks and margins, their certificate), once per case."""
    from oracle import romtime_oracle as oracle

    B = dc.basis(*case)
    dofs, _, margin = oracle.deim_greedy(B)
    return B, dofs, margin, dc.certify(B, dofs)


# ---- the certificate itself --------------------------------------------------------------------------------------------
def test_certify_against_50_digits():
    """30 x 6: the residual columns of ``certify`` against the same walk in 50-digit arithmetic, entry by entry within
    4 eps_ld S_k (measured: 0.76), and the reported maximum, argmax and margin are those of the 50-digit residuals."""
    B, dofs, _, _ = _oracle_case(("random", 30, 6, 0))
    cert, R = dc.certify(B, dofs, keep_residuals=True)
    N, m = B.shape
    worst = 0.0
    with mpmath.workdps(50):
        cols = []
        for k in range(m):
            t = [mpmath.mpf(float(v)) for v in B[:, k]]
            for j in range(k):
                c = t[dofs[j]] / cols[j][dofs[j]]
                t = [ti - rj * c for ti, rj in zip(t, cols[j])]
            cols.append(t)
            ref = np.array([LD(mpmath.nstr(v, 25)) for v in t])
            err = float(np.abs(R[:, k] - ref).max() / (EPS_LD * cert.S[k]))
            worst = max(worst, err)
            a = [abs(v) for v in t]
            i = max(range(N), key=lambda q: (a[q], -q))
            second = max(a[q] for q in range(N) if q != i)
            assert i == cert.argmax[k] == dofs[k]
            assert abs(float(a[i]) - float(cert.top[k])) <= 4 * EPS_LD * float(cert.S[k])
            assert abs(float((a[i] - second) / a[i]) - cert.margin[k]) <= 1e-15
    print("DEIM-TRUTH certify vs 50 digits: worst |r - r_mp| / (eps_ld S_k) =", worst)
    assert worst <= 4.0, worst


def test_certify_needs_extended_precision(monkeypatch):
    from tests import svd_cases as sc

    monkeypatch.setattr(sc, "LD", np.float64)
    with pytest.raises(RuntimeError):
        dc.certify(np.eye(3), [0, 1, 2])


def test_families_are_what_they_say():
    for family, N, m in dc.DUP_CASES:
        B = dc.basis(family, N, m)
        low, high = dc.dup_partner(family, N)
        assert np.all(low < high) and sorted(np.r_[low, high].tolist()) == list(range(N))
        assert np.array_equal(np.abs(B[low]), np.abs(B[high]))
    low, high = dc.dup_partner("dup_half", 2050)
    assert (high - low)[:1024].tolist() == [512] * 1024 and low[-1] == 2048 and high[-1] == 2049
    N, m, seed = dc.SCALED_CASE[1:]
    e = dc.column_exponents(N, m, seed)
    assert e.min() >= -40 and e.max() <= 40 and len(set(e.tolist())) > 10
    assert np.array_equal(dc.basis("scaled", N, m, seed), dc.basis("random", N, m, seed) * 2.0 ** e)
    N, m, seed = dc.PERMUTED_CASE[1:]
    assert np.array_equal(dc.basis("permuted", N, m, seed), dc.basis("random", N, m, seed)[dc.row_permutation(N, m, seed)])
    S = dc.basis("sine", 1023, 64)
    assert np.abs(S.T @ S - np.eye(64)).max() < 1e-13           # the discrete sine modes are orthonormal
    assert np.array_equal(dc.basis("random", 513, 17), dc.basis("random", 513, 17))
    shapes = dc.RANDOM_SHAPES
    assert {m for _, m in shapes} == {1, 2, 7, 8, 9, 16, 17, 24, 63, 64, 65, 128, 129, 136, 137, 264, 265}
    assert {N for N, _ in shapes} >= {15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 2049}
    assert all(N >= m for N, m in shapes) and all((m, m) in shapes for m in (1, 2, 7, 8, 9, 16, 17))


# ---- the oracle inside the certificate, and the condition on the inputs ---------------------------------------------------
@pytest.mark.parametrize("case", dc.TABLE, ids=dc.label)
def test_oracle_passes_the_certificate_hostlogic(cpu_ops, case):
    """``ops.deim_greedy`` through the host stand-in (oracle.deim_greedy) on every case of the device's table: every pick
    accepted - in fact the true argmax, with a shortfall of exactly 0 (``near_mirror`` apart, whose ties of a few ulps
    float64 cannot see)."""
    from romtime_amd import ops

    B, dofs, margin, cert = _oracle_case(case)
    idx, PT_U, mg = ops.deim_greedy(ops.to_device(B))
    assert np.array_equal(idx.numpy(), dofs) and np.array_equal(PT_U.numpy(), B[dofs])
    assert dc.accepted(cert).all()
    if case[0] == "near_mirror":      # float64 rounding decides every step's tie of 1e-16: either row is right
        assert float((cert.shortfall / cert.top).max()) <= 1e-15 and cert.margin.max() < 1e-12
    else:
        assert np.array_equal(cert.argmax, dofs) and float(cert.shortfall.max()) == 0.0
    np.testing.assert_allclose(mg.numpy(), cert.margin, rtol=1e-6, atol=1e-11)
    dc.assert_certified(B, dofs, label=dc.label(case), cert=cert)


@pytest.mark.parametrize("case", dc.TABLE, ids=dc.label)
def test_inputs_keep_the_rule_above_rounding(case):
    """(k + 2) eps S_k / max|r_k| <= 1e-11 at every step: float64 rounding cannot move a pick by a hundredth of 1e-9."""
    cert = _oracle_case(case)[3]
    cond = dc.condition(cert)
    print("DEIM-TRUTH condition", dc.label(case), float(cond.max()), "S/top", float((cert.S / cert.top).max()))
    assert cond.max() <= dc.CONDITION, (dc.label(case), cond.max())


def test_exact_tie_and_invariance_preconditions():
    """``dup``: the truth is an exact tie at every step (margin 0, the lower index the argmax).  ``scaled`` and ``permuted``:
    the smallest margin exceeds 1e-6, on the family and on the ``random`` matrix it is made from."""
    for family, N, m in dc.DUP_CASES:
        B, dofs, margin, cert = _oracle_case((family, N, m, 0))
        assert np.all(cert.margin == 0.0) and np.all(margin == 0.0)
        dc.assert_exact_ties(family, N, dofs, margin)
    for case in (dc.SCALED_CASE, dc.PERMUTED_CASE):
        assert _oracle_case(case)[2].min() > 1e-6
        assert _oracle_case(("random",) + tuple(case[1:]))[2].min() > 1e-6


# ---- the certificate is not vacuous -------------------------------------------------------------------------------------
REJECT_CASE = ("random", 1023, 17, 0)


def _runner_up(B, dofs, k):
    _, R = dc.certify(B, dofs, keep_residuals=True)
    a = np.abs(R[:, k])
    a[dofs[k]] = -1
    return int(np.argmax(a))


def test_a_runner_up_pick_is_rejected():
    """One pick swapped for the runner-up at a step whose true margin is at least 1e-6 (the later steps a correct greedy
    on the swapped sequence): rejected at exactly that step, by ``certify`` and by the float64 multiplier bound."""
    B, dofs, _, cert = _oracle_case(REJECT_CASE)
    assert np.array_equal(host_greedy(B), dofs)
    ks = [k for k in range(3, len(dofs)) if 1e-6 <= cert.margin[k] <= 1e-2]
    assert ks, cert.margin
    k = ks[0]
    seq = host_greedy(B, forced={**{j: int(dofs[j]) for j in range(k)}, k: _runner_up(B, dofs, k)})
    assert np.array_equal(seq[:k], dofs[:k]) and seq[k] != dofs[k] and len(set(seq.tolist())) == len(seq)
    ok = dc.accepted(dc.certify(B, seq))
    assert not ok[k] and ok[:k].all()
    with pytest.raises(AssertionError):
        dc.assert_certified(B, seq, show=lambda *_: None)
    assert dc.multiplier_bound(B, dofs) <= 1.0 + dc.NEAR_TIE
    assert dc.multiplier_bound(B, seq) >= 1.0 + 0.5 * cert.margin[k]


@pytest.mark.parametrize("fault", ["drop", "stale"])
@pytest.mark.parametrize("case", [("random", 1023, 17, 0), ("random", 1025, 63, 0), ("sine", 1023, 64, 0)], ids=dc.label)
def test_a_broken_greedy_is_rejected(case, fault):
    """A greedy that leaves one earlier column out of every residual past the first block, and one that reuses the
    coefficients of the step before once: plausible indices (distinct on ``random``; on ``sine`` the dropped column lets a
    row come back, which the distinctness assertion catches first), and the certificate says no."""
    B = dc.basis(*case)
    seq = host_greedy(B, fault=fault)
    with pytest.raises(AssertionError):
        dc.assert_certified(B, seq, show=lambda *_: None)
    if case[0] != "random" and len(set(seq.tolist())) < len(seq):
        return
    assert len(set(seq.tolist())) == len(seq)
    cert = dc.certify(B, seq)
    ok = dc.accepted(cert)
    print("DEIM-TRUTH broken", fault, dc.label(case), "rejected steps", np.nonzero(~ok)[0][:6],
          "shortfall/top", float((cert.shortfall / cert.top).max()))
    assert not ok.all()
    assert ok[:8].all() if fault == "drop" else ok[:12].all()          # and not before the fault


@pytest.mark.parametrize("family,N,m", dc.DUP_CASES)
def test_the_higher_index_of_a_pair_is_rejected(family, N, m):
    """On ``dup`` the higher row of a pair has the same residual to the last bit, so ``certify`` accepts it: the separate
    tie assertion is what catches a tie resolved to the higher index (and a margin that is not exactly 0)."""
    B, dofs, margin, _ = _oracle_case((family, N, m, 0))
    low, high = dc.dup_partner(family, N)
    partner = dict(zip(low.tolist(), high.tolist()))
    seq = dofs.copy()
    seq[m // 2] = partner[int(dofs[m // 2])]
    assert dc.accepted(dc.certify(B, seq)).all()
    with pytest.raises(AssertionError):
        dc.assert_exact_ties(family, N, seq, margin)
    off = margin.copy()
    off[m // 2] = 2.0 ** -52
    with pytest.raises(AssertionError):
        dc.assert_exact_ties(family, N, dofs, off)


# ---- the float64 multiplier certificate and the size limit's fixture -----------------------------------------------------
def test_unpivoted_upper():
    rng = np.random.RandomState(3)
    A = rng.standard_normal((150, 150)) + 20.0 * np.eye(150)
    U = dc.unpivoted_upper(A, nb=64)
    np.testing.assert_allclose(U, dc.unpivoted_upper(A, nb=150), rtol=0, atol=1e-12)
    L = np.linalg.solve(U.T, A.T).T
    assert np.abs(np.triu(L, 1)).max() < 1e-13 and np.abs(np.diag(L) - 1.0).max() < 1e-13


def test_limit_fixture_is_of_this_basis():
    """tests/golden/deim_limit_1024.npz (tests/golden/make_deim_limit.py) is the record of ``dc.LIMIT``: the generator's
    parameters, a sample of the input, no near-tie, and the recorded picks pass the float64 multiplier certificate."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deim_limit_1024.npz"), allow_pickle=False)
    assert (str(g["family"]), int(g["N"]), int(g["m"]), int(g["seed"])) == tuple(dc.LIMIT.values())
    B = dc.basis(**dc.LIMIT)
    np.testing.assert_allclose(B[dc.LIMIT_PROBE], g["probe"], rtol=0, atol=dc.LIMIT_PROBE_ATOL)
    assert g["dofs"].shape == g["margin"].shape == (1024,) and len(set(g["dofs"].tolist())) == 1024
    assert g["margin"].min() > 1e-6
    assert dc.multiplier_bound(B, g["dofs"]) <= 1.0 + dc.NEAR_TIE
