"""The one-step defect measure of the sweep truth tests, proved on the host (tests/sweep_cases.py).

* Cross-check: the long-double step, iterated as a loop of its own with a long-double Gaussian elimination, agrees with
  the oracle's loops (oracle.hrom_solve / oracle.rom_solve_nonlinear) to 1e-12 - the restatement of the header is the
  reference's loop, with and without every optional term.
* Conditions: every case of tests/test_sweep_truth_gpu.py (same generator calls) is well conditioned, has a trajectory
  worth measuring, and NumPy's own ratio stays below 4 at every step.
* Planted faults: each fault a sweep kernel could have, applied to the float64 step that plays the device, pushes the
  worst ratio of its case to at least 1000 - ten times the cap on F.  The faults that cannot show under BDF1 are shown
  to be inert there, so the BDF1 cases are known to test the rest."""
import numpy as np
import pytest

from oracle import romtime_oracle as oracle
from tests import sweep_cases as sc

SCHEMES = [pytest.param(False, id="bdf1"), pytest.param(True, id="bdf2")]
TABLES = [("hrom", sc.H_CASES), ("hrom", sc.H_GRAPH_CASES), ("hrom", sc.H_GMRES_CASES), ("hrom", sc.H_ZERO_CASES),
          ("direct", sc.D_CASES), ("direct", sc.D_GMRES_CASES), ("direct", sc.D_ZERO_CASES)]
ALL_CASES = [pytest.param(kind, name, kw, id=f"{kind}-{name}") for kind, table in TABLES for name, kw in table.items()]


@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("kind,name,kw", ALL_CASES)
def test_case_conditions(kind, name, kw, bdf2):
    c = sc.build(kind, name, kw, bdf2)
    conds = []
    uN = sc.play(c, conds=conds)
    assert len(conds) == c.n_mu * c.nt and max(conds) <= 100.0, max(conds)
    if kw.get("n_rhs", 1) == 0:
        assert not uN.any()                                  # no source, zero initial condition: the zero trajectory
        return
    assert np.abs(uN).max(axis=(1, 2)).min() >= 1e-4
    m = sc.measure(c, uN)
    assert m.ratio_numpy.max() <= 4.0, m.ratio_numpy.max()
    np.testing.assert_array_equal(m.ratio, m.ratio_numpy)    # the player IS the float64 step of the measure


H_CROSS = ["size_r16", "nl_none_r11", "nl_no_C_r11", "nl_no_S_r11", "nl_bare_r11", "lin_none_r11", "mass_only_r11",
           "rhs_two_r11", "size_r2"]
D_CROSS = ["terms_12", "tril_none", "terms_0", "terms_none", "rhs_three", "wide_r7", "empty_rows_r7"]


@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name", H_CROSS)
def test_longdouble_loop_is_the_oracles_hyper_reduced_loop(name, bdf2):
    c = sc.build("hrom", name, sc.H_CASES[name], bdf2)
    got = sc.play_longdouble(c).astype(np.float64)
    mass, lin, nl, rhs = c.terms
    for b in range(c.n_mu):
        ref = oracle.hrom_solve(mass, lin, nl, rhs, b, c.r, c.nt, c.dt, c.bdf2)
        assert np.linalg.norm(got[b].T - ref) <= 1e-12 * np.linalg.norm(ref), b
    np.testing.assert_array_equal(c.Z, np.vstack([t["basis_rom"].T for t in [mass] + lin + ([nl] if nl else [])]))


@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("name", D_CROSS)
def test_longdouble_loop_is_the_oracles_direct_loop(name, bdf2):
    c = sc.build("direct", name, sc.D_CASES[name], bdf2)
    got = sc.play_longdouble(c).astype(np.float64)
    for b in range(c.n_mu):
        ref, _ = oracle.rom_solve_nonlinear(sc.DirectFom(c, b), c.V, None, solver=np.linalg.solve)
        assert np.linalg.norm(got[b].T - ref) <= 1e-12 * np.linalg.norm(ref), b


def test_direct_models_are_what_the_issue_asks_for():
    """Mass 4 on the diagonal and dominant by rows and by columns, every row with entries has its diagonal, the rows
    of ``empty_rows`` stay empty, V orthonormal."""
    for name in ("wide_r7", "empty_rows_r7", "ragged_band_r7", "mixed_r7", "N_3_r1"):
        c = sc.build("direct", name, sc.D_CASES[name], True)
        M = sc.DirectFom(c, 0).assemble_mass(None, 0.0).toarray()
        rows = np.diff(c.indptr)
        assert (np.diag(M)[rows > 0] == 4.0).all() and ((rows == 0).sum() == (6 if name.startswith("empty") else 0))
        off = np.abs(M - np.diag(np.diag(M)))
        assert off.sum(axis=1).max() <= 0.5 and off.sum(axis=0).max() <= 0.5
        np.testing.assert_allclose(c.V.T @ c.V, np.eye(c.r), atol=1e-13)


def test_gauss_solve_in_long_double():
    rng = np.random.RandomState(0)
    K, x = rng.standard_normal((30, 30)), rng.standard_normal(30)
    K[0, 0] = 0.0                                            # a pivot search that must move
    got = sc.gauss_solve(K.astype(sc.LD), (K.astype(sc.LD) @ x.astype(sc.LD)))
    assert np.abs(got - x).max() <= 1e-15


# ---- planted faults ----------------------------------------------------------------------------------------------------------
H_FAULT_CASE, D_FAULT_CASE = "size_r16", "terms_12"
INERT_UNDER_BDF1 = ("bdf1", "ustar", "stale_prev")
H_FAULTS = ["bdf1", "ustar", "stale_prev", "drop_C", "drop_S", "row_F_mass", "row_F_lin", "row_F_rhs", "row_C_nl", "row_S_nl",
            "swap_points", "Z_T", "prev_MN", "store_prev"]
D_FAULTS = ["bdf1", "ustar", "stale_prev", "row_term_coef", "row_rhs_coef", "swap_points", "drop_term", "tril_col", "store_prev"]
FAULTS = [("hrom", H_FAULT_CASE, sc.H_CASES[H_FAULT_CASE], f) for f in H_FAULTS] + \
         [("direct", D_FAULT_CASE, sc.D_CASES[D_FAULT_CASE], f) for f in D_FAULTS]


@pytest.mark.parametrize("bdf2", SCHEMES)
@pytest.mark.parametrize("kind,name,kw,fault", [pytest.param(*f, id=f"{f[0]}-{f[3]}") for f in FAULTS])
def test_planted_fault_is_caught(kind, name, kw, fault, bdf2):
    c = sc.build(kind, name, kw, bdf2)
    clean, faulty = sc.play(c), sc.play(c, fault=fault)
    if not bdf2 and fault in INERT_UNDER_BDF1:
        np.testing.assert_array_equal(faulty, clean)         # nothing for BDF1 to get wrong here
        return
    assert sc.worst(sc.measure(c, clean))[0] <= 1.0
    w, b, s, i = sc.worst(sc.measure(c, faulty))
    assert w >= 1000.0, (w, b, s, i)


def test_a_fault_in_the_last_step_of_one_point_is_named():
    """What the end-to-end bar averages away: the last step of one point off by 1e-10 relative.  The old bar passes it;
    the defect puts it above 100, the most F may ever be, and names the point and the step."""
    c = sc.build("hrom", H_FAULT_CASE, sc.H_CASES[H_FAULT_CASE], True)
    uN = sc.play(c)
    ref = uN.copy()
    uN[2, c.nt - 1] *= 1.0 + 1e-10
    assert np.linalg.norm(uN - ref) <= 1e-10 * np.linalg.norm(ref)
    w, b, s, _ = sc.worst(sc.measure(c, uN))
    assert w >= 100.0 and (b, s) == (2, c.nt - 1), (w, b, s)
