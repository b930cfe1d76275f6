"""Oversampled (M)DEIM on the host (helpers in tests/oversample_cases.py; the device halves are
tests/test_oversample_step_gpu.py, tests/test_lstsq_gpu.py and tests/test_oversample_classes_gpu.py): the premises that keep
the acceptance rule meaningful, the NumPy restatement against its own long-double certificate, planted faults that the
certificate must catch, the ABI and every argument rule of the two new entries through their ``_plan_info`` functions, and
the class logic of ``OVERSAMPLING`` on the CPU stand-ins."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import oversample_cases as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG, RT_ERR_UNSUPPORTED = -1, -3
_certified = {}


def _case(case):
    """(B, greedy entries, restatement's result, its certificate), computed once per case."""
    if case not in _certified:
        f, N, m, m_s = case
        B = oc.basis(f, N, m)
        idx0 = oc.greedy(B)
        out = oc.oversample(B, idx0, m_s)
        _certified[case] = (B, idx0, out, oc.certify(B, out[0], m))
    return _certified[case]


# ---- premises and the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.TABLE, ids=oc.label)
def test_premise_float64_cannot_move_a_score_by_more_than_1e_11(case):
    B, idx0, _, cert = _case(case)
    f, N, m, m_s = case
    assert B.shape == (N, m) and np.abs(B.T @ B - np.eye(m)).max() < 1e-12
    assert len(set(idx0.tolist())) == m
    cond = oc.condition(cert)
    print(f"OVERSAMPLE-PREMISE {oc.label(case)} eps smax^2/g max={cert.gap_term.max():.3g} sum term max={cert.sum_term.max():.3g} "
          f"min margin={cert.margin.min():.3g}")
    assert cond.shape == (m_s - m,) and np.all(cond <= oc.CONDITION), cond.max()
    assert np.all(cert.top > 0)


@pytest.mark.parametrize("case", oc.TABLE, ids=oc.label)
def test_restatement_passes_its_own_certificate(case):
    B, idx0, (idx, PT_U, margin, sigma_min), cert = _case(case)
    f, N, m, m_s = case
    assert idx.shape == (m_s,) and np.array_equal(idx[:m], idx0) and np.array_equal(PT_U, B[idx])
    oc.assert_certified(B, idx, m, label=oc.label(case), cert=cert)          # distinct entries, sigma_min monotone
    assert np.array_equal(sigma_min, cert.sigma_min)
    err = np.abs(margin - cert.margin)
    assert np.all(err <= 1e-6 * cert.margin + 1e-11), err.max()
    assert sigma_min[-1] > 1.5 * sigma_min[0], sigma_min[[0, -1]]            # what the feature is for


def test_scores_bound_the_growth_of_sigma_min():
    """Half the score is a lower bound on the growth of sigma_min^2 when the row is added (Weyl's bound for the rank-one
    update restricted to the two smallest singular directions): what the rule rests on."""
    f, N, m, m_s = oc.TABLE[0]
    B, idx0, _, _ = _case(oc.TABLE[0])
    w, g, s = oc.direction(B[idx0])
    sc = oc.scores(B, w, g)
    for i in np.argsort(sc)[-5:]:
        grown = np.linalg.svd(np.vstack([B[idx0], B[i]]), compute_uv=False)[m - 1] ** 2
        assert grown - s[m - 1] ** 2 >= 0.5 * sc[i] * (1 - 1e-10), (i, grown - s[m - 1] ** 2, sc[i])


# ---- planted faults ---------------------------------------------------------------------------------------------------
FAULT_CASE = oc.TABLE[0]


def _fails(B, idx, m):
    idx = np.asarray(idx)
    if idx.min() < 0 or idx.max() >= B.shape[0] or len(set(idx.tolist())) != len(idx):
        return True                                 # no entry at all, or one twice: assert_certified refuses these first
    cert = oc.certify(B, idx, m)
    clear = cert.margin > oc.NEAR_TIE
    return (not np.all(oc.accepted(cert))) or not np.array_equal(np.asarray(idx)[m:][clear], cert.argmax[clear])


def test_fault_the_cancelling_score_formula():
    B, idx0, m = oc.stiff_case()
    good = oc.oversample(B, idx0, m + 1)[0]
    bad = oc.oversample(B, idx0, m + 1, score_fn=oc.cancelling_scores)[0]
    cert = oc.certify(B, good, m)
    assert oc.condition(cert).max() <= oc.CONDITION and cert.margin.min() > 1e-6     # a fair case by the premise
    assert np.all(oc.cancelling_scores(B, *oc.direction(B[idx0])[:2])[2:] == 0.0)    # the paper's form has cancelled to zero
    assert not _fails(B, good, m) and good[m] == cert.argmax[0]
    assert _fails(B, bad, m) and bad[m] == 2


def test_fault_w_of_the_wrong_singular_value():
    B, idx0, _, _ = _case(FAULT_CASE)
    m, m_s = FAULT_CASE[2:]

    def wrong(rows):
        _, s, Vt = np.linalg.svd(rows, full_matrices=False)
        return np.ascontiguousarray(Vt[m - 2]), oc.direction(rows)[1], s

    assert _fails(B, oc.oversample(B, idx0, m_s, direction_fn=wrong)[0], m)


def test_fault_g_with_the_wrong_sign():
    B, idx0, _, _ = _case(FAULT_CASE)
    m, m_s = FAULT_CASE[2:]

    def wrong(rows):
        w, g, s = oc.direction(rows)
        return w, -g, s

    def signed_scores(B, w, g):                     # the formula as it stands, without the restatement's q > 0 guard
        a = g + (B * B).sum(axis=1)
        q = 4.0 * g * (B @ w) ** 2
        return q / (a + np.sqrt(np.maximum(a * a - q, 0.0)))

    assert _fails(B, oc.oversample(B, idx0, m_s, score_fn=signed_scores, direction_fn=wrong)[0], m)


def test_fault_an_index_already_taken():
    B, idx0, (idx, _, _, _), _ = _case(FAULT_CASE)
    m, m_s = FAULT_CASE[2:]
    bad = idx.copy()
    bad[m + 2] = bad[1]
    assert _fails(B, bad, m)
    with pytest.raises(AssertionError):
        oc.assert_certified(B, bad, m, show=lambda *_: None)


def test_fault_the_second_best_pick():
    B, idx0, _, cert = _case(FAULT_CASE)
    m, m_s = FAULT_CASE[2:]
    assert cert.margin.min() > 1e-6
    assert _fails(B, oc.oversample(B, idx0, m_s, rank=1)[0], m)


# ---- ABI ---------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("rt_deim_oversample_step", "rt_deim_oversample_step_plan_info", "rt_dense_lstsq_multi",
               "rt_dense_lstsq_multi_plan_info")


def test_header_declares_and_library_exports_the_entries():
    from romtime_amd import _lib, build

    text = open(os.path.join(REPO, "include", "romtime_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", code), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert text.count("since version 450") >= 2
    assert _lib.load().rt_version() >= 450
    api = open(os.path.join(REPO, "romtime_amd", "csrc", "api.hip")).read()
    assert int(re.search(r"int rt_version\(void\) \{ return (\d+); \}", api).group(1)) >= 450
    assert "deim_oversample.hip" in build.SOURCES and "lstsq.hip" in build.SOURCES
    assert "Peherstorfer" in open(os.path.join(REPO, "PAPERS.md")).read()


def _step_plan(lib, **a):
    info = (C.c_int64 * 3)()
    rc = lib.rt_deim_oversample_step_plan_info(a["Phi"], a["N"], a["m"], a["ld"], a["layout"], a["w"], a["g"], a["taken"], a["pick"],
                                               a["top2"], info)
    return rc, tuple(int(v) for v in info)


def test_step_argument_rules_and_plan_are_host_logic():
    from romtime_amd import _lib, ops

    lib = _lib.load()
    words = (C.c_double * 4)()
    ptr = C.cast(words, C.c_void_p)
    good = dict(Phi=ptr, N=2500, m=24, ld=24, layout=0, w=ptr, g=0.25, taken=ptr, pick=ptr, top2=ptr)
    call = lambda **change: _step_plan(lib, **dict(good, **change))
    assert call() == (0, (5, 512, 16))
    assert call(layout=1, ld=2500) == (0, (5, 512, 1))
    assert call(g=0.0)[0] == 0 and call(N=1)[0] == 0 and call(N=2, m=128, ld=128)[0] == 0      # no m <= N rule here
    for m, lanes in ((2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (17, 16), (1024, 16)):
        assert call(m=m, ld=m) == (0, (5, 512, lanes)), m
    for N, groups in ((511, 1), (512, 1), (513, 2), (1024, 2), (1025, 3)):
        assert call(N=N)[1][0] == groups
    bads = (dict(Phi=None), dict(w=None), dict(taken=None), dict(pick=None), dict(top2=None), dict(N=0), dict(N=-3), dict(m=1),
            dict(m=0), dict(ld=23), dict(layout=1, ld=2499), dict(layout=2), dict(layout=-1), dict(g=-1e-300), dict(g=float("nan")),
            dict(g=float("inf")), dict(g=-float("inf")))
    for bad in bads:
        assert call(**bad)[0] == RT_ERR_ARG, bad
    assert call(m=1025, ld=1025)[0] == RT_ERR_UNSUPPORTED
    most = 512 * (2 ** 31 - 1)
    assert call(N=most, layout=1, ld=most)[0] == 0 and call(N=most + 1, layout=1, ld=most + 1)[0] == RT_ERR_UNSUPPORTED
    assert lib.rt_deim_oversample_step(None, ptr, 2500, 24, 24, 0, ptr, 0.25, ptr, ptr, ptr) == RT_ERR_ARG      # no ctx
    assert ops.deim_oversample_step_plan(2500, 24) == (5, 512, 16)
    with pytest.raises(ops.RomtimeHipError):
        ops.deim_oversample_step_plan(2500, 1)


def _lstsq_plan(lib, **a):
    info = (C.c_int64 * 3)()
    rc = lib.rt_dense_lstsq_multi_plan_info(a["A"], a["rows"], a["cols"], a["trans"], a["B"], a["X"], a["nrhs"], info)
    return rc, tuple(int(v) for v in info)


def test_lstsq_argument_rules_and_plan_are_host_logic():
    from romtime_amd import _lib, ops

    lib = _lib.load()
    words = (C.c_double * 4)()
    base = C.addressof(words)
    A, B, X = (C.c_void_p(base + 8 * i) for i in range(3))
    good = dict(A=A, rows=48, cols=32, trans=0, B=B, X=X, nrhs=1000)
    call = lambda **change: _lstsq_plan(lib, **dict(good, **change))
    lds = lambda rows, cols: 8 * (rows * (cols | 1) + 4 * cols + 256)
    assert call() == (0, (4, 256, lds(48, 32)))
    assert call(trans=1)[0] == 0 and call(nrhs=1) == (0, (1, 256, lds(48, 32)))
    assert call(nrhs=256)[1][0] == 1 and call(nrhs=257)[1][0] == 2
    for rows, cols in ((1, 1), (2, 1), (2, 2), (3, 2), (128, 128), (256, 64), (142, 128), (256, 71), (252, 72)):
        rc, info = call(rows=rows, cols=cols)
        assert rc == 0 and info[2] == lds(rows, cols) <= 160 * 1024 - 8 * 1024, (rows, cols)
    for rows in range(1, 257):                                                  # every rows x cols <= 16384 works
        cols = min(rows, 128, 16384 // rows)
        assert call(rows=rows, cols=cols)[0] == 0, (rows, cols)
    bads = (dict(A=None), dict(B=None), dict(X=None), dict(X=B), dict(rows=0), dict(cols=0), dict(nrhs=0), dict(nrhs=-1),
            dict(rows=31), dict(trans=2), dict(trans=-1))
    for bad in bads:
        assert call(**bad)[0] == RT_ERR_ARG, bad
    for rows, cols in ((129, 129), (257, 8), (256, 72), (143, 128), (200, 100)):
        assert call(rows=rows, cols=cols)[0] == RT_ERR_UNSUPPORTED, (rows, cols)
    assert lib.rt_dense_lstsq_multi(None, A, 48, 32, 0, B, X, 10, None) == RT_ERR_ARG                        # no ctx
    assert ops.dense_lstsq_plan(48, 32, 1000) == (4, 256, lds(48, 32))
    with pytest.raises(ops.RomtimeHipError):
        ops.dense_lstsq_plan(257, 8)
    from romtime_amd import DiscreteEmpiricalInterpolation as D

    assert (D.LSTSQ_MAX_ROWS, D.LSTSQ_MAX_COLS, D.LSTSQ_MAX_WORDS) == (256, 128, 18432)                      # one statement each side


# ---- class logic on the CPU stand-ins -----------------------------------------------------------------------------------
@pytest.fixture
def stub(cpu_ops, monkeypatch):
    """tests/cpu_stub.py plus NumPy stand-ins of the two new operators; ``stub.calls`` lists the oversampling calls."""
    from romtime_amd import ops

    calls = []

    def deim_oversample(Phi, idx, m_s):
        calls.append((tuple(Phi.shape), int(m_s)))
        out = oc.oversample(Phi.numpy(), idx.numpy(), int(m_s))
        return torch.from_numpy(out[0]), torch.from_numpy(np.ascontiguousarray(out[1])), out[2], out[3]

    def dense_lstsq_multi(A, B, trans=False):
        A, B = A.numpy(), B.numpy()
        X = np.linalg.pinv(A).T @ B if trans else np.linalg.lstsq(A, B, rcond=None)[0]
        return torch.from_numpy(np.ascontiguousarray(X)), torch.zeros(1, dtype=torch.int32)

    monkeypatch.setattr(ops, "deim_oversample", deim_oversample)
    monkeypatch.setattr(ops, "dense_lstsq_multi", dense_lstsq_multi)
    cpu_ops.calls = calls
    return cpu_ops


def _deim(B, factor=None):
    from romtime_amd import DiscreteEmpiricalInterpolation

    red = DiscreteEmpiricalInterpolation(assemble=lambda mu, t, entries=None: None, name="f")
    if factor is not None:
        red.OVERSAMPLING = factor
    red.load_fom_basis(basis=B)
    return red


def test_class_default_is_untouched(stub):
    from romtime_amd import DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolationNonlinear

    assert DiscreteEmpiricalInterpolation.OVERSAMPLING == 1.0
    assert MatrixDiscreteEmpiricalInterpolation.OVERSAMPLING == 1.0 and MatrixDiscreteEmpiricalInterpolationNonlinear.OVERSAMPLING == 1.0
    B = oc.basis("random", 61, 4)
    plain, one = _deim(B), _deim(B, 1.0)
    assert stub.calls == []
    idx0 = oc.greedy(B)
    for red in (plain, one):
        assert red.dofs == [(int(i),) for i in idx0] and np.array_equal(red.PT_U, B[idx0]) and red.PT_U.shape == (4, 4)
        assert red.oversampling_margin is None and red.oversampling_sigma_min is None and red.greedy_margin.shape == (4,)


def test_class_target_entries_and_shapes(stub):
    B = oc.basis("random", 61, 4)
    idx0 = oc.greedy(B)
    for factor, m_s in ((1.5, 6), (2, 8), (2.2, 9), (1.01, 5), (100.0, 61)):
        red = _deim(B, factor)
        assert stub.calls[-1] == ((61, 4), m_s)
        flat = [d[0] for d in red.dofs]
        assert len(flat) == m_s == len(set(flat)) and flat[:4] == [int(i) for i in idx0]
        assert red.PT_U.shape == (m_s, 4) and np.array_equal(red.PT_U, B[flat])
        assert red.oversampling_margin.shape == (m_s - 4,) and red.oversampling_sigma_min.shape == (m_s - 4 + 1,)
        assert np.all(np.diff(red.oversampling_sigma_min) >= -1e-15)
        f = np.random.RandomState(0).standard_normal(m_s)
        np.testing.assert_allclose(red.compute_thetas(f), np.linalg.lstsq(red.PT_U, f, rcond=None)[0], rtol=0, atol=1e-13)
    one_mode = _deim(B[:, :1].copy(), 2.0)                                    # the rule needs two singular values
    assert len(one_mode.dofs) == 1 and one_mode.PT_U.shape == (1, 1)


@pytest.mark.parametrize("bad", [0.5, 0.0, -2.0, float("nan"), float("inf"), "2", True])
def test_class_refuses_a_bad_factor(stub, bad):
    B = oc.basis("random", 61, 4)
    with pytest.raises(ValueError, match="OVERSAMPLING"):
        _deim(B, bad)


def test_class_limit_is_named_before_any_work(stub, monkeypatch):
    from romtime_amd import ops

    def no_greedy(*a, **kw):
        raise AssertionError("the greedy ran before the limit was checked")

    monkeypatch.setattr(ops, "deim_greedy", no_greedy)
    B = oc.basis("random", 400, 100)
    with pytest.raises(ValueError, match="18432"):
        _deim(B, 2.0)                                                        # 200 x 101 words
    with pytest.raises(ValueError, match="256"):
        _deim(oc.basis("random", 400, 60), 5.0)                              # 300 entries
    assert stub.calls == []


def test_class_copy_and_truncate_keep_the_setting(stub):
    from tests import interp_cases as ic

    B = oc.basis("random", 61, 4)
    red = _deim(B, 1.5)
    twin = red.copy()
    assert twin.OVERSAMPLING == 1.5 and "OVERSAMPLING" in twin.__dict__ and np.array_equal(twin.PT_U, red.PT_U) and twin.dofs == red.dofs
    assert "OVERSAMPLING" not in _deim(B).copy().__dict__
    nl, _ = ic.mock_reductor("trilinear")
    Q = oc.basis("random", len(nl.rows), 5)
    nl.OVERSAMPLING = 2.0
    nl.load_fom_basis(basis=Q)
    assert nl.PT_U.shape == (10, 5) and len(nl.dofs) == 10 and all(len(d) == 2 for d in nl.dofs)
    cut = nl.truncate(2)
    assert cut.OVERSAMPLING == 2.0 and cut.N == 3 and cut.PT_U.shape == (6, 3) and len(cut.dofs) == 6
    assert nl.copy().OVERSAMPLING == 2.0
    del nl.OVERSAMPLING
    assert nl.truncate(2).PT_U.shape == (3, 3)


def test_folds_take_a_rectangular_PT_U(stub):
    """``sweep.fold_term`` and ``interpolation.fold`` with m_s > m: Z f = basis_rom theta(f) and Psi f = basis_fom theta(f)
    for the least-squares theta, and the entry limit of the certification names MAX_M."""
    from romtime_amd import interpolation
    from romtime_amd.sweep import fold_term

    B = oc.basis("random", 61, 4)
    red = _deim(B, 2.0)
    rng = np.random.RandomState(1)
    red.basis_rom = rng.standard_normal((9, 4))
    f = rng.standard_normal(8)
    theta = np.linalg.lstsq(red.PT_U, f, rcond=None)[0]
    Zt = fold_term(red.PT_U, red.basis_rom).numpy()
    assert Zt.shape == (8, 9)
    np.testing.assert_allclose(Zt.T @ f, red.basis_rom @ theta, rtol=0, atol=1e-12)
    Psi = interpolation.fold(red).numpy()
    assert Psi.shape == (61, 8)
    np.testing.assert_allclose(Psi @ f, B @ theta, rtol=0, atol=1e-12)
    assert interpolation.fold(red) is interpolation.fold(red)                # the cache holds
    wide = _deim(oc.basis("random", 400, 70), 2.0)                            # 140 entries
    with pytest.raises(ValueError, match="128"):
        interpolation.fold(wide)
