"""rt_interpolation_errors' host side (declaration, export, version, argument checks and launch plan: none needs a GPU),
the premises of every fixture of tests/test_interpolation_gpu.py (the oracle within the bar of the long-double truth, the
bar far below the errors it certifies, exact data exact), and the host logic of romtime_amd.interpolation with the device
operators stubbed: ``cpu_ops`` plus NumPy restatements of ``ops.interpolation_errors``, ``ops.dense_solve_multi`` and
``ops.p1_local_assembly`` (tests/interp_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from romtime_amd import interpolation as _feature  # noqa: F401  (without the feature nothing here can run)
from tests import interp_cases as ic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_ARG, RT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture
def interp(cpu_ops, monkeypatch):
    """romtime_amd.interpolation on the host stand-ins; ``interp.calls`` counts the calls of the new operator."""
    from romtime_amd import interpolation, ops

    calls = []

    def counted(Psi, idx, F, group=1, pin=None, want_ref=False):
        calls.append((tuple(F.shape), group, pin))
        return ic.numpy_interpolation_errors(Psi, idx, F, group=group, pin=pin, want_ref=want_ref)

    monkeypatch.setattr(ops, "interpolation_errors", counted)
    monkeypatch.setattr(ops, "dense_solve_multi", ic.numpy_dense_solve_multi)
    monkeypatch.setattr(ops, "p1_local_assembly", ic.numpy_p1_local_assembly)
    interpolation.calls = calls
    yield interpolation
    del interpolation.calls


def test_header_declares_and_library_exports_the_entry():
    from romtime_amd import _lib, build

    text = open(os.path.join(REPO, "include", "romtime_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rt_interpolation_errors", "rt_interpolation_errors_plan_info"):
        assert re.search(rf"\bint\s+{name}\s*\(", code), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert "since\n * version 380" in text or "since version 380" in text
    assert _lib.load().rt_version() >= 380
    assert "interp_error.hip" in build.SOURCES


def _plan_call(lib, **a):
    idx = a["idx"]
    buf = None if idx is None else (C.c_int64 * len(idx))(*idx)
    info = (C.c_int64 * 3)()
    rc = lib.rt_interpolation_errors_plan_info(a["cus"], a["Psi"], a["ldpsi"], buf, a["m"], a["F"], a["ldf"], a["layout"], a["N"],
                                               a["S"], a["group"], a["pin_row"], a["pin_value"], a["err"], a["ref"], info)
    return rc, dict(grid=int(info[0]), splits=int(info[1]), tile=(int(info[2]) // 1000, int(info[2]) % 1000))


def test_argument_checks_and_plan_are_host_logic():
    """rt_interpolation_errors_plan_info runs the entry point's own checks without a ctx; of its pointers only idx (a host
    array) is read."""
    from romtime_amd import _lib

    lib = _lib.load()
    words = (C.c_double * 4)()                                     # stands for every device array: never read
    ptr = C.cast(words, C.c_void_p)
    good = dict(cus=256, Psi=ptr, ldpsi=24, idx=list(range(0, 2400, 100)), m=24, F=ptr, ldf=2500, layout=1, N=2500, S=130,
                group=5, pin_row=0, pin_value=1.0, err=ptr, ref=ptr)
    call = lambda **change: _plan_call(lib, **dict(good, **change))

    assert call() == (0, ic.interpolation_errors_plan(2500, 130, 256))
    assert call()[1] == dict(grid=9, splits=3, tile=(32, 64))
    assert call(ref=None, pin_row=-1)[0] == 0                      # optional
    assert call(layout=0, ldf=130)[0] == 0 and call(layout=0, ldf=129)[0] == RT_ERR_ARG
    assert call(m=128, ldpsi=128, idx=list(range(128)))[0] == 0
    assert call(m=129, ldpsi=129, idx=list(range(129)))[0] == RT_ERR_UNSUPPORTED
    last = good["idx"][:-1]
    bads = (dict(Psi=None), dict(idx=None), dict(F=None), dict(err=None), dict(N=0), dict(m=0), dict(S=0), dict(group=0),
            dict(N=-5), dict(group=4), dict(group=7), dict(pin_row=-2), dict(pin_row=2500), dict(ldpsi=23), dict(ldf=2499),
            dict(layout=2), dict(layout=-1), dict(cus=0), dict(idx=last + [2500]), dict(idx=last + [-1]),
            dict(idx=[-1] + good["idx"][1:]), dict(idx=last + [2 ** 40]))
    for bad in bads:
        assert call(**bad)[0] == RT_ERR_ARG, bad
    assert call(idx=last + [2499])[0] == 0                         # N - 1 is the last legal index
    for N, S, cus in ((1, 1, 256), (33, 63, 256), (1025, 65, 304), (200_000, 4096, 64), (2081, 130, 256), (300_000, 4096, 256)):
        got = call(N=N, S=S, group=1, ldf=N, pin_row=N - 1, idx=[0, N - 1] * 12, cus=cus)
        assert got == (0, ic.interpolation_errors_plan(N, S, cus)), (N, S, cus)
    one, many = (call(N=200_000, ldf=200_000, S=S, group=1)[1] for S in (1, 4096))
    assert one["splits"] == many["splits"] == 196 and many["grid"] == 64 * one["grid"]     # the slicing ignores S
    idx = (C.c_int64 * 24)(*good["idx"])
    assert lib.rt_interpolation_errors(None, ptr, 24, idx, 24, ptr, 2500, 1, 2500, 130, 5, 0, 1.0, ptr, ptr) == RT_ERR_ARG  # no ctx


@pytest.mark.parametrize("case", ic.EXACT_CASES, ids=[c[0] for c in ic.EXACT_CASES])
def test_premise_exact_cases_are_exact_in_float64(case):
    """Integer arithmetic proves the sums; the float64 restatement reproduces their correctly rounded roots bit for bit."""
    from tests.guarded import bits_equal

    _, N, S, m, _, _, _, pin_row, pin_value, group, _ = case
    Psi, idx, F = ic.exact_case(case)
    assert Psi.shape == (N, m) and F.shape == (N, S) and idx.shape == (m,) and S % group == 0
    assert idx.min() >= 0 and idx.max() < N
    if m >= 3:
        assert 0 in idx and N - 1 in idx and (pin_row < 0 or pin_row in idx)
    pin = None if pin_row < 0 else (pin_row, pin_value)
    se, sr = ic.exact_sums(Psi, idx, F, pin)
    s0 = sum((int(F[i, 0]) - (int(pin_value) if i == pin_row else sum(int(Psi[i, e]) * int(F[idx[e], 0]) for e in range(m)))) ** 2
             for i in range(N))                                    # snapshot 0 once more, in Python integers
    assert s0 == int(se[0])
    err, ref = ic.exact_expected(case, Psi, idx, F)
    got, got_ref = ic.numpy_interpolation_errors(Psi, idx, F, group=group, pin=pin, want_ref=True)
    assert bits_equal(got.numpy(), err) and bits_equal(got_ref.numpy(), ref)
    if pin is not None:                                            # the pin is visible in these data
        assert not np.array_equal(ic.exact_sums(Psi, idx, F, None)[0], se)


@pytest.mark.parametrize("case", ic.RANDOM_CASES + [ic.SMALL_RANDOM], ids=[c[0] for c in ic.RANDOM_CASES + [ic.SMALL_RANDOM]])
def test_premise_random_cases(case):
    """The oracle's float64 arithmetic and the folded restatement both sit within the bar of the long-double truth, and
    the bar is at most 1e-4 of every error it certifies."""
    c = ic.random_case(case)
    truth, bar = c["truth"], c["bar"]
    assert truth.shape == bar.shape == (c["F"].shape[1] // c["group"],)
    oracle = ic.oracle_errors(c["basis"], c["PT_U"], c["idx"], c["F"], c["pin"], c["group"])
    folded = ic.numpy_interpolation_errors(c["Psi"], c["idx"], c["F"], group=c["group"], pin=c["pin"]).numpy()
    r_oracle = float(np.max(np.abs(oracle - truth).astype(np.float64) / bar))
    r_folded = float(np.max(np.abs(folded - truth).astype(np.float64) / bar))
    rel = float(np.max(bar / truth.astype(np.float64)))
    print(f"{case[0]}: |oracle - truth| / bar = {r_oracle:.2e}, |folded - truth| / bar = {r_folded:.2e}, bar / truth = {rel:.2e}")
    assert r_oracle <= 1.0 and r_folded <= 1.0
    assert rel <= 1e-4
    off = c["off_span"]                                            # before the Dirichlet entry of a pinned case is set
    assert 5e-4 < off.min() and off.max() < 2e-3                   # the snapshots leave the span by 1e-3


@pytest.mark.parametrize("which", ic.MOCK_CASES)
def test_premise_mock_cases(cpu_ops, which):
    red, _ = ic.mock_reductor(which)
    idx = None
    from romtime_amd import interpolation

    idx = interpolation.flat_indices(red)
    for mu in ic.MOCK_MUS:
        F, group = ic.mock_samples(red, mu, ic.MOCK_TS)
        assert F.shape[0] == len(red.rows) and F[0].min() == F[0].max() == 1.0          # entry 0: the Dirichlet entry
        truth = ic.longdouble_errors(red.basis_fom, red.PT_U, idx, F, (0, 1.0), group)
        bar = ic.error_bar(red.PT_U, F, group)
        oracle = ic.oracle_errors(red.basis_fom, red.PT_U, idx, F, (0, 1.0), group)
        assert np.all(np.abs(oracle - truth).astype(np.float64) <= bar)
        assert float(truth.min()) > 1e3 * bar.max(), (which, float(truth.min()), bar.max())   # the truncation is what is measured


# ---- host logic of romtime_amd.interpolation ---------------------------------------------------------------------------

def test_flat_indices_of_a_permuted_topology(interp):
    from romtime_amd import DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation

    md = MatrixDiscreteEmpiricalInterpolation(assemble=None, name="permuted")
    md.rows = [2, 0, 1, 1, 0, 2, 1]
    md.cols = [2, 0, 0, 1, 1, 1, 2]
    md.dofs = [(1, 1), (2, 1), (0, 0), (1, 2)]
    np.testing.assert_array_equal(interp.flat_indices(md), [3, 5, 1, 6])
    assert interp.flat_indices(md).dtype == np.int64 and interp.pin_of(md) == (0, 1.0)
    md.dofs = [(0, 2)]
    with pytest.raises(KeyError):
        interp.flat_indices(md)
    d = DiscreteEmpiricalInterpolation(assemble=None, name="vector")
    d.dofs = [(7,), (0,), (3,)]
    np.testing.assert_array_equal(interp.flat_indices(d), [7, 0, 3])
    assert interp.pin_of(d) is None


def _host_and_device(which):
    """The same reductor twice: the class's host loop, and EVALUATE_ON = "device"."""
    host, _ = ic.mock_reductor(which)
    dev, _ = ic.mock_reductor(which)
    dev.EVALUATE_ON = "device"
    return host, dev


@pytest.mark.parametrize("which", ic.MOCK_CASES)
def test_device_evaluate_keeps_the_host_loops_bookkeeping(interp, which):
    from romtime_amd.conventions import Stage

    host, dev = _host_and_device(which)
    assert host.EVALUATE_ON == "host"
    host.evaluate(ic.MOCK_TS, mu_space=ic.MOCK_MUS)
    assert interp.calls == []                                      # the default never reaches the new operator
    dev.evaluate(ic.MOCK_TS, mu_space=ic.MOCK_MUS)
    assert len(interp.calls) == len(ic.MOCK_MUS)                   # one call per parameter point
    assert dev.mu_space[Stage.ONLINE] == host.mu_space[Stage.ONLINE] == ic.MOCK_MUS and dev.mu == host.mu
    assert sorted(dev.errors_rom) == sorted(host.errors_rom) == [0, 1]
    for k in host.errors_rom:
        a, b = host.errors_rom[k], dev.errors_rom[k]
        assert type(a) is type(b) is np.ndarray and a.dtype == b.dtype == np.float64 and a.shape == b.shape == (len(ic.MOCK_TS),)
        F, group = ic.mock_samples(dev, ic.MOCK_MUS[k], ic.MOCK_TS)
        bar = ic.error_bar(dev.PT_U, F, group)
        assert np.all(np.abs(a - b) <= bar), (which, k, np.abs(a - b), bar)
        assert a.min() > 1e3 * bar.max()
    if which == "trilinear":
        assert [c[1] for c in interp.calls] == [3, 3] and interp.calls[0][0][1] == 3 * len(ic.MOCK_TS)
        other = ic.mock_states()[:, :2] * 1.5                      # ``funcs``: other states than the reductor's own
        dev.evaluate(ic.MOCK_TS[:2], mu_space=[dict(ic.MOCK_MUS[0], alpha_0=2.0)], funcs=other)
        assert interp.calls[-1][:2] == ((len(dev.rows), 4), 2) and dev.errors_rom[2].shape == (2,)
    else:
        assert all(c[1] == 1 and c[2] == (0, 1.0) for c in interp.calls)


@pytest.mark.parametrize("which", ("mass", "trilinear"))
def test_chunking_does_not_change_a_bit(interp, which):
    red, _ = ic.mock_reductor(which)
    n_psi = 3 if which == "trilinear" else 1
    results = []
    for max_columns in (n_psi, 2 * n_psi, float("inf")):
        r, _ = ic.mock_reductor(which)
        del interp.calls[:]
        interp.evaluate(r, ic.MOCK_TS, mu_space=ic.MOCK_MUS[:1], max_columns=max_columns)
        chunk = len(ic.MOCK_TS) if max_columns == float("inf") else max_columns // n_psi
        assert [c[0][1] for c in interp.calls] == [chunk * n_psi] * (len(ic.MOCK_TS) // chunk)
        results.append(r.errors_rom[0])
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
    assert results[0].shape == (len(ic.MOCK_TS),)


def test_evaluate_on_routes_every_class_and_rejects_other_values(interp, monkeypatch):
    from romtime_amd import (DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation,
                             MatrixDiscreteEmpiricalInterpolationNonlinear)

    seen = []
    monkeypatch.setattr(interp, "evaluate", lambda red, ts, **kw: seen.append((type(red).__name__, sorted(kw))))
    assert DiscreteEmpiricalInterpolation.EVALUATE_ON == "host"
    for cls in (DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolationNonlinear):
        red = cls(assemble=None, name="routed")
        red.EVALUATE_ON = "device"
        red.evaluate([0.1], num=1)
        twin = red.copy()
        assert twin.EVALUATE_ON == "device" and "EVALUATE_ON" in twin.__dict__         # an instance override travels
        assert "EVALUATE_ON" not in cls(assemble=None, name="plain").copy().__dict__
        red.EVALUATE_ON = "gpu"
        with pytest.raises(ValueError, match="EVALUATE_ON"):
            red.evaluate([0.1], num=1)
    assert seen == [("DiscreteEmpiricalInterpolation", ["mu_space", "num"]),
                    ("MatrixDiscreteEmpiricalInterpolation", ["mu_space", "num"]),
                    ("MatrixDiscreteEmpiricalInterpolationNonlinear", ["funcs", "mu_space", "num"])]


def test_fold_limits_and_cache(interp):
    from romtime_amd import DiscreteEmpiricalInterpolation

    rng = np.random.default_rng(3)
    d = DiscreteEmpiricalInterpolation(assemble=None, name="wide")
    d.basis_fom = rng.standard_normal((200, 129))
    d.PT_U = d.basis_fom[:129]
    d.dofs = [(i,) for i in range(129)]
    with pytest.raises(ValueError, match="128"):
        interp.fold(d)
    with pytest.raises(ValueError, match="128"):
        interp.snapshot_errors(d, rng.standard_normal((200, 2)))
    d.basis_fom = rng.standard_normal((50, 2))
    d.PT_U = np.zeros((2, 2))
    d.dofs = [(0,), (1,)]
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        interp.fold(d)
    with pytest.raises(np.linalg.LinAlgError):
        interp.evaluate(d, [0.1], mu_space=[{}])
    assert d.mu_space["online"] == []                              # refused before any bookkeeping
    d.PT_U = d.basis_fom[:2].copy()
    Psi = interp.fold(d)
    np.testing.assert_allclose(Psi.numpy(), d.basis_fom @ np.linalg.inv(d.PT_U), rtol=1e-12, atol=1e-12)
    assert interp.fold(d) is Psi                                   # cached against the identities of basis_fom and PT_U
    d.PT_U = d.PT_U.copy()
    assert interp.fold(d) is not Psi
    got = interp.snapshot_errors(d, np.asfortranarray(d.basis_fom @ rng.standard_normal((2, 6))), group=3)
    assert got.shape == (2,) and got.max() < 1e-13                 # inside the span: interpolated exactly


def test_closed_form_snapshots_match_the_callbacks(interp):
    """evaluate_closed_form builds the same snapshots as assemble_snapshot, so it returns evaluate's errors."""
    for which, kind in (("mass", "mass"), ("stiffness_ale", "stiffness")):
        red, solver = ic.mock_reductor(which)
        got = interp.evaluate_closed_form(red, kind, solver, ic.MOCK_MUS, ic.MOCK_TS, max_columns=4)
        assert got.shape == (len(ic.MOCK_MUS), len(ic.MOCK_TS))
        interp.evaluate(red, ic.MOCK_TS, mu_space=ic.MOCK_MUS)
        for k, mu in enumerate(ic.MOCK_MUS):
            F, _ = ic.mock_samples(red, mu, ic.MOCK_TS)
            assert np.all(np.abs(got[k] - red.errors_rom[k]) <= ic.error_bar(red.PT_U, F)), (which, k)
    with pytest.raises(ValueError, match="kind"):
        interp.evaluate_closed_form(red, "trilinear", solver, ic.MOCK_MUS, ic.MOCK_TS)
    with pytest.raises(NotImplementedError):
        interp.evaluate_closed_form(red, "mass", object(), ic.MOCK_MUS, ic.MOCK_TS)
