"""Device eigensolver for Gram matrices of 1025 to 2048 snapshots (csrc/symeig.hip, the wide route): the
tridiagonalisation whose every dependency is a kernel boundary, the multisection and the eigenvector kernels at
NM = 2048, the C entry points' new limit, and ``orth`` on sets wider than 1024 columns with the host eigensolver
taken away."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import romtime_oracle as oracle
from tests import guarded as gd
from tests.guarded import guarded_operand, guarded_output

pytestmark = pytest.mark.gpu
EPS = 2.2e-16
RT_ERR_UNSUPPORTED = -3
EIG_COUNTERS = ("eig_wide_form", "eig_general_form", "eig_one_xcd")


@pytest.fixture(scope="module")
def ops():
    from romtime_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def ctx():
    from romtime_amd._lib import Context

    return Context.current()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _gram_like(n, kind):
    """The matrices of test_kernels_gpu.py::test_sym_eig_device."""
    rng = np.random.RandomState(n)
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    if kind == "decay":
        lam = 10.0 ** (-16.0 * np.arange(n) / max(n - 1, 1))
    elif kind == "flat":
        lam = 1.0 + rng.rand(n)
    else:  # repeated leading eigenvalues and an exactly singular tail
        lam = np.r_[np.full(min(4, n), 2.0), 10.0 ** (-np.arange(n - min(4, n)) * 0.5)]
        lam[n // 2:] = 0.0
    lam = np.sort(lam)[::-1]
    G = (V * lam) @ V.T
    return 0.5 * (G + G.T)


@pytest.mark.parametrize("n", [1025, 1537, 2048])
@pytest.mark.parametrize("kind", ["decay", "flat", "cluster"])
def test_wide_sym_eig_device(ops, ctx, n, kind):
    """Eigenvalues to the project's bound 20 n eps |lam_1| against LAPACK, the 12 leading vectors an invariant subspace
    to 1e-10 |lam_1|, G untouched, and the route taken is the wide one (its counter moves, the hand-off forms' do not).
    1025: one past the LDS-resident form, every tile ragged; 1537: odd, no multiple of a chunk; 2048: the limit."""
    G = _gram_like(n, kind)
    Gd = ops.to_device(G)
    before = {c: ctx.counter(c) for c in EIG_COUNTERS}
    ld, status = ops.sym_eig_values(Gd)
    W = ops.sym_eig_vectors(ld, 12).cpu().numpy()
    assert int(status.item()) == 0
    after = {c: ctx.counter(c) for c in EIG_COUNTERS}
    ref = np.linalg.eigvalsh(G)[::-1]
    got = ld.cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"n={n} {kind}: max|lam - ref| = {err:.3e}, bound {20 * n * EPS * abs(ref[0]):.3e}")
    assert err <= 20 * n * EPS * abs(ref[0]), err
    np.testing.assert_array_equal(G, Gd.cpu().numpy())  # input untouched
    Q, _ = np.linalg.qr(W)
    H = Q.T @ G @ Q
    res = np.abs(G @ Q - Q @ H).max()
    print(f"n={n} {kind}: max|GQ - QH| = {res:.3e}, bound {1e-10 * abs(ref[0]):.3e}")
    assert res <= 1e-10 * abs(ref[0]), res
    assert after["eig_wide_form"] == before["eig_wide_form"] + 1
    assert after["eig_general_form"] == before["eig_general_form"] and after["eig_one_xcd"] == before["eig_one_xcd"]


def test_wide_sym_eig_parts_guarded(ctx):
    """n = 1025, G surrounded by NaNs and misaligned by one element, lam and W inside canaries: a slice of the spectrum
    is the full call's values bit for bit and writes nothing outside the slice; operands and canaries stay intact."""
    n, k = 1025, 12
    G = _gram_like(n, "decay")
    Gd = guarded_operand(G, "C", 0, True)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lam_full = guarded_output((n,))
    ctx.check(ctx.lib.rt_sym_eig_values(ctx.handle, P(Gd), n, P(lam_full.t), P(status)), "rt_sym_eig_values")
    W = guarded_output((n, k))
    ctx.check(ctx.lib.rt_sym_eig_vectors(ctx.handle, n, k, P(lam_full.t), P(W.t)), "rt_sym_eig_vectors")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    full = lam_full.t.cpu().numpy()
    ref = np.linalg.eigvalsh(G)[::-1]
    assert np.abs(full - ref).max() <= 20 * n * EPS * abs(ref[0])
    assert lam_full.check() == [] and W.check() == []
    Q, _ = np.linalg.qr(W.t.cpu().numpy())
    assert np.abs(G @ Q - Q @ (Q.T @ G @ Q)).max() <= 1e-10 * abs(ref[0])
    for first, count in ((0, 1), (n - 1, 1), (n // 3, n // 4)):
        lam = guarded_output((n,))
        ctx.check(ctx.lib.rt_sym_eig_values_part(ctx.handle, P(Gd), n, first, count, P(lam.t), P(status)),
                  "rt_sym_eig_values_part")
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        part = lam.t[first:first + count].cpu().numpy()
        assert gd.bits_equal(part, full[first:first + count]), gd.mismatch(part, full[first:first + count])
        bits = lam.t.view(torch.int64).cpu().numpy()
        outside = np.r_[bits[:first], bits[first + count:]]
        assert np.all(outside == gd.CANARY_BITS), (first, count)
        lam.prefilled = True
        assert lam.check() == []
    assert gd.operand_intact(Gd, G) == [], gd.operand_intact(Gd, G)


def test_wide_route_is_reproducible_and_placement_free(ops):
    """n = 1100: two calls give lam and 12 vectors bit for bit, and so does a ctx confined to 8 CUs of every XCD
    ("cu_limit" 64).  The LDS-resident form needs 128 co-resident workgroups of one per CU and cannot run there: the
    wide route waits for nothing, and its grids and sums depend on n alone."""
    from romtime_amd import _lib

    n, k = 1100, 12
    Gd = ops.to_device(_gram_like(n, "decay"))

    def solve():
        lam, status = ops.sym_eig_values(Gd)
        W = ops.sym_eig_vectors(lam, k)
        return lam, W, status

    lam0, W0, s0 = solve()
    lam1, W1, s1 = solve()
    torch.cuda.synchronize()
    assert int(s0.item()) == 0 and int(s1.item()) == 0
    assert gd.bits_equal(lam0.cpu().numpy(), lam1.cpu().numpy()) and gd.bits_equal(W0.cpu().numpy(), W1.cpu().numpy())

    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rt_stream_create_cu_range(0, 0, 8, C.byref(h)) == 0 and h.value
    masked = _lib.Context(0)
    masked.set_option("cu_limit", 64)
    st = torch.cuda.ExternalStream(h.value)
    torch.cuda.synchronize()
    with masked.use(st):
        lam2, W2, s2 = solve()
        wide = masked.counter("eig_wide_form")
    st.synchronize()
    masked.set_option("cu_limit", 0)
    # (this stream stays: torch's allocator remembers the stream of every block handed out under it)
    assert int(s2.item()) == 0 and wide == 1
    assert gd.bits_equal(lam0.cpu().numpy(), lam2.cpu().numpy()), gd.mismatch(lam2.cpu().numpy(), lam0.cpu().numpy())
    assert gd.bits_equal(W0.cpu().numpy(), W2.cpu().numpy()), gd.mismatch(W2.cpu().numpy(), W0.cpu().numpy())


def test_limit_is_2048(ctx):
    n = 2049
    Gd = torch.eye(n, dtype=torch.float64, device="cuda")
    lam = torch.empty(n, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert ctx.lib.rt_sym_eig_values(ctx.handle, P(Gd), n, P(lam), P(status)) == RT_ERR_UNSUPPORTED
    assert b"2048" in ctx.lib.rt_last_error(ctx.handle)
    assert ctx.lib.rt_sym_eig_values_part(ctx.handle, P(Gd), n, 0, 1, P(lam), P(status)) == RT_ERR_UNSUPPORTED
    X = torch.ones((2100, n), dtype=torch.float64, device="cuda")
    Q = torch.empty((2100, 4), dtype=torch.float64, device="cuda")
    s, energy = np.empty(n), np.empty(n)
    r, levels = C.c_int64(0), C.c_int(0)
    rc = ctx.lib.rt_pod_orth(ctx.handle, P(X), 2100, n, n, 0, 4, 0.0, 1, P(Q), 4, C.byref(r), s.ctypes.data,
                             energy.ctypes.data, C.byref(levels))
    assert rc == RT_ERR_UNSUPPORTED
    assert b"2048" in ctx.lib.rt_last_error(ctx.handle)


# ---- orth on wide sets ------------------------------------------------------------------------------------------------

def _matrix(rng, N, n, decay):
    """As in test_pipeline_gpu.py."""
    U, _ = np.linalg.qr(rng.standard_normal((N, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (U * 10.0 ** (-decay * np.arange(n) / (n - 1))) @ V.T


def _mu_level(seed=7, N=3000, blocks=30, cols=40, rank=60):
    """What the mu level of a tree walk stacks: the time-level bases of ``blocks`` parameter points, each an orthonormal
    basis of ``cols`` modes out of one shared ``rank``-dimensional space with a spectrum six decades deep."""
    rng = np.random.RandomState(seed)
    U0, _ = np.linalg.qr(rng.standard_normal((N, rank)))
    w = 10.0 ** (-6.0 * np.arange(rank) / (rank - 1))
    out = []
    for _ in range(blocks):
        B = (U0 * w) @ rng.standard_normal((rank, cols)) + 1e-9 * rng.standard_normal((N, cols))
        out.append(np.linalg.qr(B)[0])
    return np.hstack(out)


_INPUTS: dict = {}
_SVDS: dict = {}


def _input(name):
    """Built once per session; the tests only read them."""
    if not _INPUTS:
        rng = np.random.RandomState(21)
        _INPUTS["shallow_1100"] = _matrix(rng, 2500, 1100, 2.0)
        _INPUTS["deep_1300"] = _matrix(rng, 2600, 1300, 9.0)      # deep spectrum: deflated levels
        _INPUTS["mu_1200"] = _mu_level()
        _INPUTS["limit_2048"] = _matrix(np.random.RandomState(22), 2200, 2048, 5.0)
    return _INPUTS[name]


LIMIT_KW = dict(num=7, normalize=True)
PROBE = (slice(None, None, 317), slice(None, None, 293))


def _oracle_orth(name, **kw):
    """oracle.orth on the named input; its dgesvd of (input, normalize) is computed once and shared by the cases.  The
    2200 x 2048 set's dgesvd takes a minute: oracle.orth's result on it is recorded (tests/golden/make_wide_eig.py),
    together with a sample of the input it belongs to."""
    if name == "limit_2048":
        assert kw == LIMIT_KW
        ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_eig_limit_2048.npz"))
        np.testing.assert_allclose(_input(name)[PROBE], ref["probe"], rtol=0, atol=1e-13)   # the same input (entries <= 1)
        return ref["Q"], ref["s"], ref["energy"]
    real = oracle.svd
    key = (name, bool(kw.get("normalize", True)))

    def shared_svd(a, **opts):
        if key not in _SVDS:
            _SVDS[key] = real(a, **opts)
        return _SVDS[key]

    oracle.svd = shared_svd
    try:
        return oracle.orth(_input(name), **kw)
    finally:
        oracle.svd = real


ORTH_CASES = [(name, kw) for name in ("shallow_1100", "deep_1300")
              for kw in (dict(tol=1.0 - 1e-9, normalize=True), dict(num=7, normalize=True), dict(normalize=True))]
ORTH_CASES += [("mu_1200", dict(num=40, normalize=False)), ("mu_1200", dict(tol=1.0 - 1e-9, normalize=False)),
               ("mu_1200", dict(normalize=True)), ("limit_2048", LIMIT_KW)]


@pytest.mark.parametrize("name,kw", ORTH_CASES, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for n, kw in ORTH_CASES])
def test_orth_on_wide_sets_without_the_host_eigensolver(monkeypatch, name, kw):
    """The public ``orth`` on sets of 1100 to 2048 columns with ``pod._eigh_desc`` (host LAPACK) taken away: rank,
    singular values, orthogonality and subspace against the oracle's dgesvd, to the bars of
    test_pipeline_gpu.py::test_workers_match_single_pods_any_truncation."""
    import romtime_amd
    from romtime_amd import pod

    def no_host(*a, **k):
        raise AssertionError("the host eigensolver was called")

    monkeypatch.setattr(pod, "_eigh_desc", no_host)
    monkeypatch.setattr(pod, "DEVICE_EIG_MAX_N", 2048)
    X = _input(name)
    Q, s, energy = romtime_amd.orth(X, **kw)
    Qo, so, eo = _oracle_orth(name, **kw)
    assert Q.shape[1] == Qo.shape[1], (Q.shape, Qo.shape)
    bar = 2e-13 * so[0] + 8 * EPS * so[0] ** 2 / np.maximum(so, 1e-300)
    orth_err = np.abs(Q.T @ Q - np.eye(Q.shape[1])).max()
    sub = np.linalg.norm(Q - Qo @ (Qo.T @ Q), 2)
    print(f"{name} {kw}: r = {Q.shape[1]}, worst |s - s_ref| / bar = {(np.abs(s - so) / bar).max():.3f}, "
          f"|Q^T Q - I| = {orth_err:.2e}, subspace = {sub:.2e}")
    assert np.all(np.abs(s - so) <= bar)
    assert orth_err < 1e-9
    assert sub <= 1e-7


def test_composite_pod_orth_on_a_wide_set(ops, monkeypatch):
    """rt_pod_orth at 2500 x 1100 (one foreign call, its own host logic) against pod.pod_device: rank and s."""
    from romtime_amd import pod

    monkeypatch.setattr(pod, "DEVICE_EIG_MAX_N", 2048)
    Xd = ops.to_device(_input("shallow_1100"))
    for kw in (dict(tol=1.0 - 1e-9), dict(num=7), dict()):
        single = pod.pod_device(Xd, normalize=True, **kw)
        Q, s, energy, levels = ops.pod_orth(Xd, normalize=True, **kw)
        so = single["s"]
        assert Q.shape[1] == single["r"], kw
        bar = 2e-13 * so[0] + 8 * EPS * so[0] ** 2 / np.maximum(so, 1e-300)
        assert np.all(np.abs(s - so) <= bar), kw
