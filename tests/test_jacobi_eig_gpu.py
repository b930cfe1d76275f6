"""The device Jacobi eigensolver (csrc/symjacobi.hip, rt_sym_jacobi_eigh, ops.sym_jacobi_eigh) and the two-pass POD
route that runs on it (``orth(..., passes=2)`` on a device tensor), on an MI355X.  Helpers, matrices, the long-double
truth and the host routine's figures: tests/jacobi_cases.py (premises: tests/test_jacobi_eig_cpu.py).

Exact answers inside NaN guards and canaries; accuracy against the truth, every bar four times the larger of 1 and
rt_host_jacobi_eigh's ratio on the same matrix and at most 20; the shapes around the tile edges and the limit; bits
that depend on n alone; the POD route with the host routine taken away.

Measured on an MI355X (units of n eps; the host routine's figure on the same matrix in brackets), over the twenty
matrices of ``test_accuracy_against_the_truth`` - n = 7, 64, 129, 257, 512, four kinds each:
relative error of every positive eigenvalue 0.032 ... 0.179 (0.026 ... 0.150), |W^T W - I| 0.278 ... 1.017 (0.342 ... 0.699),
residuals 0.005 ... 0.037 (0.006 ... 0.113); 4 ... 6 sweeps, the closing one included (the host's own count, which leaves
it out: 2 ... 4), the largest excess being the allowed 2 (``graded_1e-1`` at n = 512: 6 against 4; n = 7 and 64: 4
against 2).  lam, W and the sweep count are those of the NumPy restatement bit for bit (asserted below on three of the
matrices), and these figures are the restatement's on the matrices as committed; an MI355X run on an earlier draw of
the same four kinds (Gaussian E) gave 0.030 ... 0.226, 0.354 ... 0.997 and 0.004 ... 0.121 with the same sweep counts."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

from tests import guarded as gd
from tests import jacobi_cases as jc
from tests import svd_cases as sc
from tests.guarded import guarded_operand, guarded_output

pytestmark = pytest.mark.gpu
RT_ERR_ARG, RT_ERR_UNSUPPORTED = -1, -3


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


def _cdiv(a, b):
    return -(-a // b)


def _solve_guarded(ctx, G, max_sweeps=60):
    """rt_sym_jacobi_eigh on ``G`` surrounded by NaNs and misaligned by 8 bytes, lam and W between canaries.  Returns
    (lam, W, sweeps, status) as host values after checking operand, canaries and rt_last_launch_info."""
    G = np.array(G, dtype=np.float64)      # a writable copy: the cached matrices are read-only
    n = G.shape[0]
    Gd = guarded_operand(G, "C", 0, True)
    lam, W = guarded_output((n,)), guarded_output((n, n))
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    sweeps = C.c_int(-1)
    ctx.check(ctx.lib.rt_sym_jacobi_eigh(ctx.handle, P(Gd), n, P(lam.t), P(W.t), max_sweeps, C.byref(sweeps), P(status)),
              "rt_sym_jacobi_eigh")
    torch.cuda.synchronize()
    assert lam.check() == [] and W.check() == [], (lam.check(), W.check())
    assert gd.operand_intact(Gd, G) == [], gd.operand_intact(Gd, G)
    info = (C.c_int64 * 3)()
    assert ctx.lib.rt_last_launch_info(ctx.handle, info) == 0
    pairs = (n + n % 2) // 2
    assert list(info) == [sweeps.value, n - 1 + n % 2, _cdiv(pairs, 64) * (_cdiv(pairs, 16) + _cdiv(n, 32))], list(info)
    return lam.t.cpu().numpy(), W.t.cpu().numpy(), int(sweeps.value), int(status.item())


# ---- exact answers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 65, 130])
def test_diagonal_matrices_exactly(ctx, n):
    """Unsorted integer diagonals with repeated values and zeros: no rotation, one sweep, the sorted diagonal bit for bit,
    W exactly the permutation with ties in index order."""
    rng = np.random.RandomState(n)
    d = rng.randint(0, max(n // 2, 2), size=n).astype(np.float64)
    if n >= 3:
        d[0], d[n // 2], d[-1] = 0.0, d[1], 0.0
    lam, W, sweeps, status = _solve_guarded(ctx, np.diag(d))
    order = np.argsort(-d, kind="stable")
    assert sweeps == 1 and status == 0
    assert gd.bits_equal(lam, d[order]), gd.mismatch(lam, d[order])
    assert gd.bits_equal(W, np.eye(n)[:, order]), gd.mismatch(W, np.eye(n)[:, order])


def _coupled(n, rng):
    """Blocks [[a, b], [b, a]] with integers a > b > 0 on randomly coupled index pairs (one 1 x 1 block for odd n) whose
    meetings fall in different rounds; (G, sorted a +- b, partner of every index)."""
    where = {}
    for rnd, (p, q) in enumerate(jc.rounds(n)):
        for a, b in zip(p, q):
            where[(min(a, b), max(a, b))] = rnd
    for _ in range(100):
        perm = rng.permutation(n)
        couples = [(int(perm[2 * k]), int(perm[2 * k + 1])) for k in range(n // 2)]
        meet = {where[(min(a, b), max(a, b))] for a, b in couples}
        if len(meet) >= min(len(couples), 3):
            break
    else:
        raise AssertionError("no coupling whose pairs meet in different rounds")
    G, lam, partner = np.zeros((n, n)), [], np.arange(n)
    for i, j in couples:
        b = float(rng.randint(1, 50))
        a = b + float(rng.randint(1, 50))
        G[i, i] = G[j, j] = a
        G[i, j] = G[j, i] = b
        lam += [a + b, a - b]
        partner[i], partner[j] = j, i
    if n % 2:
        G[perm[-1], perm[-1]] = float(rng.randint(1, 100))
        lam.append(G[perm[-1], perm[-1]])
    return G, np.sort(np.array(lam))[::-1], partner


@pytest.mark.parametrize("n", [2, 3, 7, 64, 65, 130])
def test_two_by_two_blocks_exactly(ctx, n):
    """theta = 0, t = 1: one rotating sweep and the closing one, lam exactly the sorted a +- b, every entry of W within
    an ulp of 0 or +-sqrt(1/2) and a column's two entries on one coupled pair."""
    G, want, partner = _coupled(n, np.random.RandomState(1000 + n))
    lam, W, sweeps, status = _solve_guarded(ctx, G)
    assert sweeps == 2 and status == 0
    assert gd.bits_equal(lam, want), gd.mismatch(lam, want)
    h = np.sqrt(0.5)
    mag = np.abs(W)
    is_zero, is_half, is_one = mag == 0.0, np.abs(mag - h) <= np.spacing(h), mag == 1.0
    assert np.all(is_zero | is_half | is_one)
    for col in range(n):
        rows = np.flatnonzero(~is_zero[:, col])
        if len(rows) == 1:
            assert n % 2 == 1 and is_one[rows[0], col] and partner[rows[0]] == rows[0]
        else:
            assert len(rows) == 2 and partner[rows[0]] == rows[1] and np.all(is_half[rows, col])


def test_arguments_limit_and_status(ctx):
    """Null or non-positive arguments: RT_ERR_ARG; n = 2049: RT_ERR_UNSUPPORTED with the limit in rt_last_error;
    max_sweeps reached: status 1, lam and W written all the same."""
    n = 8
    G = torch.eye(n, dtype=torch.float64, device="cuda")
    lam = torch.empty(n, dtype=torch.float64, device="cuda")
    W = torch.empty((n, n), dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    f, h = ctx.lib.rt_sym_jacobi_eigh, ctx.handle
    assert f(h, None, n, P(lam), P(W), 60, None, P(status)) == RT_ERR_ARG
    assert f(h, P(G), n, None, P(W), 60, None, P(status)) == RT_ERR_ARG
    assert f(h, P(G), n, P(lam), None, 60, None, P(status)) == RT_ERR_ARG
    assert f(h, P(G), n, P(lam), P(W), 60, None, None) == RT_ERR_ARG
    assert f(h, P(G), 0, P(lam), P(W), 60, None, P(status)) == RT_ERR_ARG
    assert f(h, P(G), -3, P(lam), P(W), 60, None, P(status)) == RT_ERR_ARG
    assert f(h, P(G), n, P(lam), P(W), 0, None, P(status)) == RT_ERR_ARG
    assert f(h, P(G), n, P(lam), P(W), 60, None, P(status)) == 0          # sweeps_done may be null
    big = torch.eye(2049, dtype=torch.float64, device="cuda")
    assert f(h, P(big), 2049, P(lam), P(W), 60, None, P(status)) == RT_ERR_UNSUPPORTED
    assert b"2048" in ctx.lib.rt_last_error(h)
    Gm, _ = jc.matrix("graded_1e-1", 64)
    lam1, W1, sweeps, st = _solve_guarded(ctx, Gm, max_sweeps=1)
    assert sweeps == 1 and st == 1
    assert np.all(np.isfinite(lam1)) and np.all(np.isfinite(W1)) and np.all(lam1[:-1] >= lam1[1:])
    assert np.abs(W1.T @ W1 - np.eye(64)).max() <= 4 * 64 * jc.EPS    # a product of rotations all the same


# ---- accuracy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", jc.cases(jc.GPU_SIZES), ids=[jc.label(k, n) for k, n in jc.cases(jc.GPU_SIZES)])
def test_accuracy_against_the_truth(ctx, kind, n):
    """Every positive eigenvalue relative to the long-double truth, |W^T W - I| and the residuals, in units of n eps:
    each bar four times the larger of 1 and the host routine's ratio on the same matrix, at most 20; the sweeps at most
    two more than the host's."""
    G, _ = jc.matrix(kind, n)
    truth, host = jc.truth(kind, n), jc.host_reference(kind, n)
    lam, W, sweeps, status = _solve_guarded(ctx, G)
    got = jc.ratios(G, lam, W, truth)
    print(f"JACOBI-DEVICE {jc.label(kind, n)} lam={got['lam']:.3f} ({host['lam']:.3f}) orth={got['orth']:.3f} "
          f"({host['orth']:.3f}) res={got['res']:.3f} ({host['res']:.3f}) sweeps={sweeps} ({host['sweeps']})")
    assert status == 0
    for key in ("lam", "orth", "res"):
        assert got[key] <= jc.bar(host[key]), (key, got, host)
    assert sweeps <= host["sweeps"] + jc.MAX_EXTRA_SWEEPS, (sweeps, host["sweeps"])
    if kind == "singular_tail":
        assert np.count_nonzero(lam == 0.0) == max(n // 4, 1)


@pytest.mark.parametrize("kind,n", [("graded_1e-1", 7), ("cluster", 64), ("singular_tail", 129)])
def test_bits_are_those_of_the_numpy_restatement(ctx, kind, n):
    """No contraction, IEEE division and square root: NumPy reproduces lam, W and the sweep count bit for bit."""
    G, _ = jc.matrix(kind, n)
    lam, W, sweeps, _ = _solve_guarded(ctx, G)
    lam_r, W_r, sweeps_r, _ = jc.restated(G)
    assert sweeps == sweeps_r
    assert np.array_equal(lam, lam_r), gd.mismatch(lam, lam_r)      # == : a zero's sign is not part of the claim
    assert np.array_equal(W, W_r), gd.mismatch(W, W_r)


# ---- shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 7, 63, 64, 65, 129, 130])
def test_shapes_around_the_pairing_and_the_tiles(ctx, n):
    """Odd n (an idle index every round), one side of a tile of 64 column pairs / 16 row pairs / 32 rows of W and one
    past it: a dense well-conditioned matrix against LAPACK to the project's 20 n eps |lam_1|, W orthogonal and
    G W = W diag(lam) to the same."""
    rng = np.random.RandomState(7 * n)
    B = rng.standard_normal((n, n))
    G = B @ B.T + n * np.eye(n)
    G = np.triu(G) + np.triu(G, 1).T
    lam, W, sweeps, status = _solve_guarded(ctx, G)
    ref = np.linalg.eigvalsh(G)[::-1]
    bound = 20 * n * jc.EPS * ref[0]
    print(f"JACOBI-SHAPE n={n} sweeps={sweeps} |lam - lapack|={np.abs(lam - ref).max():.2e} bound {bound:.2e}")
    assert status == 0 and sweeps <= 12
    assert np.abs(lam - ref).max() <= bound
    assert np.abs(W.T @ W - np.eye(n)).max() <= 20 * n * jc.EPS
    assert np.abs(G @ W - W * lam).max() <= bound


def test_the_limit_2048(ops):
    """n = 2048, diagonally dominant: a few sweeps of 2047 launches; eigenvalues against LAPACK, W orthogonal."""
    n = 2048
    rng = np.random.RandomState(2048)
    B = 1e-5 * rng.standard_normal((n, n))       # row sums of about 0.03 beside a diagonal of 1 ... 33
    G = np.diag(1.0 + np.arange(n, dtype=np.float64)[::-1] / 64.0) + (B + B.T)
    Gd = ops.to_device(G)
    lam, W, sweeps = ops.sym_jacobi_eigh(Gd)
    ref = np.linalg.eigvalsh(G)[::-1]
    err = np.abs(lam.cpu().numpy() - ref).max()
    orth = float((W.T @ W - torch.eye(n, dtype=torch.float64, device="cuda")).abs().max())
    res = float((Gd @ W - W * lam[None, :]).abs().max())
    print(f"JACOBI-LIMIT n=2048 sweeps={sweeps} |lam - lapack|={err:.2e} orth={orth:.2e} res={res:.2e}")
    assert sweeps <= 8
    assert err <= 20 * n * jc.EPS * ref[0] and orth <= 20 * n * jc.EPS and res <= 20 * n * jc.EPS * ref[0]
    assert torch.equal(Gd.cpu(), torch.from_numpy(G))


# ---- reproducible and placement-free --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [130, 257])
def test_reproducible_and_placement_free(ops, n):
    """Two calls give lam and W bit for bit, and so does a ctx confined to 8 CUs of every XCD: grids and sums depend on
    n alone (the pattern of test_wide_route_is_reproducible_and_placement_free)."""
    from romtime_amd import _lib

    Gd = ops.to_device(jc.matrix("graded_1e-1", 257)[0][:n, :n].copy())
    lam0, W0, s0 = ops.sym_jacobi_eigh(Gd)
    lam1, W1, s1 = ops.sym_jacobi_eigh(Gd)
    assert s0 == s1
    assert gd.bits_equal(lam0.cpu().numpy(), lam1.cpu().numpy()) and gd.bits_equal(W0.cpu().numpy(), W1.cpu().numpy())
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rt_stream_create_cu_range(0, 0, 8, C.byref(h)) == 0 and h.value
    masked = _lib.Context(0)
    masked.set_option("cu_limit", 64)
    st = torch.cuda.ExternalStream(h.value)
    torch.cuda.synchronize()
    with masked.use(st):
        lam2, W2, s2 = ops.sym_jacobi_eigh(Gd)
    st.synchronize()
    masked.set_option("cu_limit", 0)
    # (this stream stays: torch's allocator remembers the stream of every block handed out under it)
    assert s2 == s0
    assert gd.bits_equal(lam0.cpu().numpy(), lam2.cpu().numpy()), gd.mismatch(lam2.cpu().numpy(), lam0.cpu().numpy())
    assert gd.bits_equal(W0.cpu().numpy(), W2.cpu().numpy()), gd.mismatch(W2.cpu().numpy(), W0.cpu().numpy())


# ---- the POD route --------------------------------------------------------------------------------------------------------
def _no_host_jacobi(*a, **k):
    raise AssertionError("the host Jacobi routine was called")


_ids = dict(ids=lambda c: c.label)


@pytest.mark.parametrize("case", sc.SMALL_CASES, **_ids)
def test_two_pass_pod_stays_on_the_device(monkeypatch, case):
    """orth(X, passes=2, return_VT=True, num / tol of the case) at 600 x 32 and 1536 x 64 over the five families with
    pod.jacobi_eigh taken away, to the factors of tests/test_pod_truth_gpu.py."""
    from romtime_amd import pod

    monkeypatch.setattr(pod, "jacobi_eigh", _no_host_jacobi)
    sc.check_pod_against_truth(case, ("two_pass",))


def test_two_pass_pod_on_a_stream_row(monkeypatch):
    """98304 x 128 ``graded``: the streaming Gram and back-projection kernels around the device solver."""
    from romtime_amd import pod

    monkeypatch.setattr(pod, "jacobi_eigh", _no_host_jacobi)
    case = next(c for c in sc.STREAM_128 if c.family == "graded")
    sc.check_pod_against_truth(case, ("two_pass",))


def test_two_pass_pod_without_vt_matches_with_vt(monkeypatch, ops):
    """return_VT only adds the device product W W2_r: Q, s and energy are the same bits either way."""
    import romtime_amd
    from romtime_amd import pod

    monkeypatch.setattr(pod, "jacobi_eigh", _no_host_jacobi)
    case = sc.SMALL_CASES[0]
    X, _ = sc.snapshots(case)
    Xd = ops.to_device(X)
    Q0, s0, e0 = romtime_amd.orth(Xd, passes=2, **case.kwargs)
    Q1, s1, e1, VT = romtime_amd.orth(Xd, passes=2, return_VT=True, **case.kwargs)
    assert gd.bits_equal(Q0.cpu().numpy(), Q1.cpu().numpy()) and gd.bits_equal(s0, s1) and gd.bits_equal(e0, e1)
    assert VT.shape == (Q1.shape[1], case.n)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, X, kwargs, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from romtime_amd import pod
        from romtime_amd._lib import Context

        pod.jacobi_eigh = _no_host_jacobi
        Context.current().set_option("eig_one_xcd", 0)   # the ranks share one GPU: none of them can have a whole XCD
        rows = np.array_split(np.arange(X.shape[0]), world)[rank]
        out = pod.pod_device(torch.from_numpy(X[rows]).cuda(), group=dist.group.WORLD, want_vt=True, **kwargs)
        ret[rank] = dict(rows=rows, Q=out["Q"].cpu().numpy(), s=out["s"], energy=out["energy"], r=out["r"], VT=out["VT"])
    finally:
        dist.destroy_process_group()


def test_two_pass_pod_row_sharded_over_two_ranks():
    """passes=2 with a group: two ranks on the one GPU over gloo (as tests/test_distributed_gpu.py).  Both ranks solve
    the same all-reduced G2 and must return the same bits; together they are the single-device POD."""
    import torch.multiprocessing as mp
    from romtime_amd import pod

    rng = np.random.RandomState(12)
    N, n = 20_000, 45
    U0, _ = np.linalg.qr(rng.standard_normal((N, n)))
    V0, _ = np.linalg.qr(rng.standard_normal((n, n)))
    X = (U0 * 10.0 ** (-np.arange(n) * 0.22)) @ V0.T
    kwargs = dict(num=20, normalize=True, passes=2)
    single = pod.pod_device(torch.from_numpy(X).cuda(), want_vt=True, **kwargs)
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), X, kwargs, ret), nprocs=world, join=True)
    assert set(ret.keys()) == set(range(world))
    a, b = ret[0], ret[1]
    assert a["r"] == b["r"] == single["r"] == 20
    assert gd.bits_equal(a["s"], b["s"]) and gd.bits_equal(a["energy"], b["energy"]) and gd.bits_equal(a["VT"], b["VT"])
    s1 = single["s"]
    assert np.all(np.abs(a["s"] - s1) <= sc.F_S * sc.model_sigma(s1, np.full(n, s1[0])))     # the bar of svd_cases, s_L = s_1
    Q = np.empty((N, 20))
    Q[a["rows"]], Q[b["rows"]] = a["Q"], b["Q"]
    assert np.abs(Q.T @ Q - np.eye(20)).max() <= 1e-9
    Qs = single["Q"].cpu().numpy()
    cos = np.abs(np.sum(Q * Qs, axis=0))
    assert cos.min() > 1 - 1e-8, cos.min()
