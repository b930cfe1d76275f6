"""Device POD beyond 2048 snapshots: the block Rayleigh-Ritz route (rt_sym_eig_blocked, csrc/symeig_blocked.hip;
``ops.sym_eig_blocked``; ``pod.WIDE_EIG = "device"``; the ctx option "pod_blocked" of rt_pod_orth) against a truth that
needs no extended-precision SVD at these sizes (tests/blocked_cases.py), at n = 2049 (blocks of 1025 and 1024: the wide
and the LDS-resident eigensolver get one each) and n = 4097 (three blocks).

The bars.  b = BAR_FACTOR n eps lam_1 is what the eigensolver's own truth tests grant a direct solve of a matrix of that
size and norm (tests/eig_cases.py: ``bar(1)`` units of n eps lam_1); the Ritz values may sit up to p tau^2 below the
eigenvalues on top of it ("Block Rayleigh-Ritz").  Through the POD the bars are those of
tests/svd_cases.py (``model_sigma`` / ``model_columns`` with F_S / F_COL) plus the Rayleigh-Ritz terms, per deflated
level (``blocked_cases.pod_bars``).  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import blocked_cases as bc
from tests import eig_cases as ec
from tests import guarded as gd
from tests import svd_cases as svd

pytestmark = pytest.mark.gpu
EPS = ec.EPS
LD = ec.LD
K = bc.K
RT_ERR_UNSUPPORTED = -3


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


_DEVICE = {}


def device_snapshots(case, order="C"):
    """One upload per case and memory order, shared by the tests."""
    key = (case, order)
    if key not in _DEVICE:
        X = torch.from_numpy(bc.snapshots(case)).cuda()
        _DEVICE[key] = X if order == "C" else X.t().contiguous().t()
    return _DEVICE[key]


def host_blocks(G, n):
    """Per diagonal block: the eigenvalues LAPACK finds (descending).  Also the check that the reference itself stays
    reducible: every block has rank <= K above the floor."""
    from romtime_amd import pod_rules

    widths = pod_rules.block_partition(n)
    off = np.r_[0, np.cumsum(widths)]
    return [np.linalg.eigvalsh(G[off[b]:off[b + 1], off[b]:off[b + 1]])[::-1] for b in range(len(widths))]


def check_ritz_pairs(case, G_host, lam, W, info, straddle=False):
    """The assertions on one ``sym_eig_blocked`` result: G_host is the float64 matrix the device saw.  ``straddle``: the
    blocks discard part of the signal, and the residual of a Ritz pair is first order in that: with G = R^T R its part in
    the discarded directions Z is (R Z)^T (R W y), at most tau sqrt(p) sqrt(theta_i)."""
    from romtime_amd import pod_rules

    n = case.n
    _, s, _ = bc.factors(case)
    truth = np.zeros(n, dtype=LD)
    truth[:K] = s * s
    lam1 = float(truth[0])
    blocks = host_blocks(G_host, n)
    p = len(blocks)
    floor = pod_rules.blocked_floor(n) * max(float(l[0]) for l in blocks)       # tau^2
    host_ranks = [int(np.count_nonzero(l > floor)) for l in blocks]
    assert sum(host_ranks) <= 2048 and max(host_ranks) <= K, host_ranks              # the reference stays reducible
    b = ec.bar(1.0) * n * EPS * lam1
    R = info["resolved"]
    theta = lam[:K].astype(LD)
    d = (truth[:K] - theta).astype(np.float64)
    print(f"BLOCKED-EIG {case.label} p={p} R={R} ranks={info['block_ranks']} host ranks={host_ranks} "
          f"min (lam - theta) / b = {d.min() / b:.3f} max (lam - theta - p tau2) / b = {(d.max() - p * floor) / b:.3f}")
    assert info["status"] == 0
    assert np.all(d >= -b) and np.all(d <= p * floor + b), d
    assert R >= K and R == sum(info["block_ranks"]) and R <= 2048
    for l, got in zip(blocks, info["block_ranks"]):
        bb = ec.bar(1.0) * len(l) * EPS * float(l[0])          # a direct solve of that block
        near = int(np.count_nonzero(np.abs(l - floor) <= 2 * bb))
        assert got >= int(np.count_nonzero(l > floor)) - near, (got, near)
    assert np.all(lam[R:] == 0.0)
    assert W.shape == (n, K)
    m = ec.measure(truth, np.arange(K), lam[:K], np.arange(K), W, bc.gram_apply(case))
    Wl = W.astype(LD)
    gram_err = float(np.max(np.abs(Wl.T @ Wl - np.eye(K, dtype=LD))) / (n * EPS))
    print(f"BLOCKED-EIG {case.label} res={m['res']:.3f} norm={m['norm']:.3f} orth={m['orth']:.3f} (bars {ec.bar(1.0)}; "
          f"norm in eps, orth gap-weighted in n eps as eig_cases.measure has them) unweighted max|(WY)^T(WY) - I| / (n eps) = "
          f"{gram_err:.3f}")
    # (WY)^T (WY) - I as the eigensolver's own tests hold it for a direct solve: the diagonal through ``norm``, the
    # off-diagonal through ``orth`` - weighted by the eigenvalue gap, since no solver separates close pairs better
    assert m["norm"] <= ec.bar(1.0) and m["orth"] <= ec.bar(1.0), m
    if straddle:
        Rl = bc.gram_apply(case)(Wl) - Wl * theta
        res = np.sqrt(np.sum(Rl * Rl, axis=0)).astype(np.float64)
        first_order = np.sqrt(p * floor * np.maximum(lam[:K], 0.0))
        print(f"BLOCKED-EIG {case.label} worst residual / (b + tau sqrt(p theta)) = {float(np.max(res / (b + first_order))):.3g}, "
              f"/ b = {float(np.max(res / b)):.3g}")
        assert np.all(res <= b + first_order)
    else:
        assert m["res"] <= ec.bar(1.0), m
    return m


@pytest.mark.parametrize("source", ["gram", "host"])
@pytest.mark.parametrize("case", [bc.SPREAD_2049, bc.SPREAD_4097, bc.LAST_2049], ids=lambda c: c.label)
def test_ritz_pairs_against_the_truth(ops, ctx, case, source):
    """``ops.sym_eig_blocked`` on G = X^T X, computed by rt_gram and supplied from the host in long double, rounded:
    -b <= lam_i - theta_i <= p tau^2 + b for the 24 resolved values, the ranks, zeros beyond R, and the residual and the
    orthogonality of W Y within the bar of a direct solve.  ``last``: lam_max comes from the last block."""
    if source == "gram":
        Gd = ops.gram(device_snapshots(case))
        G_host = Gd.cpu().numpy()
    else:
        G_host = bc.gram_host(case)
        Gd = torch.from_numpy(G_host).cuda()
    before = ctx.counter("eig_blocked")
    lam, W, info = ops.sym_eig_blocked(Gd, K)
    assert ctx.counter("eig_blocked") == before + 1 and ctx.counter("eig_blocked_rank") == info["resolved"]
    if case.outer_scale != 1.0:
        blocks = host_blocks(G_host, case.n)
        assert float(blocks[-1][0]) > 1e3 * float(blocks[0][0]) and info["block_ranks"][0] == 0
    check_ritz_pairs(case, G_host, lam.cpu().numpy(), W.cpu().numpy(), info)
    assert np.array_equal(Gd.cpu().numpy(), G_host)              # G untouched


def test_signal_that_straddles_the_floor(ops, ctx):
    """The first block holds 1e-6 of the energy, so nine of its 24 eigenvalues lie below the floor and are discarded with
    the signal they carry: the Ritz values stay within p tau^2 below the eigenvalues (second order), the residuals are
    first order, tau sqrt(p theta_i), and held to that."""
    case = bc.STRADDLE_2049
    G_host = bc.gram_host(case)
    lam, W, info = ops.sym_eig_blocked(torch.from_numpy(G_host).cuda(), K)
    assert 0 < info["block_ranks"][0] < K and info["block_ranks"][1] == K
    check_ritz_pairs(case, G_host, lam.cpu().numpy(), W.cpu().numpy(), info, straddle=True)


def test_outputs_stay_inside_their_extents(ctx):
    """n = 2049 with G surrounded by NaNs and lam and W inside canaries: every word of the outputs is written, nothing
    outside them is, and G and its guards are intact."""
    case, n = bc.SPREAD_2049, 2049
    G_host = bc.gram_host(case)
    Gd = gd.guarded_operand(G_host, "C", 0, False)
    lam, W = gd.guarded_output((n,)), gd.guarded_output((n, K))
    resolved, status, ranks = C.c_int64(0), C.c_int(-1), (C.c_int64 * 8)()
    floor_rel = n * float(np.finfo(float).eps)
    ctx.check(ctx.lib.rt_sym_eig_blocked(ctx.handle, P(Gd), n, floor_rel, K, P(lam.t), P(W.t), C.byref(resolved), ranks,
                                         C.byref(status)), "rt_sym_eig_blocked")
    assert status.value == 0 and resolved.value >= K
    assert lam.check() == [] and W.check() == []
    assert gd.operand_intact(Gd, G_host) == []
    info = dict(status=0, resolved=int(resolved.value), block_ranks=[int(ranks[0]), int(ranks[1])])
    check_ritz_pairs(case, G_host, lam.t.cpu().numpy(), W.t.cpu().numpy(), info)
    # k = 0 with a null W: values only
    lam0 = gd.guarded_output((n,))
    ctx.check(ctx.lib.rt_sym_eig_blocked(ctx.handle, P(Gd), n, floor_rel, 0, P(lam0.t), None, C.byref(resolved), ranks,
                                         C.byref(status)), "rt_sym_eig_blocked")
    assert status.value == 0 and lam0.check() == []
    assert gd.bits_equal(lam0.t.cpu().numpy(), lam.t.cpu().numpy())


def test_argument_limits(ctx):
    n = 2048
    Gd = torch.eye(n, dtype=torch.float64, device="cuda")
    lam = torch.empty(n, dtype=torch.float64, device="cuda")
    resolved, status, ranks = C.c_int64(0), C.c_int(0), (C.c_int64 * 8)()
    rc = ctx.lib.rt_sym_eig_blocked(ctx.handle, P(Gd), n, 1e-12, 0, P(lam), None, C.byref(resolved), ranks, C.byref(status))
    assert rc == -1 and b"rt_sym_eig_values" in ctx.lib.rt_last_error(ctx.handle)
    for bad in (dict(floor_rel=0.0), dict(k=-1), dict(k=2050), dict(n=16385)):
        a = dict(n=2049, floor_rel=1e-12, k=0)
        a.update(bad)
        rc = ctx.lib.rt_sym_eig_blocked(ctx.handle, P(Gd), a["n"], a["floor_rel"], a["k"], P(lam), None, C.byref(resolved), ranks,
                                        C.byref(status))
        assert rc == (RT_ERR_UNSUPPORTED if "n" in bad else -1), bad
    rc = ctx.lib.rt_sym_eig_blocked(ctx.handle, P(Gd), 2049, 1e-12, 4, P(lam), None, C.byref(resolved), ranks, C.byref(status))
    assert rc == -1                                              # k > 0 needs W


def test_not_reducible_set_takes_the_host_route(ops, ctx, monkeypatch):
    """A standard-normal 4096 x 2100 set: status 1, lam and W untouched inside their canaries, the counter bumped; and
    ``pod_device`` with WIDE_EIG = "device" returns what the host route returns bit for bit - it is the host route."""
    from romtime_amd import pod

    n = 2100
    X = torch.from_numpy(np.random.RandomState(11).standard_normal((4096, n))).cuda()
    Gd = ops.gram(X)
    lam, W = gd.guarded_output((n,)), gd.guarded_output((n, 8))
    before = ctx.counter("eig_blocked_not_reducible"), ctx.counter("eig_blocked")
    _, _, info = ops.sym_eig_blocked(Gd, 8, lam=lam.t, W=W.t)
    print(f"BLOCKED-EIG not reducible: {info}")
    assert info["status"] == 1 and info["resolved"] > 2048 and sum(info["block_ranks"]) == info["resolved"]
    assert ctx.counter("eig_blocked_not_reducible") == before[0] + 1 and ctx.counter("eig_blocked") == before[1]
    for out in (lam, W):
        assert bool((out.buf.view(torch.int64) == gd.CANARY_BITS).all())
    host = pod.pod_device(X, num=12)
    monkeypatch.setattr(pod, "WIDE_EIG", "device")
    with pytest.warns(RuntimeWarning, match="not reducible"):
        dev = pod.pod_device(X, num=12)
    assert ctx.counter("eig_blocked_not_reducible") == before[0] + 2
    assert gd.bits_equal(dev["s"], host["s"]) and gd.bits_equal(dev["energy"], host["energy"])
    assert gd.bits_equal(dev["Q"].cpu().numpy(), host["Q"].cpu().numpy())


# ---- through the POD ------------------------------------------------------------------------------------------------------
def check_pod(case, normalize, num, tol, Q, s, energy, tag):
    bars = bc.pod_bars(case, normalize, num, tol)
    U, _ = bc.pod_truth(case, normalize)
    n, r, sf = case.n, bars["r"], bars["sf"]
    assert Q.shape == (bc.N_ROWS, r), (Q.shape, r)
    m = min(n, bc.N_ROWS)                                  # the thin SVD has only min(N, n) singular values
    assert s.shape == (m,) and energy.shape == (m,)
    sf_n, sf = sf, sf[:m]
    ds = np.abs(s - sf)
    ratio_s = ds[:K] / bars["s_bar"][:K]
    Ur = U[:, :r].astype(np.float64)
    dist = svd.subspace_distance(Q, Ur)
    col, _ = svd.column_errors(Q, Ur)
    tail_bar = np.sqrt(ec.bar(1.0) * n * EPS) * bc.level_tops(sf_n, num or 0, tol or 0.0)[K:m]
    e_true = np.cumsum(sf * sf) / np.sum(sf * sf)
    e_err = float(np.max(np.abs(energy[:K] - e_true[:K]) / e_true[:K]))
    orth = float(np.max(np.abs(Q.T @ Q - np.eye(r)) / svd.model_orthogonality(sf[:K], r)))
    print(f"BLOCKED-POD {tag} {case.label} normalize={normalize} num={num} tol={tol} r={r} worst |ds| / bar = "
          f"{ratio_s.max():.3g} at {int(ratio_s.argmax())} subspace distance / bar = {dist / bars['dist_bar']:.3g} "
          f"({dist:.3g}) worst column / bar = {float(np.max(col / bars['col_bar'][:r])):.3g} tail / bar = "
          f"{float(np.max(s[K:] / tail_bar)):.3g} energy = {e_err:.3g} orth / model = {orth:.3g}")
    assert np.all(ratio_s <= 1.0), ratio_s
    assert np.all(s[K:] <= tail_bar)
    assert dist <= bars["dist_bar"], (dist, bars["dist_bar"])
    assert e_err <= 1e-10


POD_CASES = [(bc.SPREAD_2049, order, normalize, entry) for order in ("C", "F") for normalize in (False, True)
             for entry in ("pod_device", "orth")] + [(bc.SPREAD_4097, "C", False, "pod_device")]


@pytest.mark.parametrize("case,order,normalize,entry", POD_CASES,
                         ids=[f"{c.label}-{o}-{'norm' if nm else 'raw'}-{e}" for c, o, nm, e in POD_CASES])
def test_pod_through_the_blocked_route(ops, ctx, monkeypatch, case, order, normalize, entry):
    """``pod_device(X, num=12)`` and ``orth(X, tol=1 - 1e-9)`` with WIDE_EIG = "device": both are deep (s_12 / s_1 =
    4e-3), so level 0 and the deflated levels all take the blocked route."""
    from romtime_amd import pod

    monkeypatch.setattr(pod, "WIDE_EIG", "device")
    X = device_snapshots(case, order)
    before = ctx.counter("eig_blocked")
    if entry == "pod_device":
        num, tol = 12, None
        out = pod.pod_device(X, num=num, normalize=normalize)
        Q, s, energy = out["Q"], out["s"], out["energy"]
    else:
        num, tol = None, 1.0 - 1e-9
        Q, s, energy = pod.orth(X, tol=tol, normalize=normalize)
    assert ctx.counter("eig_blocked") >= before + 2               # level 0 and at least one deflated level
    check_pod(case, normalize, num, tol, Q.cpu().numpy(), s, energy, entry)


def test_deep_spectrum_runs_its_levels_on_the_blocked_route(ops, ctx, monkeypatch):
    """s down to 1e-9 and num = 24: eight deflated levels of three modes, each level's Gram matrix through the blocked
    route with its own lam_max, each held to the bars of its level."""
    from romtime_amd import pod

    monkeypatch.setattr(pod, "WIDE_EIG", "device")
    case = bc.DEEP_2049
    before = ctx.counter("eig_blocked")
    out = pod.pod_device(device_snapshots(case), num=24, normalize=False)
    assert ctx.counter("eig_blocked") == before + 8
    check_pod(case, False, 24, None, out["Q"].cpu().numpy(), out["s"], out["energy"], "deep")


def test_rt_pod_orth_takes_the_route_behind_its_option(ops, ctx):
    """"pod_blocked" = 1: rt_pod_orth on the n = 2049 case agrees with the truth within the bars ``pod_device`` is held
    to; with the option at 0 the call returns RT_ERR_UNSUPPORTED exactly as before."""
    from romtime_amd._lib import RomtimeHipError

    case = bc.SPREAD_2049
    X = device_snapshots(case)
    assert ctx.options.get("pod_blocked", 0) == 0
    with pytest.raises(RomtimeHipError, match=r"\(-3\).*more than 2048 snapshots"):
        ops.pod_orth(X, num=12, normalize=False)
    ctx.set_option("pod_blocked", 1)
    try:
        for normalize in (False, True):
            Q, s, energy, levels = ops.pod_orth(X, num=12, normalize=normalize)
            assert levels == 2
            check_pod(case, normalize, 12, None, Q.cpu().numpy(), s, energy, "rt_pod_orth")
        Xr = torch.from_numpy(np.random.RandomState(3).standard_normal((2304, 2100))).cuda()
        with pytest.raises(RomtimeHipError, match=r"\(-3\).*not reducible"):
            ops.pod_orth(Xr, num=4, normalize=False)
    finally:
        ctx.set_option("pod_blocked", 0)


def test_blocked_route_is_reproducible_and_placement_free(ops):
    """n = 4097: two calls give lam and W bit for bit, and so does a ctx confined to 8 CUs of every XCD ("cu_limit" 64):
    the blocks take the wide eigensolver, whose grids depend on n alone, and the products run without contraction
    splits."""
    from romtime_amd import _lib

    case = bc.SPREAD_4097
    Gd = torch.from_numpy(bc.gram_host(case)).cuda()
    lam0, W0, i0 = ops.sym_eig_blocked(Gd, K)
    lam1, W1, i1 = ops.sym_eig_blocked(Gd, K)
    assert i0 == i1 and i0["status"] == 0
    assert gd.bits_equal(lam0.cpu().numpy(), lam1.cpu().numpy()) and gd.bits_equal(W0.cpu().numpy(), W1.cpu().numpy())

    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rt_stream_create_cu_range(0, 0, 8, C.byref(h)) == 0 and h.value
    masked = _lib.Context(0)
    masked.set_option("cu_limit", 64)
    st = torch.cuda.ExternalStream(h.value)
    torch.cuda.synchronize()
    with masked.use(st):
        lam2, W2, i2 = ops.sym_eig_blocked(Gd, K)
    st.synchronize()
    masked.set_option("cu_limit", 0)
    # (this stream stays: torch's allocator remembers the stream of every block handed out under it)
    assert i2 == i0
    assert gd.bits_equal(lam0.cpu().numpy(), lam2.cpu().numpy()), gd.mismatch(lam2.cpu().numpy(), lam0.cpu().numpy())
    assert gd.bits_equal(W0.cpu().numpy(), W2.cpu().numpy()), gd.mismatch(W2.cpu().numpy(), W0.cpu().numpy())
