"""The block Rayleigh-Ritz route for Gram matrices of more than 2048 snapshots (rt_sym_eig_blocked,
csrc/symeig_blocked.hip, DESIGN.md "Block Rayleigh-Ritz") as far as a host without a GPU can hold it: the partition rule
in both languages, the premises of the method on a long-double model of it, and the switch ``pod.WIDE_EIG``."""
import ctypes as C

import numpy as np
import pytest
import torch

from romtime_amd import _lib, ops, pod, pod_rules
from tests.blocked_cases import dct_columns
from tests.svd_cases import LD, longdouble_svd

EPS_LD = float(np.finfo(LD).eps)


# ---- 1. the partition rule --------------------------------------------------------------------------------------------
def _plan(n, block_max):
    lib = _lib.load()
    p, widths = C.c_int64(-1), (C.c_int64 * 8)()
    rc = lib.rt_sym_eig_blocked_plan_info(n, block_max, C.byref(p), widths)
    return rc, int(p.value), [int(w) for w in widths[: max(0, min(int(p.value), 8))]]


@pytest.mark.parametrize("n,block_max", [(2049, 2048), (4096, 2048), (4097, 2048), (6145, 2048), (16384, 2048),
                                         (17, 8), (20, 8), (33, 8), (40, 8), (64, 8), (19, 9), (28, 9), (72, 9)])
def test_partition_rule_is_the_same_in_both_languages(n, block_max):
    rc, p, widths = _plan(n, block_max)
    assert rc == 0
    mine = pod_rules.block_partition(n, block_max)
    assert p == -(-n // block_max) == len(mine)
    assert widths == mine.tolist() == ops.sym_eig_blocked_plan(n, block_max).tolist()
    assert sum(widths) == n and max(widths) - min(widths) <= 1 and max(widths) <= block_max
    assert widths == sorted(widths, reverse=True)          # the wider blocks first
    if block_max == 2048:
        assert min(widths) >= 1024                           # every block is a size the device eigensolver takes


def test_partition_of_the_sizes_the_tests_use():
    assert pod_rules.block_partition(2049).tolist() == [1025, 1024]
    assert pod_rules.block_partition(4097).tolist() == [1366, 1366, 1365]
    assert pod_rules.block_partition(16384).tolist() == [2048] * 8


@pytest.mark.parametrize("n,block_max,rc_want", [(0, 8, -1), (-3, 8, -1), (8, 0, -1), (65, 8, -3), (16385, 2048, -3)])
def test_partition_refuses_outside_the_limits(n, block_max, rc_want):
    rc, _, _ = _plan(n, block_max)
    assert rc == rc_want
    with pytest.raises(ValueError):
        pod_rules.block_partition(n, block_max)
    with pytest.raises(_lib.RomtimeHipError):
        ops.sym_eig_blocked_plan(n, block_max)


def test_plan_takes_a_null_width_array_and_refuses_a_null_count():
    lib = _lib.load()
    p = C.c_int64(0)
    assert lib.rt_sym_eig_blocked_plan_info(4097, 2048, C.byref(p), None) == 0 and p.value == 3
    assert lib.rt_sym_eig_blocked_plan_info(4097, 2048, None, None) == -1


def test_floor_and_abi():
    assert pod_rules.blocked_floor(4097) == 4097 * np.finfo(float).eps
    assert _lib.load().rt_version() >= 400
    assert {"rt_sym_eig_blocked", "rt_sym_eig_blocked_plan_info"} <= set(_lib.SIGNATURES)
    from romtime_amd import build

    assert "symeig_blocked.hip" in build.SOURCES


# ---- 2. the premises, on a long-double model of the method ------------------------------------------------------------------
def model(X, block_max, floor_rel):
    """The method of rt_sym_eig_blocked on G = X^T X in long double, every eigensolve a long-double SVD of the factor:
    dict(status, ranks, R, theta, WY, p, tau2)."""
    n = X.shape[1]
    widths = pod_rules.block_partition(n, block_max)
    off = np.r_[0, np.cumsum(widths)]
    pairs = []
    for b in range(len(widths)):
        _, sb, Vb = longdouble_svd(X[:, off[b]:off[b + 1]])
        pairs.append((sb * sb, Vb))
    lam_max = max(l[0] for l, _ in pairs)
    tau2 = LD(floor_rel) * lam_max
    ranks = [int(np.count_nonzero(l > tau2)) for l, _ in pairs]
    R = sum(ranks)
    out = dict(status=0, ranks=ranks, R=R, p=len(widths), tau2=tau2)
    if R > block_max:
        out["status"] = 1
        return out
    W = np.zeros((n, R), dtype=LD)
    c = 0
    for b, (_, Vb) in enumerate(pairs):
        W[off[b]:off[b + 1], c:c + ranks[b]] = Vb[:, :ranks[b]]
        c += ranks[b]
    _, sm, Y = longdouble_svd(X @ W)              # G_M = W^T G W = (X W)^T (X W)
    out.update(theta=sm * sm, WY=W @ Y)
    return out


def factored(N, n, s, seed):
    """X = A diag(s) B^T in long double: A, B orthonormal DCT vectors, B's rows permuted so that no block sees a zero panel.
    (s, A) is its exact SVD; the eigenvalues of X^T X are s^2 and n - len(s) zeros."""
    k = len(s)
    perm = np.random.RandomState(seed).permutation(n)
    return (dct_columns(N, k) * np.asarray(s, dtype=LD)) @ dct_columns(n, k)[perm].T


MODEL_CASES = [
    # n, singular values, floor_rel: ranks stay within block_max = 8 - two or three modes above the floor per block - and
    # a tail below the floor that the blocks discard, so that theta < lambda by something the bound has to cover
    (20, (1.0, 1e-2, 1e-5, 1e-6), 1e-6),
    (24, (1.0, 0.5, 3e-4, 1e-5), 1e-6),
    (31, (1.0, 1e-1, 2e-4, 1e-4, 5e-5), 1e-5),
    (40, (1.0, 2e-4, 1e-4), 1e-5),
    (33, (1.0, 1e-9), 40 * 2.2e-16),               # the default floor, n eps: nothing near it
]


@pytest.mark.parametrize("n,s,floor_rel", MODEL_CASES)
def test_ritz_values_sit_within_p_tau2_below_the_eigenvalues(n, s, floor_rel):
    N = 48
    X = factored(N, n, s, seed=n)
    m = model(X, 8, floor_rel)
    assert m["status"] == 0 and 1 <= m["R"] <= 8, m["ranks"]
    lam = np.zeros(n, dtype=LD)
    lam[:len(s)] = np.asarray(s, dtype=LD) ** 2
    R, theta, p, tau2 = m["R"], m["theta"], m["p"], m["tau2"]
    slack = 64 * n * EPS_LD * lam[0]               # the long-double SVDs' own rounding
    gap = lam[:R] - theta
    print(f"BLOCKED-MODEL n={n} p={p} ranks={m['ranks']} R={R} max gap / (p tau2)={float(np.max(gap) / (p * tau2)):.3g}")
    assert np.all(gap >= -slack), gap
    assert np.all(gap <= p * tau2 + slack), (gap, p * tau2)
    # something was discarded in the cases with a tail: the bound is not vacuous
    if floor_rel >= 1e-6:
        assert float(np.max(gap)) > 0.0
    # Q = X (W Y) theta^(-1/2) is orthonormal by construction: to the rounding of the products, grown by lam_1 / theta
    Q = (X @ m["WY"]) / np.sqrt(theta)
    E = Q.T @ Q - np.eye(R, dtype=LD)
    bar = 64 * n * EPS_LD * lam[0] / np.sqrt(theta[:, None] * theta[None, :])
    assert np.all(np.abs(E) <= bar), float(np.max(np.abs(E) / bar))
    WY = m["WY"]
    assert float(np.max(np.abs(WY.T @ WY - np.eye(R, dtype=LD)))) <= 64 * n * EPS_LD


def test_full_rank_set_is_not_reducible():
    X = np.random.RandomState(5).standard_normal((48, 24)).astype(LD)
    m = model(X, 8, 24 * 2.2e-16)
    assert m["status"] == 1 and m["ranks"] == [8, 8, 8] and m["R"] == 24


# ---- 3. the switch ------------------------------------------------------------------------------------------------------
def test_wide_eig_defaults_to_host_and_rejects_other_values(monkeypatch):
    assert pod.WIDE_EIG == "host"
    G = torch.eye(4, dtype=torch.float64)
    assert pod._SmallEig(G).on_device is False
    for bad in ("gpu", "Device", None, 1):
        monkeypatch.setattr(pod, "WIDE_EIG", bad)
        with pytest.raises(ValueError, match="WIDE_EIG"):
            pod._SmallEig(G)
    monkeypatch.setattr(pod, "WIDE_EIG", "device")
    e = pod._SmallEig(G)                                # a host tensor keeps the host route whatever the switch says
    assert e.on_device is False and e.trace is None
