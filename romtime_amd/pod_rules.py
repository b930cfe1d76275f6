"""The decisions every POD entry point takes from a spectrum, stated once for the Python side (pod.pod_device,
pipeline.PodPipeline / PodLanes); csrc/host_dense.{h,cpp} states the same rules once for rt_pod_orth, and
tests/test_pod_rules_cpu.py holds the two against each other.  Pure NumPy: no torch, no library.

Every acceptance is written through positive comparisons, so a NaN among the eigenvalues rejects."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

DROP_TOLERANCE = 1e-7  # pod.py:4 (the reference's docstring says 1e-8; the code is 1e-7)
RR_GAP = 1e-4           # smallest eigenvalue gap (relative to lam_1) for which inverse iteration is trusted as is
TWO_PASS_RATIO = 1e-2  # one Gram pass: vectors good to ~eps (sigma_1/sigma_i)^2 <= 2e-12 above this ratio
# A deflated level accepts the modes within this ratio of its largest singular value sigma_L.  A Gram pass resolves a mode
# to eps (sigma_L/sigma_i)^2, sigma_L/sigma_i times what a backward stable SVD delivers: with 1e-2 here the modes at the
# bottom of a level were up to 18 times (Q^T Q - I: 21 times) outside that (tests/test_pod_truth_gpu.py); 0.08 bounds the
# loss by 12.5 and costs a level per 1.1 decades of kept spectrum instead of one per two.
LEVEL_RATIO = 0.08
MAX_LEVELS = 16   # n eps sigma_1 (level_size's floor) is reached after 13 levels of 1.1 decades


def sigma(lam):
    """Singular values from Gram eigenvalues (rounding can leave tiny negative ones)."""
    return np.sqrt(np.clip(lam, 0.0, None))


def energy(s):
    ev = np.power(s, 2)
    return np.cumsum(ev) / np.sum(ev)


def truncation_rank(s, energy, num=None, tol=None) -> int:
    """Number of modes kept, with the reference's precedence (pod.py:46-57).

    ``energy < tol`` is strict, so the mode that crosses ``tol`` is excluded; the energy curve is
    non-decreasing and ``s`` non-increasing, hence every mask is a prefix."""
    if tol:
        return int(np.count_nonzero(energy < tol))
    if num:
        return int(min(num, len(s)))
    return int(np.count_nonzero(s > DROP_TOLERANCE))


def separated(lam, k) -> bool:
    """Inverse iteration resolves an eigenvector to ~eps ||G|| / gap: with every gap among the k kept eigenvalues (and
    to the first discarded one; to zero when k == n) at least RR_GAP * lam_1 that is <= 2e-12 and the vectors are used
    as they are; closer eigenvalues get a k x k Rayleigh-Ritz step on G."""
    n = len(lam)
    gaps = lam[:k] - lam[1:k + 1] if k < n else np.r_[lam[:k - 1] - lam[1:k], lam[k - 1]]
    return bool(gaps.min() >= RR_GAP * max(lam[0], 1e-300))


def deep(s, r) -> bool:
    """A kept mode below TWO_PASS_RATIO of the largest: one Gram pass does not resolve it, deflated levels do."""
    return bool(r > 0 and s[0] > 0 and s[r - 1] < TWO_PASS_RATIO * s[0])


def single_pass_rank(lam, status, n_rows, k, num=None, tol=None):
    """``r`` when the ``k`` single-pass vectors enqueued ahead of the spectrum ``lam`` may be handed out (their first
    ``r``), else None: the eigensolve finished, the set has at least as many rows as columns, the truncation rule keeps
    1 .. k modes, and they are neither deep nor clustered."""
    n = len(lam)
    s = sigma(lam)
    r = truncation_rank(s, energy(s), num=num, tol=tol)
    ok = (status == 0 and n_rows >= n and 1 <= r <= k and s[0] > 0 and s[r - 1] >= TWO_PASS_RATIO * s[0]
          and separated(lam, r))
    return r if ok else None


# ---- deflated levels -----------------------------------------------------------------------------------------------------
def level_size(sig, first, room, n) -> int:
    """Modes a deflated level accepts from its singular values ``sig``: those within LEVEL_RATIO of the largest, at
    least one, at most ``room``.  ``first``: the first singular value accepted so far (None on level 0) - below
    n eps sigma_1 the deflated snapshots hold rounding residue, not modes: the numerical rank is reached and the
    remaining columns of a ``num`` basis stay zero (what the single-pass route returns too)."""
    floor = n * np.finfo(float).eps * first if first is not None else 0.0
    return int(min(max(1, np.count_nonzero(sig >= LEVEL_RATIO * sig[0])), room)) if sig[0] > floor else 0


def merged_spectrum(accepted, sig, k, total):
    """(s, energy, tail) after a level: the accepted singular values (a list of arrays, this level's ``sig[:k]`` last),
    then the level's tail ``sig[k:]`` as far as n entries go, zeros beyond; the energy over ``total``, the trace of the
    level-0 Gram matrix."""
    n = len(sig)
    got = sum(len(x) for x in accepted)
    tail = sig[k:k + (n - got)]
    s = np.concatenate(list(accepted) + [tail, np.zeros(max(0, n - got - len(tail)))])
    return s, np.cumsum(np.power(s, 2)) / total, tail


def levels_done(r, got, k, n, levels, tail) -> bool:
    """The kept modes are covered, the level accepted nothing, the spectrum or the level budget is used up, or nothing
    but zeros is left."""
    return bool(r <= got or k == 0 or got >= n or levels >= MAX_LEVELS or tail.size == 0 or not tail[0] > 0.0)


# ---- what travels to the host ahead of every decision ----------------------------------------------------------------------
class Head(NamedTuple):
    """lam (n) | eigensolver status | zero-norm flag | row count, as one float64 vector (packed on the device by
    ``pod.pack_head``, which needs torch; this module does not)."""
    lam: np.ndarray
    status: int
    zero_norm: int
    n_rows: int


def parse_head(head, n, n_rows=None) -> Head:
    """``head``: the host copy of what ``pod.pack_head`` made, n + 1, n + 2 or n + 3 numbers.  A field that was not
    packed is None (the Gram matrix of a deflated level has no flag and no row count; PodLanes knows the row count on
    the host and passes it as ``n_rows``)."""
    extra = len(head) - n
    return Head(head[:n], int(head[n]), int(head[n + 1]) if extra > 1 else None,
                int(round(float(head[n + 2]))) if extra > 2 else n_rows)


def zero_norm_error() -> ValueError:
    # the reference divides by a zero norm and scipy.linalg.svd then rejects the NaNs (pod.py:32-38)
    return ValueError("array must not contain infs or NaNs (zero-norm snapshot with normalize=True)")


# ---- Gram matrices wider than the device eigensolver takes (rt_sym_eig_blocked, csrc/symeig_blocked.hip) --------------------
BLOCK_MAX = 2048        # the device eigensolver's limit: the widest diagonal block
MAX_BLOCKS = 8          # 16384 = 8 x 2048


def block_partition(n, block_max=BLOCK_MAX):
    """Widths of the p = ceil(n / block_max) contiguous column blocks of the block Rayleigh-Ritz route: they differ by
    at most one, the wider ones first.  The rule of rt_sym_eig_blocked_plan_info, which refuses the same arguments."""
    n, block_max = int(n), int(block_max)
    if n < 1 or block_max < 1:
        raise ValueError("block_partition: n and block_max must be positive")
    p = -(-n // block_max)
    if p > MAX_BLOCKS:
        raise ValueError(f"block_partition: {p} blocks of at most {block_max} columns (more than {MAX_BLOCKS})")
    return np.array([n // p + (1 if b < n % p else 0) for b in range(p)], dtype=np.int64)


def blocked_floor(n) -> float:
    """``floor_rel`` of the block Rayleigh-Ritz route: a block keeps the eigenvectors above floor_rel * lam_max.  n eps:
    with it p tau^2 <= p n eps lam_1, the level to which any Gram eigensolve resolves an eigenvalue anyway."""
    return float(int(n) * np.finfo(float).eps)
