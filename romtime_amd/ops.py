"""Device operators of the POD / (M)DEIM / reduced-solve path (thin wrappers over the C ABI).

Inputs are float64 CUDA ``torch.Tensor``s (torch is the allocator / stream provider only);
``to_device`` moves NumPy data over PCIe preserving its C/F memory order so that no host
transpose is ever made.  Every function raises if the HIP library or the GPU is absent.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, pod_rules
from ._lib import COL_MAJOR, ROW_MAJOR, Context, RomtimeHipError

_p = C.c_void_p


def _ptr(t):
    return _p(t.data_ptr()) if t is not None else _p(None)


def _need_gpu():
    if not torch.cuda.is_available():
        raise RomtimeHipError("no MI355X visible: romtime_amd's hot path runs on the GPU only (there is no CPU fallback)")


def to_device(a, device=None) -> torch.Tensor:
    """NumPy (or tensor) -> float64 CUDA tensor with the same logical shape and memory order."""
    _need_gpu()
    if isinstance(a, torch.Tensor):
        t = a.to(dtype=torch.float64)
        return t.cuda(device) if not t.is_cuda else t
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 2 and a.flags.f_contiguous and not a.flags.c_contiguous:
        return torch.from_numpy(np.ascontiguousarray(a.T)).cuda(device).T
    return torch.from_numpy(np.ascontiguousarray(a)).cuda(device)


def to_device_index(a, device=None) -> torch.Tensor:
    _need_gpu()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).cuda(device)


def _layout(t: torch.Tensor):
    """(tensor, ld, layout) for a 2-D float64 CUDA tensor; copies only if it has no unit stride."""
    if t.dtype != torch.float64 or not t.is_cuda or t.dim() != 2:
        raise RomtimeHipError("expected a 2-D float64 CUDA tensor")
    r, c = t.shape
    s0, s1 = t.stride()
    if s1 == 1 and (s0 >= c or r == 1):
        return t, max(s0, c), ROW_MAJOR
    if s0 == 1 and (s1 >= r or c == 1):
        return t, max(s1, r), COL_MAJOR
    t = t.contiguous()
    return t, c, ROW_MAJOR


def gram(X: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """G = X^T X (n x n). rt_gram.  ``out``: optional contiguous n x n tensor to write into."""
    ctx = Context.current()
    X, ld, lay = _layout(X)
    N, n = X.shape
    G = out if out is not None else torch.empty((n, n), dtype=torch.float64, device=X.device)
    assert G.shape == (n, n) and G.is_contiguous()
    ctx.check(ctx.lib.rt_gram(ctx.handle, _ptr(X), N, n, ld, lay, _ptr(G)), "rt_gram")
    return G


def gram_scale(G: torch.Tensor, normalize: bool):
    """In place: returns (colnorm, status_flag tensor). rt_gram_scale."""
    ctx = Context.current()
    n = G.shape[0]
    assert G.is_contiguous() and G.shape == (n, n)
    colnorm = torch.empty(n, dtype=torch.float64, device=G.device)
    flag = torch.zeros(1, dtype=torch.int32, device=G.device)
    ctx.check(ctx.lib.rt_gram_scale(ctx.handle, _ptr(G), n, _ptr(colnorm), int(bool(normalize)), _ptr(flag)),
              "rt_gram_scale")
    return colnorm, flag


def pod_orth(X: torch.Tensor, num=None, tol=None, normalize=True, q_cols=None):
    """The composite C entry point rt_pod_orth (the whole of pod.py:7-62 in one call): returns
    ``(Q[:, :r] device, s host, energy host, levels)``.  The Python drop-in ``orth`` uses ``pod.pod_device`` instead (it
    overlaps the eigenvalue fetch with the back-projection and handles process groups); this wrapper exists for parity
    tests of what a non-Python host gets."""
    ctx = Context.current()
    X, ld, lay = _layout(X)
    N, n = X.shape
    cap = int(q_cols) if q_cols is not None else (int(min(num, n)) if (num and not tol) else min(N, n))
    Q = torch.empty((N, max(cap, 1)), dtype=torch.float64, device=X.device)
    length = min(N, n)
    s, energy = np.empty(length), np.empty(length)
    r, levels = C.c_int64(0), C.c_int(0)
    rc = ctx.lib.rt_pod_orth(ctx.handle, _ptr(X), N, n, ld, lay, int(num or 0), float(tol or 0.0), int(bool(normalize)),
                             _ptr(Q), cap, C.byref(r), s.ctypes.data, energy.ctypes.data, C.byref(levels))
    if rc == _lib.WARN_ZERO_NORM:
        raise pod_rules.zero_norm_error()
    ctx.check(rc, "rt_pod_orth")
    return Q[:, : r.value], s, energy, levels.value


def backproject_weights(Z: torch.Tensor, lam: torch.Tensor, colnorm: torch.Tensor = None) -> torch.Tensor:
    """D^-1 Z S^-1 (n x k) from the device eigenvalues ``lam`` (first k used).  rt_pod_backproject_weights."""
    ctx = Context.current()
    Z = Z.contiguous()
    n, k = Z.shape
    out = torch.empty_like(Z)
    ctx.check(ctx.lib.rt_pod_backproject_weights(ctx.handle, _ptr(Z), n, k, _ptr(colnorm), _ptr(lam), _ptr(out)),
              "rt_pod_backproject_weights")
    return out


def gemm_tn(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """C = A^T B with the contraction over the rows (DoFs). rt_gemm_tn."""
    ctx = Context.current()
    if B.dim() == 1:
        return gemm_tn(A, B.unsqueeze(1)).squeeze(1)
    same = A is B
    A, lda, la = _layout(A)
    if same:
        B, ldb, lb = A, lda, la
    else:
        B, ldb, lb = _layout(B)
    N, m = A.shape
    N2, n = B.shape
    if N != N2:
        raise RomtimeHipError(f"gemm_tn: row counts differ ({N} vs {N2})")
    Cm = torch.empty((m, n), dtype=torch.float64, device=A.device)
    ctx.check(ctx.lib.rt_gemm_tn(ctx.handle, _ptr(A), lda, la, _ptr(B), ldb, lb, N, m, n, _ptr(Cm), n), "rt_gemm_tn")
    return Cm


def gemm_nn(X: torch.Tensor, T: torch.Tensor, out: torch.Tensor = None, alpha: float = 1.0, beta: float = 0.0) -> torch.Tensor:
    """Y = X T (N x k, row-major), or ``out = beta out + alpha X T`` in place (``out``: N x k with unit column
    stride).  rt_gemm_nn / rt_gemm_nn_axpby."""
    ctx = Context.current()
    if T.dim() == 1:
        assert out is None
        return gemm_nn(X, T.unsqueeze(1)).squeeze(1)
    X, ldx, lx = _layout(X)
    T = T.contiguous()
    N, n = X.shape
    n2, k = T.shape
    if n != n2:
        raise RomtimeHipError(f"gemm_nn: inner dimensions differ ({n} vs {n2})")
    if out is None:
        if beta != 0.0:
            raise RomtimeHipError("gemm_nn: beta != 0 needs an output to accumulate into")
        Y, ldy, ly = torch.empty((N, k), dtype=torch.float64, device=X.device), k, ROW_MAJOR
    else:
        Y, ldy, ly = _layout(out)
        if Y is not out or tuple(out.shape) != (N, k):
            raise RomtimeHipError("gemm_nn: `out` must be an N x k float64 CUDA tensor with a unit stride")
    ctx.check(ctx.lib.rt_gemm_nn_axpby(ctx.handle, _ptr(X), ldx, lx, _ptr(T), k, N, n, k, float(alpha), float(beta),
                                       _ptr(Y), ldy, ly), "rt_gemm_nn_axpby")
    return Y


def _layout_last2(t: torch.Tensor):
    """(ld, layout) of the trailing two dimensions of a float64 CUDA tensor, or None where neither has unit stride."""
    r, c = t.shape[-2:]
    s0, s1 = t.stride()[-2:]
    if s1 == 1 and (s0 >= c or r == 1):
        return max(s0, c), ROW_MAJOR
    if s0 == 1 and (s1 >= r or c == 1):
        return max(s1, r), COL_MAJOR
    return None


def trajectory_errors(B: torch.Tensor, A: torch.Tensor, U: torch.Tensor = None, want_ref: bool = False):
    """err[j, t] = ||U_j[:, t] - B A_j[t, :]||_2 / sqrt(N) without storing the lifted trajectories B A_j^T
    (rt_trajectory_errors).  B: N x k basis (k <= 128); A: (nt, k) or (n, nt, k) coefficients, as the sweeps return
    them; U: None (then err = ||B A_j[t]|| / sqrt(N), the estimator), an N x nt matrix or (n, N, nt), either memory
    order.  Returns err (n, nt), and with ``want_ref`` also ref[j, t] = ||U_j[:, t]||_2 / sqrt(N)."""
    ctx = Context.current()
    for name, t in (("B", B), ("A", A), ("U", U)):
        if t is not None and (t.dtype != torch.float64 or not t.is_cuda):
            raise RomtimeHipError(f"trajectory_errors: {name} must be a float64 CUDA tensor")
    if B.dim() != 2 or A.dim() not in (2, 3) or (U is not None and U.dim() not in (2, 3)):
        raise RomtimeHipError("trajectory_errors: B must be 2-D, A and U 2-D or 3-D")
    if want_ref and U is None:
        raise RomtimeHipError("trajectory_errors: the reference norms are those of U")
    if A.dim() == 2:
        A = A.unsqueeze(0)
    if U is not None and U.dim() == 2:
        U = U.unsqueeze(0)
    N, k = B.shape
    n, nt, k2 = A.shape
    if k2 != k or (U is not None and tuple(U.shape) != (n, N, nt)):
        raise RomtimeHipError(f"trajectory_errors: shapes do not match (B {tuple(B.shape)}, A {tuple(A.shape)}, "
                              f"U {None if U is None else tuple(U.shape)})")
    if _layout_last2(B) is None or _layout_last2(B)[1] != ROW_MAJOR:
        B = B.contiguous()
    if _layout_last2(A) is None or _layout_last2(A)[1] != ROW_MAJOR:
        A = A.contiguous()
    ldb, lda = _layout_last2(B)[0], _layout_last2(A)[0]
    ldu, lu, su = 0, ROW_MAJOR, 0
    if U is not None:
        if _layout_last2(U) is None:
            U = U.contiguous()
        (ldu, lu), su = _layout_last2(U), U.stride(0)
    err = torch.empty((n, nt), dtype=torch.float64, device=B.device)
    ref = torch.empty((n, nt), dtype=torch.float64, device=B.device) if want_ref else None
    ctx.check(ctx.lib.rt_trajectory_errors(ctx.handle, _ptr(B), ldb, _ptr(A), lda, A.stride(0), _ptr(U), ldu, lu, su, N, k, nt,
                                           n, _ptr(err), _ptr(ref)), "rt_trajectory_errors")
    return (err, ref) if want_ref else err


FN_KINDS = dict(power=0)       # RT_FN_*


def trajectory_integrals(E: torch.Tensor, A: torch.Tensor, w: torch.Tensor = None, scale: torch.Tensor = None,
                         fn=("power", 0.0, 1.0, 1.0)) -> torch.Tensor:
    """out[j, t] = scale[j, t] * sum_i w[i] f(E[i, :] . A_j[t, :]) without storing the lifted trajectories E A_j^T
    (rt_trajectory_integrals).  E: n_pts x k basis at the quadrature points (k <= 128); A: (nt, k) or (n, nt, k)
    coefficients, as the sweeps return them; w: n_pts weights or None (1); scale: (n, nt) (or (nt,) for one trajectory) or
    None (1); fn: ("power", c0, c1, p) for f(z) = (c0 + c1 z)^p.  Returns (n, nt)."""
    ctx = Context.current()
    for name, t in (("E", E), ("A", A), ("w", w), ("scale", scale)):
        if t is not None and (t.dtype != torch.float64 or not t.is_cuda):
            raise RomtimeHipError(f"trajectory_integrals: {name} must be a float64 CUDA tensor")
    if E.dim() != 2 or A.dim() not in (2, 3):
        raise RomtimeHipError("trajectory_integrals: E must be 2-D, A 2-D or 3-D")
    if len(fn) != 4 or fn[0] not in FN_KINDS:
        raise RomtimeHipError(f"trajectory_integrals: fn must be ('power', c0, c1, p), not {fn!r}")
    if A.dim() == 2:
        A = A.unsqueeze(0)
    n_pts, k = E.shape
    n, nt, k2 = A.shape
    if scale is not None and scale.dim() == 1 and n == 1:
        scale = scale.unsqueeze(0)
    if k2 != k or (w is not None and tuple(w.shape) != (n_pts,)) or (scale is not None and tuple(scale.shape) != (n, nt)):
        raise RomtimeHipError(f"trajectory_integrals: shapes do not match (E {tuple(E.shape)}, A {tuple(A.shape)}, "
                              f"w {None if w is None else tuple(w.shape)}, scale {None if scale is None else tuple(scale.shape)})")
    if _layout_last2(E) is None or _layout_last2(E)[1] != ROW_MAJOR:
        E = E.contiguous()
    if _layout_last2(A) is None or _layout_last2(A)[1] != ROW_MAJOR:
        A = A.contiguous()
    lde, lda = _layout_last2(E)[0], _layout_last2(A)[0]
    w = None if w is None else w.contiguous()
    scale = None if scale is None else scale.contiguous()
    par = (C.c_double * 3)(float(fn[1]), float(fn[2]), float(fn[3]))
    out = torch.empty((n, nt), dtype=torch.float64, device=E.device)
    ctx.check(ctx.lib.rt_trajectory_integrals(ctx.handle, _ptr(E), lde, _ptr(w), _ptr(A), lda, A.stride(0), _ptr(scale), n_pts, k,
                                              nt, n, FN_KINDS[fn[0]], par, _ptr(out)), "rt_trajectory_integrals")
    return out


def interpolation_errors(Psi: torch.Tensor, idx, F: torch.Tensor, group: int = 1, pin=None, want_ref: bool = False):
    """err[q] = mean over the ``group`` snapshots s = q group + i of ||F[:, s] - I(F[:, s])||_2 / sqrt(N), with
    I(f) = Psi f[idx] (rt_interpolation_errors): the (M)DEIM interpolation error of every snapshot of a block, neither
    thetas nor interpolants stored.  Psi: N x m (m <= 128), the basis with the theta solve folded in
    (``interpolation.fold``); idx: m flat indices on the host, each in [0, N); F: N x S snapshots, either memory order;
    pin: None or (row, value), the entry of the interpolant that is replaced by a constant (MDEIM's Dirichlet entry).
    Returns err (S / group,), and with ``want_ref`` also the same mean of ||F[:, s]||_2 / sqrt(N)."""
    ctx = Context.current()
    for name, t in (("Psi", Psi), ("F", F)):
        if t.dtype != torch.float64 or not t.is_cuda or t.dim() != 2:
            raise RomtimeHipError(f"interpolation_errors: {name} must be a 2-D float64 CUDA tensor")
    N, m = Psi.shape
    S = F.shape[1]
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    group = int(group)
    if F.shape[0] != N or idx.size != m or group < 1 or S % group:
        raise RomtimeHipError(f"interpolation_errors: shapes do not match (Psi {tuple(Psi.shape)}, idx {idx.size}, "
                              f"F {tuple(F.shape)}, group {group})")
    if _layout_last2(Psi) is None or _layout_last2(Psi)[1] != ROW_MAJOR:
        Psi = Psi.contiguous()
    if _layout_last2(F) is None:
        F = F.contiguous()
    ldpsi, (ldf, lf) = _layout_last2(Psi)[0], _layout_last2(F)
    pin_row, pin_value = (-1, 0.0) if pin is None else (int(pin[0]), float(pin[1]))
    if pin is not None and not 0 <= pin_row < N:
        raise RomtimeHipError(f"interpolation_errors: pinned row {pin_row} outside [0, {N})")
    err = torch.empty(S // group, dtype=torch.float64, device=Psi.device)
    ref = torch.empty(S // group, dtype=torch.float64, device=Psi.device) if want_ref else None
    ctx.check(ctx.lib.rt_interpolation_errors(ctx.handle, _ptr(Psi), ldpsi, idx.ctypes.data_as(C.POINTER(C.c_int64)), m, _ptr(F),
                                              ldf, lf, N, S, group, pin_row, pin_value, _ptr(err), _ptr(ref)),
              "rt_interpolation_errors")
    return (err, ref) if want_ref else err


def rank_update(Ysrc: torch.Tensor, X: torch.Tensor, T: torch.Tensor, alpha: float = -1.0, colscale: torch.Tensor = None,
                out: torch.Tensor = None) -> torch.Tensor:
    """``out = Ysrc diag(colscale) + alpha X T`` for a tall row-major Ysrc (N x n), thin X (N x k) and T (k x n);
    ``out`` may be Ysrc itself.  k <= 64 runs the streaming kernel (rt_rank_update), larger k the GEMM epilogue."""
    ctx = Context.current()
    N, n = Ysrc.shape
    k = X.shape[1]
    if tuple(T.shape) != (k, n) or X.shape[0] != N:
        raise RomtimeHipError("rank_update: shapes do not match")
    row_major = all(t.is_contiguous() or (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) for t in (Ysrc, X))
    if k > 64 or not row_major or (out is not None and not out.is_contiguous()):
        base = Ysrc * colscale[None, :] if colscale is not None else Ysrc
        out = base.clone() if (out is None and base is Ysrc) else (base if out is None else out.copy_(base))
        return gemm_nn(X, T, out=out, alpha=alpha, beta=1.0)
    T = T.contiguous()
    if out is None:
        out = torch.empty((N, n), dtype=torch.float64, device=Ysrc.device)
    ctx.check(ctx.lib.rt_rank_update(ctx.handle, _ptr(Ysrc), Ysrc.stride(0), _ptr(colscale) if colscale is not None else None,
                                     _ptr(X), X.stride(0), _ptr(T), n, N, k, n, float(alpha), _ptr(out), out.stride(0)),
              "rt_rank_update")
    return out


def deim_greedy(Phi: torch.Tensor, want_margin: bool = True):
    """(idx int64[m], PT_U [m,m], margin [m] or None), all on the device. rt_deim_greedy."""
    ctx = Context.current()
    Phi, ld, lay = _layout(Phi)
    N, m = Phi.shape
    idx = torch.empty(m, dtype=torch.int64, device=Phi.device)
    PT_U = torch.empty((m, m), dtype=torch.float64, device=Phi.device)
    margin = torch.empty(m, dtype=torch.float64, device=Phi.device) if want_margin else None
    ctx.check(ctx.lib.rt_deim_greedy(ctx.handle, _ptr(Phi), N, m, ld, lay, _ptr(idx), _ptr(PT_U), _ptr(margin)),
              "rt_deim_greedy")
    return idx, PT_U, margin


def deim_oversample_step_plan(N: int, m: int, layout: int = ROW_MAJOR, ld: int = None):
    """(workgroups, rows per workgroup, lanes per row) of ``deim_oversample_step`` - host logic only, no GPU
    (rt_deim_oversample_step_plan_info); raises where the step would refuse the sizes."""
    lib = _lib.load()
    some = (C.c_double * 2)()   # the checks only see that the operands are there
    sp = C.cast(some, _p)
    ld = (int(N) if layout == COL_MAJOR else int(m)) if ld is None else int(ld)
    info3 = (C.c_int64 * 3)()
    rc = lib.rt_deim_oversample_step_plan_info(sp, int(N), int(m), ld, int(layout), sp, 1.0, sp, sp, sp, info3)
    if rc != 0:
        raise RomtimeHipError(f"rt_deim_oversample_step_plan_info failed ({rc}) for N = {N}, m = {m}, ld = {ld}")
    return int(info3[0]), int(info3[1]), int(info3[2])


def deim_oversample_step(Phi: torch.Tensor, w: torch.Tensor, g: float, taken: torch.Tensor, pick: torch.Tensor = None,
                         top2: torch.Tensor = None):
    """One GappyPOD+E selection step (rt_deim_oversample_step): ``(pick, top2)`` on the device and not waited for -
    pick (int64[1]) the row of Phi (N x m, either memory order, any leading dimension) with the largest score among
    the rows whose byte of ``taken`` (uint8[N]) is zero, -1 when there is none; top2 (float64[2]) the best score and the
    runner-up.  ``w`` (float64[m]) and ``g`` come from the SVD of the rows picked so far (``deim_oversample``)."""
    ctx = Context.current()
    Phi, ld, lay = _layout(Phi)
    N, m = Phi.shape
    if (w.dtype != torch.float64 or not w.is_cuda or tuple(w.shape) != (m,) or not w.is_contiguous()
            or taken.dtype != torch.uint8 or not taken.is_cuda or tuple(taken.shape) != (N,) or not taken.is_contiguous()):
        raise RomtimeHipError("deim_oversample_step: w must be a contiguous float64[m] and taken a contiguous uint8[N] CUDA tensor")
    pick = torch.empty(1, dtype=torch.int64, device=Phi.device) if pick is None else pick
    top2 = torch.empty(2, dtype=torch.float64, device=Phi.device) if top2 is None else top2
    ctx.check(ctx.lib.rt_deim_oversample_step(ctx.handle, _ptr(Phi), N, m, ld, lay, _ptr(w), float(g), _ptr(taken), _ptr(pick),
                                              _ptr(top2)), "rt_deim_oversample_step")
    return pick, top2


def oversample_direction(rows: np.ndarray):
    """(w, g, sigma) of the rows picked so far (len(p) x m, m >= 2, host): the right singular vector of the smallest
    singular value, the gap sigma_{m-1}^2 - sigma_m^2 formed as a product so that it cannot come out negative, and the
    singular values.  The one host step of ``deim_oversample``."""
    _, s, Vt = np.linalg.svd(rows, full_matrices=False)
    m = rows.shape[1]
    g = float((s[m - 2] - s[m - 1]) * (s[m - 2] + s[m - 1]))
    return np.ascontiguousarray(Vt[m - 1]), g, s


def deim_oversample(Phi: torch.Tensor, idx, m_s: int):
    """Oversampled (M)DEIM entries by GappyPOD+E (Peherstorfer, Drmac, Gugercin 2020): the m greedy indices ``idx`` of
    the basis Phi (N x m, m >= 2) are extended to m_s <= N, every new one the row that is certified to raise
    sigma_min(Phi[idx, :]) most.  Per added entry: the SVD of the rows gathered so far on the host (``oversample_direction``),
    one pass over Phi on the device (``deim_oversample_step``), the pick and its row read back, the byte mask updated
    on the device.  Returns ``(idx, PT_U, margin, sigma_min)``: idx (int64[m_s], device) whose first m entries are the
    input, PT_U = Phi[idx, :] (m_s x m, device), margin ((top1 - top2) / top1 of the scores per added entry, host) and
    sigma_min (host, m_s - m + 1 values: before the first addition and after each)."""
    _need_gpu()
    if Phi.dtype != torch.float64 or not Phi.is_cuda or Phi.dim() != 2:
        raise RomtimeHipError("deim_oversample: Phi must be a 2-D float64 CUDA tensor")
    N, m = Phi.shape
    idx = idx if isinstance(idx, torch.Tensor) else to_device_index(idx, Phi.device)
    idx = idx.to(device=Phi.device, dtype=torch.int64).reshape(-1)
    m_s = int(m_s)
    if idx.numel() != m or m < 2 or not m <= m_s <= N:
        raise RomtimeHipError(f"deim_oversample: need m >= 2 indices for the m = {m} modes and m <= m_s <= N "
                              f"(got {idx.numel()} indices, m_s = {m_s}, N = {N})")
    rows = np.empty((m_s, m))
    rows[:m] = Phi[idx, :].cpu().numpy()
    out_idx = np.empty(m_s, dtype=np.int64)
    out_idx[:m] = idx.cpu().numpy()
    taken = torch.zeros(N, dtype=torch.uint8, device=Phi.device)
    taken[idx] = 1
    pick = torch.empty(1, dtype=torch.int64, device=Phi.device)
    top2 = torch.empty(2, dtype=torch.float64, device=Phi.device)
    margin, sigma_min = np.zeros(m_s - m), np.empty(m_s - m + 1)
    for n in range(m, m_s):
        w, g, s = oversample_direction(rows[:n])
        sigma_min[n - m] = s[m - 1]
        deim_oversample_step(Phi, to_device(w, Phi.device), g, taken, pick, top2)
        p = int(pick.item())
        if p < 0:
            raise RomtimeHipError("deim_oversample: no free row left")
        t1, t2 = top2.cpu().numpy()
        margin[n - m] = (t1 - max(t2, 0.0)) / t1 if t1 > 0.0 else 0.0
        rows[n] = Phi[p, :].cpu().numpy()
        out_idx[n] = p
        taken[p] = 1
    sigma_min[m_s - m] = np.linalg.svd(rows, compute_uv=False)[m - 1]
    return to_device_index(out_idx, Phi.device), to_device(rows, Phi.device), margin, sigma_min


def csr_spmm(indptr, indices, data, V: torch.Tensor) -> torch.Tensor:
    ctx = Context.current()
    V = V.contiguous()
    N = indptr.numel() - 1
    r = V.shape[1]
    Y = torch.empty((N, r), dtype=torch.float64, device=V.device)
    ctx.check(ctx.lib.rt_csr_spmm(ctx.handle, _ptr(indptr), _ptr(indices), _ptr(data), N, _ptr(V), r, r, _ptr(Y), r),
              "rt_csr_spmm")
    return Y


def project_csr(indptr, indices, data, V: torch.Tensor) -> torch.Tensor:
    """A_N = V^T (A V). rt_project_csr."""
    ctx = Context.current()
    V = V.contiguous()
    N = indptr.numel() - 1
    if V.shape[0] != N:
        raise RomtimeHipError("project_csr: V has the wrong number of rows")
    r = V.shape[1]
    AN = torch.empty((r, r), dtype=torch.float64, device=V.device)
    ctx.check(ctx.lib.rt_project_csr(ctx.handle, _ptr(indptr), _ptr(indices), _ptr(data), N, _ptr(V), r, r, _ptr(AN)),
              "rt_project_csr")
    return AN


def project_csr_batched(indptr, indices, data_batch: torch.Tensor, V: torch.Tensor) -> torch.Tensor:
    """data_batch is (nnz x B) (modes as columns, either memory order) -> (B, r, r)."""
    ctx = Context.current()
    V = V.contiguous()
    data_batch, ld, lay = _layout(data_batch)
    nnz, B = data_batch.shape
    # C-ordered (nnz x B) vectors are read in place: a workgroup's entry loads then touch one 8-byte word per
    # 8 B-byte row, which the L2 absorbs (measured: same kernel time as contiguous vectors, and the transpose pass
    # that used to make them contiguous cost 0.25 ms at 5e5 x 120)
    N = indptr.numel() - 1
    r = V.shape[1]
    AN = torch.empty((B, r, r), dtype=torch.float64, device=V.device)
    ctx.check(ctx.lib.rt_project_csr_batched(ctx.handle, _ptr(indptr), _ptr(indices), _ptr(data_batch), ld, lay, B, N,
                                             _ptr(V), r, r, _ptr(AN)), "rt_project_csr_batched")
    return AN


def project_stage_info(indptr, indices):
    """The stage table the fused projection reads for this pattern (device index tensors), read back:
    (records, any_unwindowed) with records an int64 array [stages][6] = (e0, lo, ne, nrow, mr, uni) per stage of 32 rows;
    nrow = 0 marks a stage that is not windowed.  rt_project_stage_info; synchronises the stream."""
    ctx = Context.current()
    N = indptr.numel() - 1
    records = np.zeros(((N + 31) // 32, 6), dtype=np.int64)
    any_unwindowed = C.c_int(0)
    ctx.check(ctx.lib.rt_project_stage_info(ctx.handle, _ptr(indptr), _ptr(indices), N,
                                            records.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(any_unwindowed)),
              "rt_project_stage_info")
    return records, bool(any_unwindowed.value)


def dense_solve(K: torch.Tensor, b: torch.Tensor):
    """Solve K x = b (K: [r,r] or [B,r,r]; b: [r] or [B,r]). Returns (x, info). Inputs are not modified."""
    ctx = Context.current()
    single = K.dim() == 2
    Kw = K.reshape(-1, K.shape[-2], K.shape[-1]).contiguous().clone()
    bw = b.reshape(Kw.shape[0], -1).contiguous().clone()
    B, r, _ = Kw.shape
    info = torch.zeros(B, dtype=torch.int32, device=K.device)
    ctx.check(ctx.lib.rt_dense_solve_batched(ctx.handle, _ptr(Kw), _ptr(bw), r, B, _ptr(info)),
              "rt_dense_solve_batched")
    return (bw[0] if single else bw), info


def gmres_solve(K: torch.Tensor, b: torch.Tensor, opts=None):
    """``scipy.sparse.linalg.gmres(K, b, **opts)`` on the device (rt_gmres_batched): restarted GMRES from x0 = 0 with
    SciPy's stopping decisions, for K [r,r] or [B,r,r] (r <= 128) and b [r] or [B,r].  ``opts``: SciPy's keywords as
    ``romtime_amd.gmres.gmres_opts`` reads them (None: SciPy's defaults).  Returns (x, info, iters) - SciPy's info (0, or
    maxiter when the tolerance was not met) and the inner iterations per system, scalars for a single system.  Inputs
    are not modified."""
    from .gmres import gmres_opts

    ctx = Context.current()
    single = K.dim() == 2
    Kw = K.reshape(-1, K.shape[-2], K.shape[-1]).contiguous()
    bw = b.reshape(Kw.shape[0], -1).contiguous()
    B, r, c = Kw.shape
    if c != r or bw.shape[1] != r or Kw.dtype != torch.float64 or bw.dtype != torch.float64:
        raise RomtimeHipError("gmres_solve: K must be float64 [r,r] / [B,r,r] and b float64 [r] / [B,r]")
    o = gmres_opts(opts, r)
    x = torch.empty_like(bw)
    info = torch.empty(B, dtype=torch.int64, device=K.device)
    iters = torch.empty(B, dtype=torch.int32, device=K.device)
    ctx.check(ctx.lib.rt_gmres_batched(ctx.handle, _ptr(Kw), _ptr(bw), _ptr(x), r, B, C.byref(o), _ptr(info), _ptr(iters)),
              "rt_gmres_batched")
    return (x[0], info[0], iters[0]) if single else (x, info, iters)


def dense_solve_multi(K: torch.Tensor, B: torch.Tensor):
    """X with K X = B for an r x r matrix (r <= 128) and r x nrhs right-hand sides.  Returns (X, info).
    rt_dense_solve_multi."""
    ctx = Context.current()
    K, B = K.contiguous(), B.contiguous()
    r, nrhs = B.shape
    if tuple(K.shape) != (r, r):
        raise RomtimeHipError("dense_solve_multi: K must be r x r and B r x nrhs")
    X = torch.empty_like(B)
    info = torch.zeros(1, dtype=torch.int32, device=K.device)
    ctx.check(ctx.lib.rt_dense_solve_multi(ctx.handle, _ptr(K), r, _ptr(B), _ptr(X), nrhs, _ptr(info)), "rt_dense_solve_multi")
    return X, info


def dense_lstsq_plan(rows: int, cols: int, nrhs: int = 1, trans: int = 0):
    """(workgroups, right-hand sides per workgroup, LDS bytes) of ``dense_lstsq_multi`` - host logic only, no GPU
    (rt_dense_lstsq_multi_plan_info); raises where the solve would refuse the sizes."""
    lib = _lib.load()
    some = (C.c_double * 4)()   # the checks only see that the operands are there and distinct
    info3 = (C.c_int64 * 3)()
    rc = lib.rt_dense_lstsq_multi_plan_info(C.cast(some, _p), int(rows), int(cols), int(trans), _p(C.addressof(some) + 8),
                                            _p(C.addressof(some) + 16), int(nrhs), info3)
    if rc != 0:
        raise RomtimeHipError(f"rt_dense_lstsq_multi_plan_info failed ({rc}) for rows = {rows}, cols = {cols}, nrhs = {nrhs}")
    return int(info3[0]), int(info3[1]), int(info3[2])


def dense_lstsq_multi(A: torch.Tensor, B: torch.Tensor, trans: bool = False):
    """Least squares against one rows x cols matrix A (rows >= cols; cols <= 128, rows <= 256) by Householder QR
    (rt_dense_lstsq_multi).  ``trans`` False: X (cols x nrhs) minimises ||A X - B|| column by column, B rows x nrhs;
    ``trans`` True: X (rows x nrhs) is the minimum-norm solution of A^T X = B, B cols x nrhs - X = pinv(A)^T B.
    Returns (X, info); info is RT_WARN_SINGULAR where R has an exactly zero diagonal entry.  Inputs are not modified."""
    ctx = Context.current()
    A, B = A.contiguous(), B.contiguous()
    if A.dim() != 2 or B.dim() != 2 or A.dtype != torch.float64 or B.dtype != torch.float64:
        raise RomtimeHipError("dense_lstsq_multi: A and B must be 2-D float64 CUDA tensors")
    rows, cols = A.shape
    nrhs = B.shape[1]
    if B.shape[0] != (cols if trans else rows):
        raise RomtimeHipError(f"dense_lstsq_multi: B must have {cols if trans else rows} rows for A {tuple(A.shape)}, "
                              f"trans = {bool(trans)}")
    X = torch.empty((rows if trans else cols, nrhs), dtype=torch.float64, device=A.device)
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    ctx.check(ctx.lib.rt_dense_lstsq_multi(ctx.handle, _ptr(A), rows, cols, int(bool(trans)), _ptr(B), _ptr(X), nrhs, _ptr(info)),
              "rt_dense_lstsq_multi")
    return X, info


def pod_enqueue(X: torch.Tensor, k: int, normalize: bool):
    """One single-pass POD enqueued on the ctx stream with ONE host call (rt_pod_enqueue): returns the device tensors
    (Q, lam, status2, colnorm) and a tuple of the work buffers to keep alive until the stream has run them."""
    ctx = Context.current()
    X, ld, lay = _layout(X)
    N, n = X.shape
    dev = X.device
    work = torch.empty(n * n + 2 * n + 2 * n * k, dtype=torch.float64, device=dev)
    G, colnorm, lam = work[: n * n].view(n, n), work[n * n: n * n + n], work[n * n + n: n * n + 2 * n]
    Z, Zs = work[n * n + 2 * n: n * n + 2 * n + n * k].view(n, k), work[n * n + 2 * n + n * k:].view(n, k)
    status2 = torch.empty(2, dtype=torch.int32, device=dev)
    Q = torch.empty((N, k), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.rt_pod_enqueue(ctx.handle, _ptr(X), N, n, ld, lay, k, int(bool(normalize)), _ptr(G), _ptr(colnorm),
                                     _ptr(lam), _ptr(status2), _ptr(Z), _ptr(Zs), _ptr(Q)), "rt_pod_enqueue")
    return Q, lam, status2, colnorm, (work, X)


def tracked_solve(K: torch.Tensor, b: torch.Tensor, Xinv: torch.Tensor = None):
    """Solve K x = b for a batch ([B,r,r], [B,r]) with the inverse tracked in ``Xinv`` ([B,r,r], carried from call to
    call; None = first call).  Returns (x, info, Xinv).  rt_tracked_solve_batched (r <= 80)."""
    ctx = Context.current()
    Kw = K.reshape(-1, K.shape[-2], K.shape[-1]).contiguous()
    bw = b.reshape(Kw.shape[0], -1).contiguous().clone()
    B, r, _ = Kw.shape
    have_prev = Xinv is not None
    if Xinv is None:
        Xinv = torch.zeros_like(Kw)
    info = torch.zeros(B, dtype=torch.int32, device=K.device)
    ctx.check(ctx.lib.rt_tracked_solve_batched(ctx.handle, _ptr(Kw), _ptr(Xinv), _ptr(bw), r, B, int(have_prev), _ptr(info)),
              "rt_tracked_solve_batched")
    return bw, info, Xinv


P1_KINDS = dict(mass=0, stiffness=1, convection=2, trilinear=3, load=4, load_p2=5)


def p1_local_assembly(kind: str, nx: int, rows, cols, h, coef=None, state=None, ramp=None, poly=None) -> torch.Tensor:
    """Closed-form 1-D P1 operator values at the entries (rows[e], cols[e]) for every state: (n_states, m) table.
    ``h`` (n_states) cell sizes, ``coef`` (n_states) optional factors, ``state`` (n_states, nx + 1) nodal values or
    ``ramp`` (n_states) amplitudes of amp * node / nx for the trilinear / load kinds.  ``load_p2`` (the exact integral
    of degree-2 data, fom/heat.py:119): ``state`` is (n_states, 2 nx + 1) vertex / midpoint values, or ``poly``
    (n_states, 3) the coefficients of a0 + a1 x + a2 x^2 in the physical coordinate.  rt_p1_local_assembly."""
    ctx = Context.current()
    rows = rows if isinstance(rows, torch.Tensor) else to_device_index(rows)
    cols = None if cols is None else (cols if isinstance(cols, torch.Tensor) else to_device_index(cols))
    h = to_device(np.atleast_1d(h) if not isinstance(h, torch.Tensor) else h).contiguous()
    n_states, m = h.numel(), rows.numel()
    coef = None if coef is None else to_device(np.atleast_1d(coef) if not isinstance(coef, torch.Tensor) else coef).contiguous()
    mode, st = 0, None
    if state is not None:
        st = to_device(state).contiguous()
        width = 2 * nx + 1 if kind == "load_p2" else nx + 1
        if tuple(st.shape) != (n_states, width):
            raise RomtimeHipError(f"p1_local_assembly: `state` must be (n_states, {width}) for kind {kind!r}")
        mode = 1
    elif ramp is not None:
        st = to_device(np.atleast_1d(ramp) if not isinstance(ramp, torch.Tensor) else ramp).contiguous()
        mode = 2
    elif poly is not None:
        st = to_device(poly).contiguous()
        if tuple(st.shape) != (n_states, 3):
            raise RomtimeHipError("p1_local_assembly: `poly` must be (n_states, 3)")
        mode = 3
    out = torch.empty((n_states, m), dtype=torch.float64, device=h.device)
    ctx.check(ctx.lib.rt_p1_local_assembly(ctx.handle, P1_KINDS[kind], int(nx), _ptr(rows), _ptr(cols), m, n_states, _ptr(h),
                                           _ptr(coef), mode, _ptr(st), _ptr(out)), "rt_p1_local_assembly")
    return out


def p1_snapshot_sets(kind: str, nx: int, rows, cols, h, coef=None, ramp=None, poly=None, fun=None, zero_first: bool = False,
                     out: torch.Tensor = None, beta: float = 0.0) -> torch.Tensor:
    """Closed-form 1-D P1 operator values over a product grid: the (n_par * n_fun, m) table whose row ``p * n_fun + f`` is
    the operator of parameter row p - ``h`` (n_par) cell sizes, ``coef`` (n_par) optional factors, ``ramp`` (n_par)
    amplitudes or ``poly`` (n_par, 3) coefficients as in ``p1_local_assembly`` - and nodal function f of ``fun`` (n_fun,
    nx + 1; (n_fun, 2 nx + 1) for ``load_p2``), shared by every parameter row.  Exactly one of ``ramp`` / ``poly`` / ``fun``
    for the trilinear and load kinds, none for the others.  Its ``.T`` is the column-major m x S snapshot set the POD
    takes; values are bit for bit those of ``p1_local_assembly``.  ``zero_first``: entry 0 of every column is 0 (the MDEIM
    convention).  ``out``, ``beta``: the result is ``beta * out + table`` written into ``out`` (beta = 0 does not read it).
    rt_p1_snapshot_sets."""
    ctx = Context.current()
    rows = rows if isinstance(rows, torch.Tensor) else to_device_index(rows)
    cols = None if cols is None else (cols if isinstance(cols, torch.Tensor) else to_device_index(cols))
    h = to_device(np.atleast_1d(h) if not isinstance(h, torch.Tensor) else h).contiguous().reshape(-1)
    n_par, m = h.numel(), rows.numel()
    coef = None if coef is None else to_device(np.atleast_1d(coef) if not isinstance(coef, torch.Tensor) else coef).contiguous()
    if coef is not None and coef.numel() != n_par:
        raise RomtimeHipError("p1_snapshot_sets: `coef` must have one value per parameter row")
    mode, par, n_fun, fn = 0, None, 1, None
    if ramp is not None:
        par = to_device(np.atleast_1d(ramp) if not isinstance(ramp, torch.Tensor) else ramp).contiguous()
        if par.numel() != n_par:
            raise RomtimeHipError("p1_snapshot_sets: `ramp` must have one amplitude per parameter row")
        mode = 2
    if poly is not None:
        if par is not None:
            raise RomtimeHipError("p1_snapshot_sets: `ramp` and `poly` exclude each other")
        par = to_device(poly).contiguous()
        if tuple(par.shape) != (n_par, 3):
            raise RomtimeHipError("p1_snapshot_sets: `poly` must be (n_par, 3)")
        mode = 3
    if fun is not None:
        fn = to_device(fun).contiguous()
        width = 2 * nx + 1 if kind == "load_p2" else nx + 1
        if fn.dim() != 2 or fn.shape[1] != width or fn.shape[0] < 1:
            raise RomtimeHipError(f"p1_snapshot_sets: `fun` must be (n_fun, {width}) for kind {kind!r}")
        n_fun = int(fn.shape[0])
    if out is None:
        if beta != 0.0:
            raise RomtimeHipError("p1_snapshot_sets: beta != 0 needs `out`")
        out = torch.empty((n_par * n_fun, m), dtype=torch.float64, device=h.device)
    elif tuple(out.shape) != (n_par * n_fun, m) or out.dtype != torch.float64 or not out.is_contiguous():
        raise RomtimeHipError(f"p1_snapshot_sets: `out` must be a contiguous float64 ({n_par * n_fun}, {m}) tensor")
    ctx.check(ctx.lib.rt_p1_snapshot_sets(ctx.handle, P1_KINDS[kind], int(nx), _ptr(rows), _ptr(cols), m, n_par, _ptr(h), _ptr(coef),
                                          mode, _ptr(par), n_fun, _ptr(fn), int(bool(zero_first)), float(beta), _ptr(out)),
              "rt_p1_snapshot_sets")
    return out


def p1_fom_plan(nx: int, n_mu: int = 1, nt: int = 1, num_cus: int = 256):
    """(workgroups, partitions per system, rows per partition) of ``p1_fom_bdf_sweep`` for nx cells - host logic only,
    no GPU (rt_p1_fom_bdf_sweep_plan_info); raises where the sweep would refuse the sizes."""
    lib = _lib.load()
    Nh = int(nx) + 1
    tab = (C.c_double * 7)()   # the checks only see that the table is there
    desc = _lib.FomDesc(int(nx), int(n_mu), int(nt), 0, 1.0, 0, 0, C.cast(tab, _p), None)
    info3 = (C.c_int64 * 3)()
    rc = lib.rt_p1_fom_bdf_sweep_plan_info(int(num_cus), C.byref(desc), Nh, int(nt) * Nh, info3)
    if rc != 0:
        raise RomtimeHipError(f"rt_p1_fom_bdf_sweep_plan_info failed ({rc}) for nx = {nx}, n_mu = {n_mu}, nt = {nt}")
    return int(info3[0]), int(info3[1]), int(info3[2])


def p1_fom_bdf_sweep(nx: int, tab, dt: float, bdf2: bool, state_in_w: bool, u_init: torch.Tensor = None, first_step: int = 0):
    """Full-order BDF sweep of a closed-form 1-D P1 model for every parameter point of ``tab`` (nt, n_mu, 7: h, alpha, c0,
    c1, a0, a1, a2 per step and point; ``MockHeatEquation.p1_fom_recipe`` / ``MockBurgers.p1_fom_recipe``), the whole
    time loop in one launch.  ``u_init`` (n_mu, 2, nx + 1): u^n and u^{n-1} of a sweep continued at global step
    ``first_step``; None = zero initial state.  Returns ``(U, info)``: U (n_mu, nt, nx + 1) homogeneous snapshots - every
    ``U[j].T`` the N_h x nt column-major snapshot matrix the POD and ``trajectory_errors`` take - and info (n_mu int32): 0,
    or 1 + the global step at which a row lost diagonal dominance or a pivot was not finite.  rt_p1_fom_bdf_sweep."""
    ctx = Context.current()
    tab = to_device(tab).contiguous()
    if tab.dim() != 3 or tab.shape[2] != 7:
        raise RomtimeHipError("p1_fom_bdf_sweep: `tab` must be (nt, n_mu, 7)")
    nt, n_mu, Nh = int(tab.shape[0]), int(tab.shape[1]), int(nx) + 1
    if u_init is not None:
        u_init = to_device(u_init).contiguous()
        if tuple(u_init.shape) != (n_mu, 2, Nh):
            raise RomtimeHipError(f"p1_fom_bdf_sweep: `u_init` must be (n_mu, 2, {Nh})")
    out = torch.empty((n_mu, nt, Nh), dtype=torch.float64, device=tab.device)
    info = torch.empty(n_mu, dtype=torch.int32, device=tab.device)
    desc = _lib.FomDesc(int(nx), n_mu, nt, int(first_step), float(dt), int(bool(bdf2)), int(bool(state_in_w)), _ptr(tab),
                        _ptr(u_init))
    ctx.check(ctx.lib.rt_p1_fom_bdf_sweep(ctx.handle, C.byref(desc), _ptr(out), Nh, nt * Nh, _ptr(info)),
              "rt_p1_fom_bdf_sweep")
    return out, info


def p1_fom_plan_info_certified(nx: int, n_mu: int = 1, nt: int = 1, num_cus: int = 256):
    """(workgroups, partitions per system, rows per partition, scratch bytes per point) of
    ``p1_fom_bdf_sweep_certified`` - the twin of ``p1_fom_plan``, host logic only
    (rt_p1_fom_bdf_sweep_certified_plan_info)."""
    lib = _lib.load()
    Nh = int(nx) + 1
    tab = (C.c_double * 7)()   # the checks only see that the table is there
    desc = _lib.FomDesc(int(nx), int(n_mu), int(nt), 0, 1.0, 0, 0, C.cast(tab, _p), None)
    info4 = (C.c_int64 * 4)()
    rc = lib.rt_p1_fom_bdf_sweep_certified_plan_info(int(num_cus), C.byref(desc), Nh, int(nt) * Nh, info4)
    if rc != 0:
        raise RomtimeHipError(f"rt_p1_fom_bdf_sweep_certified_plan_info failed ({rc}) for nx = {nx}, n_mu = {n_mu}, nt = {nt}")
    return int(info4[0]), int(info4[1]), int(info4[2]), int(info4[3])


def p1_fom_bdf_sweep_certified(nx: int, tab, dt: float, bdf2: bool, state_in_w: bool, u_init: torch.Tensor = None,
                               first_step: int = 0, defect_tol: float = 1e-10):
    """``p1_fom_bdf_sweep`` - the same solve, the same bits in U - certified by the backward error of every step instead of
    by diagonal dominance.  Returns ``(U, info, defect)``: defect (n_mu, nt) float64, the componentwise backward error of
    every step's solve (+inf where a pivot or a state value was not finite), and info (n_mu int32): 0, or 1 + the global
    step of the first defect that is not finite or above ``defect_tol``.  rt_p1_fom_bdf_sweep_certified."""
    ctx = Context.current()
    tab = to_device(tab).contiguous()
    if tab.dim() != 3 or tab.shape[2] != 7:
        raise RomtimeHipError("p1_fom_bdf_sweep_certified: `tab` must be (nt, n_mu, 7)")
    nt, n_mu, Nh = int(tab.shape[0]), int(tab.shape[1]), int(nx) + 1
    if u_init is not None:
        u_init = to_device(u_init).contiguous()
        if tuple(u_init.shape) != (n_mu, 2, Nh):
            raise RomtimeHipError(f"p1_fom_bdf_sweep_certified: `u_init` must be (n_mu, 2, {Nh})")
    out = torch.empty((n_mu, nt, Nh), dtype=torch.float64, device=tab.device)
    info = torch.empty(n_mu, dtype=torch.int32, device=tab.device)
    defect = torch.empty((n_mu, nt), dtype=torch.float64, device=tab.device)
    desc = _lib.FomDesc(int(nx), n_mu, nt, int(first_step), float(dt), int(bool(bdf2)), int(bool(state_in_w)), _ptr(tab),
                        _ptr(u_init))
    ctx.check(ctx.lib.rt_p1_fom_bdf_sweep_certified(ctx.handle, C.byref(desc), _ptr(out), Nh, nt * Nh, float(defect_tol),
                                                    _ptr(defect), _ptr(info)), "rt_p1_fom_bdf_sweep_certified")
    return out, info, defect


def trajectory_residuals_plan(nx: int, k: int = 1, nt: int = 1, n_traj: int = 1, num_cus: int = 256):
    """(workgroups, row slices, tile) of ``trajectory_residuals`` for nx cells on a ctx of ``num_cus`` CUs - host logic
    only, no GPU (rt_trajectory_residuals_plan_info); tile = 1000 x rows a stage evaluates + steps a block evaluates.
    Raises where the call would refuse the sizes."""
    lib = _lib.load()
    some = (C.c_double * 7)()   # the checks only see that the operands are there
    desc = _lib.FomDesc(int(nx), int(n_traj), int(nt), 0, 1.0, 0, 0, C.cast(some, _p), None)
    info3 = (C.c_int64 * 3)()
    sp = C.cast(some, _p)
    rc = lib.rt_trajectory_residuals_plan_info(int(num_cus), C.byref(desc), sp, int(k), int(k), sp, int(k), int(nt) * int(k), None,
                                               sp, None, info3)
    if rc != 0:
        raise RomtimeHipError(f"rt_trajectory_residuals_plan_info failed ({rc}) for nx = {nx}, k = {k}, nt = {nt}, "
                              f"n_traj = {n_traj}")
    return int(info3[0]), int(info3[1]), int(info3[2])


def trajectory_residuals(V: torch.Tensor, uN: torch.Tensor, nx: int, tab, dt: float, bdf2: bool, state_in_w: bool,
                         a_init: torch.Tensor = None, first_step: int = 0):
    """Residuals of the lifted trajectories x^t = V uN[j, t] in the full-order step system of ``p1_fom_bdf_sweep``, without
    storing them and without a full-order solve (rt_trajectory_residuals).  V: (nx + 1) x k basis (k <= 128; its rows 0
    and nx are not looked at: the lifted values there are 0); uN: (nt, k) or (n, nt, k) coefficients, as the sweeps return
    them; ``tab`` (nt, n, 7), dt and the flags as for ``p1_fom_bdf_sweep``; ``a_init`` (n, 2, k): the coefficients of the
    two steps before ``first_step`` (newest first), None = zero states.  Returns ``(res, scale)``, (n, nt) each:
    res[j, s] = ||rhs - K x^s||_2 over the interior rows of step s, scale[j, s] = || |K| |x^s| + |rhs| ||_2."""
    ctx = Context.current()
    tab = to_device(tab).contiguous()
    for name, t in (("V", V), ("uN", uN), ("a_init", a_init)):
        if t is not None and (t.dtype != torch.float64 or not t.is_cuda):
            raise RomtimeHipError(f"trajectory_residuals: {name} must be a float64 CUDA tensor")
    if V.dim() != 2 or uN.dim() not in (2, 3):
        raise RomtimeHipError("trajectory_residuals: V must be 2-D, uN 2-D or 3-D")
    if uN.dim() == 2:
        uN = uN.unsqueeze(0)
    Nh, k = V.shape
    n, nt, k2 = uN.shape
    if Nh != int(nx) + 1 or k2 != k or tab.dim() != 3 or tuple(tab.shape) != (nt, n, 7):
        raise RomtimeHipError(f"trajectory_residuals: shapes do not match (nx = {nx}, V {tuple(V.shape)}, uN {tuple(uN.shape)}, "
                              f"tab {tuple(tab.shape)})")
    if a_init is not None:
        a_init = a_init.contiguous()
        if tuple(a_init.shape) != (n, 2, k):
            raise RomtimeHipError(f"trajectory_residuals: `a_init` must be ({n}, 2, {k})")
    if _layout_last2(V) is None or _layout_last2(V)[1] != ROW_MAJOR:
        V = V.contiguous()
    if _layout_last2(uN) is None or _layout_last2(uN)[1] != ROW_MAJOR:
        uN = uN.contiguous()
    ldb, lda = _layout_last2(V)[0], _layout_last2(uN)[0]
    res = torch.empty((n, nt), dtype=torch.float64, device=V.device)
    scale = torch.empty((n, nt), dtype=torch.float64, device=V.device)
    desc = _lib.FomDesc(int(nx), n, nt, int(first_step), float(dt), int(bool(bdf2)), int(bool(state_in_w)), _ptr(tab), None)
    ctx.check(ctx.lib.rt_trajectory_residuals(ctx.handle, C.byref(desc), _ptr(V), ldb, k, _ptr(uN), lda, uN.stride(0),
                                              _ptr(a_init), _ptr(res), _ptr(scale)), "rt_trajectory_residuals")
    return res, scale


def sym_eig_values(G: torch.Tensor, first: int = 0, count: int | None = None):
    """Eigenvalues (descending, device) of the symmetric n x n G; (lam, status).  With ``first`` / ``count`` only
    lam[first:first+count] is computed (the rest of ``lam`` is left unset).  rt_sym_eig_values(_part)."""
    ctx = Context.current()
    n = G.shape[0]
    assert G.is_contiguous() and G.shape == (n, n)
    count = n - first if count is None else count
    lam = torch.empty(n, dtype=torch.float64, device=G.device)
    status = torch.zeros(1, dtype=torch.int32, device=G.device)
    ctx.check(ctx.lib.rt_sym_eig_values_part(ctx.handle, _ptr(G), n, first, count, _ptr(lam), _ptr(status)),
              "rt_sym_eig_values_part")
    return lam, status


def sym_eig_vectors(lam: torch.Tensor, k: int, first: int = 0) -> torch.Tensor:
    """Eigenvectors (n x k) of lam[first:first+k] (descending eigenvalues); directly after sym_eig_values.
    rt_sym_eig_vectors."""
    ctx = Context.current()
    n = lam.numel()
    W = torch.empty((n, k), dtype=torch.float64, device=lam.device)
    ctx.check(ctx.lib.rt_sym_eig_vectors(ctx.handle, n, k, _ptr(lam[first:]), _ptr(W)), "rt_sym_eig_vectors")
    return W


def sym_eig_blocked_plan(n: int, block_max: int = 2048):
    """Block widths of ``sym_eig_blocked`` for n columns - host logic only, no GPU (rt_sym_eig_blocked_plan_info); raises
    where the library refuses the sizes.  ``pod_rules.block_partition`` states the same rule in NumPy."""
    lib = _lib.load()
    p = C.c_int64(0)
    widths = (C.c_int64 * 8)()
    rc = lib.rt_sym_eig_blocked_plan_info(int(n), int(block_max), C.byref(p), widths)
    if rc != 0:
        raise RomtimeHipError(f"rt_sym_eig_blocked_plan_info failed ({rc}) for n = {n}, block_max = {block_max}")
    return np.array(widths[: p.value], dtype=np.int64)


def sym_eig_blocked(G: torch.Tensor, k: int, floor_rel: float = None, lam: torch.Tensor = None, W: torch.Tensor = None):
    """Leading eigenpairs of a symmetric positive semi-definite n x n G with a decaying spectrum, 2048 < n <= 16384, by
    the block Rayleigh-Ritz route (rt_sym_eig_blocked): ``(lam, W, info)`` with ``lam`` (n, device) the R Ritz values in
    descending order and zeros beyond, ``W`` (n x min(k, R), device) their vectors, and ``info`` a dict of ``status`` (0;
    1: more than 2048 block eigenvalues above the floor - the set is not reducible, ``lam`` and ``W`` are None unless the
    caller passed buffers, which are left untouched; 2: an eigensolve timed out), ``resolved`` (R) and ``block_ranks``.
    ``floor_rel`` None = ``pod_rules.blocked_floor(n)`` = n eps.  ``lam`` / ``W``: buffers to write into instead (W: n x k;
    the library writes n x min(k, R) with leading dimension min(k, R), so pass one only where k <= R is known).
    Synchronises the stream."""
    ctx = Context.current()
    n = G.shape[0]
    if G.dtype != torch.float64 or not G.is_cuda or G.dim() != 2 or G.shape != (n, n) or not G.is_contiguous():
        raise RomtimeHipError("sym_eig_blocked: expected a contiguous square float64 CUDA tensor")
    k = int(k)
    floor_rel = pod_rules.blocked_floor(n) if floor_rel is None else float(floor_rel)
    own = lam is None
    lam = torch.empty(n, dtype=torch.float64, device=G.device) if lam is None else lam
    Wbuf = torch.empty((n, k), dtype=torch.float64, device=G.device) if (W is None and k > 0) else W
    resolved, status = C.c_int64(0), C.c_int(0)
    ranks = (C.c_int64 * 8)()
    ctx.check(ctx.lib.rt_sym_eig_blocked(ctx.handle, _ptr(G), n, floor_rel, k, _ptr(lam), _ptr(Wbuf), C.byref(resolved), ranks,
                                         C.byref(status)), "rt_sym_eig_blocked")
    R = int(resolved.value)
    info = dict(status=int(status.value), resolved=R,
                block_ranks=[int(ranks[b]) for b in range(len(pod_rules.block_partition(n)))])
    if info["status"] != 0:
        return (None, None, info) if own else (lam, W, info)
    kk = min(k, R)
    if W is None:
        # the library wrote n x kk with leading dimension kk into the front of the buffer
        Wout = Wbuf.reshape(-1)[: n * kk].view(n, kk) if k > 0 else torch.empty((n, 0), dtype=torch.float64, device=G.device)
    else:
        Wout = W
    return lam, Wout, info


def sym_jacobi_eigh(G: torch.Tensor, max_sweeps: int = 60):
    """(lam, W, sweeps) of the symmetric n x n G (n <= 2048, not modified) by two-sided Jacobi on the device: ``lam``
    descending (device), eigenvectors in the columns of ``W`` (device, n x n), ``sweeps`` the sweeps run (the closing
    one without rotations included).  Small eigenvalues of a graded matrix come out to high relative accuracy.  Warns
    if ``max_sweeps`` ended the loop (what the sweeps reached is returned, as the host routine does).  Synchronises the
    stream once per sweep.  rt_sym_jacobi_eigh."""
    ctx = Context.current()
    n = G.shape[0]
    if G.dtype != torch.float64 or not G.is_cuda or G.dim() != 2 or G.shape != (n, n):
        raise RomtimeHipError("sym_jacobi_eigh: expected a square float64 CUDA tensor")
    G = G.contiguous()
    lam = torch.empty(n, dtype=torch.float64, device=G.device)
    W = torch.empty((n, n), dtype=torch.float64, device=G.device)
    status = torch.zeros(1, dtype=torch.int32, device=G.device)
    sweeps = C.c_int(0)
    ctx.check(ctx.lib.rt_sym_jacobi_eigh(ctx.handle, _ptr(G), n, _ptr(lam), _ptr(W), int(max_sweeps), C.byref(sweeps),
                                         _ptr(status)), "rt_sym_jacobi_eigh")
    if sweeps.value >= max_sweeps and int(status.item()) != 0:
        import warnings

        warnings.warn(f"romtime_amd: sym_jacobi_eigh stopped at max_sweeps = {max_sweeps} with rotations still applied",
                      RuntimeWarning)
    return lam, W, int(sweeps.value)


def transpose(src: torch.Tensor) -> torch.Tensor:
    ctx = Context.current()
    src = src.contiguous()
    rows, cols = src.shape
    dst = torch.empty((cols, rows), dtype=torch.float64, device=src.device)
    ctx.check(ctx.lib.rt_transpose(ctx.handle, _ptr(src), rows, cols, cols, _ptr(dst), rows), "rt_transpose")
    return dst


def bench_mfma_f64(iters: int = 20000) -> float:
    ctx = Context.current()
    out = C.c_double()
    ctx.check(ctx.lib.rt_bench_mfma_f64(ctx.handle, iters, C.byref(out)), "rt_bench_mfma_f64")
    return out.value


def bench_copy(nbytes: int = 1 << 30, reps: int = 10) -> float:
    ctx = Context.current()
    src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    out = C.c_double()
    ctx.check(ctx.lib.rt_bench_copy(ctx.handle, _ptr(dst), _ptr(src), nbytes, reps, C.byref(out)), "rt_bench_copy")
    return out.value
