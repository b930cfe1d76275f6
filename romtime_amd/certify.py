"""Error certification of whole sweep trajectories on the device: what ``HyperReducedPiston._evaluate``
(rom/hrom.py:546-582) computes one time step at a time on the host - the ROM and S-ROM errors against the FOM snapshots
(``compute_error``, rom/base.py:52-73) and the S-ROM estimator (``compute_rom_difference``, utils.py:173-212) - for the
``(n_mu, nt, r)`` trajectories the online sweeps return (``romtime_amd.sweep``).

Everything goes through ``ops.trajectory_errors`` (rt_trajectory_errors): the lifted trajectories ``V u_N`` are never
stored.  Full-order snapshots are taken one parameter point at a time, NumPy or device tensors in either memory order;
host arrays are uploaded one at a time and never held together here.  Results are NumPy arrays in the discrete l2 norm
of the reference, ``||.||_2 / sqrt(N_h)``.

``trajectory_residuals`` needs no full-order snapshots at all: it holds the lifted trajectories against the full-order
step system itself (``ops.trajectory_residuals``, rt_trajectory_residuals), for FOMs that state it (``p1_fom_recipe``)."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .conventions import Errors

MAX_COLUMNS = 128      # rt_trajectory_errors: basis columns plus lifting columns


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _coefficients(uN, what="uN"):
    """(n_mu, nt, r) device tensor from (n_mu, nt, r) or (nt, r) coefficients."""
    t = ops.to_device(uN)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f"{what} must be (n_mu, nt, r) or (nt, r), not {tuple(t.shape)}")
    return t


def _operands(V, uN, lift):
    """Basis [V | lifting shapes] and coefficients [u_N | lifting coefficients]: uc_h = V u_N + g_h (rom.py:507-520) with
    a low-rank g_h = shapes coef^T is one more product of the same form."""
    B = ops.to_device(V)
    if B.dim() != 2:
        raise ValueError("the basis must be N x r")
    A = _coefficients(uN)
    if A.shape[2] != B.shape[1]:
        raise ValueError(f"uN has {A.shape[2]} coefficients per step for a basis of {B.shape[1]} columns")
    if lift is not None:
        shapes, coef = lift
        shapes = ops.to_device(shapes)
        if shapes.dim() == 1:
            shapes = shapes.unsqueeze(1)
        coef = ops.to_device(coef)
        if coef.dim() == 2 and shapes.shape[1] == 1 and tuple(coef.shape) == tuple(A.shape[:2]):
            coef = coef.unsqueeze(2)
        coef = _coefficients(coef, "the lifting coefficients")
        if shapes.shape[0] != B.shape[0] or tuple(coef.shape) != (A.shape[0], A.shape[1], shapes.shape[1]):
            raise ValueError(f"lift: shapes {tuple(shapes.shape)} and coefficients {tuple(coef.shape)} do not match "
                             f"N = {B.shape[0]}, (n_mu, nt) = {tuple(A.shape[:2])}")
        B = torch.cat([B, shapes], dim=1)
        A = torch.cat([A, coef], dim=2)
    if B.shape[1] > MAX_COLUMNS:
        raise ValueError(f"{B.shape[1]} basis and lifting columns: at most {MAX_COLUMNS}")
    return B.contiguous(), A.contiguous()


def _snapshot_sets(U, n_mu):
    """The full-order trajectories as a list of n_mu N x nt matrices (entries may be None), not uploaded yet."""
    if U is None:
        return [None] * n_mu
    if isinstance(U, (np.ndarray, torch.Tensor)):
        sets = [U] if U.ndim == 2 else list(U)
    else:
        sets = list(U)
    if len(sets) != n_mu:
        raise ValueError(f"{len(sets)} snapshot matrices for {n_mu} trajectories")
    return sets


def _upload(Uj, N, nt):
    Ud = ops.to_device(Uj)
    if tuple(Ud.shape) != (N, nt):
        raise ValueError(f"snapshots are {tuple(Ud.shape)}, the trajectory has N = {N}, nt = {nt}")
    return Ud


def trajectory_errors(V, uN, U=None, lift=None, relative=False):
    """||U_j[:, t] - (V u_N[j, t] + g_h[j, t])||_2 / sqrt(N) for every parameter point j and step t: an (n_mu, nt) array.

    ``uN``: (n_mu, nt, r) as the sweeps return it, or (nt, r).  ``U``: one N x nt matrix or a sequence of n_mu of them;
    None leaves the term out (the norm of the lifted trajectory itself).  ``lift = (shapes N x q, coef n_mu x nt x q)``
    adds the lifting g_h = shapes coef^T - for the piston and heat problems the ramp ``node / nx`` times the amplitude
    ``fom.p1_closed_form(...)["lift"]`` supplies; a lifting that is not low-rank is subtracted from U by the caller.
    ``relative``: divide by ||U_j[:, t]||_2 / sqrt(N)."""
    if relative and U is None:
        raise ValueError("relative errors are relative to the snapshots U")
    B, A = _operands(V, uN, lift)
    n_mu, nt = A.shape[:2]
    if U is None:
        return _host(ops.trajectory_errors(B, A))
    out = np.empty((n_mu, nt))
    for j, Uj in enumerate(_snapshot_sets(U, n_mu)):
        Ud = _upload(Uj, B.shape[0], nt)
        if relative:
            err, ref = ops.trajectory_errors(B, A[j], Ud, want_ref=True)
            out[j] = _host(err)[0] / _host(ref)[0]
        else:
            out[j] = _host(ops.trajectory_errors(B, A[j], Ud))[0]
    return out


def _srom_minus_rom(uN, uN_srom):
    """u_s - [u; 0]: the ROM's coefficients zero-padded to the S-ROM's size (utils.py:192-200)."""
    a, s = _coefficients(uN), _coefficients(uN_srom, "uN_srom")
    if tuple(a.shape[:2]) != tuple(s.shape[:2]) or a.shape[2] > s.shape[2]:
        raise ValueError(f"ROM trajectories {tuple(a.shape)} do not pair with S-ROM trajectories {tuple(s.shape)}")
    d = s.clone()
    d[:, :, : a.shape[2]] -= a
    return d


def rom_difference(uN, uN_srom, V_srom):
    """The S-ROM estimator ||V_s (u_s - [u; 0])||_2 / sqrt(N) for whole trajectories: (n_mu, nt)."""
    return trajectory_errors(V_srom, _srom_minus_rom(uN, uN_srom))


def projection_errors(V, U):
    """Best-approximation error ||U_t - V V^T U_t||_2 / sqrt(N) per step of one N x nt snapshot matrix (a sequence of
    them: one row each): what no reduced solve on this basis can beat."""
    Vd = ops.to_device(V)
    single = isinstance(U, (np.ndarray, torch.Tensor)) and U.ndim == 2
    rows = []
    for Uj in ([U] if single else list(U)):
        Ud = ops.to_device(Uj)
        if Ud.dim() != 2 or Ud.shape[0] != Vd.shape[0]:
            raise ValueError(f"snapshots are {tuple(Ud.shape)}, the basis has N = {Vd.shape[0]}")
        coef = ops.gemm_tn(Vd, Ud)                                 # r x nt
        rows.append(trajectory_errors(Vd, coef.T, Ud)[0])
    return rows[0] if single else np.array(rows)


def evaluate(V_rom, uN_rom, V_srom, uN_srom, U, lift=None):
    """The payload of hrom.py:578-582 for every parameter point: a list of dicts with ``Errors.ESTIMATOR``,
    ``Errors.ROM`` and ``Errors.SACRIFICIAL`` curves of nt entries each.  ``U``: the FOM trajectories, a sequence of
    n_mu N x nt matrices (one matrix for a single point); each is uploaded once and serves both models.  An entry that is
    None (or ``U=None``) leaves that point with its estimator alone - online points whose FOM was never run."""
    B_rom, A_rom = _operands(V_rom, uN_rom, lift)
    B_srom, A_srom = _operands(V_srom, uN_srom, lift)
    n_mu, nt = A_rom.shape[:2]
    if tuple(A_srom.shape[:2]) != (n_mu, nt):
        raise ValueError(f"ROM trajectories {tuple(A_rom.shape)} do not pair with S-ROM trajectories {tuple(A_srom.shape)}")
    estimator = rom_difference(uN_rom, uN_srom, V_srom)
    out = []
    for j, Uj in enumerate(_snapshot_sets(U, n_mu)):
        entry = {Errors.ESTIMATOR: estimator[j]}
        if Uj is not None:
            Ud = _upload(Uj, B_rom.shape[0], nt)
            entry[Errors.ROM] = _host(ops.trajectory_errors(B_rom, A_rom[j], Ud))[0]
            entry[Errors.SACRIFICIAL] = _host(ops.trajectory_errors(B_srom, A_srom[j], Ud))[0]
        out.append(entry)
    return out


def trajectory_residuals(fom, V, uN, mus, rec=None, relative=True, chunk=None):
    """Residuals of the reduced trajectories in the FULL-ORDER step system, with no full-order solve: for every point j
    and step s, ``res = ||rhs - K x^s||_2`` and ``scale = || |K| |x^s| + |rhs| ||_2`` over the interior rows of the system
    ``fom_sweep`` solves at that step, evaluated at the lifted states x^t = V uN[j, t] (the rows formed from x^{s-1} and
    x^{s-2}, zero before the first step).  ``res / scale`` is a few eps for the full-order trajectory itself; for an
    exact Galerkin model the residual is orthogonal to V, for a hyper-reduced one it is not, so the curve shows the
    hyper-reduction error directly.

    ``fom`` states its step system through ``p1_fom_recipe`` (NotImplementedError otherwise); ``rec`` is that recipe when
    the caller already has it.  ``uN``: (len(mus), nt, r); ``V``: (nx + 1) x r, r <= 128.  Returns the (n_mu, nt) NumPy
    array ``res / scale`` (0 where scale is 0), or the pair ``(res, scale)`` with ``relative=False``.  ``chunk`` = steps
    per kernel call (None: the whole horizon in one); the two last coefficient rows are carried from call to call, and
    the result does not depend on how the horizon is cut."""
    from . import fom as device_fom

    mus = list(mus)
    rec = device_fom.recipe(fom, mus) if rec is None else rec
    B = ops.to_device(V)
    A = ops.to_device(uN)
    tab = ops.to_device(rec["tab"])
    nx = int(fom.nx)
    nt = int(tab.shape[0])
    if B.dim() != 2 or B.shape[0] != nx + 1:
        raise ValueError(f"the basis must be (nx + 1) x r = {nx + 1} x r, not {tuple(B.shape)}")
    if B.shape[1] > MAX_COLUMNS:
        raise ValueError(f"{B.shape[1]} basis columns: at most {MAX_COLUMNS}")
    if tuple(A.shape) != (len(mus), nt, B.shape[1]):
        raise ValueError(f"uN must be (n_mu, nt, r) = {(len(mus), nt, int(B.shape[1]))}, not {tuple(A.shape)}")
    if int(tab.shape[1]) != len(mus):
        raise ValueError(f"the recipe's table is for {int(tab.shape[1])} parameter points, not {len(mus)}")
    steps = nt if chunk is None else int(chunk)
    if steps < 1:
        raise ValueError(f"chunk must be a positive number of steps, not {chunk!r}")
    res, scale = np.empty((len(mus), nt)), np.empty((len(mus), nt))
    a_init = None
    for first in range(0, nt, steps):
        block = A[:, first:first + steps]
        r, s = ops.trajectory_residuals(B, block, nx, tab[first:first + steps], fom.dt, rec["bdf2"], rec["state_in_w"],
                                        a_init=a_init, first_step=first)
        res[:, first:first + steps], scale[:, first:first + steps] = _host(r), _host(s)
        older = block[:, -2] if block.shape[1] > 1 else (a_init[:, 0] if a_init is not None else torch.zeros_like(block[:, -1]))
        a_init = torch.stack([block[:, -1], older], dim=1)
    if not relative:
        return res, scale
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(scale == 0.0, 0.0, res / np.where(scale == 0.0, 1.0, scale))
