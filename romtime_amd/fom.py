"""Full-order trajectories of the closed-form 1-D P1 models on the device: what ``fom.solve()`` computes one parameter
point and one time step at a time on the host (testing/mock.py; the reference's ``OneDimensionalSolver.solve``,
fom/base.py:693-831) for a whole sampling space in one kernel launch (``ops.p1_fom_bdf_sweep``, rt_p1_fom_bdf_sweep; or
``ops.p1_fom_bdf_sweep_certified``, which holds every step to a measured backward error where the rows are not
diagonally dominant - the convection-dominated piston).

The full-order model describes itself through ``p1_fom_recipe(mus, ts)`` (a table of seven scalars per step and point,
two flags and the lifting ramp).  The snapshots stay on the device as ``(n_mu, nt, N_h)`` blocks whose ``[j].T`` is the
N_h x nt snapshot matrix the POD walks and ``certify.trajectory_errors`` take unchanged."""
from __future__ import annotations

import numpy as np
import torch

from . import ops


def _times(fom):
    return fom.dt * np.arange(1, int(fom.domain["nt"]) + 1)


def recipe(fom, mus):
    """``fom.p1_fom_recipe`` over the model's own time grid."""
    if not hasattr(fom, "p1_fom_recipe"):
        raise NotImplementedError(f"{type(fom).__name__} has no p1_fom_recipe(mus, ts): its full-order sweep runs on the host only")
    if not getattr(fom, "is_setup", True):
        fom.setup()
    return fom.p1_fom_recipe(list(mus), _times(fom))


CHECKS = ("dominance", "defect")
DEFECT_TOL = 1e-10        # the relative residual the reference accepts for a linear solve (GMRES_OPTIONS, rom.py:36)


def fom_sweep(fom, mus, chunk=None, rec=None, check="dominance", defect_tol=None, report=None):
    """Generator over ``(first_step, U_block)``: the homogeneous snapshots of every mu for steps first_step ..
    first_step + U_block.shape[1] - 1 as an (n_mu, steps, N_h) device tensor.  ``chunk`` = steps per kernel call (None: the
    whole horizon in one); the two last states are carried from call to call, and the snapshots do not depend on how the
    horizon is cut.

    ``check`` says what a step is trusted by.  "dominance": every row diagonally dominant, |d| >= |l| + |u| - which holds
    only where about |w| dt/h <= 2 bdf/3 + 2 alpha dt/h^2 (a CFL number below one or a cell Peclet number below two).
    "defect": the componentwise backward error of every step's solve, measured on the device
    (``ops.p1_fom_bdf_sweep_certified``), at most ``defect_tol`` (None: 1e-10); the snapshots are the same bits, and
    ``report`` (a dict) receives ``report["defect"]``, the (n_mu, nt) NumPy array of the steps swept so far.  A point that
    fails the check, or meets a non-finite pivot, raises ArithmeticError."""
    if check not in CHECKS:
        raise ValueError(f"check must be 'dominance' or 'defect', not {check!r}")
    certified = check == "defect"
    tol = DEFECT_TOL if defect_tol is None else float(defect_tol)
    if not tol >= 0.0:
        raise ValueError(f"defect_tol must be a non-negative number, not {defect_tol!r}")
    mus = list(mus)
    rec = recipe(fom, mus) if rec is None else rec
    tab = ops.to_device(rec["tab"])
    nt, n_mu, Nh = int(tab.shape[0]), int(tab.shape[1]), int(fom.nx) + 1
    if n_mu != len(mus):
        raise ValueError(f"the recipe's table is for {n_mu} parameter points, not {len(mus)}")
    steps = nt if chunk is None else int(chunk)
    if steps < 1:
        raise ValueError(f"chunk must be a positive number of steps, not {chunk!r}")
    steps = min(steps, nt)
    if tab.is_cuda:
        need, free = n_mu * steps * Nh * 8, torch.cuda.mem_get_info(tab.device)[0]
        if need > free:
            raise MemoryError(f"a block of {steps} steps for {n_mu} parameter points of {Nh} dofs takes {need} bytes and "
                              f"{free} are free on the device: pass a smaller `chunk` (steps per call)")
    if certified and report is not None:
        report["defect"] = np.zeros((n_mu, 0))
    u_init = None
    for first in range(0, nt, steps):
        if certified:
            U, info, defect = ops.p1_fom_bdf_sweep_certified(fom.nx, tab[first:first + steps], fom.dt, rec["bdf2"], rec["state_in_w"],
                                                             u_init=u_init, first_step=first, defect_tol=tol)
            defect = defect.cpu().numpy()
            if report is not None:
                report["defect"] = np.concatenate([report["defect"], defect], axis=1)
        else:
            U, info = ops.p1_fom_bdf_sweep(fom.nx, tab[first:first + steps], fom.dt, rec["bdf2"], rec["state_in_w"], u_init=u_init,
                                           first_step=first)
        flags = info.cpu().numpy()
        if flags.any():
            j = int(np.flatnonzero(flags)[0])
            step = int(flags[j]) - 1
            if certified:
                raise ArithmeticError(f"full-order sweep: mu = {mus[j]} has a backward error (defect) of {defect[j, step - first]:.3e} "
                                      f"at step {step}, above defect_tol = {tol:.3e} or not finite")
            raise ArithmeticError(f"full-order sweep: mu = {mus[j]} has a row that is not diagonally dominant or a pivot that "
                                  f"is not finite at step {step}")
        if first + steps < nt:
            older = U[:, -2] if U.shape[1] > 1 else (u_init[:, 0] if u_init is not None else torch.zeros_like(U[:, -1]))
            u_init = torch.stack([U[:, -1], older], dim=1)
        yield first, U


def full_solution(U_block, lift_block):
    """Homogeneous snapshots (n_mu, steps, N_h) + the lifting ramp g0 + g1 i/nx of ``lift_block`` (steps, n_mu, 2: the
    recipe's ``lift`` rows of these steps)."""
    Nh = U_block.shape[2]
    lift = ops.to_device(lift_block).to(U_block.device).permute(1, 0, 2)
    ramp = torch.arange(Nh, dtype=torch.float64, device=U_block.device) / float(Nh - 1)
    return U_block + lift[:, :, 0:1] + lift[:, :, 1:2] * ramp


def csr_pattern(nx):
    """(rows, cols) of the CSR entries of the P1 matrices, Dirichlet rows reduced to their diagonal (mock._assemble_matrix)."""
    i = np.arange(1, nx)
    rows = np.concatenate([[0], np.repeat(i, 3), [nx]])
    cols = np.concatenate([[0], (i[:, None] + np.array([-1, 0, 1])[None, :]).ravel(), [nx]])
    return rows.astype(np.int64), cols.astype(np.int64)


def nonlinear_snapshots(fom, U_mu):
    """The nnz x nt snapshot set of the state-dependent operator for ONE parameter point from its (nt, N_h) device
    snapshots: column s holds the CSR values of the trilinear form of u* of step s (0, 2u^0, 2u^n - u^{n-1} under BDF2;
    u^n under BDF1) - what ``build_reduced_basis`` builds from ``fom.nonlinear_snapshots[1:]``, first row zeroed."""
    nt, Nh = int(U_mu.shape[0]), int(U_mu.shape[1])
    ustar = torch.zeros_like(U_mu)
    if nt > 1:
        ustar[1:] = U_mu[:-1]
        if getattr(fom, "BDF_SCHEME", "1") == "2":
            ustar[1:] *= 2.0
            ustar[2:] -= U_mu[:-2]
    rows, cols = csr_pattern(Nh - 1)
    ones = torch.ones(nt, dtype=torch.float64, device=U_mu.device)
    vals = ops.p1_local_assembly("trilinear", Nh - 1, rows, cols, ones, state=ustar)
    vals[:, 0] = 0.0
    return vals.T
