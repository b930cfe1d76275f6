"""Certification of the (M)DEIM interpolants over whole snapshot sets on the device: ``evaluate`` of the three classes
(deim.py:226-261, nonlinear.py:470-540; what ``run_offline_hyperreduction(evaluate=True)`` and ``evaluate_deim`` run for
each of the six hyper-reductors, hrom.py:419, 491-502, 796-809, 957, 1092).

The host loop of the classes makes, per sample, two FOM callbacks, one theta solve and one expansion with their
transfers.  Here the theta solve is folded into the basis once, ``Psi = basis_fom PT_U^-1`` (as ``sweep.hrom_bdf_sweep``
folds it into ``basis_rom``), the exact snapshots of a parameter point are uploaded as one block and a single kernel
call (``ops.interpolation_errors``) returns the error of every snapshot of the block.

Two rounding-level deviations from the reference, stated in DESIGN.md: the coefficients of a snapshot are its own
entries at the interpolation indices, where the reference assembles them a second time entry by entry; and
``Psi f[idx]`` replaces ``basis_fom @ solve(PT_U, f[idx])``.  Interpolation sets of more than 128 entries are refused:
there is no host route."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .conventions import EmpiricalInterpolation, Stage

MAX_M = 128                      # interpolation ENTRIES (m_s with oversampling): rt_interpolation_errors and rt_dense_solve_multi
MAX_COLUMNS = 4096               # snapshots per kernel call unless the caller says otherwise
CLOSED_FORM_KINDS = ("mass", "stiffness", "convection", "nonlinear_lifting", "lifting", "trilinear", "forcing", "rhs")
COLLECT_KINDS = ("trilinear", "forcing", "rhs")      # through ``collect.assemble`` (rt_p1_snapshot_sets)


def fold(reductor) -> torch.Tensor:
    """``Psi = basis_fom PT_U^-1`` (N_h x m) on the device, cached in the reductor against the identities of
    ``basis_fom`` and ``PT_U``: the interpolant of a snapshot f is then ``Psi f[idx]``.  Solved as
    ``PT_U^T Psi^T = basis_fom^T`` by the device's pivoted LU; a zero pivot raises what ``np.linalg.solve`` raises
    (deim.py:491-492).  With oversampled entries ``PT_U`` is m_s x m and ``Psi = basis_fom pinv(PT_U)`` is N_h x m_s, the
    minimum-norm solution of the same equation by Householder QR (``ops.dense_lstsq_multi``): ``Psi f[idx]`` is the basis
    times the least-squares theta.  ``MAX_M`` bounds the entries, m_s."""
    basis, PT_U = reductor.basis_fom, reductor.PT_U
    hit = reductor._dev_cache.get("interpolation_psi")
    if hit is not None and hit[0] is basis and hit[1] is PT_U:
        return hit[2]
    m = int(np.shape(PT_U)[0])
    if m > MAX_M:
        raise ValueError(f"{reductor}: {m} interpolation entries, the device certification takes at most {MAX_M}")
    B = reductor._device("basis_fom", basis).T.contiguous()                       # modes x N_h
    if np.shape(PT_U)[0] != np.shape(PT_U)[1]:        # oversampled entries: Psi = basis_fom pinv(PT_U), N_h x m_s
        Zt, info = ops.dense_lstsq_multi(ops.to_device(np.ascontiguousarray(np.asarray(PT_U, dtype=np.float64))), B, trans=True)
    else:
        K = ops.to_device(np.ascontiguousarray(np.asarray(PT_U, dtype=np.float64).T))
        Zt, info = ops.dense_solve_multi(K, B)
    if int(info.reshape(-1)[0].item()) != 0:
        raise np.linalg.LinAlgError("Singular matrix")
    Psi = Zt.T.contiguous()
    reductor._dev_cache["interpolation_psi"] = (basis, PT_U, Psi)
    return Psi


def flat_indices(reductor) -> np.ndarray:
    """Where the interpolation entries sit in a snapshot vector: DEIM's ``dofs`` themselves, for the matrix kinds the
    position of every ``(row, col)`` of ``dofs`` in the reductor's ``(rows, cols)`` topology (one pass over the topology,
    remembered in the reductor against the identities of ``dofs``, ``rows`` and ``cols``)."""
    if reductor.TYPE == EmpiricalInterpolation.DEIM:
        return np.array([int(d[0]) for d in reductor.dofs], dtype=np.int64)
    dofs, rows, cols = reductor.dofs, reductor.rows, reductor.cols
    hit = reductor._dev_cache.get("interpolation_idx")
    if hit is not None and hit[0] is dofs and hit[1] is rows and hit[2] is cols:
        return hit[3]
    wanted = {(int(r), int(c)) for r, c in dofs}
    where = {}
    for pos, rc in enumerate(zip(rows, cols)):
        rc = (int(rc[0]), int(rc[1]))
        if rc in wanted:
            where.setdefault(rc, pos)
    idx = np.array([where[(int(r), int(c))] for r, c in dofs], dtype=np.int64)
    reductor._dev_cache["interpolation_idx"] = (dofs, rows, cols, idx)
    return idx


def pin_of(reductor):
    """The entry of the FOM-form interpolant the reference overwrites: ``approximation[0] = 1.0`` for MDEIM
    (deim.py:449-450) and N-MDEIM (nonlinear.py:280-281), none for DEIM."""
    return None if reductor.TYPE == EmpiricalInterpolation.DEIM else (0, 1.0)


def snapshot_errors(reductor, F, group=1) -> np.ndarray:
    """Interpolation errors of one block of exact snapshots (N_h x S, NumPy or device, either memory order): per
    snapshot ``compute_error(interpolant, snapshot)``, averaged over consecutive groups of ``group``."""
    Fd = F if isinstance(F, torch.Tensor) else ops.to_device(F)
    err = ops.interpolation_errors(fold(reductor), flat_indices(reductor), Fd, group=group, pin=pin_of(reductor))
    return err.cpu().numpy()


def _space(reductor, num, mu_space):
    if mu_space:
        return mu_space
    assert num, "Provide number of samples to test"
    return reductor.build_sampling_space(num=num)


def evaluate(reductor, ts, num=None, mu_space=None, funcs=None, max_columns=MAX_COLUMNS):
    """The classes' ``evaluate`` with the same bookkeeping - ``add_mu(step=ONLINE)``, ``errors_rom[mu_idx]`` an array of
    ``len(ts)`` errors - and one FOM callback per sample: the exact snapshots of a parameter point are stacked on the
    device (``walks.upload_columns``) and certified by one kernel call per chunk of at most ``max_columns`` columns.
    N-MDEIM: the columns run over (t, psi), the error of a time instant is the mean over the states ``funcs`` (default
    the reductor's ``u_n``), and a chunk holds whole time instants.  A reductor with ``SNAPSHOTS_ON = "device"`` takes
    its exact snapshots from ``collect`` (one launch per chunk) instead: no FOM callback at all."""
    from . import walks

    ts = list(ts)
    on_device = reductor._snapshots_on_device()
    nonlinear = reductor.TYPE == EmpiricalInterpolation.NONLINEAR
    if nonlinear:
        u_n = reductor.u_n if funcs is None else funcs
        n_psi = int(u_n.shape[1])
    else:
        n_psi = 1
    per_chunk = max(int(max_columns) // n_psi, 1) if np.isfinite(max_columns) else max(len(ts), 1)   # time instants
    fold(reductor)                                       # a singular PT_U or too many entries: before any bookkeeping
    space = _space(reductor, num, mu_space)
    if on_device:
        from . import collect

        space = list(space)
        resolved = collect.resolve(reductor, space, ts)  # no closed form: before any bookkeeping
    for mu in space:
        mu_idx, mu = reductor.add_mu(step=Stage.ONLINE, mu=mu)
        errors = list(reductor.errors_rom[mu_idx])
        for lo in range(0, len(ts), per_chunk):
            if on_device:
                F = collect.exact_snapshots(reductor, mu, ts[lo:lo + per_chunk], funcs=u_n if nonlinear else None,
                                            resolved=resolved)
                errors.extend(snapshot_errors(reductor, F, group=n_psi))
                continue
            if nonlinear:
                columns = [reductor.assemble_snapshot(mu=mu, t=t, u_n=u_n[:, i]) for t in ts[lo:lo + per_chunk]
                           for i in range(n_psi)]
            else:
                columns = [reductor.assemble_snapshot(mu, t) for t in ts[lo:lo + per_chunk]]
            errors.extend(snapshot_errors(reductor, walks.upload_columns(columns), group=n_psi))
        reductor.errors_rom[mu_idx] = np.array(errors)


def evaluate_closed_form(reductor, kind, fom, mus, ts, max_columns=MAX_COLUMNS, funcs=None) -> np.ndarray:
    """Interpolation errors at every ``(mu, t)`` for a FOM with ``p1_closed_form`` (the counterpart of
    ``sweep.hrom_terms_on_device``): the exact snapshots are built on the device by ``ops.p1_local_assembly`` over the
    reductor's whole topology, in chunks of (t, mu) states, and never exist on the host.  ``kind``: "mass",
    "stiffness", "convection", "nonlinear_lifting" (the trilinear form with the lifting ramp) or "lifting" (the load
    vector of the lifting's time derivative); through the kind rules of ``collect.assemble``: "trilinear" (the
    state-dependent operator of the states ``funcs``, N_h x N_psi; the error of a (mu, t) is the mean over the states, as
    N-MDEIM's ``evaluate`` forms it), "forcing" and "rhs" (the load vectors of a DEIM reductor).  No FOM callback.
    Returns (n_mu, len(ts))."""
    if kind not in CLOSED_FORM_KINDS:
        raise ValueError(f"kind must be one of {CLOSED_FORM_KINDS}, not {kind!r}")
    if kind == "trilinear" and funcs is None:
        raise ValueError("kind 'trilinear' needs the states: funcs=(N_h x N_psi)")
    if not hasattr(fom, "p1_closed_form"):
        raise NotImplementedError("the FOM does not expose closed-form P1 scalars (p1_closed_form)")
    mus, ts = list(mus), np.asarray(ts, dtype=float)
    cf = fom.p1_closed_form(mus, ts)
    nx, n_mu, nt = int(cf["nx"]), len(mus), ts.size
    if kind in ("lifting", "forcing", "rhs"):
        rows, cols = ops.to_device_index(np.arange(nx + 1)), None
    else:
        rows, cols = ops.to_device_index(reductor.rows), ops.to_device_index(reductor.cols)
    Psi, idx, pin = fold(reductor), flat_indices(reductor), pin_of(reductor)
    flat = lambda a, lo, hi: np.ascontiguousarray(np.asarray(a, dtype=np.float64)[lo:hi]).reshape(-1)
    n_psi = 1
    if kind == "trilinear":
        from . import collect

        fun = collect._functions(reductor, funcs)
        n_psi = int(fun.shape[0])
    per_chunk = max(int(max_columns) // (n_mu * n_psi), 1) if np.isfinite(max_columns) else nt
    out = np.empty((nt, n_mu))
    for lo in range(0, nt, per_chunk):
        hi = min(lo + per_chunk, nt)
        if kind in COLLECT_KINDS:
            from . import collect

            table = collect.assemble(kind, cf, rows, cols, fun=fun if kind == "trilinear" else None, lo=lo, hi=hi)
            err = ops.interpolation_errors(Psi, idx, table.T, group=n_psi, pin=pin)
            out[lo:hi] = err.cpu().numpy().reshape(hi - lo, n_mu)
            continue
        h = flat(cf["h"], lo, hi)
        if kind == "mass":
            table = ops.p1_local_assembly("mass", nx, rows, cols, h)
        elif kind == "stiffness":
            table = ops.p1_local_assembly("stiffness", nx, rows, cols, h, coef=flat(cf["alpha"], lo, hi))
        elif kind == "convection":
            table = ops.p1_local_assembly("convection", nx, rows, cols, h)
        elif kind == "nonlinear_lifting":
            table = ops.p1_local_assembly("trilinear", nx, rows, cols, h, ramp=flat(cf["lift"], lo, hi))
        else:
            table = ops.p1_local_assembly("load", nx, rows, cols, h, ramp=flat(cf["lift_dot"], lo, hi))
        err = ops.interpolation_errors(Psi, idx, table.T, group=1, pin=pin)      # (n_states, N_h) rows = contiguous snapshots
        out[lo:hi] = err.cpu().numpy().reshape(hi - lo, n_mu)
    return np.ascontiguousarray(out.T)
