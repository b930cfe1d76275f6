"""The (M)DEIM snapshot sets of closed-form P1 models, collected on the device: the first half of
``run_offline_hyperreduction`` (rom/hrom.py:419-448, 1092-1146) without a FOM callback.

The offline walks of the three classes train on whole operators: one per (mu, t) for DEIM and MDEIM (deim/deim.py:384-389),
one per (mu, t, psi) for N-MDEIM (deim/nonlinear.py:437-443).  By default (``SNAPSHOTS_ON = "host"``) every one of them is
a FOM callback on the host, stacked and uploaded.  For a FOM with ``p1_closed_form`` the operators are closed forms in a
few scalars per (mu, t), and ``ops.p1_snapshot_sets`` writes a parameter point's whole set - a product grid of the (t)
scalars and, for N-MDEIM, the (psi) functions - in one launch, in the column-major layout the POD takes.

``resolve`` finds the closed form behind a reductor's callback; the kind rules - which device kind and which scalars an
operator name stands for - are those of ``online._ClosedForm.table`` (the online tables at the interpolation entries), here
over the reductor's whole topology.  ``online._ClosedForm`` and the first five kinds of
``interpolation.evaluate_closed_form`` keep their own statement of them over ``ops.p1_local_assembly``: the host-logic
tests replace that operator alone."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .conventions import EmpiricalInterpolation

# bound-method name of the FOM -> kind
CALLBACK_KINDS = {
    "assemble_mass": "mass", "assemble_stiffness": "stiffness", "assemble_convection": "convection",
    "assemble_nonlinear_lifting": "nonlinear_lifting", "assemble_forcing": "forcing", "assemble_lifting": "lifting",
    "assemble_trilinear": "trilinear", "assemble_rhs": "rhs",
}
VECTOR_KINDS = ("forcing", "lifting", "rhs")             # DEIM: load vectors over all nx + 1 rows
STATE_KINDS = ("trilinear",)                             # N-MDEIM: the state-dependent operator


def _lifting_keys(keys):
    return "lifting_poly" in keys or "lift_dot" in keys


# what ``p1_closed_form()`` must carry for a kind (beside ``nx`` and ``h``)
_NEEDS = {
    "mass": lambda keys: True,
    "stiffness": lambda keys: "alpha" in keys,
    "convection": lambda keys: True,
    "nonlinear_lifting": lambda keys: "lift" in keys,
    "trilinear": lambda keys: True,
    "forcing": lambda keys: "forcing_poly" in keys,
    "lifting": _lifting_keys,
    "rhs": lambda keys: "forcing_poly" in keys and _lifting_keys(keys),
}


def _refuse(reductor, why):
    name = getattr(reductor.assemble, "__qualname__", None) or repr(reductor.assemble)
    return NotImplementedError(f"{reductor}: no closed form for the callback {name} ({why}); SNAPSHOTS_ON = 'host' serves it")


def resolve(reductor, mus=None, ts=None):
    """``(fom, kind)`` of the closed form behind ``reductor.assemble``: the FOM is the bound method's ``__self__``, the
    kind follows from its name (``CALLBACK_KINDS``); an instance attribute ``reductor.closed_form = (fom, kind)`` overrides
    both.  NotImplementedError - naming the callback and the host route - for an unbound or unknown callback, a FOM
    without ``p1_closed_form``, a kind that does not fit the reductor's class, and a kind whose scalars
    ``p1_closed_form()`` lacks.  The last is asked of the table of one parameter point: the first of ``mus`` (with the
    first of ``ts``), else one drawn from the reductor's ``grid`` with a generator of its own (no random state of the
    caller moves); without either it is left to the first launch."""
    override = getattr(reductor, "closed_form", None)
    if override is not None:
        fom, kind = override
    else:
        fom = getattr(reductor.assemble, "__self__", None)
        name = getattr(reductor.assemble, "__name__", None)
        if fom is None or isinstance(fom, type):
            raise _refuse(reductor, "it is not a bound method of a FOM")
        kind = CALLBACK_KINDS.get(name)
    if kind not in _NEEDS:
        raise _refuse(reductor, f"unknown operator; known: {sorted(CALLBACK_KINDS)}")
    if not hasattr(fom, "p1_closed_form"):
        raise _refuse(reductor, f"{type(fom).__name__} has no p1_closed_form")
    if reductor.TYPE == EmpiricalInterpolation.DEIM:
        fits = kind in VECTOR_KINDS
    elif reductor.TYPE == EmpiricalInterpolation.NONLINEAR:
        fits = kind in STATE_KINDS
    else:
        fits = kind not in VECTOR_KINDS and kind not in STATE_KINDS
    if not fits:
        raise _refuse(reductor, f"a {reductor.TYPE} reductor does not take the kind {kind!r}")
    probe = None
    if mus is not None and len(mus):
        probe = mus[0]
    elif getattr(reductor, "grid", None):
        from sklearn.model_selection import ParameterSampler

        probe = list(ParameterSampler(param_distributions=reductor.grid, n_iter=1, random_state=np.random.RandomState(0)))[0]
    if probe is not None:
        t0 = 1.0 if ts is None or not len(ts) else float(np.asarray(ts, dtype=float).reshape(-1)[0])
        keys = set(fom.p1_closed_form([probe], [t0]))
        if not _NEEDS[kind](keys):
            raise _refuse(reductor, f"p1_closed_form() of {type(fom).__name__} lacks the scalars of {kind!r}, it has {sorted(keys)}")
    return fom, kind


def _topology(reductor, nx):
    """Device (rows, cols) of the entries a snapshot runs over: all ``nx + 1`` rows for DEIM (cols None), the reductor's
    ``(rows, cols)`` otherwise; kept in the reductor's device cache against the identities of the lists."""
    cache = reductor._dev_cache
    if reductor.TYPE == EmpiricalInterpolation.DEIM:
        hit = cache.get("collect_rows")
        if hit is None or hit[0] != nx:
            hit = cache["collect_rows"] = (nx, ops.to_device_index(np.arange(nx + 1)))
        return hit[1], None
    rows, cols = reductor.rows, reductor.cols
    if rows is None or cols is None:
        raise ValueError(f"{reductor}: no matrix topology (rows / cols); run setup() first")
    hit = cache.get("collect_topology")
    if hit is None or hit[0] is not rows or hit[1] is not cols:
        hit = cache["collect_topology"] = (rows, cols, ops.to_device_index(rows), ops.to_device_index(cols))
    return hit[2], hit[3]


def assemble(kind, cf, rows, cols, fun=None, zero_first=False, lo=None, hi=None) -> torch.Tensor:
    """The kind rules, stated once for the whole-topology sets: the ``(n_par * n_fun, m)`` table of operator ``kind`` over
    the parameter rows ``cf[...][lo:hi]`` flattened - ``cf`` the (nt, n_mu) tables of ``p1_closed_form`` - and the nodal
    functions ``fun`` (trilinear only).

      mass, stiffness (coef = alpha), nonlinear_lifting (trilinear, ramp = lift), trilinear (fun): their device kinds;
      convection   minus the trilinear ramp of ``mesh_velocity`` where the table has one (ALE), else the constant kind;
      forcing      load_p2 of ``forcing_poly``;
      lifting      load_p2 of ``lifting_poly`` with coef = -1 where the table has one, else load of the ramp ``lift_dot``;
      rhs          forcing, then lifting added into the same table (beta = 1: one rounding per entry, no temporary)."""
    nx = int(cf["nx"])

    def flat(key, sign=1.0, width=None):
        if key not in cf:
            raise NotImplementedError(f"p1_closed_form() has no {key!r}: the operator {kind!r} has no closed form here; "
                                      "SNAPSHOTS_ON = 'host' serves it")
        a = np.asarray(cf[key], dtype=np.float64)[lo:hi]
        a = np.ascontiguousarray(sign * a if sign != 1.0 else a)
        return a.reshape(-1) if width is None else a.reshape(-1, width)

    h = ops.to_device(flat("h"))
    call = lambda device_kind, **kw: ops.p1_snapshot_sets(device_kind, nx, rows, cols, h, zero_first=zero_first, **kw)
    forcing = lambda **kw: call("load_p2", poly=flat("forcing_poly", width=3), **kw)

    def lifting(**kw):
        if "lifting_poly" in cf:                                      # degree-2 data (fom/heat.py:131-169)
            return call("load_p2", coef=torch.full_like(h, -1.0), poly=flat("lifting_poly", width=3), **kw)
        return call("load", ramp=flat("lift_dot"), **kw)

    if kind == "mass":
        return call("mass")
    if kind == "stiffness":
        return call("stiffness", coef=flat("alpha"))
    if kind == "convection":
        if "mesh_velocity" in cf:
            return call("trilinear", ramp=flat("mesh_velocity", sign=-1.0))
        return call("convection")
    if kind == "nonlinear_lifting":
        return call("trilinear", ramp=flat("lift"))
    if kind == "trilinear":
        if fun is None:
            raise ValueError("kind 'trilinear' needs the nodal functions (funcs=)")
        return call("trilinear", fun=fun)
    if kind == "forcing":
        return forcing()
    if kind == "lifting":
        return lifting()
    if kind == "rhs":
        return lifting(out=forcing(), beta=1.0)
    raise ValueError(f"unknown kind {kind!r}")


def _functions(reductor, u_n) -> torch.Tensor:
    """``u_n`` (N_h x N_psi, columns = states) as the device ``(N_psi, N_h)`` block of nodal functions, kept against the
    identity of ``u_n``."""
    hit = reductor._dev_cache.get("collect_fun")
    if hit is not None and hit[0] is u_n:
        return hit[1]
    a = np.asarray(u_n, dtype=np.float64)
    a = a.reshape(a.shape[0], 1) if a.ndim == 1 else a
    fun = ops.to_device(np.ascontiguousarray(a.T))
    reductor._dev_cache["collect_fun"] = (u_n, fun)
    return fun


def table(reductor, mus, ts, funcs=None, zero_first=False, resolved=None) -> torch.Tensor:
    """Rows = whole operators of the reductor's kind, in the order (t, mu[, psi]) with the last fastest, each over the
    reductor's topology: ``(len(ts) * len(mus) * n_psi, N)``."""
    fom, kind = resolved if resolved is not None else resolve(reductor, mus, ts)
    cf = fom.p1_closed_form(list(mus), np.asarray(ts, dtype=float))
    rows, cols = _topology(reductor, int(cf["nx"]))
    fun = _functions(reductor, funcs) if kind in STATE_KINDS else None
    return assemble(kind, cf, rows, cols, fun=fun, zero_first=zero_first)


def time_level_set(reductor, mu, ts, resolved=None) -> torch.Tensor:
    """The device ``N x len(ts)`` snapshot set of one parameter point (what ``walks.upload_columns`` of the
    ``assemble_snapshot(mu, t)`` columns gives, deim/deim.py:384-389): column-major, entry 0 zeroed for MDEIM."""
    zero = reductor.TYPE == EmpiricalInterpolation.MDEIM
    return table(reductor, [mu], ts, zero_first=zero, resolved=resolved).T


def state_level_sets(reductor, mu, ts, u_n, resolved=None) -> list:
    """The ``len(ts)`` basis-level sets ``N x N_psi`` of one parameter point of the N-MDEIM walk (deim/nonlinear.py:
    437-443), entry 0 zeroed: one launch, the sets are views of its one buffer."""
    tab = table(reductor, [mu], ts, funcs=u_n, zero_first=True, resolved=resolved)
    per_t = tab.view(len(ts), -1, tab.shape[1])
    return [per_t[k].T for k in range(len(ts))]


def exact_snapshots(reductor, mu, ts, funcs=None, resolved=None) -> torch.Tensor:
    """The exact snapshots ``evaluate`` certifies for one parameter point, ``N x (len(ts) * n_psi)`` column-major with
    psi fastest: the operators as they are (the Dirichlet entry included)."""
    return table(reductor, [mu], ts, funcs=funcs, resolved=resolved).T
