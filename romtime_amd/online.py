"""The online stage of the ``RomConstructor*`` classes on the device: what lies between ``sweep.hrom_bdf_sweep``
(rt_hrom_bdf_sweep, the BDF loop for many parameter points without a host round trip per step) and
``rom.solve(mu, step)`` / ``rom.solve_many(mus)`` with ``ONLINE_ON = "device"`` - the route a model can take (``plan``),
its tables for all three classes (``terms``), the classes' bookkeeping (``solve_many``) and the driver's ``_evaluate``
(rom/hrom.py:504-621) as one call (``evaluate``).

Routes (``plan``):
  * "closed_form": every operator of the class has a projected (M)DEIM and the FOM has ``p1_closed_form(mus, ts)``: the
    tables of local operator entries are built on the device (``ops.p1_local_assembly``), no FOM callback;
  * "callbacks":   the same reductors, any FOM: the tables are ``red._local_values(mu, t)`` for all steps and points up
    front (a FEniCS FOM takes this route); the step loop itself is on the device all the same;
  * "affine":      no reductor at all, the FOM has ``descriptor(mus)`` (``testing.mock.AffineBurgers.descriptor``): every
    affine term is projected once (``hrom_terms_from_affine``) and the loop has size r only.
Anything else - some operators hyper-reduced and some not, no reductors and no descriptor, r > 128 - raises
``NotImplementedError``; ``ONLINE_ON = "host"`` serves those models.

Operators per class: ``RomConstructor`` mass, stiffness and a source (``deim_rhs``, or ``deim_fh`` with ``deim_fgh``);
``RomConstructorMoving`` adds convection; ``RomConstructorNonlinear`` mass, stiffness, convection, nonlinear lifting,
trilinear and lifting.  The host loop of the two linear classes reads ``deim_rhs`` only (rom.py:617-640) and projects the
FOM's own forcing and lifting otherwise; with ``deim_fh`` / ``deim_fgh`` the device route interpolates them, so the two
differ by those interpolants' errors."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .conventions import BDF, PistonParameters, ProblemType, Stage
from .storage import RomSolutionsStorage

MAX_R = 128                      # rt_hrom_bdf_sweep: the reduced system stays in the LDS
ROUTES = ("closed_form", "callbacks", "affine")
SLOTS = dict(mass="mdeim_Mh", stiffness="mdeim_Ah", convection="mdeim_Ch", nonlinear_lifting="mdeim_Nh_hat",
             trilinear="mdeim_Nh", forcing="deim_fh", lifting="deim_fgh", rhs="deim_rhs")


def operators(rom) -> dict:
    """The operator table of the model's class: ``lin`` (summed into K_N besides the mass matrix), ``nl`` (the
    state-dependent operator or None) and ``sources`` (the alternatives for the right-hand side, first choice first)."""
    from .rom import RomConstructorMoving, RomConstructorNonlinear

    if isinstance(rom, RomConstructorNonlinear):      # no forcing term for Burgers (rom.py:913-915)
        return dict(lin=("stiffness", "convection", "nonlinear_lifting"), nl="trilinear", sources=(("lifting",),))
    lin = ("stiffness", "convection") if isinstance(rom, RomConstructorMoving) else ("stiffness",)
    return dict(lin=lin, nl=None, sources=(("rhs",), ("forcing", "lifting")))


def _reductors(rom):
    """(table, source, {operator: reductor or None}) with the source alternative that has the most reductors attached."""
    table = operators(rom)
    attached = lambda alt: sum(bool(getattr(rom, SLOTS[n])) for n in alt)
    source = max(table["sources"], key=attached)      # ties: the first alternative
    names = ("mass",) + table["lin"] + ((table["nl"],) if table["nl"] else ()) + source
    return table, source, {n: (getattr(rom, SLOTS[n]) or None) for n in names}


def _projected(red, r):
    return red.basis_rom is not None and np.shape(red.basis_rom)[0] in (r, r * r)


def plan(rom) -> str:
    """The device route of ``rom`` ("closed_form", "callbacks" or "affine"), from its class, its reductor slots and what
    its FOM offers; ``NotImplementedError`` names the operators in the way."""
    table, source, reds = _reductors(rom)
    fom, r = rom.fom, int(rom.basis.shape[1])
    host = "ONLINE_ON = 'host' serves this model"
    if r > MAX_R:
        raise NotImplementedError(f"r = {r} reduced unknowns, the device sweep takes at most {MAX_R}; {host}")
    missing = [n for n, red in reds.items() if red is None]
    if len(missing) == len(reds):
        if hasattr(fom, "descriptor"):
            return "affine"
        if len(table["sources"]) > 1:
            missing = [n for n in missing if n not in source] + ["rhs (or forcing and lifting)"]
        raise NotImplementedError(f"operators without a hyper-reductor: {missing}, and {type(fom).__name__} has no "
                                  f"descriptor(mus) of an affine model; {host}")
    if missing:
        raise NotImplementedError(f"operators without a hyper-reductor: {missing}; the device sweep needs every operator of "
                                  f"{type(rom).__name__} hyper-reduced (or none, and an affine descriptor); {host}")
    stale = [n for n, red in reds.items() if not _projected(red, r)]
    if stale:
        raise NotImplementedError(f"operators whose reductor is not projected on this basis: {stale}; call "
                                  f"project_reductors() first; {host}")
    return "closed_form" if hasattr(fom, "p1_closed_form") else "callbacks"


def times(fom) -> np.ndarray:
    """The time instants of the host loop, accumulated as it accumulates them (rom.py:476)."""
    t, out = 0.0, []
    for _ in range(int(fom.domain["nt"])):
        t += fom.dt
        out.append(t)
    return np.array(out)


def _cache(rom) -> dict:
    return rom.__dict__.setdefault("_online_cache", {})


# ---- tables ---------------------------------------------------------------------------------------------------------
def _term(red, F):
    return dict(PT_U=red.PT_U, basis_rom=red.basis_rom, F=F, cache=red._dev_cache)


def _callback_table(red, mus, ts):
    return np.array([[red._local_values(mu, t) for mu in mus] for t in ts])


class _ClosedForm:
    """``ops.p1_local_assembly`` at a reductor's entries for every (t, mu): the device kinds of every operator."""

    def __init__(self, fom, mus, ts):
        self.cf = fom.p1_closed_form(mus, ts)
        self.nx, self.nt, self.n_mu = int(self.cf["nx"]), len(ts), len(mus)
        self.h = self._flat("h")

    def _flat(self, key, sign=1.0, width=None):
        if key not in self.cf:
            raise NotImplementedError(f"p1_closed_form() has no {key!r}: this operator has no closed form here; "
                                      "terms(rom, mus, route='callbacks') builds its table from the FOM's callbacks")
        a = sign * np.asarray(self.cf[key], dtype=np.float64)
        return ops.to_device(np.ascontiguousarray(a).reshape(-1) if width is None else np.ascontiguousarray(a).reshape(-1, width))

    def table(self, name, red):
        d = np.asarray(red.dofs, dtype=np.int64)
        rows = ops.to_device_index(d[:, 0])
        cols = ops.to_device_index(d[:, 1]) if d.shape[1] == 2 else None
        asm = lambda kind, **kw: ops.p1_local_assembly(kind, self.nx, rows, cols, self.h, **kw).view(self.nt, self.n_mu, -1)
        heat = "lifting_poly" in self.cf                                  # degree-2 data (fom/heat.py:99-188)
        forcing = lambda: asm("load_p2", poly=self._flat("forcing_poly", width=3))
        lifting = lambda: asm("load_p2", coef=torch.full_like(self.h, -1.0), poly=self._flat("lifting_poly", width=3))
        if name == "mass":
            return asm("mass")
        if name == "stiffness":
            return asm("stiffness", coef=self._flat("alpha"))
        if name == "convection":                                          # ALE: minus the trilinear form of the mesh velocity
            if "mesh_velocity" in self.cf:
                return asm("trilinear", ramp=self._flat("mesh_velocity", sign=-1.0))
            return asm("convection")
        if name == "nonlinear_lifting":
            return asm("trilinear", ramp=self._flat("lift"))
        if name == "forcing":
            return forcing()
        if name == "lifting":
            return lifting() if heat else asm("load", ramp=self._flat("lift_dot"))
        if name == "rhs":
            return forcing() + lifting()
        raise KeyError(name)


def _state_map(rom, red, route, mus, ts):
    """(W, c0) of the state-dependent operator: its entries at the reductor's entries are ``W u_N + c0``, an affine map
    of the state that does not depend on (mu, t) (a trilinear form on a reference mesh plus constant Dirichlet entries).
    Kept per model against the identities of the basis and the entries."""
    hit = _cache(rom).get(("state_map", route))
    if hit is not None and hit[0] is rom.basis and hit[1] is red.dofs:
        return hit[2], hit[3]
    V = rom.basis
    if route == "closed_form":
        d = np.asarray(red.dofs, dtype=np.int64)
        states = np.vstack([np.ascontiguousarray(V.T), np.zeros((1, V.shape[0]))])      # the basis functions, then zero
        both = ops.p1_local_assembly("trilinear", V.shape[0] - 1, ops.to_device_index(d[:, 0]), ops.to_device_index(d[:, 1]),
                                     ops.to_device(np.ones(V.shape[1] + 1)), state=states)
        c0 = both[-1].contiguous()
        W = (both[:-1] - c0[None, :]).T.contiguous()                                  # m x r
    else:
        c0 = red._local_values(mus[0], ts[0], u_n=np.zeros(V.shape[0]))
        W = np.stack([red._local_values(mus[0], ts[0], u_n=V[:, k]) - c0 for k in range(V.shape[1])], axis=1)
        probe = np.random.RandomState(0).standard_normal(V.shape[1])
        again = red._local_values(mus[-1], ts[-1], u_n=V @ probe)
        if not np.allclose(again, W @ probe + c0, rtol=1e-10, atol=1e-12 * max(1.0, np.abs(W).max())):
            raise NotImplementedError("state-dependent operator is not a (mu, t)-independent affine map of the state; "
                                      "ONLINE_ON = 'host' serves this model")
    _cache(rom)[("state_map", route)] = (rom.basis, red.dofs, W, c0)
    return W, c0


def hrom_terms_from_affine(desc, V) -> dict:
    """The terms of an affine model (``descriptor`` in the layout of ``testing.mock.AffineBurgers.descriptor``) for
    ``hrom_bdf_sweep``: the classical split, every affine term projected once.  Every term has ``PT_U = I``; mass: one
    column ``vec(V^T M V)`` with F = 1; ``lin``: one term, column q = ``vec(V^T A_q V)``, F = ``term_coef``; ``nl``:
    column k = ``vec(V^T diag(v_k) T V)`` with W = I_r (entries = u_N*); ``rhs``: ``V^T rhs_terms^T`` with F =
    ``rhs_coef``.  All ``n_terms + 1 + r`` value vectors go through one ``ops.project_csr_batched`` on the one pattern;
    ``vec`` is the row-major flatten of ``mdeim.project_basis``."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    r = V.shape[1]
    indptr, indices = np.asarray(desc["indptr"], dtype=np.int64), np.asarray(desc["indices"], dtype=np.int64)
    values = [np.asarray(desc["mass"], dtype=np.float64)[None, :]]
    A = desc.get("terms")
    n_terms = 0 if A is None else int(np.shape(A)[0])
    if n_terms:
        values.append(np.asarray(A, dtype=np.float64))
    tril = desc.get("tril")
    if tril is not None:
        row_of_entry = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
        values.append(V[row_of_entry, :].T * np.asarray(tril, dtype=np.float64)[None, :])
    data = ops.to_device(np.ascontiguousarray(np.vstack(values).T))                   # nnz x (1 + n_terms + r)
    Vd = ops.to_device(V)
    AN = ops.project_csr_batched(ops.to_device_index(indptr), ops.to_device_index(indices), data, Vd)
    cols = AN.reshape(AN.shape[0], -1).T.contiguous().cpu().numpy()                  # r^2 x (1 + n_terms + r)
    term = lambda basis_rom, **kw: dict(PT_U=np.eye(basis_rom.shape[1]), basis_rom=np.ascontiguousarray(basis_rom), cache={}, **kw)
    tc = None if desc.get("term_coef") is None else np.asarray(desc["term_coef"], dtype=np.float64)
    rc = None if desc.get("rhs_coef") is None else np.asarray(desc["rhs_coef"], dtype=np.float64)
    nt, n_mu = (tc if tc is not None else rc).shape[:2]
    out = dict(mass=term(cols[:, :1], F=np.ones((nt, n_mu, 1))), lin=[], nl=None, rhs=[], dt=float(desc["dt"]),
               bdf2=bool(desc["bdf2"]))
    if n_terms:
        out["lin"].append(term(cols[:, 1:1 + n_terms], F=tc))
    if tril is not None:
        out["nl"] = term(cols[:, 1 + n_terms:], W=np.eye(r))
    f = desc.get("rhs_terms")
    if f is not None and np.shape(f)[0]:
        fN = ops.gemm_tn(Vd, ops.to_device(np.ascontiguousarray(np.asarray(f, dtype=np.float64).T))).cpu().numpy()
        out["rhs"].append(term(fN, F=rc))
    return out


def _affine_terms(rom, mus):
    """``hrom_terms_from_affine`` with the projections kept per model (against the identity of the basis): a second
    ``solve`` only evaluates the coefficient tables."""
    desc = rom.fom.descriptor(mus)
    if operators(rom)["nl"] is None and desc.get("tril") is not None:
        raise NotImplementedError(f"the descriptor has a state-dependent term and {type(rom).__name__} has no such "
                                  "operator; ONLINE_ON = 'host' serves this model")
    hit = _cache(rom).get("affine")
    if hit is None or hit[0] is not rom.basis:
        hit = (rom.basis, hrom_terms_from_affine(desc, rom.basis))
        _cache(rom)["affine"] = hit
    kept = hit[1]
    nt, n_mu = np.shape(desc["term_coef"] if desc.get("term_coef") is not None else desc["rhs_coef"])[:2]
    out = dict(kept, mass=dict(kept["mass"], F=np.ones((nt, n_mu, 1))), dt=float(desc["dt"]), bdf2=bool(desc["bdf2"]))
    out["lin"] = [dict(t, F=np.asarray(desc["term_coef"], dtype=np.float64)) for t in kept["lin"]]
    out["rhs"] = [dict(t, F=np.asarray(desc["rhs_coef"], dtype=np.float64)) for t in kept["rhs"]]
    return out


def terms(rom, mus, route=None) -> dict:
    """The dict ``hrom_bdf_sweep`` takes - ``mass``, ``lin``, ``nl`` (None for the linear classes), ``rhs``, ``dt``,
    ``bdf2`` - for the parameter points ``mus`` on the model's own time grid.  ``route``: None = ``plan(rom)``;
    "callbacks" may be asked for where the plan says "closed_form".  Reductor terms carry the reductor's device cache
    (``cache``), where ``fold`` keeps what it solved."""
    planned = plan(rom)
    route = planned if route is None else route
    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}, not {route!r}")
    if route != planned and not (planned == "closed_form" and route == "callbacks"):
        raise NotImplementedError(f"route {route!r} is not open to this model: its route is {planned!r}")
    mus = list(mus)
    if route == "affine":
        return _affine_terms(rom, mus)
    fom, ts = rom.fom, times(rom.fom)
    table, source, reds = _reductors(rom)
    if route == "closed_form":
        closed = _ClosedForm(fom, mus, ts)
        F = lambda name: closed.table(name, reds[name])
    else:
        F = lambda name: _callback_table(reds[name], mus, ts)
    out = dict(mass=_term(reds["mass"], F("mass")), lin=[_term(reds[n], F(n)) for n in table["lin"]], nl=None,
               rhs=[_term(reds[n], F(n)) for n in source], dt=fom.dt, bdf2=(fom.BDF_SCHEME == BDF.TWO))
    if table["nl"]:
        red = reds[table["nl"]]
        W, c0 = _state_map(rom, red, route, mus, ts)
        if isinstance(c0, torch.Tensor):
            C = c0.expand(len(ts), len(mus), c0.numel()).contiguous()
        else:
            C = np.broadcast_to(c0, (len(ts), len(mus), c0.size)).copy()
        out["nl"] = dict(PT_U=red.PT_U, basis_rom=red.basis_rom, W=W, C=C, cache=red._dev_cache)
    return out


# ---- fold cache and the sweep -----------------------------------------------------------------------------------------
def fold(term) -> torch.Tensor:
    """``sweep.fold_term`` of a term, kept on the device in the term's ``cache`` (a reductor's ``_dev_cache``) against
    the identities of ``PT_U`` and ``basis_rom``, as ``interpolation.fold`` keeps ``Psi``: ``project_basis`` assigns a new
    ``basis_rom``, which invalidates it.  A per-mu ``solve`` then pays for no r^2 solves."""
    from .sweep import fold_term

    PT_U, basis_rom, cache = term["PT_U"], term["basis_rom"], term.get("cache")
    hit = None if cache is None else cache.get("online_fold")
    if hit is not None and hit[0] is PT_U and hit[1] is basis_rom:
        return hit[2]
    Zt = fold_term(PT_U, basis_rom)
    if cache is not None:
        cache["online_fold"] = (PT_U, basis_rom, Zt)
    return Zt


def sweep(rom, tm) -> torch.Tensor:
    """``hrom_bdf_sweep`` of the terms ``tm`` with the model's reduced solver (``REDUCED_SOLVER`` / ``GMRES_OPTIONS``) and
    the cached folds: ``uN`` (n_mu, nt, r) on the device."""
    from .sweep import hrom_bdf_sweep

    folded = lambda t: None if t is None else dict(t, Zt=fold(t))
    solver = rom.REDUCED_SOLVER
    return hrom_bdf_sweep(folded(tm["mass"]), [folded(t) for t in tm["lin"]], folded(tm["nl"]), [folded(t) for t in tm["rhs"]],
                          tm["dt"], tm["bdf2"], solver=solver, gmres_options=rom.GMRES_OPTIONS if solver == "gmres" else None)


# ---- the classes' bookkeeping -------------------------------------------------------------------------------------------
def lifting(fom, mus, ts):
    """The lifting function of every (mu, t) as the low-rank operand ``certify`` and ``outputs`` take,
    ``(shapes N_h x q, coef n_mu x nt x q)``: the ramp of ``p1_closed_form()["lift"]``, else the ``g0 + g1 i / nx`` of
    ``p1_fom_recipe()["lift"]``; None for a FOM that states neither."""
    mus = list(mus)
    if hasattr(fom, "p1_closed_form"):
        cf = fom.p1_closed_form(mus, ts)
        if "lift" in cf:
            nx = int(cf["nx"])
            return np.arange(nx + 1) / nx, np.ascontiguousarray(np.asarray(cf["lift"]).T)
    if hasattr(fom, "p1_fom_recipe"):
        lift = np.asarray(fom.p1_fom_recipe(mus, ts)["lift"])                      # (nt, n_mu, 2)
        Nh = int(fom.nx) + 1
        return np.column_stack([np.ones(Nh), np.arange(Nh) / (Nh - 1)]), np.ascontiguousarray(lift.transpose(1, 0, 2))
    return None


class OnlineSolutions:
    """What ``solve_many`` returns: ``idx`` (the models' indices of the points), ``mus``, ``ts``, ``uN`` - the reduced
    trajectories (n_mu, nt, r) on the device - and ``storage(j)``, the ``RomSolutionsStorage`` of point j (``rom`` r x nt,
    ``fom`` = V u_N + g_h with ``domain`` and g_h from the model's ``_lifting_on_grid`` per step), lifted when asked for."""

    def __init__(self, rom, idx, mus, ts, uN, storages=None):
        self.idx, self.mus, self.ts, self.uN = list(idx), list(mus), np.asarray(ts), uN
        self._rom, self._V, self._storages = rom, rom._V(), storages

    def __len__(self):
        return len(self.mus)

    def grid(self, j):
        """(domain N_h x nt, g_h N_h x nt) of point j."""
        cols = [self._rom._lifting_on_grid(self.mus[j], t) for t in self.ts]
        return np.hstack([np.asarray(x).reshape(-1, 1) for x, _ in cols]), np.array([np.asarray(g) for _, g in cols]).T

    def storage(self, j, grid=None):
        if self._storages is not None:
            return self._storages[j]
        coef = self.uN[j].T.contiguous()                                             # r x nt
        uh = ops.gemm_nn(self._V, coef).cpu().numpy()
        domain, G = self.grid(j) if grid is None else grid
        return RomSolutionsStorage(ts=list(self.ts), mu=self.mus[j], domain=domain, fom=uh + G, rom=coef.cpu().numpy())


def solve_many(rom, mus, step=Stage.ONLINE, chunk=None) -> OnlineSolutions:
    """``rom.solve_many``: ``add_mu`` for every point in order, one sweep per chunk of at most ``chunk`` points (None:
    all; the chunk bounds the nt x n_mu x m tables), ``rom.solutions`` = the last point's storage as a loop over
    ``solve`` leaves it, ``errors`` / ``exact`` filled when the FOM has an exact solution.  With ``ONLINE_ON = "host"``
    it is that loop, and the object is filled from its results."""
    from . import certify

    mus = list(mus)
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"chunk must be a positive number of points, not {chunk!r}")
    if not rom._online_on_device():
        idx, storages = [], []
        for mu in mus:
            idx.append(rom.solve(mu=mu, step=step))
            storages.append(rom.solutions)
        r, nt = rom.N, int(rom.fom.domain["nt"])
        uN = ops.to_device(np.array([s.rom.T for s in storages]).reshape(len(mus), nt, r))
        return OnlineSolutions(rom, idx, mus, storages[-1].ts if storages else times(rom.fom), uN, storages=storages)
    route = plan(rom)                                        # a model with no device route: before any bookkeeping
    fom, ts = rom.fom, times(rom.fom)
    idx = [rom.add_mu(mu=mu, step=step)[0] for mu in mus]
    per = len(mus) if chunk is None else int(chunk)
    blocks = [sweep(rom, terms(rom, mus[lo:lo + per], route)) for lo in range(0, len(mus), per)]
    uN = torch.cat(blocks, dim=0) if blocks else torch.empty((0, len(ts), rom.N), dtype=torch.float64, device=rom._V().device)
    out = OnlineSolutions(rom, idx, mus, ts, uN)
    last = None
    if fom.exact_solution is not None:
        for j, mu in enumerate(mus):
            exact = {t: rom._exact_on_grid(mu, t) for t in ts}
            last = out.grid(j)
            U = np.array([exact[t] for t in ts]).T - last[1]          # the lifting is not low-rank in general: off the truth
            rom.errors.update({idx[j]: certify.trajectory_errors(out._V, uN[j], U=U)[0]})
            rom.exact.update({idx[j]: exact})
    if mus:
        rom.solutions = out.storage(len(mus) - 1, grid=last)
    return out


def solve(rom, mu, step):
    """``rom.solve(mu, step)`` with ``ONLINE_ON = "device"``: one point through ``solve_many``; returns its index."""
    return solve_many(rom, [mu], step).idx[0]


# ---- the driver's _evaluate ---------------------------------------------------------------------------------------------
class Evaluation(dict):
    """``{idx_mu: {Errors.ESTIMATOR, Errors.ROM, Errors.SACRIFICIAL}}`` (hrom.py:578-584) with, for FOMs that state their
    closed forms, ``mass`` = ``{idx_mu: {ProblemType.ROM: payload, ProblemType.FOM: payload}}`` (hrom.py:604-621) and
    ``probes`` = ``{idx_mu: (nt, len(x))}`` of the ROM; both are empty dicts otherwise.  ``solutions`` holds what
    ``solve_many`` returned per chunk, ``{ProblemType.ROM: [...], ProblemType.SROM: [...]}`` (reduced trajectories and
    storages on demand: nothing of size N_h x nt).  ``residuals`` = ``{idx_mu: {ProblemType.ROM: curve, ProblemType.SROM:
    curve}}``, the full-order residual curves of ``certify.trajectory_residuals``, when asked for (empty otherwise)."""

    def __init__(self):
        super().__init__()
        self.mass, self.probes, self.residuals = {}, {}, {}
        self.solutions = {ProblemType.ROM: [], ProblemType.SROM: []}


def _is_piston(fom, mus, ts):
    """Mass conservation is the piston problem's output: the closed forms hold the lifting ramp and every point its a0."""
    return (hasattr(fom, "p1_closed_form") and all(PistonParameters.A0 in mu for mu in mus)
            and "lift" in fom.p1_closed_form(mus[:1], ts[:1]))


def residuals(rom, mus, which) -> dict:
    """``{idx_mu: curve}``: ``rom.solve_many(mus, step=which)`` and the relative full-order residual of every step of every
    reduced trajectory (``certify.trajectory_residuals``).  No full-order solve is made: the FOM states its step system
    through ``p1_fom_recipe`` (NotImplementedError otherwise)."""
    from . import certify

    mus = list(mus)
    sol = rom.solve_many(mus, step=which)
    curves = certify.trajectory_residuals(rom.fom, sol._V, sol.uN, mus)
    return {i: curves[j] for j, i in enumerate(sol.idx)}


def evaluate(rom, srom, mus, which, fom_solutions=None, gamma=1.4, probes=None, chunk=None, residuals=False) -> Evaluation:
    """``HyperReducedPiston._evaluate`` (hrom.py:504-621) as one call: ``solve_many`` on the ROM and the S-ROM, the FOM
    truth of every point - ``fom_solutions[idx]`` (the validation storage, full solutions N_h x nt), else one device sweep
    of the chunk when the FOM has ``p1_fom_recipe``, else the host ``fom.solve()`` - and the three error curves per point
    from ``certify.evaluate``.  The lifting is the same on both sides of every difference, so the homogeneous parts are
    compared (a stored full solution has its lifting taken off) and the lifting is added only where an output needs it:
    the mass-conservation payloads of the piston problem (``outputs.mass_conservation`` for the ROM,
    ``outputs.snapshot_mass_conservation`` for the FOM) and ``outputs.probes`` at the positions ``probes``.  Points go in
    chunks of ``chunk`` (None: all at once); no N_h x nt matrix of a point outlives its chunk.  ``residuals=True`` adds,
    for a FOM with ``p1_fom_recipe``, ``result.residuals[idx]``: the full-order residual curves of both models
    (``certify.trajectory_residuals``)."""
    from . import certify, outputs
    from . import fom as device_fom

    mus = list(mus)
    fom, ts = rom.fom, times(rom.fom)
    dt, nt = fom.dt, len(ts)
    result = Evaluation()
    per = max(len(mus), 1) if chunk is None else int(chunk)
    if per < 1:
        raise ValueError(f"chunk must be a positive number of points, not {chunk!r}")
    for lo in range(0, len(mus), per):
        part = mus[lo:lo + per]
        sol, ssol = rom.solve_many(part, step=which), srom.solve_many(part, step=which)
        result.solutions[ProblemType.ROM].append(sol)
        result.solutions[ProblemType.SROM].append(ssol)
        lift = lifting(fom, part, ts)
        stored = [None if fom_solutions is None else fom_solutions.get(i) for i in sol.idx]

        def homogeneous(j, full):
            if lift is not None:
                shapes, coef = ops.to_device(lift[0]), ops.to_device(lift[1][j])
                return ops.to_device(full) - (shapes.reshape(shapes.shape[0], -1) @ coef.reshape(nt, -1).T)
            return ops.to_device(np.asarray(full) - sol.grid(j)[1])

        U = [None if full is None else homogeneous(j, full) for j, full in enumerate(stored)]
        need = [j for j, full in enumerate(stored) if full is None]
        if need and hasattr(fom, "p1_fom_recipe"):
            (_, block), = device_fom.fom_sweep(fom, [part[j] for j in need],      # (n_need, nt, N_h), homogeneous
                                               check=getattr(rom, "FOM_CHECK", "dominance"))
            for k, j in enumerate(need):
                U[j] = block[k].T
        else:
            for j in need:
                fom.setup()
                fom.update_parametrization(part[j])
                fom.solve()
                U[j] = homogeneous(j, fom.solutions.fom)
        for j, payload in enumerate(certify.evaluate(sol._V, sol.uN, ssol._V, ssol.uN, U)):
            result[sol.idx[j]] = payload
        if residuals and hasattr(fom, "p1_fom_recipe"):
            rec = device_fom.recipe(fom, part)
            curves = {kind: certify.trajectory_residuals(fom, s._V, s.uN, part, rec=rec)
                      for kind, s in ((ProblemType.ROM, sol), (ProblemType.SROM, ssol))}
            for j in range(len(part)):
                result.residuals[sol.idx[j]] = {kind: c[j] for kind, c in curves.items()}
        if _is_piston(fom, part, ts):
            L = np.ascontiguousarray(np.asarray(fom.p1_closed_form(part, ts)["h"]).T) * int(fom.nx)      # (n_mu, nt)
            mass = outputs.mass_conservation(rom.basis, sol.uN, part, dt, L, gamma=gamma, lift=lift, ts=ts)
            shapes, coef = ops.to_device(lift[0]), ops.to_device(lift[1])
            for j, mu in enumerate(part):
                full = U[j] + shapes.reshape(shapes.shape[0], -1) @ coef[j].reshape(nt, -1).T
                result.mass[sol.idx[j]] = {ProblemType.ROM: mass[j], ProblemType.FOM: outputs.snapshot_mass_conservation(
                    full, mu, dt, L[j], gamma=gamma, ts=ts)}
        if probes is not None and hasattr(fom, "p1_closed_form"):
            L = np.ascontiguousarray(np.asarray(fom.p1_closed_form(part, ts)["h"]).T) * int(fom.nx)
            p = outputs.probes(rom.basis, sol.uN, probes, L, lift=lift)
            for j in range(len(part)):
                result.probes[sol.idx[j]] = p[j]
        del U
    return result
