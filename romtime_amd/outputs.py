"""Physical outputs of whole sweep trajectories on the device: the third block of ``HyperReducedPiston._evaluate``
(rom/hrom.py:586-621) - the mass ``int rho(u) dx`` on the moving mesh, its time derivative and the piston outflow
(``compute_mass_conservation``, fom/nonlinear.py:601-683), and the probes (``SolutionsStorage.compute_at``,
base.py:45-67) - for the ``(n_mu, nt, r)`` trajectories the online sweeps return (``romtime_amd.sweep``).

The integrals go through ``ops.trajectory_integrals`` (rt_trajectory_integrals): the lifted trajectories ``V u_N`` are
never stored.  The mesh is the uniform 1-D P1 mesh of the piston problem, node i of nx + 1 at ``x = L(mu, t) i / nx``: the
rows of the basis are the nodes in that order (node 0 at x = 0, the outflow; the last node at the piston).  Results are
NumPy arrays.

Unverified: ``points = 2`` is what FEniCS is remembered to use for ``assemble(rho * dx)`` - UFL estimates the degree of a
power with a non-integer exponent as degree(base) + 2 = 3, and ``2.0 / (1.4 - 1.0)`` is 5.000000000000001, not an integer;
FEniCS was not at hand to confirm it.  With another rule the curves differ by the quadrature error, not by rounding."""
from __future__ import annotations

import numpy as np
import torch

from . import certify, ops
from .conventions import MassConservation, PistonParameters, ProblemType

MAX_POINTS = 4


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def gauss_unit_interval(points):
    """Gauss-Legendre points and weights of [0, 1]."""
    if points not in range(1, MAX_POINTS + 1):
        raise ValueError(f"points must be 1 .. {MAX_POINTS}, not {points!r}")
    x, gw = np.polynomial.legendre.leggauss(points)
    return 0.5 * (x + 1.0), 0.5 * gw


def quadrature_basis(B, points=2):
    """``(E, w)`` on the device for a uniform 1-D P1 mesh whose nodes are the rows of ``B`` (nx + 1 of them, in mesh order):
    ``E = (1 - xi_g) B[:-1] + xi_g B[1:]`` stacked over the Gauss-Legendre points ``xi_g`` of [0, 1] (points x nx rows), and
    ``w = gw_g / nx``, the weights of the unit interval - the domain length is the ``scale`` of the integral.  ``points``:
    1 .. 4; the default 2 is exact for cubics, and is the rule FEniCS is remembered to pick for the reference's
    ``assemble(rho * dx)`` - unverified, see the module docstring."""
    xi, gw = gauss_unit_interval(points)
    B = ops.to_device(B)
    if B.dim() != 2 or B.shape[0] < 2:
        raise ValueError("the basis must be (nx + 1) x k with at least one cell")
    nx = B.shape[0] - 1
    E = torch.cat([(1.0 - float(x)) * B[:-1] + float(x) * B[1:] for x in xi], dim=0).contiguous()
    w = torch.cat([torch.full((nx,), float(g) / nx, dtype=torch.float64, device=B.device) for g in gw])
    return E, w


def _gas(gamma):
    gamma = float(gamma)
    if not gamma > 1.0:
        raise ValueError("gamma must exceed 1")
    return (gamma - 1.0) / 2.0


def density(gamma=1.4):
    """``fn`` of ``compute_rho`` (fom/nonlinear.py:601-612): rho = (1 - (gamma - 1) / 2 u)^(2 / (gamma - 1))."""
    return ("power", 1.0, -_gas(gamma), 2.0 / (float(gamma) - 1.0))


def pressure(gamma=1.4):
    """``fn`` of ``compute_p`` (fom/nonlinear.py:614-625): p = (1 - (gamma - 1) / 2 u)^(2 gamma / (gamma - 1))."""
    return ("power", 1.0, -_gas(gamma), 2.0 * (float(gamma) / (float(gamma) - 1.0)))


def _length(length, n_mu, nt):
    """The domain lengths as an (n_mu, nt) device tensor; (nt,) serves a single trajectory."""
    if length is None:
        return None
    L = ops.to_device(length)
    if L.dim() == 1 and n_mu == 1:
        L = L.unsqueeze(0)
    if tuple(L.shape) != (n_mu, nt):
        raise ValueError(f"length must be (n_mu, nt) = ({n_mu}, {nt}), not {tuple(L.shape)}: p1_closed_form()['h'] is "
                         "(nt, n_mu), so pass p1_closed_form()['h'].T * nx")
    return L.contiguous()


def trajectory_integrals(V, uN, fn, lift=None, length=None, points=2):
    """``length[j, t] * int_0^1 f(u_j(t))`` for every parameter point j and step t, u = V u_N + g_h the P1 function on the
    uniform mesh: an (n_mu, nt) array.  ``uN`` and ``lift`` as ``certify.trajectory_errors`` takes them; ``fn``:
    ``("power", c0, c1, p)`` for f(u) = (c0 + c1 u)^p (``density``, ``pressure``); ``length``: (n_mu, nt) domain lengths
    L(mu_j, t) (None: 1) - NOT the (nt, n_mu) of ``p1_closed_form()["h"] * nx``, which goes in transposed."""
    B, A = certify._operands(V, uN, lift)
    scale = _length(length, A.shape[0], A.shape[1])
    E, w = quadrature_basis(B, points)
    return _host(ops.trajectory_integrals(E, A, w, scale, fn))


def probes(V, uN, x, length, lift=None):
    """u_j(t) at the physical positions ``x`` on the moving uniform mesh, ``np.interp(x, L i / nx, u)`` per step
    (``SolutionsStorage.compute_at`` without its scaling by a0): (n_mu, nt, len(x)).  Positions outside [0, L(mu_j, t)]
    take the end values, as np.interp's do: ``x = [0.0, 0.5, np.inf]`` are the reference's three probes (ProbeLocations:
    outflow, halfway and the moving piston, rom.py:859-875).  ``length`` (n_mu, nt) as for ``trajectory_integrals``.  Two rows of
    [V | lifting shapes] are gathered per (j, t, x) and contracted with the coefficients: n_mu nt k work, no kernel."""
    B, A = certify._operands(V, uN, lift)
    n_mu, nt = A.shape[:2]
    L = _length(length, n_mu, nt)
    if L is None:
        raise ValueError("probes need the domain lengths")
    xs = ops.to_device(np.atleast_1d(np.asarray(x, dtype=np.float64)))
    if xs.dim() != 1:
        raise ValueError("x must be a scalar or a 1-D sequence of positions")
    nx = B.shape[0] - 1
    out = np.empty((n_mu, nt, xs.numel()))
    for j in range(n_mu):                                           # one trajectory at a time: 2 nt len(x) k words gathered
        s = (xs[None, :] / L[j][:, None] * nx).clamp(0.0, float(nx))
        cell = s.floor().clamp(max=float(nx - 1))
        theta = s - cell
        idx = cell.to(torch.int64)
        lo = torch.einsum("tmk,tk->tm", B[idx], A[j])
        hi = torch.einsum("tmk,tk->tm", B[idx + 1], A[j])
        out[j] = _host((1.0 - theta) * lo + theta * hi)
    return out


def _a0(mu):
    return float(mu[PistonParameters.A0]) if isinstance(mu, dict) else float(mu)


def _payload(mass, u0, mus, dt, gamma, which, ts):
    """The dicts of fom/nonlinear.py:662-681 from the mass curves (n_mu, nt) and the values at node 0 (n_mu, nt)."""
    n_mu, nt = mass.shape
    if len(mus) != n_mu:
        raise ValueError(f"{len(mus)} parameter points for {n_mu} trajectories")
    if nt < 3:
        raise ValueError("np.gradient(edge_order=2) needs at least three steps")
    ts = float(dt) * np.arange(nt) if ts is None else np.asarray(ts, dtype=np.float64)
    if ts.shape != (nt,):
        raise ValueError(f"ts must hold the {nt} time steps")
    _, c0, c1, p = density(gamma)
    out = []
    for j, mu in enumerate(mus):
        rho0 = (c0 + c1 * u0[j]) ** p
        out.append({MassConservation.WHICH: which, MassConservation.TIMESTEPS: ts, MassConservation.MASS: mass[j],
                    MassConservation.MASS_CHANGE: np.gradient(mass[j], float(dt), edge_order=2),
                    MassConservation.OUTFLOW: _a0(mu) * (rho0 * u0[j])})
    return out


def mass_conservation(V, uN, mus, dt, length, gamma=1.4, lift=None, which=ProblemType.ROM, points=2, ts=None):
    """The payload of ``compute_mass_conservation`` (fom/nonlinear.py:627-683) for every parameter point: a list of dicts
    with ``MassConservation.WHICH``, ``TIMESTEPS``, ``MASS`` (the integral of the density over the moving domain),
    ``MASS_CHANGE`` (``np.gradient(mass, dt, edge_order=2)``) and ``OUTFLOW`` (a0 rho(u(0)) u(0), from node 0's row).
    ``mus``: the parameter dicts (key ``a0``) or the a0 values; ``length`` (n_mu, nt) as for ``trajectory_integrals``;
    ``ts``: the time steps to report (default dt * arange(nt))."""
    B, A = certify._operands(V, uN, lift)
    mass = trajectory_integrals(V, uN, density(gamma), lift=lift, length=length, points=points)
    u0 = _host(A @ B[0])
    return _payload(mass, u0, list(mus), dt, gamma, which, ts)


def snapshot_mass_conservation(U, mu, dt, length, gamma=1.4, which=ProblemType.FOM, points=2, ts=None):
    """The same rule for one full-order trajectory ``U`` ((nx + 1) x nt, nodes in mesh order), in plain torch: one FOM
    trajectory at a time is bound by its upload, so it gets no kernel - it exists so that the FOM curve follows the same
    quadrature as the ROM's.  ``length``: (nt,).  Returns one dict."""
    Ud = ops.to_device(U)
    if Ud.dim() != 2:
        raise ValueError("U must be (nx + 1) x nt")
    nt = Ud.shape[1]
    L = _length(length, 1, nt)
    if L is None:
        raise ValueError("the mass needs the domain lengths")
    E, w = quadrature_basis(Ud, points)                              # the nodal values are their own basis
    _, c0, c1, p = density(gamma)
    mass = L[0] * (w[:, None] * (c0 + c1 * E) ** p).sum(dim=0)
    return _payload(_host(mass)[None], _host(Ud[0])[None], [mu], dt, gamma, which, ts)[0]
