"""Shared models of the online-stage tests (tests/test_online_cpu.py, tests/test_online_gpu.py): the moving-mesh heat
problem with every operator of ``RomConstructorMoving`` hyper-reduced, the affine Burgers model at the sizes of the issue,
and a FOM wrapper that hides ``p1_closed_form``.  Plain module, not a conftest."""
import numpy as np

AFFINE_SIZES = [(96, 6, 5), (40, 12, 1), (200, 8, 12)]          # (N, nt, r); r = 1 is one of them
AFFINE_MUS = [dict(alpha=0.5 + 0.2 * i, beta=1.0 - 0.1 * i, delta=0.3 + 0.05 * i, omega=7.0 + i) for i in range(3)]
HEAT_MUS = [dict(delta=0.5, beta=3.0, alpha_0=0.6, omega=1.5), dict(delta=1.1, beta=5.5, alpha_0=0.9, omega=2.5)]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def affine_rom(N, nt, r, bdf2):
    """RomConstructorNonlinear on AffineBurgers with a smooth orthonormal basis, no reductor: the "affine" route."""
    from romtime_amd import RomConstructorNonlinear
    from romtime_amd.testing.mock import AffineBurgers

    fom = AffineBurgers(N=N, nt=nt, dt=2e-3, bdf2=bdf2, seed=3)
    rng = np.random.RandomState(0)
    xs = (np.arange(N) + 0.5) / N
    V, _ = np.linalg.qr(np.stack([np.sin((k + 1) * np.pi * xs) for k in range(r)], axis=1) + 1e-3 * rng.standard_normal((N, r)))
    rom = RomConstructorNonlinear(fom=fom, grid=None, name="affine")
    rom.setup(rnd=0)
    rom.basis = V
    return fom, rom


def heat_rom(source):
    """MockHeatEquation on a moving mesh (nx = 40, nt = 10) behind RomConstructorMoving with an MDEIM on mass, stiffness
    and convection and, ``source`` = "rhs": a DEIM on the right-hand side; "split": DEIMs on forcing and lifting."""
    from scipy.stats.distributions import uniform

    from romtime_amd import DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation, RomConstructorMoving
    from romtime_amd.conventions import OperatorType
    from romtime_amd.testing.walk_inputs import heat_problem

    fom, V, _ = heat_problem(True, nx=40, nt=10, r=5)
    rom = RomConstructorMoving(fom=fom, grid=None, name=f"heat-{source}")
    rom.setup(rnd=0)
    rom.basis = V
    grid = dict(delta=uniform(0.3, 1.2), beta=uniform(2.0, 5.0), alpha_0=uniform(0.3, 1.0), omega=uniform(1.0, 2.0))
    tw = {"ts": np.linspace(0.05, 1.0, 8), "num_snapshots": 4}
    matrices = [("mass", fom.assemble_mass, OperatorType.MASS), ("stiffness", fom.assemble_stiffness, OperatorType.STIFFNESS),
                ("convection", fom.assemble_convection, OperatorType.CONVECTION)]
    vectors = {"rhs": [("rhs", fom.assemble_rhs, OperatorType.RHS)],
               "split": [("forcing", fom.assemble_forcing, OperatorType.FORCING),
                         ("lifting", fom.assemble_lifting, OperatorType.LIFTING)]}[source]
    for kind, group in ((MatrixDiscreteEmpiricalInterpolation, matrices), (DiscreteEmpiricalInterpolation, vectors)):
        for name, assemble, which in group:
            red = kind(name=name, assemble=assemble, grid=grid, tree_walk_params=tw)
            red.setup(rnd=np.random.RandomState(1))
            red.run()
            rom.add_hyper_reductor(red, which)
    rom.project_reductors()
    return fom, rom, HEAT_MUS


class HideClosedForm:
    """A FOM as a FEniCS solver presents itself: every attribute of the wrapped model except ``p1_closed_form`` and
    ``p1_fom_recipe``."""

    def __init__(self, fom):
        object.__setattr__(self, "_fom", fom)

    def __getattr__(self, name):
        if name in ("p1_closed_form", "p1_fom_recipe"):
            raise AttributeError(name)
        return getattr(object.__getattribute__(self, "_fom"), name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, "_fom"), name, value)


def host_storages(rom, mus, step):
    """The host loop's storages of ``mus`` (ONLINE_ON = "host" for the duration), with the returned indices."""
    keep = rom.__dict__.get("ONLINE_ON")
    rom.ONLINE_ON = "host"
    try:
        out = []
        for mu in mus:
            idx = rom.solve(mu=mu, step=step)
            out.append((idx, rom.solutions))
        return out
    finally:
        if keep is None:
            del rom.ONLINE_ON
        else:
            rom.ONLINE_ON = keep
