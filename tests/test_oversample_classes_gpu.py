"""Oversampled (M)DEIM through the loop and the classes on the device (helpers in tests/oversample_cases.py).

* ``ops.deim_oversample`` on the case table: its first m entries are the device greedy's, every added entry is held to the
  long-double scores of its own sequence (the rule of tests/test_oversample_cpu.py), sigma_min never falls.
* The three reductor kinds on the mock piston (nx = 60) with ``OVERSAMPLING = 2`` beside their plain twins: ``run()``, the
  FOM-form interpolant against ``basis_fom @ lstsq(PT_U, f[dofs])`` in NumPy (rtol 1e-7, atol 1e-12: the bar of
  tests/test_configs_gpu.py for an interpolant against its NumPy restatement), the device ``evaluate`` against the host
  ``evaluate`` (the bar of tests/test_interpolation_gpu.py), 1 / sigma_min against the twin's, ``copy`` and ``truncate``.
* The fully hyper-reduced piston model of tests/test_surface.py with every reductor oversampled: ``solve_many`` on the device
  against the host loop at 1.1e-9 (tests/test_online_gpu.py)."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests import interp_cases as ic
from tests import oversample_cases as oc
from tests.online_cases import host_storages, rel

pytestmark = pytest.mark.gpu

ROUTES_BAR = 1.1e-9
ONLINE = "online"


@pytest.fixture(scope="module")
def ops():
    from romtime_amd import ops as _ops

    return _ops


# ---- the loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.TABLE, ids=oc.label)
def test_deim_oversample_is_certified(ops, case):
    f, N, m, m_s = case
    B = oc.basis(f, N, m)
    out = []
    for Phi in (ops.to_device(np.ascontiguousarray(B)), ops.to_device(np.asfortranarray(B))):
        idx0, _, _ = ops.deim_greedy(Phi)
        idx, PT_U, margin, sigma_min = ops.deim_oversample(Phi, idx0, m_s)
        idx, idx0 = idx.cpu().numpy(), idx0.cpu().numpy()
        assert idx.shape == (m_s,) and np.array_equal(idx[:m], idx0)
        assert np.array_equal(PT_U.cpu().numpy(), B[idx]) and margin.shape == (m_s - m,) and sigma_min.shape == (m_s - m + 1,)
        cert = oc.assert_certified(B, idx, m, label=oc.label(case))
        assert np.array_equal(sigma_min, cert.sigma_min)
        err = np.abs(margin - cert.margin)
        assert np.all(err <= 1e-6 * cert.margin + 1e-11), err.max()
        out.append(idx)
    assert np.array_equal(out[0], out[1])          # no margin of the table is a near-tie: both layouts pick the true argmax
    assert np.array_equal(out[0], oc.oversample(B, out[0][:m], m_s)[0])


# ---- the three kinds -------------------------------------------------------------------------------------------------------
KINDS = ("deim", "mdeim", "nmdeim")
TS = [0.3, 1.1, 2.4]


def _reductor(kind, factor):
    """A reductor of the mock piston (nx = 60) whose operator family has rank above one - the system matrix
    M + A + C + N_hat (MDEIM), its product with a fixed state (DEIM), the trilinear form over three states (N-MDEIM) - run
    through its own ``run()``."""
    from scipy.stats.distributions import uniform

    from romtime_amd import (DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation,
                             MatrixDiscreteEmpiricalInterpolationNonlinear)

    solver = ic.mock_solver(60)
    grid = dict(alpha_0=uniform(0.5, 1.0), delta=uniform(0.1, 0.8), omega=uniform(8.5, 3.0))
    tw = {"ts": np.linspace(0.2, 4.5, 8), "num_snapshots": 4}
    x0 = np.sin(np.linspace(0.0, 3.0, solver.Nh)) + 1.5

    def system(mu=None, t=None, entries=None):
        return sum(fn(mu=mu, t=t, entries=entries) for fn in (solver.assemble_mass, solver.assemble_stiffness,
                                                               solver.assemble_convection, solver.assemble_nonlinear_lifting))

    def load(mu=None, t=None, entries=None):
        full = system(mu=mu, t=t) @ x0
        return full if entries is None else full[[int(e[0]) for e in entries]]

    if kind == "deim":
        red = DiscreteEmpiricalInterpolation(name="load", assemble=load, grid=grid, tree_walk_params=tw)
    elif kind == "mdeim":
        red = MatrixDiscreteEmpiricalInterpolation(name="system", assemble=system, grid=grid, tree_walk_params=tw)
    else:
        red = MatrixDiscreteEmpiricalInterpolationNonlinear(name="trilinear", assemble=solver.assemble_trilinear, grid=grid,
                                                            tree_walk_params=tw)
    if factor is not None:
        red.OVERSAMPLING = factor
    if kind == "nmdeim":
        red.setup(rnd=np.random.RandomState(1), u_n=np.linspace(0.0, 1.0, solver.Nh))
        red.run(u_n=ic.mock_states(60))
    else:
        red.setup(rnd=np.random.RandomState(1))
        red.run()
    return red


@pytest.fixture(scope="module", params=KINDS)
def pair(request):
    return request.param, _reductor(request.param, None), _reductor(request.param, 2.0)


def _sigma_min(red):
    return np.linalg.svd(red.PT_U, compute_uv=False)[-1]


def test_run_extends_the_plain_entries(pair):
    kind, plain, over = pair
    m = plain.N
    avail = plain.basis_fom.shape[0]
    assert m >= 2 and np.array_equal(plain.basis_fom, over.basis_fom)        # the same walk: the twin differs in the entries only
    assert plain.PT_U.shape == (m, m) and plain.oversampling_sigma_min is None
    m_s = min(avail, 2 * m)
    assert len(over.dofs) == m_s and over.dofs[:m] == plain.dofs and len(set(over.dofs)) == m_s
    assert over.PT_U.shape == (m_s, m) and np.array_equal(over.PT_U[:m], plain.PT_U)
    assert over.oversampling_margin.shape == (m_s - m,) and over.oversampling_sigma_min.shape == (m_s - m + 1,)
    assert np.array_equal(over.greedy_margin, plain.greedy_margin)
    s_plain, s_over = _sigma_min(plain), _sigma_min(over)
    print(f"OVERSAMPLE-CLASS {kind}: m={m} m_s={m_s} 1/sigma_min {1 / s_plain:.4g} -> {1 / s_over:.4g}")
    assert 1 / s_over <= 1 / s_plain
    assert abs(over.oversampling_sigma_min[0] - s_plain) <= 1e-12 * s_plain and abs(over.oversampling_sigma_min[-1] - s_over) <= 1e-12 * s_over


def test_interpolant_is_the_least_squares_fit(pair):
    kind, _, over = pair
    mu, kw = ic.MOCK_MUS[0], ({"u_n": ic.mock_states(60)[:, 1]} if pair[0] == "nmdeim" else {})
    for t in TS:
        local = over._local_values(mu, t, **kw)
        assert local.shape == (len(over.dofs),)
        expected = over.basis_fom @ np.linalg.lstsq(over.PT_U, local, rcond=None)[0]
        if kind != "deim":
            expected[0] = 1.0
        got = over._interpolate(mu=mu, t=t, which=over.FOM, **kw)
        assert_allclose(got, expected, rtol=1e-7, atol=1e-12)
        public = over.interpolate(mu=mu, t=t, which=over.FOM, **kw)
        assert_allclose(public if kind == "deim" else public.data, expected, rtol=1e-7, atol=1e-12)


def test_device_evaluate_equals_host_evaluate(pair):
    kind, _, over = pair
    host, dev = over.copy(), over.copy()
    for twin in (host, dev):
        assert twin.OVERSAMPLING == 2.0
        if kind == "nmdeim":
            twin.u_n = over.u_n
    dev.EVALUATE_ON = "device"
    host.evaluate(TS, mu_space=ic.MOCK_MUS)
    dev.evaluate(TS, mu_space=ic.MOCK_MUS)
    assert sorted(host.errors_rom) == sorted(dev.errors_rom) == [0, 1]
    for k, mu in enumerate(ic.MOCK_MUS):
        if kind == "deim":
            F, group = np.array([dev.assemble_snapshot(mu, t) for t in TS]).T, 1
        else:
            F, group = ic.mock_samples(dev, mu, TS)
        bar = ic.error_bar(dev.PT_U, F, group)
        a, b = host.errors_rom[k], dev.errors_rom[k]
        print(f"OVERSAMPLE-CLASS {kind} mu {k}: errors {a}, worst |device - host| / bar = {float((np.abs(a - b) / bar).max()):.3e}")
        assert a.shape == b.shape == (len(TS),) and np.all(np.abs(a - b) <= bar), (kind, k, np.abs(a - b), bar)


def test_copy_and_truncate_keep_the_setting(pair):
    kind, plain, over = pair
    twin = over.copy()
    assert twin.__dict__["OVERSAMPLING"] == 2.0 and twin.dofs == over.dofs and np.array_equal(twin.PT_U, over.PT_U)
    assert "OVERSAMPLING" not in plain.copy().__dict__
    if kind == "nmdeim":
        cut, plain_cut = over.truncate(1), plain.truncate(1)
        m = over.N - 1
        assert cut.OVERSAMPLING == 2.0 and cut.N == plain_cut.N == m
        assert cut.PT_U.shape == ((2 * m, m) if m >= 2 else (m, m)) and plain_cut.PT_U.shape == (m, m)
        assert cut.dofs[:m] == plain_cut.dofs and 1 / _sigma_min(cut) <= 1 / _sigma_min(plain_cut)


# ---- the whole model --------------------------------------------------------------------------------------------------
SLOTS = ("mdeim_Mh", "mdeim_Ah", "mdeim_Ch", "mdeim_Nh_hat", "mdeim_Nh", "deim_fgh")


@pytest.fixture(scope="module")
def models():
    """tests.test_surface._fully_hyper_reduced_rom() twice: as it stands, and with ``OVERSAMPLING = 2`` on every reductor
    (the class attribute for the duration of the build, an instance attribute on every reductor afterwards)."""
    from romtime_amd import DiscreteEmpiricalInterpolation
    from tests.test_surface import _fully_hyper_reduced_rom

    fom, plain, mus = _fully_hyper_reduced_rom()
    DiscreteEmpiricalInterpolation.OVERSAMPLING = 2.0
    try:
        fom2, over, _ = _fully_hyper_reduced_rom()
    finally:
        DiscreteEmpiricalInterpolation.OVERSAMPLING = 1.0
    for slot in SLOTS:
        getattr(over, slot).OVERSAMPLING = 2.0
    return dict(fom=fom2, plain=plain, over=over, mus=mus)


def test_every_reductor_of_the_model(models):
    plain, over = models["plain"], models["over"]
    assert np.array_equal(plain.basis, over.basis)
    grown = 0
    for slot in SLOTS:
        p, o = getattr(plain, slot), getattr(over, slot)
        m, avail = p.N, p.basis_fom.shape[0]
        assert np.array_equal(p.basis_fom, o.basis_fom)
        m_s = min(avail, 2 * m) if m >= 2 else m
        assert len(o.dofs) == m_s and o.dofs[:m] == p.dofs and o.PT_U.shape == (m_s, m)
        assert o.basis_rom.shape == p.basis_rom.shape                         # modes, not entries
        print(f"OVERSAMPLE-MODEL {slot}: m={m} m_s={m_s} 1/sigma_min {1 / _sigma_min(p):.4g} -> {1 / _sigma_min(o):.4g}")
        assert 1 / _sigma_min(o) <= 1 / _sigma_min(p) * (1 + 1e-12)
        grown += m_s > m
    assert over.mdeim_Nh.PT_U.shape[0] > over.mdeim_Nh.N and grown >= 2


def test_solve_many_on_the_device_equals_the_host_loop(models):
    from romtime_amd import online

    rom, mus = models["over"], models["mus"]
    rom.mu_space[ONLINE] = []
    host = host_storages(rom, mus, ONLINE)
    rom.mu_space[ONLINE] = []
    rom.ONLINE_ON = "device"
    try:
        tm = online.terms(rom, mus)
        assert tm["nl"]["W"].shape[0] == len(rom.mdeim_Nh.dofs) and tm["mass"]["F"].shape[2] == len(rom.mdeim_Mh.dofs)
        many = rom.solve_many(mus)
    finally:
        del rom.ONLINE_ON
    assert tuple(many.uN.shape) == (len(mus), models["fom"].domain["nt"], rom.N)
    for b in range(len(mus)):
        got, want = many.storage(b), host[b][1]
        d = dict(rom=rel(got.rom, want.rom), fom=rel(got.fom, want.fom))
        print(f"OVERSAMPLE-MODEL solve_many point {b} vs host loop: {d}")
        assert max(d.values()) <= ROUTES_BAR, (b, d)
    # for the record, no bar: how far the extra entries move the trajectories of the plain twin
    plain = models["plain"]
    plain.mu_space[ONLINE] = []
    ref = host_storages(plain, mus, ONLINE)
    for b in range(len(mus)):
        print(f"OVERSAMPLE-MODEL point {b}: oversampled vs plain host loop {rel(host[b][1].fom, ref[b][1].fom):.3e}")
