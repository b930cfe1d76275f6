"""Host logic of the classes' device online stage (romtime_amd/online.py): the route rules, the ONLINE_ON attribute, and
the tables of the affine and the heat-class routes pushed through the oracle's loops (device operators stubbed by the
``cpu_ops`` fixture; the sweep itself runs in tests/test_online_gpu.py)."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import romtime_oracle as oracle
from tests.online_cases import AFFINE_MUS, AFFINE_SIZES, affine_rom, heat_rom, rel

ALL = dict(mass="mdeim_Mh", stiffness="mdeim_Ah", convection="mdeim_Ch", nonlinear_lifting="mdeim_Nh_hat",
           trilinear="mdeim_Nh", forcing="deim_fh", lifting="deim_fgh", rhs="deim_rhs")
NEEDS = {"RomConstructor": ("mass", "stiffness", "rhs"), "RomConstructorMoving": ("mass", "stiffness", "convection", "rhs"),
         "RomConstructorNonlinear": ("mass", "stiffness", "convection", "nonlinear_lifting", "trilinear", "lifting")}


def _model(cls_name, attached, closed_form=False, descriptor=False, r=4):
    import romtime_amd

    fom = SimpleNamespace(domain=dict(nt=3), dt=0.1, BDF_SCHEME="1", exact_solution=None)
    if closed_form:
        fom.p1_closed_form = lambda mus, ts: {}
    if descriptor:
        fom.descriptor = lambda mus: {}
    rom = getattr(romtime_amd, cls_name)(fom=fom, grid=None)
    rom.basis = np.zeros((20, r))
    for name in attached:
        width = r if name in ("forcing", "lifting", "rhs") else r * r
        setattr(rom, ALL[name], SimpleNamespace(basis_rom=np.zeros((width, 2))))
    return rom


@pytest.mark.parametrize("cls_name", sorted(NEEDS))
def test_plan_routes(cls_name):
    from romtime_amd import online

    needs = NEEDS[cls_name]
    assert online.plan(_model(cls_name, needs, closed_form=True)) == "closed_form"
    assert online.plan(_model(cls_name, needs, closed_form=True, descriptor=True)) == "closed_form"
    assert online.plan(_model(cls_name, needs)) == "callbacks"
    assert online.plan(_model(cls_name, (), descriptor=True)) == "affine"
    assert online.plan(_model(cls_name, (), descriptor=True, closed_form=True)) == "affine"
    # some reductors: the missing operators are named, whatever the FOM offers
    for kw in (dict(), dict(closed_form=True), dict(descriptor=True)):
        with pytest.raises(NotImplementedError) as exc:
            online.plan(_model(cls_name, needs[:-2], **kw))
        text = str(exc.value)
        assert all(repr(n) in text for n in needs[-2:]) and not any(repr(n) in text for n in needs[:-2]), text
        assert "ONLINE_ON = 'host'" in text
    # none, and no descriptor
    for kw in (dict(), dict(closed_form=True)):
        with pytest.raises(NotImplementedError) as exc:
            online.plan(_model(cls_name, (), **kw))
        text = str(exc.value)
        assert all(n in text for n in needs) and "descriptor" in text and "ONLINE_ON = 'host'" in text, text
    # r > 128
    with pytest.raises(NotImplementedError, match="at most 128"):
        online.plan(_model(cls_name, needs, closed_form=True, r=129))
    assert online.plan(_model(cls_name, needs, closed_form=True, r=128)) == "closed_form"


def test_plan_source_alternatives_and_stale_projections():
    from romtime_amd import online

    split = ("mass", "stiffness", "forcing", "lifting")
    assert online.plan(_model("RomConstructor", split)) == "callbacks"
    with pytest.raises(NotImplementedError) as exc:                       # forcing without lifting: lifting is what is missing
        online.plan(_model("RomConstructor", ("mass", "stiffness", "forcing")))
    assert "['lifting']" in str(exc.value)
    rom = _model("RomConstructorMoving", NEEDS["RomConstructorMoving"])
    rom.mdeim_Ch.basis_rom = None                                          # attached, never projected
    with pytest.raises(NotImplementedError, match=r"not projected on this basis: \['convection'\].*project_reductors"):
        online.plan(rom)
    rom.mdeim_Ch.basis_rom = np.zeros((9, 2))                              # projected on another basis (r = 3)
    with pytest.raises(NotImplementedError, match="convection"):
        online.plan(rom)
    # a forced route must be open to the model
    with pytest.raises(ValueError):
        online.terms(_model("RomConstructor", NEEDS["RomConstructor"]), [{}], route="fast")
    with pytest.raises(NotImplementedError):
        online.terms(_model("RomConstructor", NEEDS["RomConstructor"]), [{}], route="closed_form")
    with pytest.raises(NotImplementedError):
        online.terms(_model("RomConstructor", NEEDS["RomConstructor"], closed_form=True), [{}], route="affine")


def _small_burgers_rom(cls=None):
    from romtime_amd import RomConstructorNonlinear
    from tests.test_surface import _burgers

    fom = _burgers(True, nx=30, nt=6)
    rng = np.random.RandomState(2)
    x = np.linspace(0.0, 1.0, fom.Nh)
    modes = np.array([np.sin((k + 1) * np.pi * x) for k in range(4)]).T + 1e-3 * rng.standard_normal((fom.Nh, 4))
    modes[0, :] = modes[-1, :] = 0.0
    rom = (cls or RomConstructorNonlinear)(fom=fom, grid=None)
    rom.setup(rnd=0)
    rom.basis = np.linalg.qr(modes)[0]
    return rom


def test_online_on_values_and_truncate(cpu_ops):
    from romtime_amd import RomConstructor, RomConstructorNonlinear

    assert RomConstructor.ONLINE_ON == "host" and RomConstructorNonlinear.ONLINE_ON == "host"
    rom = _small_burgers_rom()
    mu = dict(alpha_0=0.07, delta=0.3, omega=9.0)
    rom.ONLINE_ON = "gpu"
    with pytest.raises(ValueError, match="ONLINE_ON"):
        rom.solve(mu=mu, step="online")
    with pytest.raises(ValueError, match="ONLINE_ON"):
        rom.solve_many([mu])
    assert rom.mu_space["online"] == []                                    # refused before any bookkeeping
    rom.ONLINE_ON = "device"
    rom.mu_space = {"offline": [], "online": [], "validation": []}
    assert rom.truncate(1).ONLINE_ON == "device" and rom.truncate(1).N == rom.N - 1
    del rom.ONLINE_ON
    assert rom.truncate(1).ONLINE_ON == "host"
    # the device route of a model that has none: refused by name, before any bookkeeping
    rom.ONLINE_ON = "device"
    with pytest.raises(NotImplementedError, match="without a hyper-reductor"):
        rom.solve(mu=mu, step="online")
    assert rom.mu_space["online"] == []


def test_default_route_is_the_host_loop(cpu_ops, monkeypatch):
    """ONLINE_ON = "host" (the default): ``solve`` never enters the device route, and ``solve_many`` is the loop over
    ``solve`` - the same bits in ``solutions``, the same indices, the last point's storage left behind."""
    from romtime_amd import online

    mus = [dict(alpha_0=0.07, delta=0.3, omega=9.0), dict(alpha_0=0.09, delta=0.31, omega=10.0)]
    a, b = _small_burgers_rom(), _small_burgers_rom()
    for name in ("plan", "terms", "sweep", "solve"):
        monkeypatch.setattr(online, name, lambda *args, **kw: pytest.fail("the device route was entered"))
    loop = []
    for mu in mus:
        idx = a.solve(mu=mu, step="online")
        loop.append((idx, a.solutions))
    many = b.solve_many(mus)
    assert many.idx == [i for i, _ in loop] == [0, 1] and many.mus == mus
    assert b.mu_space["online"] == a.mu_space["online"] == mus
    assert tuple(many.uN.shape) == (2, 6, 4)
    for j, (_, want) in enumerate(loop):
        got = many.storage(j)
        for field in ("ts", "domain", "fom", "rom"):
            x, y = getattr(got, field), getattr(want, field)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (j, field)
        assert got.mu == want.mu
        assert np.array_equal(many.uN[j].numpy().T, want.rom)
    assert b.solutions is many.storage(1) and np.array_equal(many.ts, a.solutions.ts)
    ref_rom, ref_fom = oracle.rom_solve_nonlinear(a.fom, a.basis, mus[1], solver=np.linalg.solve)
    assert rel(a.solutions.rom, ref_rom) <= 1e-10 and rel(a.solutions.fom, ref_fom) <= 1e-10


@pytest.mark.parametrize("bdf2", [False, True], ids=["bdf1", "bdf2"])
@pytest.mark.parametrize("size", AFFINE_SIZES, ids=lambda s: "N%d_nt%d_r%d" % s)
def test_affine_terms_through_the_oracle(cpu_ops, size, bdf2):
    """hrom_terms_from_affine -> oracle.hrom_solve against the direct loop oracle.rom_solve_nonlinear with an exact
    solver: <= 1e-10 relative (the bar of tests/test_surface.py:207-208)."""
    from romtime_amd import online

    N, nt, r = size
    fom, rom = affine_rom(N, nt, r, bdf2)
    tm = online.hrom_terms_from_affine(fom.descriptor(AFFINE_MUS), rom.basis)
    assert tm["mass"]["basis_rom"].shape == (r * r, 1) and tm["lin"][0]["basis_rom"].shape == (r * r, 3)
    assert tm["nl"]["basis_rom"].shape == (r * r, r) and np.array_equal(tm["nl"]["W"], np.eye(r))
    assert tm["rhs"][0]["basis_rom"].shape == (r, 2) and tm["bdf2"] == bdf2
    for t in [tm["mass"], tm["nl"]] + tm["lin"] + tm["rhs"]:
        assert np.array_equal(t["PT_U"], np.eye(t["basis_rom"].shape[1]))
    worst = 0.0
    for b, mu in enumerate(AFFINE_MUS):
        got = oracle.hrom_solve(tm["mass"], tm["lin"], tm["nl"], tm["rhs"], b, r, nt, tm["dt"], tm["bdf2"])
        want, _ = oracle.rom_solve_nonlinear(fom, rom.basis, mu, solver=np.linalg.solve)
        worst = max(worst, rel(got, want))
        assert np.abs(want).max() > 1e-6
    print(f"affine terms vs direct loop, N={N} nt={nt} r={r} bdf2={bdf2}: {worst:.3e}")
    assert worst <= 1e-10, worst
    # the model's own terms: the same projections (kept per basis), the tables of the points asked for
    assert online.plan(rom) == "affine"
    mine = online.terms(rom, AFFINE_MUS[1:])
    assert np.array_equal(mine["lin"][0]["basis_rom"], tm["lin"][0]["basis_rom"])
    assert np.array_equal(mine["lin"][0]["F"], tm["lin"][0]["F"][:, 1:]) and mine["mass"]["F"].shape == (nt, 2, 1)
    assert online.terms(rom, AFFINE_MUS[:1])["nl"]["basis_rom"] is mine["nl"]["basis_rom"]


@pytest.mark.parametrize("source", ["rhs", "split"])
def test_heat_class_tables_through_the_oracle(cpu_ops, source):
    """RomConstructorMoving on the moving-mesh heat problem, every operator hyper-reduced: the callback tables of
    ``online.terms`` through oracle.hrom_solve equal the class's host loop to 1e-9 (tests/test_surface.py:305).  With
    separate DEIMs on forcing and lifting the host loop projects the FOM's own vectors (rom.py:617-640); both lie in
    two-dimensional spaces here, which the DEIMs reproduce to rounding."""
    from romtime_amd import online

    fom, rom, mus = heat_rom(source)
    assert online.plan(rom) == "closed_form"
    tm = online.terms(rom, mus, route="callbacks")
    assert tm["nl"] is None and len(tm["lin"]) == 2 and len(tm["rhs"]) == (1 if source == "rhs" else 2)
    assert tm["bdf2"] is False and tm["dt"] == fom.dt
    r, nt = rom.N, fom.domain["nt"]
    for b, mu in enumerate(mus):
        rom.solve(mu=mu, step="online")
        host = rom.solutions.rom.copy()
        ref = oracle.hrom_solve(tm["mass"], tm["lin"], tm["nl"], tm["rhs"], b, r, nt, tm["dt"], tm["bdf2"])
        print(f"heat {source} point {b}: tables vs host loop {rel(ref, host):.3e}")
        assert host.shape == ref.shape == (r, nt) and np.abs(host).max() > 1e-3
        assert np.linalg.norm(host - ref) <= 1e-9 * np.linalg.norm(ref), (b, rel(host, ref))
