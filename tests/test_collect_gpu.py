"""rt_p1_snapshot_sets and the device route of the offline (M)DEIM walks (``SNAPSHOTS_ON = "device"``) on the GPU.

* Bit rule: for every kind and every way it takes its nodal function, ``ops.p1_snapshot_sets`` equals
  ``ops.p1_local_assembly`` on the replicated operands bit for bit, with every operand and the output inside NaN-poisoned
  guard buffers (tests/guarded.py), at the smallest shapes that reach each edge of the launch.
* Sets against the callbacks: nx = 100, 3 points, 4 instants, 5 states - every operator the three mock FOMs have a closed
  form for against the stacked ``assemble_snapshot`` columns, with the bounds tests/test_p1_assembly_gpu.py applies to this
  kernel family against the same callbacks (rtol 1e-12, atol 1e-14 max|ref|; rhs twice the atol for its one more addition).
* Walk parity, no callbacks, evaluate: ``run()`` and ``evaluate`` on the two routes."""
import numpy as np
import pytest
import torch

from romtime_amd import collect                      # noqa: F401  (without the feature nothing here can run)
from tests import collect_cases as cc
from tests import guarded as gd

pytestmark = pytest.mark.gpu


def _pattern(nx):
    rows, cols = [0], [0]
    for i in range(1, nx):
        rows += [i, i, i]
        cols += [i - 1, i, i + 1]
    rows.append(nx)
    cols.append(nx)
    return np.array(rows), np.array(cols)


def _entries(kind, nx, m, rng):
    """m entries (vector kinds: rows) of the nx-cell operator in no sorted order: entry 0 a live interior one, then both
    Dirichlet rows and entries off the band as far as m allows, the rest drawn from the interior of the tridiagonal
    pattern."""
    if kind in ("load", "load_p2"):
        rows = rng.integers(1, nx, size=m)
        for k, i in enumerate([0, nx][:max(m - 1, 0)]):
            rows[1 + k] = i
        return rows, None
    r, c = _pattern(nx)
    pick = rng.integers(1, r.size - 1, size=m)
    rows, cols = r[pick], c[pick]
    for k, (i, j) in enumerate([(0, 0), (nx, nx), (1, nx - 1), (nx, 0), (0, 1)][:max(m - 1, 0)]):
        rows[1 + k], cols[1 + k] = i, j
    if kind == "convection" and rows[0] == cols[0]:
        cols[0] = rows[0] + 1                                        # its diagonal is zero
    return rows, cols


# kind, mode: how the nodal function arrives
MODES = [("mass", "none"), ("stiffness", "none"), ("convection", "none"), ("trilinear", "fun"), ("trilinear", "ramp"),
         ("load", "fun"), ("load", "ramp"), ("load_p2", "fun"), ("load_p2", "poly")]


def _operands(kind, mode, nx, n_par, n_fun, rng):
    h = rng.uniform(0.1, 0.4, n_par)
    coef = rng.uniform(0.5, 2.0, n_par) * rng.choice([-1.0, 1.0], n_par)
    width = 2 * nx + 1 if kind == "load_p2" else nx + 1
    par = fun = None
    if mode == "fun":
        fun = rng.standard_normal((n_fun, width))
    elif mode == "ramp":
        par = rng.uniform(-2.0, 2.0, n_par)
    elif mode == "poly":
        par = rng.uniform(-2.0, 2.0, (n_par, 3))
    return h, coef, par, fun


def _both(kind, mode, nx, rows, cols, h, coef, par, fun, zero_first=False, beta=0.0, prefill=None, with_coef=True):
    """(snapshot sets in guarded buffers, local assembly on the replicated operands): two (S, m) device tensors.  Asserts
    that nothing outside the output was written, every word of it was, and the operands and their poison are intact."""
    from romtime_amd import ops

    n_par, n_fun, m = h.size, (1 if fun is None else fun.shape[0]), rows.size
    host = dict(h=h.reshape(-1, 1), coef=coef.reshape(-1, 1) if with_coef else None,
                par=None if par is None else par.reshape(n_par, -1), fun=fun)
    dev = {k: (None if v is None else gd.guarded_operand(v)) for k, v in host.items()}
    out = gd.guarded_output((n_par * n_fun, m))
    if prefill is not None:
        out.fill(prefill)
    kw = {}
    if mode == "ramp":
        kw["ramp"] = dev["par"].reshape(-1)
    elif mode == "poly":
        kw["poly"] = dev["par"]
    elif mode == "fun":
        kw["fun"] = dev["fun"]
    rd, cd = ops.to_device_index(rows), (None if cols is None else ops.to_device_index(cols))
    got = ops.p1_snapshot_sets(kind, nx, rd, cd, dev["h"].reshape(-1), coef=None if dev["coef"] is None else dev["coef"].reshape(-1),
                               zero_first=zero_first, out=out.t, beta=beta, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.t.data_ptr()
    assert out.check() == [], out.check()
    for k, v in host.items():
        if v is not None:
            assert gd.operand_intact(dev[k], v) == [], (k, gd.operand_intact(dev[k], v))
    rep = lambda a: None if a is None else np.repeat(a, n_fun, axis=0)
    lkw = {}
    if mode == "ramp":
        lkw["ramp"] = rep(par)
    elif mode == "poly":
        lkw["poly"] = rep(par)
    elif mode == "fun":
        lkw["state"] = np.tile(fun, (n_par, 1))
    ref = ops.p1_local_assembly(kind, nx, rd, cd, rep(h), coef=rep(coef) if with_coef else None, **lkw)
    return got, ref


# n_par, n_fun (where the kind takes functions), nx, m
SHAPES = [(3, 2, 2, 9), (3, 2, 60, 1), (3, 2, 60, 127), (3, 2, 60, 128), (3, 2, 60, 129), (1, 1, 60, 255), (1, 1, 60, 256),
          (1, 1, 60, 257), (5, 1, 60, 129), (257, 256, 4, 3), (64, 128, 100, 298)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("kind,mode", MODES, ids=[f"{k}-{m}" for k, m in MODES])
def test_bit_rule_in_guard_buffers(kind, mode, shape):
    """nx = 2: one interior row, every entry of the 3 x 3 matrix; m = 1, 127, 128, 129 and 255, 256, 257: either side of a
    wave pair and of a workgroup's 256 words, alone (one column) and with columns that start inside a workgroup;
    n_fun = 1; 257 x 256 columns of 3 entries: 65792 columns, 771 workgroups whose lanes cross column ends; 64 x 128 x 298 =
    2.4 x 10^6 words: more than the 8192 workgroups of one pass, so the grid stride runs."""
    n_par, n_fun, nx, m = shape
    if mode != "fun":
        if (n_par, n_fun) == (257, 256):
            n_par, n_fun = 257 * 256, 1                        # the same 65792 columns, as parameter rows
        elif n_fun > 1 and n_par > 3:
            n_par, n_fun = n_par * n_fun, 1
        else:
            n_fun = 1
    rng = np.random.default_rng(1000 * len(kind) + 10 * len(mode) + m)
    if nx == 2:
        rows, cols = (np.arange(3), None) if kind in ("load", "load_p2") else [a.reshape(-1) for a in np.divmod(np.arange(9), 3)]
    else:
        rows, cols = _entries(kind, nx, m, rng)
    h, coef, par, fun = _operands(kind, mode, nx, n_par, n_fun, rng)
    got, ref = _both(kind, mode, nx, rows, cols, h, coef, par, fun)
    assert got.shape == ref.shape == (n_par * n_fun, rows.size)
    assert torch.equal(got, ref), gd.mismatch(got.cpu().numpy(), ref.cpu().numpy())
    assert not torch.isnan(got).any()                           # beta = 0: the NaN payload of the output buffer is not read
    if kind != "convection" and got.shape[0] > 1:
        assert not torch.equal(got[0], got[-1])                 # the columns differ: an index slip would show


@pytest.mark.parametrize("kind,mode", MODES, ids=[f"{k}-{m}" for k, m in MODES])
def test_zero_first_beta_and_no_coef(kind, mode):
    """zero_first touches entry 0 of every column and nothing else; beta = 1 is the sum of two calls rounded once per
    entry (and reads what beta = 0 does not); coef = NULL is coef = 1."""
    nx, m, n_par, n_fun = 40, 37, 6, (3 if mode == "fun" else 1)
    rng = np.random.default_rng(7 + len(kind) + len(mode))
    rows, cols = _entries(kind, nx, m, rng)
    h, coef, par, fun = _operands(kind, mode, nx, n_par, n_fun, rng)
    plain, ref = _both(kind, mode, nx, rows, cols, h, coef, par, fun)
    assert torch.equal(plain, ref) and bool((plain[:, 0] != 0).all())
    zeroed, _ = _both(kind, mode, nx, rows, cols, h, coef, par, fun, zero_first=True)
    assert torch.equal(zeroed[:, 1:], plain[:, 1:]) and bool((zeroed[:, 0] == 0).all())
    start = rng.standard_normal((n_par * n_fun, m))
    summed, _ = _both(kind, mode, nx, rows, cols, h, coef, par, fun, beta=1.0, prefill=start)
    assert torch.equal(summed, torch.from_numpy(start).cuda() + plain)
    scaled, _ = _both(kind, mode, nx, rows, cols, h, coef, par, fun, beta=-0.5, prefill=start, zero_first=True)
    assert torch.equal(scaled, -0.5 * torch.from_numpy(start).cuda() + zeroed)
    none, ref1 = _both(kind, mode, nx, rows, cols, h, np.ones(n_par), par, fun, with_coef=False)
    one, _ = _both(kind, mode, nx, rows, cols, h, np.ones(n_par), par, fun)
    assert torch.equal(none, one) and torch.equal(none, ref1)


def test_more_than_2_to_32_words():
    """4099 x 2^20 words: past the 32-bit index arithmetic of the narrow kernel.  Sampled columns - the first, the last, and
    the ones around words 2^31 and 2^32 - against rt_p1_local_assembly of those columns; 34 GB, so it needs the room."""
    from romtime_amd import ops

    nx, m, n_par, n_fun = 1500, 4099, 1024, 1024
    need = 8 * m * n_par * n_fun
    if torch.cuda.mem_get_info()[0] < need + (4 << 30):
        pytest.skip("less than 38 GB of device memory free")
    rng = np.random.default_rng(11)
    rows, cols = _entries("trilinear", nx, m, rng)
    h, coef = rng.uniform(0.1, 0.4, n_par), rng.uniform(0.5, 2.0, n_par)
    fun = rng.standard_normal((n_fun, nx + 1))
    rd, cd = ops.to_device_index(rows), ops.to_device_index(cols)
    out = ops.p1_snapshot_sets("trilinear", nx, rd, cd, h, coef=coef, fun=fun)
    assert tuple(out.shape) == (n_par * n_fun, m) and out.numel() > 2 ** 32
    S = n_par * n_fun
    around = lambda word: [word // m - 1, word // m, word // m + 1]
    picks = sorted(set([0, 1, S - 2, S - 1] + around(2 ** 31) + around(2 ** 32 - 1) + around(2 ** 32)))
    p, f = np.divmod(np.array(picks), n_fun)
    ref = ops.p1_local_assembly("trilinear", nx, rd, cd, h[p], coef=coef[p], state=fun[f])
    assert torch.equal(out[torch.as_tensor(picks, device=out.device)], ref)
    del out
    torch.cuda.empty_cache()


# ---- sets against the callbacks ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def set_differences():
    """Filled by the test below: (fom, kind) -> largest |device - callbacks| / max|callbacks| over the sets."""
    return {}


@pytest.mark.parametrize("which,kind", cc.CASES, ids=[f"{w}-{k}" for w, k in cc.CASES])
def test_sets_against_the_callbacks(which, kind, set_differences):
    from romtime_amd.conventions import EmpiricalInterpolation as EI

    fom, mus = cc.make_fom(which), cc.mus_of(which)
    red = cc.make_reductor(fom, kind, mus)
    u_n = red.u_n if kind == "trilinear" else None
    ref = cc.callback_columns(red, mus, cc.TS, u_n)
    per_mu = ref.shape[1] // len(mus)
    scale = np.abs(ref).max()
    atol = (2e-14 if kind == "rhs" else 1e-14) * scale
    worst = 0.0
    for j, mu in enumerate(mus):
        want = ref[:, j * per_mu:(j + 1) * per_mu].copy()
        exact = collect.exact_snapshots(red, mu, cc.TS, funcs=u_n).cpu().numpy()
        if red.TYPE != EI.DEIM:
            assert np.all(want[0] == 1.0) and np.all(exact[0] == 1.0)
        if kind == "trilinear":
            sets = collect.state_level_sets(red, mu, cc.TS, u_n)
            assert len(sets) == len(cc.TS) and all(tuple(S.shape) == (len(red.rows), cc.N_PSI) and S.stride(0) == 1 for S in sets)
            assert sets[1].data_ptr() == sets[0].data_ptr() + 8 * cc.N_PSI * len(red.rows)        # views of one buffer
            got = np.hstack([S.cpu().numpy() for S in sets])
        else:
            S = collect.time_level_set(red, mu, cc.TS)
            assert tuple(S.shape) == (want.shape[0], len(cc.TS)) and S.stride(0) == 1           # column-major, as the POD takes it
            got = S.cpu().numpy()
        worst = max(worst, np.abs(exact - want).max() / scale)
        print(f"{which}-{kind} mu {j}: max |device - callbacks| = {np.abs(exact - want).max():.3e}, max |callbacks| = {scale:.3e}, "
              f"worst relative entry = {np.max(np.abs(exact - want) / np.maximum(np.abs(want), 1e-300)):.3e}")
        np.testing.assert_allclose(exact, want, rtol=1e-12, atol=atol)
        zeroed = want.copy()
        if red.TYPE != EI.DEIM:
            zeroed[0] = 0.0                                       # deim.py:388-389, nonlinear.py:443
            assert np.all(got[0] == 0.0)
        np.testing.assert_allclose(got, zeroed, rtol=1e-12, atol=atol)
        assert np.array_equal(got[1:], exact[1:])                 # the zeroed entry is the only difference
    set_differences[(which, kind)] = worst


# ---- walks: parity, no callbacks ---------------------------------------------------------------------------------------------

TOL_CASES = (("deim_tol", {"tol_mu": 1.0 - 1e-9, "tol_time": 1.0 - 1e-10}), ("rb_tol", {"tol_time": 1.0 - 1e-11, "tol_mu": 1.0 - 1e-10}))
WALK_TS = list(np.linspace(0.05, 0.95, 7))


PISTON_KINDS = ("mass", "stiffness", "convection", "nonlinear_lifting", "lifting", "trilinear")     # the six hyper-reductors
# The piston's convection operator is constant and its lifting load one pattern times a scalar: sets of rank one.  The
# reference's energy rule is strict (pod.py:46-57: the mode that crosses ``tol`` is excluded), so a ``tol`` walk keeps no
# mode of them on either route; they run with the default rule in test_no_callbacks_from_the_six_reductors.
RANK_ONE = ("convection", "lifting")


def _walk_problem(which):
    """heat: ``walk_inputs.heat_problem(moving=True)`` (nx = 160, nt = 40) at its own states' parameter points; piston:
    the Burgers-type FOM of the reduced-basis fixtures with points drawn from ``piston_grid()`` by the reductor's ``rnd``."""
    from romtime_amd.testing import walk_inputs as wi

    if which == "heat":
        fom, _, states = wi.heat_problem(moving=True)
        return fom, None, [dict(mu) for mu, _ in states[:3]], ("mass", "stiffness", "convection", "forcing", "lifting", "rhs")
    return wi.rb_fom(), wi.piston_grid(), None, PISTON_KINDS


def _run(which, kind, params, route):
    fom, grid, mus, _ = _walk_problem(which)
    probe = mus if mus is not None else [dict(a0=15.0, omega=10.0, delta=0.3, alpha_0=0.06)]
    red = cc.make_reductor(fom, kind, probe, ts=WALK_TS, params=dict(params, num_snapshots=3), grid=grid)
    counter = cc.Counted(fom)
    red.assemble = getattr(fom, "assemble_" + kind)
    red.SNAPSHOTS_ON = route
    space = None if mus is None else [dict(m) for m in mus]
    red.random_state = np.random.RandomState(3)                  # the same rnd on both routes
    if kind == "trilinear":
        red.run(u_n=cc.states(fom.nx, 4), mu_space=space)
    else:
        red.run(mu_space=space)
    return red, counter.calls


def _set_difference(host, dev_route, kind):
    """Largest 2-norm difference between a device set and the callbacks' set over the walk's own parameter points, and the
    largest set norm."""
    from romtime_amd.conventions import Stage

    worst = top = 0.0
    for mu in host.mu_space[Stage.OFFLINE]:
        if kind == "trilinear":
            a = np.hstack([S.cpu().numpy() for S in collect.state_level_sets(dev_route, mu, WALK_TS, host.u_n)])
            b = cc.callback_columns(host, [mu], WALK_TS, host.u_n)
            b[0] = 0.0
        else:
            a = collect.time_level_set(dev_route, mu, WALK_TS).cpu().numpy()
            b = host._time_level_snapshots(mu, WALK_TS)
        worst, top = max(worst, np.linalg.norm(a - b, 2)), max(top, np.linalg.norm(b, 2))
    return worst, top


@pytest.mark.parametrize("which", ("heat", "piston"))
def test_walk_parity_and_no_callbacks(which):
    """``run()`` on the two routes, same rnd and mu_space: the host route makes n_mu len(ts) (x N_psi) callbacks, the device
    route none; the reports' integers are equal, spectra and spans within tests/test_walks.py's bounds for the measured
    set difference, dofs identical wherever test_walks._check_dofs' own condition holds on the host result."""
    from romtime_amd.conventions import Stage
    from tests.test_walks import C_BW, EPS, _boundary_error, _has_cluster, _span_check, _spectrum_check

    kinds = [k for k in _walk_problem(which)[3] if which == "heat" or k not in RANK_ONE]
    pinned = {}
    for label, params in TOL_CASES:
        for kind in kinds:
            host, n_host = _run(which, kind, params, "host")
            dev, n_dev = _run(which, kind, params, "device")
            n_psi = 4 if kind == "trilinear" else 1
            assert n_host == 3 * len(WALK_TS) * n_psi and n_dev == 0, (kind, n_host, n_dev)
            assert dev.mu_space == host.mu_space and len(host.mu_space[Stage.OFFLINE]) == 3
            a, b = host.report[Stage.OFFLINE], dev.report[Stage.OFFLINE]
            assert sorted(a) == sorted(b)
            key = (which, label, kind)
            assert [a["basis-shape-time"][i] for i in range(3)] == [b["basis-shape-time"][i] for i in range(3)], key
            assert a["basis-shape-after-tree-walk"] == b["basis-shape-after-tree-walk"], key
            assert a["basis-shape-final"] == b["basis-shape-final"] == dev.N == host.N, key
            dX, top = _set_difference(host, dev, kind)
            # what a set difference dX does to a level's kept span (Wedin), beside the level's own boundary error
            E_in = 0.0
            for i in range(3):
                s, kept = np.asarray(a["spectrum-time"][i]), int(a["basis-shape-time"][i])
                scale = 1.0 if kind != "trilinear" else top          # N-MDEIM normalises its sets: spectra of unit columns
                rel = dX / top if kind == "trilinear" else dX
                nxt = s[kept] if kept < len(s) else 0.0
                E_in = max(E_in, _boundary_error(s, kept) + rel / max(s[kept - 1] - nxt, 1e-300))
                _spectrum_check(b["spectrum-time"][i], s, (10.0 if kind == "trilinear" else 1.0) * rel / s[0], key + ("time", i))
            if kind == "trilinear":
                E_in *= 10.0                                       # two inner levels, as tests/test_walks.py allows
            print(f"{key}: set difference {dX:.3e} of {top:.3e}, E_in {E_in:.3e}, kept {a['basis-shape-final']}")
            _spectrum_check(b["spectrum-mu"], a["spectrum-mu"], E_in, key + ("mu",))
            s_mu = np.asarray(a["spectrum-mu"])
            _span_check(dev.basis_fom, host.basis_fom, s_mu, E_in, key)
            gaps = np.abs(np.diff(s_mu[: host.N + 1]))
            basis_tol = 1e-9 + (E_in + C_BW * EPS * s_mu[0]) / max(gaps.min(), 1e-300) if gaps.size else 1e-9
            if not _has_cluster(s_mu, host.N) and basis_tol < 1e-3 * np.min(host.greedy_margin):
                assert dev.dofs == host.dofs, key
                pinned.setdefault(type(host).__name__, []).append(key)
    print("dofs compared exactly:", pinned)
    if which == "heat":
        for name in ("DiscreteEmpiricalInterpolation", "MatrixDiscreteEmpiricalInterpolation"):
            assert pinned.get(name), (name, pinned)               # at least one case per class pins the indices
    else:
        # The bare trilinear form does not depend on (mu, t) (testing/walk_inputs.py: walk_state_operator says why), so
        # every level of the N-MDEIM walk stacks copies of ONE subspace and its kept singular values coincide: a cluster,
        # where _check_dofs' condition cannot hold and any rotation of the basis is a valid answer.  No closed-form
        # N-MDEIM case can pin the indices; its counts and spectra are held above.
        assert "MatrixDiscreteEmpiricalInterpolationNonlinear" not in pinned


def test_no_callbacks_from_the_six_reductors():
    """The six hyper-reductors of the piston workflow with the default truncation rule: the host ``run()`` makes
    n_mu len(ts) callbacks (x N_psi for N-MDEIM), the device ``run()`` none, and the reports' integers agree."""
    from romtime_amd.conventions import Stage

    for kind in PISTON_KINDS:
        host, n_host = _run("piston", kind, {}, "host")
        dev, n_dev = _run("piston", kind, {}, "device")
        assert n_host == 3 * len(WALK_TS) * (4 if kind == "trilinear" else 1) and n_dev == 0, (kind, n_host, n_dev)
        a, b = host.report[Stage.OFFLINE], dev.report[Stage.OFFLINE]
        assert dev.mu_space == host.mu_space and sorted(a) == sorted(b)
        assert a["basis-shape-time"] == b["basis-shape-time"] and len(a["basis-shape-time"]) == 3, kind
        assert a["basis-shape-after-tree-walk"] == b["basis-shape-after-tree-walk"], kind
        assert a["basis-shape-final"] == b["basis-shape-final"] == dev.N == host.N >= 1, kind


# ---- evaluate --------------------------------------------------------------------------------------------------------------------

EVALUATE_CASES = [("burgers", "mass"), ("burgers", "stiffness"), ("burgers", "nonlinear_lifting"), ("burgers", "trilinear"),
                  ("heat", "convection"), ("heat", "rhs")]


@pytest.mark.parametrize("which,kind", EVALUATE_CASES, ids=[f"{w}-{k}" for w, k in EVALUATE_CASES])
def test_device_evaluate_without_callbacks(which, kind):
    """Both attributes on "device": ``evaluate`` returns what it returns with ``SNAPSHOTS_ON = "host"`` to rtol 1e-9 and
    makes no callback; ``evaluate_closed_form(..., "trilinear", funcs=V)`` equals N-MDEIM's ``evaluate``.  One trained
    reductor for both.  The sets have rank 2 to 5 and the reference's energy rule excludes the mode that crosses ``tol``
    (pod.py:46-57), so every basis lacks a direction the snapshots have and the errors are truncation errors - 1e-9 of a
    rounding-level error would be nothing to hold anyone to."""
    from romtime_amd import interpolation
    from romtime_amd.conventions import Stage

    mus = cc.mus_of(which)
    test_mus = [dict(m, alpha_0=1.1 * m["alpha_0"], delta=0.9 * m["delta"], omega=1.05 * m["omega"]) for m in mus[:2]]
    fom = cc.make_fom(which)
    red = cc.make_reductor(fom, kind, mus, params={"tol_mu": 1.0 - 1e-12, "tol_time": 1.0 - 1e-12})
    if kind == "trilinear":
        red.run(u_n=cc.states(), mu_space=mus)
    else:
        red.run(mu_space=mus)
    counter = cc.Counted(fom)
    red.assemble = getattr(fom, "assemble_" + kind)
    results = {}
    for route in ("host", "device"):
        twin = red.copy()
        twin.u_n = red.u_n if kind == "trilinear" else None
        twin.EVALUATE_ON, twin.SNAPSHOTS_ON = "device", route
        before = counter.calls
        twin.evaluate(cc.TS, mu_space=[dict(m) for m in test_mus])
        results[route] = (twin, counter.calls - before)
    (host, n_host), (dev, n_dev) = results["host"], results["device"]
    assert n_host == len(test_mus) * len(cc.TS) * (cc.N_PSI if kind == "trilinear" else 1) and n_dev == 0
    assert dev.mu_space[Stage.ONLINE] == host.mu_space[Stage.ONLINE] == test_mus
    assert sorted(dev.errors_rom) == sorted(host.errors_rom) == [0, 1]
    for k in host.errors_rom:
        assert dev.errors_rom[k].shape == (len(cc.TS),)
        print(f"{which}-{kind} mu {k}: host-snapshot errors {host.errors_rom[k]}, device-snapshot errors {dev.errors_rom[k]}")
        assert host.errors_rom[k].min() > 1e-7                     # truncation errors, not rounding
        np.testing.assert_allclose(dev.errors_rom[k], host.errors_rom[k], rtol=1e-9)
    if kind == "trilinear":
        V = cc.states()[:, :3] * 1.5
        got = interpolation.evaluate_closed_form(dev, "trilinear", fom, test_mus, cc.TS, funcs=V, max_columns=6)
        twin = red.copy()
        twin.u_n, twin.EVALUATE_ON = red.u_n, "device"
        twin.evaluate(cc.TS, funcs=V, mu_space=[dict(m) for m in test_mus])
        assert got.shape == (len(test_mus), len(cc.TS))
        for k in range(len(test_mus)):
            np.testing.assert_allclose(got[k], twin.errors_rom[k], rtol=1e-9)
