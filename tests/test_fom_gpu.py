"""rt_p1_fom_bdf_sweep on the device against the extended-precision recipe (tests/fom_cases.py): every partition boundary
read from the plan, the four flag combinations, batches beyond the CU count, guard buffers, bit determinism, the
dominance flag, N_h = 1e5, and the class surface (romtime_amd.fom, RomConstructor.SNAPSHOTS_ON).

Bar: d_dev <= 8 d_host + 64 eps, both relative L2 distances from the long-double truth over the whole block, d_host that
of the float64 host loop (mock.solve()).  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fom_cases as fc
from tests import guarded

pytestmark = pytest.mark.gpu


def _sweep(c, tab=None, **kw):
    from romtime_amd import ops

    tab = c["rec"]["tab"] if tab is None else tab
    U, info = ops.p1_fom_bdf_sweep(c["fom"].nx, tab, c["fom"].dt, c["bdf2"], c["state_in_w"], **kw)
    return U, info


def _hold(c, U, info, what):
    U, info = U.cpu().numpy(), info.cpu().numpy()
    d = fc.rel(U, c["truth"])
    print(f"{what}: d_host {c['d_host']:.3e} d_dev {d:.3e} bar {fc.bar(c['d_host']):.3e} margin {c['margin']:.3e}")
    assert c["margin"] > 0 and not info.any(), info
    assert d <= fc.bar(c["d_host"])
    assert (U[:, :, 0] == 0).all() and (U[:, :, -1] == 0).all()
    return d


@pytest.mark.parametrize("key", fc.row_case_keys(), ids=lambda k: f"{k[0]}-rows{k[1] - 1}")
def test_partition_boundaries(key):
    from romtime_amd import ops

    c = fc.case(*key)
    n = key[1] - 1
    _, parts, rows = ops.p1_fom_plan(key[1])
    assert rows == -(-n // fc.partitions()) and parts == -(-n // rows)
    _hold(c, *_sweep(c), f"{key[0]} interior rows {n} = {parts} partitions x {rows}")


@pytest.mark.parametrize("key", fc.step_case_keys(), ids=lambda k: f"nt{k[2]}-bdf2_{int(k[5][0])}-state_{int(k[5][1])}")
def test_steps_and_flags(key):
    c = fc.case(*key)
    _hold(c, *_sweep(c), f"{key[0]} table, nx {key[1]}, nt {key[2]}, bdf2 {key[5][0]}, state_in_w {key[5][1]}")


@pytest.mark.parametrize("kind", ["burgers", "heat"])
def test_more_points_than_compute_units(kind):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_mu = 2 * cus + 1
    c3 = fc.case(kind, 64, 3, True, 3)
    fom = c3["fom"]
    rec = fc.recipe(fom, fc.mus_of(kind, n_mu))
    U, info = _sweep(c3, tab=rec["tab"])
    assert tuple(U.shape) == (n_mu, 3, 65)
    pick = np.arange(n_mu) % 3
    wide = dict(c3, truth=c3["truth"][pick], d_host=fc.rel(c3["host"][pick], c3["truth"][pick]))
    _hold(wide, U, info, f"{kind} {n_mu} points on {cus} CUs")
    U3, _ = _sweep(c3)
    assert torch.equal(U, U3[torch.from_numpy(pick).to(U.device)])      # a point's bits do not depend on the batch


@pytest.mark.parametrize("kind,nx", [("burgers", 64), ("heat", 2 * fc.partitions() + 2)])
def test_nothing_written_outside_the_trajectories(kind, nx):
    from romtime_amd import _lib
    from romtime_amd._lib import Context

    guarded.require_clean_env()
    c = fc.case(kind, nx, 3, True, 3)
    Nh, nt, n_mu = nx + 1, 3, 3
    ld, slots = Nh + 5, nt + 2                                         # padded steps, padded trajectories
    out = guarded.guarded_output((n_mu * slots, Nh), ld=ld, misalign=True)
    U = out.buf.as_strided((n_mu, nt, Nh), (slots * ld, ld, 1), out.view2d.storage_offset())
    flags = torch.full((n_mu + 64,), -77, dtype=torch.int32, device="cuda")
    init_host = np.zeros((n_mu * 2, Nh))
    init = guarded.guarded_operand(init_host)                          # u_init has no leading dimension: contiguous rows
    tab_host = c["rec"]["tab"].reshape(nt, n_mu * 7)
    tab = guarded.guarded_operand(tab_host)
    ctx = Context.current()
    desc = _lib.FomDesc(nx, n_mu, nt, 0, c["fom"].dt, int(c["bdf2"]), int(c["state_in_w"]), C.c_void_p(tab.data_ptr()),
                        C.c_void_p(init.data_ptr()))
    ctx.check(ctx.lib.rt_p1_fom_bdf_sweep(ctx.handle, C.byref(desc), C.c_void_p(U.data_ptr()), ld, slots * ld,
                                          C.c_void_p(flags[32:].data_ptr())), "rt_p1_fom_bdf_sweep")
    torch.cuda.synchronize()
    got = U.clone()
    assert not (guarded._as_bits(got) == guarded.CANARY_BITS).any()     # every word of every trajectory written
    info = flags[32:32 + n_mu].clone()
    assert (flags[:32] == -77).all() and (flags[32 + n_mu:] == -77).all()
    assert guarded.operand_intact(tab, tab_host) == [] and guarded.operand_intact(init, init_host) == []
    guarded._as_bits(U).fill_(guarded.CANARY_BITS)
    assert (guarded._as_bits(out.buf) == guarded.CANARY_BITS).all()     # ... and not one outside them
    _hold(c, got, info, f"{kind} nx {nx} in guard buffers, zero u_init given")
    plain, _ = _sweep(c)
    assert torch.equal(got, plain)                                      # zero states handed over = no states


def test_bits_do_not_depend_on_batch_place_or_chunking():
    nx = 2 * fc.partitions() + 2
    for kind in ("burgers", "heat"):
        c = fc.case(kind, nx, 4, True, 3, (True, kind == "burgers"))
        tab = c["rec"]["tab"]
        U, info = _sweep(c)
        _hold(c, U, info, f"{kind} nx {nx} nt 4 BDF2")
        again, _ = _sweep(c)
        assert torch.equal(U, again)
        for j in range(3):
            alone, _ = _sweep(c, tab=tab[:, j:j + 1])
            assert torch.equal(alone[0], U[j])
        moved, _ = _sweep(c, tab=tab[:, [2, 2, 0, 1, 0]])
        assert torch.equal(moved, U[[2, 2, 0, 1, 0]])
        zeros = torch.zeros_like(U[:, 0])
        for cut in (1, 2):
            head, _ = _sweep(c, tab=tab[:cut])
            older = head[:, -2] if cut > 1 else zeros
            tail, _ = _sweep(c, tab=tab[cut:], u_init=torch.stack([head[:, -1], older], dim=1), first_step=cut)
            assert torch.equal(torch.cat([head, tail], dim=1), U), (kind, cut)


def test_chunked_fom_sweep_equals_one_call():
    from romtime_amd import fom as dfom

    c = fc.case("burgers", 200, 9, True, 3)
    (_, whole), = dfom.fom_sweep(c["fom"], c["mus"])
    for chunk in (1, 4):
        blocks = list(dfom.fom_sweep(c["fom"], c["mus"], chunk=chunk))
        assert torch.equal(torch.cat([b for _, b in blocks], dim=1), whole)
    with pytest.raises(MemoryError, match="chunk"):
        big = fc.make_fom("heat", 1 << 20, 1 << 20)
        list(dfom.fom_sweep(big, fc.mus_of("heat", 1), rec=dict(tab=np.zeros((1 << 20, 1, 7)), bdf2=False, state_in_w=False)))


def test_dominance_flag_of_one_point():
    from romtime_amd import fom as dfom
    from romtime_amd import ops

    nx, nt, bad = 64, 4, 2
    fom, mus, rec = fc.flag_table(nx, nt, bad)
    _, _, want = fc.truth(nx, rec["tab"], fom.dt, False, False)
    U, info = ops.p1_fom_bdf_sweep(nx, rec["tab"], fom.dt, False, False)
    print("info", info.tolist(), "truth", want.tolist())
    assert info.tolist() == want.tolist() == [0, 1 + bad, 0]
    for j in (0, 2):                                                    # the neighbours keep their bits
        alone, flag = ops.p1_fom_bdf_sweep(nx, rec["tab"][:, j:j + 1], fom.dt, False, False)
        assert flag.tolist() == [0] and torch.equal(alone[0], U[j])
    # a chunk that starts after step 0 reports the GLOBAL step
    head, _ = ops.p1_fom_bdf_sweep(nx, rec["tab"][:1], fom.dt, False, False)
    init = torch.stack([head[:, -1], torch.zeros_like(head[:, -1])], dim=1)
    _, info = ops.p1_fom_bdf_sweep(nx, rec["tab"][1:], fom.dt, False, False, u_init=init, first_step=1)
    assert info.tolist() == [0, 1 + bad, 0]
    with pytest.raises(ArithmeticError, match="step 2"):
        list(dfom.fom_sweep(fom, mus, rec=rec))


@pytest.mark.parametrize("key", fc.size_case_keys(), ids=lambda k: f"{k[0]}-nx{k[1]}")
def test_full_size(key):
    from romtime_amd import ops

    c = fc.case(*key)
    _, parts, rows = ops.p1_fom_plan(key[1])
    assert rows > 64                                                    # many tiles of rows per partition
    _hold(c, *_sweep(c), f"{key[0]} nx {key[1]} ({parts} partitions x {rows} rows), 2 points, 3 steps")


# ---- class surface ---------------------------------------------------------------------------------------------------------
def _build(kind, where):
    from romtime_amd.conventions import RomParameters
    from romtime_amd.rom import RomConstructor

    fom = fc.make_fom(kind, 200, 40)
    mus = fc.mus_of(kind, 3)
    rom = RomConstructor(fom=fom, grid={k: [v] for k, v in mus[0].items()})
    rom.SNAPSHOTS_ON = where
    rom.setup(rnd=0)
    sols = rom.build_reduced_basis(mu_space=[dict(mu) for mu in mus], num_basis=8, tolerances={RomParameters.TOL_TIME: 1.0 - 1e-6})
    return rom, sols


@pytest.mark.parametrize("kind", ["burgers", "heat"])
def test_build_reduced_basis_from_device_snapshots(kind):
    from romtime_amd import fom as dfom
    from romtime_amd.conventions import Stage, Treewalk, TreewalkNonlinear

    c = fc.case(kind, 200, 40, True, 3)
    host_rom, host_sols = _build(kind, "host")
    dev_rom, dev_sols = _build(kind, "device")
    truth_full = dfom.full_solution(torch.from_numpy(c["truth"].astype(np.float64)), c["rec"]["lift"]).numpy()
    for j in range(3):
        d_host, d_dev = fc.rel(host_sols[j].T, truth_full[j]), fc.rel(dev_sols[j].T, truth_full[j])
        print(f"{kind} fom_solutions[{j}]: d_host {d_host:.3e} d_dev {d_dev:.3e}")
        assert dev_sols[j].shape == host_sols[j].shape == (201, 40)
        assert d_dev <= fc.bar(d_host)
    off_h, off_d = host_rom.report[Stage.OFFLINE], dev_rom.report[Stage.OFFLINE]
    print("time-level counts", off_h[Treewalk.BASIS_TIME], off_d[Treewalk.BASIS_TIME])
    assert off_h[Treewalk.BASIS_TIME] == off_d[Treewalk.BASIS_TIME]
    assert off_h[Treewalk.BASIS_FINAL] == off_d[Treewalk.BASIS_FINAL] == dev_rom.basis.shape[1] == min(8, off_h[Treewalk.BASIS_AFTER_WALK])
    assert off_h[Treewalk.BASIS_AFTER_WALK] == off_d[Treewalk.BASIS_AFTER_WALK]
    if kind == "burgers":
        assert off_h[TreewalkNonlinear.BASIS_TIME] == off_d[TreewalkNonlinear.BASIS_TIME]
        assert off_h[TreewalkNonlinear.BASIS_FINAL] == off_d[TreewalkNonlinear.BASIS_FINAL]
    else:
        assert dev_rom.basis_nonlinear is None and host_rom.basis_nonlinear is None
    # the device-route basis spans the host snapshots as well as the host-route basis does
    (_, U), = dfom.fom_sweep(c["fom"], c["mus"])
    X = np.hstack([c["host"][j].T for j in range(3)])
    dX = np.linalg.norm(X - np.hstack([U[j].T.cpu().numpy() for j in range(3)]))
    err = lambda V: np.linalg.norm(X - V @ (V.T @ X))
    e_host, e_dev = err(host_rom.basis), err(dev_rom.basis)
    print(f"{kind} projection error: host basis {e_host:.6e}, device basis {e_dev:.6e}, |dX|_F {dX:.3e}")
    assert e_dev <= e_host + 4.0 * dX


def test_nonlinear_snapshot_sets_are_the_hosts():
    from romtime_amd import fom as dfom
    from romtime_amd import ops

    c = fc.case("burgers", 200, 40, True, 3)
    for j in range(3):
        ref = c["host_nl"][j]
        got = dfom.nonlinear_snapshots(c["fom"], ops.to_device(c["host"][j])).cpu().numpy()
        assert got.shape == ref.shape == (3 * 199 + 2, 40) and (got[0] == 0).all()
        np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-14 * np.abs(ref).max())


def test_certification_takes_a_device_block_unchanged():
    from romtime_amd import certify
    from romtime_amd import fom as dfom

    c = fc.case("heat", 200, 40, True, 3)
    (_, U), = dfom.fom_sweep(c["fom"], c["mus"])
    rng = np.random.default_rng(5)
    V, _ = np.linalg.qr(rng.standard_normal((201, 6)))
    uN = rng.standard_normal((3, 40, 6)) * 0.1
    on_device = certify.trajectory_errors(V, uN, [U[j].T for j in range(3)])
    uploaded = certify.trajectory_errors(V, uN, [U[j].T.cpu().numpy() for j in range(3)])
    np.testing.assert_array_equal(on_device, uploaded)
    ref = np.array([np.linalg.norm(U[j].T.cpu().numpy() - V @ uN[j].T, axis=0) / np.sqrt(201) for j in range(3)])
    np.testing.assert_allclose(on_device, ref, rtol=1e-12)
