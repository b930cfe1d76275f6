#!/usr/bin/env python3
"""The online stage through the classes: ``RomConstructorNonlinear`` on ``MockBurgers``, every operator hyper-reduced
(the model of tests/test_surface.py::_fully_hyper_reduced_rom at nx = 2000, nt = 500), 8 parameter points, three ways:

  host        ONLINE_ON = "host":   ``solve`` per point, the reference's loop (one FOM callback per operator and step)
  device      ONLINE_ON = "device": ``solve`` per point (one sweep of one point each; tables built on the device)
  solve_many  ONLINE_ON = "device": ``solve_many`` of all points (one sweep)

Each runs once after a warm-up (one point through each way), timed by the wall clock between two device synchronisations
and including everything the call does: tables, sweep, lifting to ``solutions``.  Prints point-steps per second and the
distance of the device trajectories from the host loop's, and writes the record to ``--out``.  A record, not a pass
criterion."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_model(nx, nt, r_max=8):
    from scipy.stats.distributions import uniform

    from romtime_amd import (DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation,
                             MatrixDiscreteEmpiricalInterpolationNonlinear, RomConstructorNonlinear)
    from romtime_amd.conventions import OperatorType, RomParameters
    from romtime_amd.testing.mock import MockBurgers

    fom = MockBurgers(domain=dict(L0=1.0, nx=nx, T=0.5, nt=nt), Lt=lambda t, **mu: 1.0 - 0.1 * np.sin(mu["omega"] * t), bdf2=True)
    fom.setup()
    train = [dict(alpha_0=0.05 + 0.02 * i, delta=0.3, omega=9.0 + i) for i in range(3)]
    srom = RomConstructorNonlinear(fom=fom, grid=None, name="srom")
    srom.setup(rnd=0)
    srom.build_reduced_basis(mu_space=train, tolerances={RomParameters.TOL_TIME: None, RomParameters.TOL_MU: None})
    rom = srom.truncate(srom.N - r_max) if srom.N > r_max else srom
    grid = dict(alpha_0=uniform(0.04, 0.08), delta=uniform(0.29, 0.02), omega=uniform(8.5, 3.0))
    tw = {"ts": np.linspace(0.01, 0.5, 8), "num_snapshots": 4}
    matrices = dict(mass=(fom.assemble_mass, OperatorType.MASS), stiffness=(fom.assemble_stiffness, OperatorType.STIFFNESS),
                    convection=(fom.assemble_convection, OperatorType.CONVECTION),
                    nonlinear_lifting=(fom.assemble_nonlinear_lifting, OperatorType.NONLINEAR_LIFTING))
    for name, (assemble, which) in matrices.items():
        md = MatrixDiscreteEmpiricalInterpolation(name=name, assemble=assemble, grid=grid, tree_walk_params=tw)
        md.setup(rnd=np.random.RandomState(1))
        md.run()
        rom.add_hyper_reductor(md, which)
    nm = MatrixDiscreteEmpiricalInterpolationNonlinear(name="trilinear", assemble=fom.assemble_trilinear, grid=grid,
                                                       tree_walk_params=tw)
    nm.setup(rnd=np.random.RandomState(1), u_n=np.linspace(0.0, 1.0, fom.Nh))
    nm.run(u_n=rom.basis)
    rom.add_hyper_reductor(nm, OperatorType.TRILINEAR)
    dl = DiscreteEmpiricalInterpolation(name="lifting", assemble=fom.assemble_lifting, grid=grid, tree_walk_params=tw)
    dl.setup(rnd=np.random.RandomState(1))
    dl.run()
    rom.add_hyper_reductor(dl, OperatorType.LIFTING)
    rom.project_reductors()
    return fom, rom


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--nt", type=int, default=500)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "online_classes_ab.txt"))
    a = ap.parse_args()
    from romtime_amd import online
    from romtime_amd.conventions import Stage

    fom, rom = build_model(a.nx, a.nt)
    mus = [dict(alpha_0=0.045 + 0.009 * i, delta=0.295 + 0.002 * i, omega=8.7 + 0.35 * i) for i in range(a.points)]
    warm = dict(alpha_0=0.06, delta=0.3, omega=9.5)
    steps = a.nt * a.points

    def per_point():
        out = []
        for mu in mus:
            rom.solve(mu=mu, step=Stage.ONLINE)
            out.append(rom.solutions.rom.copy())
        return out

    rom.ONLINE_ON = "host"
    rom.solve(mu=warm, step=Stage.ONLINE)
    t_host, host = timed(per_point)
    rom.ONLINE_ON = "device"
    route = online.plan(rom)
    rom.solve(mu=warm, step=Stage.ONLINE)
    rom.solve_many([warm, warm])
    t_dev, dev = timed(per_point)
    t_many, many = timed(lambda: rom.solve_many(mus))
    uN = many.uN.cpu().numpy()
    rel = lambda x, y: float(np.linalg.norm(x - y) / np.linalg.norm(y))
    rec = dict(nx=a.nx, nt=a.nt, points=a.points, r=int(rom.N), route=route, gpu=torch.cuda.get_device_name(0),
               entries={k: int(np.shape(getattr(rom, s).PT_U)[0]) for k, s in online.SLOTS.items() if getattr(rom, s)},
               host_s=t_host, device_s=t_dev, solve_many_s=t_many, host_steps_per_s=steps / t_host,
               device_steps_per_s=steps / t_dev, solve_many_steps_per_s=steps / t_many,
               device_vs_host=max(rel(d, h) for d, h in zip(dev, host)),
               solve_many_vs_host=max(rel(uN[j].T, host[j]) for j in range(a.points)))
    lines = [
        "The online stage through the classes: host loop, per-point device solve, solve_many",
        "===================================================================================",
        "",
        f"tools/bench_online_classes.py, one {rec['gpu']}, one process.  RomConstructorNonlinear on MockBurgers, nx = {a.nx}, "
        f"nt = {a.nt} (BDF2), r = {rec['r']},",
        f"every operator hyper-reduced (interpolation entries: {rec['entries']}), {a.points} parameter points, route "
        f"{route!r}.  Each way once after a warm-up,",
        "wall clock between two device synchronisations, everything the call does included (tables, sweep, lifting to",
        "`solutions` / `storage`); point-steps per second = points x nt / seconds.",
        "",
        "way                                   seconds   point-steps/s   x host   max rel-L2 distance from the host loop",
        f"host        ONLINE_ON = 'host'      {t_host:9.3f}   {steps / t_host:13.1f}   {1.0:6.1f}",
        f"device      solve per point         {t_dev:9.3f}   {steps / t_dev:13.1f}   {t_host / t_dev:6.1f}   {rec['device_vs_host']:.3e}",
        f"solve_many  all points, one sweep   {t_many:9.3f}   {steps / t_many:13.1f}   {t_host / t_many:6.1f}   {rec['solve_many_vs_host']:.3e}",
        "",
        "raw: " + json.dumps(rec),
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
