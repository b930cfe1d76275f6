#!/usr/bin/env python3
"""The first half of the offline hyper-reduction through the classes: ``run()`` of the six (M)DEIM reductors of the piston
workflow on ``MockBurgers`` and of the six operators of ``MockHeatEquation`` on a moving interval, at nx = 2000 with the
FOM's nt = 500 instants and 8 parameter points (the sizes of tools/bench_online_classes.py), two ways on one commit:

  host     SNAPSHOTS_ON = "host":   one FOM callback per sample, stacked into pinned memory and uploaded
  device   SNAPSHOTS_ON = "device": the set of a parameter point in one launch (rt_p1_snapshot_sets), no callback

Each reductor runs once per way after a warm-up (one point, few instants), twice: plain, timed by the wall clock between
two device synchronisations, and once more with the stages bracketed - collect (the callbacks and the upload, or the
launch; ended by a wait for the producing stream), greedy (``build_interpolation_mesh``) and walk (the rest: the PODs) -
which costs the overlap between a set's production and the PODs in flight, so the stage times add up to a little more
than the plain time.  Callbacks are counted.  Truncation is the default rule (singular values above 1e-7): the piston's
convection and lifting sets have rank one, and the energy rule keeps no mode of those; N-MDEIM keeps four modes per
instant and level (``num_time``).  Writes the record to ``--out``.
A record, not a pass criterion."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PISTON = ("mass", "stiffness", "convection", "nonlinear_lifting", "trilinear", "lifting")
HEAT = ("mass", "stiffness", "convection", "forcing", "lifting", "rhs")
VECTORS = ("forcing", "lifting", "rhs")


def make_fom(which, nx, nt):
    from romtime_amd.testing.mock import MockBurgers, MockHeatEquation

    if which == "piston":
        fom = MockBurgers(domain=dict(L0=1.0, nx=nx, T=0.5, nt=nt), Lt=lambda t, **mu: 1.0 - 0.1 * np.sin(mu["omega"] * t), bdf2=True)
    else:
        fom = MockHeatEquation(domain=dict(L0=2.0, nx=nx, T=1.0, nt=nt), Lt=lambda t, **mu: 1.0 - 0.25 * np.sin(mu["omega"] * t),
                               dLt_dt=lambda t, **mu: -0.25 * mu["omega"] * np.cos(mu["omega"] * t))
    fom.setup()
    return fom


def points(which, n):
    if which == "piston":
        return [dict(alpha_0=0.045 + 0.009 * i, delta=0.295 + 0.002 * i, omega=8.7 + 0.35 * i) for i in range(n)]
    return [dict(delta=0.4 + 0.1 * i, beta=2.0 + 0.5 * i, alpha_0=0.3 + 0.08 * i, omega=1.0 + 0.3 * i) for i in range(n)]


def states(nx, n):
    """Smooth states in the role of the reduced basis (N-MDEIM.run, nonlinear.py:159-170)."""
    x = np.linspace(0.0, 1.0, nx + 1)
    return np.stack([(1.0 + x) ** (k + 1) + 0.1 * np.sin((k + 1) * np.pi * x) for k in range(n)], axis=1)


class Counter:
    def __init__(self):
        self.calls = 0
        self.depth = 0

    def wrap(self, method):
        def counted(*a, **kw):
            if self.depth == 0:
                self.calls += 1
            self.depth += 1
            try:
                return method(*a, **kw)
            finally:
                self.depth -= 1

        counted.__self__, counted.__name__, counted.__qualname__ = method.__self__, method.__name__, method.__qualname__
        return counted


def make_reductor(fom, kind, mus, ts, route, counter):
    from romtime_amd import (DiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolation,
                             MatrixDiscreteEmpiricalInterpolationNonlinear)
    from romtime_amd.base import Reductor

    p = {"ts": ts, "num_snapshots": len(mus)}
    callback = getattr(fom, "assemble_" + kind)
    if kind in VECTORS:
        red = DiscreteEmpiricalInterpolation(assemble=callback, tree_walk_params=p, name=kind)
        Reductor.setup(red, rnd=np.random.RandomState(0))
    elif kind == "trilinear":
        p["num_time"] = 4          # four modes per instant: the time level's 4 nt columns stay within one device eigensolve
        red = MatrixDiscreteEmpiricalInterpolationNonlinear(assemble=callback, tree_walk_params=p, name=kind)
        Reductor.setup(red, rnd=np.random.RandomState(0))
        red.rows, red.cols = red.get_matrix_topology(mu=mus[0], t=1.0, u_n=np.linspace(0.0, 1.0, fom.Nh))
    else:
        red = MatrixDiscreteEmpiricalInterpolation(assemble=callback, tree_walk_params=p, name=kind)
        Reductor.setup(red, rnd=np.random.RandomState(0))
        red.rows, red.cols = red.get_matrix_topology(mu=mus[0], t=0.3 * float(ts[-1]))
    red.assemble = counter.wrap(callback)
    red.SNAPSHOTS_ON = route
    return red


class Stages:
    """Brackets the collect and greedy stages of one ``run()`` (see the module docstring)."""

    def __init__(self):
        self.collect = self.greedy = 0.0

    def _timed(self, fn, field, device_wide):
        def wrapped(*a, **kw):
            if device_wide:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            (torch.cuda.synchronize if device_wide else torch.cuda.current_stream().synchronize)()
            setattr(self, field, getattr(self, field) + time.perf_counter() - t0)
            return out

        return wrapped

    def install(self, red):
        from romtime_amd import collect, walks

        self.saved = (walks.upload_columns, collect.time_level_set, collect.state_level_sets)
        if red.SNAPSHOTS_ON == "host":
            # the callbacks run inside the argument list of upload_columns: bracket them one by one as well
            red.assemble_snapshot = self._timed(red.assemble_snapshot, "collect", False)
            walks.upload_columns = self._timed(walks.upload_columns, "collect", False)
        else:
            collect.time_level_set = self._timed(collect.time_level_set, "collect", False)
            collect.state_level_sets = self._timed(collect.state_level_sets, "collect", False)
        red.build_interpolation_mesh = self._timed(red.build_interpolation_mesh, "greedy", True)

    def remove(self):
        from romtime_amd import collect, walks

        walks.upload_columns, collect.time_level_set, collect.state_level_sets = self.saved


def run_once(which, kind, mus, ts, route, nx, nt, n_psi, staged):
    fom = make_fom(which, nx, nt)
    counter = Counter()
    red = make_reductor(fom, kind, mus, ts, route, counter)
    stages = Stages()
    if staged:
        stages.install(red)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "trilinear":
            red.run(u_n=states(nx, n_psi), mu_space=[dict(m) for m in mus])
        else:
            red.run(mu_space=[dict(m) for m in mus])
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        if staged:
            stages.remove()
    return dict(total=total, collect=stages.collect, greedy=stages.greedy, walk=total - stages.collect - stages.greedy,
                calls=counter.calls, N=int(red.N), dofs=[tuple(int(x) for x in d) for d in red.dofs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--nt", type=int, default=500)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--states", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "offline_hyperreduction_ab.txt"))
    a = ap.parse_args()
    rows, rec = [], dict(nx=a.nx, nt=a.nt, points=a.points, states=a.states, gpu=torch.cuda.get_device_name(0), runs=[])
    for which, kinds in (("piston", PISTON), ("heat", HEAT)):
        fom = make_fom(which, a.nx, a.nt)
        ts = fom.dt * np.arange(1, a.nt + 1)
        mus = points(which, a.points)
        for kind in kinds:
            res = {}
            try:
                for route in ("host", "device"):
                    run_once(which, kind, mus[:1], ts[:4], route, a.nx, a.nt, a.states, False)       # warm-up
                    plain = run_once(which, kind, mus, ts, route, a.nx, a.nt, a.states, False)
                    staged = run_once(which, kind, mus, ts, route, a.nx, a.nt, a.states, True)
                    res[route] = (plain, staged)
                    print(f"{which} {kind} {route}: {plain['total']:.3f} s, {plain['calls']} callbacks, N = {plain['N']}", flush=True)
            except Exception as exc:                      # a record: say what did not run and go on
                rows.append(f"{which:7s} {kind:18s} did not run: {type(exc).__name__}: {str(exc)[:120]}")
                print(rows[-1], flush=True)
                continue
            (hp, hs), (dp, ds) = res["host"], res["device"]
            same = hp["dofs"] == dp["dofs"] and hp["N"] == dp["N"]
            rec["runs"].append(dict(fom=which, kind=kind, host=hp["total"], device=dp["total"], host_calls=hp["calls"],
                                    device_calls=dp["calls"], host_stages=[hs["collect"], hs["walk"], hs["greedy"]],
                                    device_stages=[ds["collect"], ds["walk"], ds["greedy"]], N=hp["N"], same_dofs=same))
            rows.append(f"{which:7s} {kind:18s} {hp['calls']:7d} {dp['calls']:5d}   {hp['total']:8.3f}  {hs['collect']:8.3f} {hs['walk']:7.3f} "
                        f"{hs['greedy']:7.3f}   {dp['total']:8.3f}  {ds['collect']:8.3f} {ds['walk']:7.3f} {ds['greedy']:7.3f}   "
                        f"{hp['total'] / dp['total']:7.1f}   {hp['N']:2d}  {'yes' if same else 'no'}")
    th, td = sum(r["host"] for r in rec["runs"]), sum(r["device"] for r in rec["runs"])
    rec.update(host_s=th, device_s=td)
    lines = [
        "Collecting the (M)DEIM snapshot sets: FOM callbacks on the host beside rt_p1_snapshot_sets on the device",
        "========================================================================================================",
        "",
        f"tools/bench_offline_hyperreduction.py, one {rec['gpu']}, one process.  run() of the six reductors of the piston workflow",
        f"(MockBurgers, N-MDEIM over {a.states} states) and of the six operators of MockHeatEquation on a moving interval, nx = {a.nx},",
        f"the FOM's nt = {a.nt} instants, {a.points} parameter points, default truncation.  Each run once after a warm-up, wall clock",
        "between two device synchronisations.  `total` is the plain run; collect / walk / greedy come from a second run with the",
        "stages bracketed (collect = callbacks + upload, or the launch; greedy = build_interpolation_mesh; walk = the rest), which",
        "costs the overlap of a set's production with the PODs in flight.  Seconds.  `same dofs`: the two routes end with the same",
        "interpolation indices; where they do not, the sets of an operator span the same few patterns at every parameter point, the",
        "mu-level singular values coincide and the basis inside such a cluster is fixed only up to a rotation (tests/test_walks.py).",
        "",
        "                             callbacks        host                                  device                               host /",
        "fom     reductor              host   dev      total   collect    walk  greedy      total   collect    walk  greedy    device    N  same dofs",
    ] + rows + [
        "",
        f"all {len(rec['runs'])} that ran: host {th:.3f} s, device {td:.3f} s, {th / td:.1f} x",
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
