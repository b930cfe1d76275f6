#!/usr/bin/env python3
"""Full-order sweeps at N_h = 1e5: the device sweep (``ops.p1_fom_bdf_sweep`` -> rt_p1_fom_bdf_sweep) beside the host loop
``mock.solve()`` - the only route there was - for the two closed-form problems (MockBurgers BDF2, MockHeatEquation BDF1,
both on a moving interval; the cases of tests/fom_cases.py).

Per problem: the host loop timed over ``--host-steps`` steps of ``--host-points`` parameter points (wall clock, SciPy CSR
assembly + SuperLU per step); the distances d_host and d_dev of both routes from the long-double recipe over those steps
(relative L2 over the block, tests/fom_cases.py); the device sweep over ``--steps`` steps for 1, 32 and 256 parameter
points, device-event times of ``--reps`` launches after a warm-up (median, min, max).  Writes a table and one JSON line
per problem to ``--out`` and prints the JSON lines.

``--piston`` measures the convection-dominated row instead and APPENDS it to ``--out``: MockBurgers at the sizes of the
reference's piston runs (nt = 100, T = 1, alpha_0 = 1e-6, delta = 0.1, omega = 6; tests/fom_defect_cases.py) at ``--nx``
cells, where every step loses diagonal dominance - the dominance entry beside ``ops.p1_fom_bdf_sweep_certified``, the
worst reported defect, and the cost of the defect pass per step."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import ops  # noqa: E402
from tests import fom_cases as fc  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def piston_row(a):
    """The convection-dominated row: both entries on the same table, 1, 32 and 256 points."""
    from tests import fom_defect_cases as dc

    fom = dc.make_fom(a.nx, 100, True, T=1.0)
    mu = dict(dc.CONV_MUS[0])
    lines = [f"piston sizes, nx = {a.nx}, nt = 100, T = 1, alpha_0 = 1e-6 (BDF2), median of {a.reps} launches (min - max), ms for 100 steps",
             "points   dominance entry          certified entry          defect pass us/step   flagged by dominance   worst defect   flagged by defect"]
    raw = dict(problem="piston", nx=a.nx, nt=100, reps=a.reps, gpu=torch.cuda.get_device_name(0), device=[])
    for n_mu in (1, 32, 256):
        rec = fc.recipe(fom, [mu] * n_mu)
        tab = ops.to_device(rec["tab"])
        plain = lambda: ops.p1_fom_bdf_sweep(a.nx, tab, fom.dt, rec["bdf2"], rec["state_in_w"])
        cert = lambda: ops.p1_fom_bdf_sweep_certified(a.nx, tab, fom.dt, rec["bdf2"], rec["state_in_w"])
        _, flags = plain()
        _, cflags, defect = cert()
        torch.cuda.synchronize()
        ms0, ms1 = timed(plain, a.reps), timed(cert, a.reps)
        m0, m1 = float(np.median(ms0)), float(np.median(ms1))
        dev = dict(points=n_mu, dominance_ms=ms0, certified_ms=ms1, dominance_median_ms=m0, certified_median_ms=m1,
                   defect_pass_us_per_step=10.0 * (m1 - m0), flagged_by_dominance=int(flags.count_nonzero()),
                   worst_defect=float(defect.max()), flagged_by_defect=int(cflags.count_nonzero()))
        raw["device"].append(dev)
        lines.append(f"{n_mu:6d}   {m0:8.2f} ({min(ms0):.2f} - {max(ms0):.2f})   {m1:8.2f} ({min(ms1):.2f} - {max(ms1):.2f})   "
                     f"{dev['defect_pass_us_per_step']:19.1f}   {dev['flagged_by_dominance']:20d}   {dev['worst_defect']:.3e}   {dev['flagged_by_defect']:17d}")
    print(json.dumps(raw), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fp:
        fp.write("\n" + "\n".join(lines) + "\n\nraw: " + json.dumps(raw) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=100, help="steps of a timed device sweep")
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "fom_sweep_ab.txt"))
    ap.add_argument("--piston", action="store_true", help="the convection-dominated row, both entries, appended to --out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fom.py measures on the GPU only")
    if a.piston:
        return piston_row(a)
    plan = ops.p1_fom_plan(a.nx)
    lines, raws = [], []
    lines.append("problem    host ms/step/point   host steps/s   d_host      d_dev       bar         | points   device ms (min - max) for "
                 f"{a.steps} steps   us/step   steps/s per point   point-steps/s   device / host")
    for kind in ("burgers", "heat"):
        # accuracy and the host loop, a few steps
        fom = fc.make_fom(kind, a.nx, a.host_steps)
        mus = fc.mus_of(kind, a.host_points)
        rec = fc.recipe(fom, mus)
        t0 = time.perf_counter()
        host, _, _ = fc.host_solutions(fom, mus)
        host_s = time.perf_counter() - t0
        T, margin, _ = fc.truth(a.nx, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"])
        U, info = ops.p1_fom_bdf_sweep(a.nx, rec["tab"], fom.dt, rec["bdf2"], rec["state_in_w"])
        d_host, d_dev = fc.rel(host, T), fc.rel(U.cpu().numpy(), T)
        host_ms = 1e3 * host_s / (a.host_steps * a.host_points)
        raw = dict(problem=kind, nx=a.nx, plan=dict(workgroups_per_point=1, partitions=plan[1], rows_per_partition=plan[2]),
                   host_steps=a.host_steps, host_points=a.host_points, host_ms_per_step_per_point=host_ms, d_host=d_host,
                   d_dev=d_dev, bar=fc.bar(d_host), dominance_margin=margin, info=info.tolist(), device=[],
                   gpu=torch.cuda.get_device_name(0))
        # the device sweep over a longer horizon
        big = fc.make_fom(kind, a.nx, a.steps)
        for n_mu in (1, 32, 256):
            tab = ops.to_device(fc.recipe(big, fc.mus_of(kind, n_mu))["tab"])
            run = lambda: ops.p1_fom_bdf_sweep(a.nx, tab, big.dt, rec["bdf2"], rec["state_in_w"])
            _, flags = run()
            torch.cuda.synchronize()
            ms = timed(run, a.reps)
            med = float(np.median(ms))
            dev = dict(points=n_mu, steps=a.steps, median_ms=med, min_ms=float(min(ms)), max_ms=float(max(ms)),
                       us_per_step=1e3 * med / a.steps, steps_per_s_per_point=a.steps / med * 1e3,
                       point_steps_per_s=n_mu * a.steps / med * 1e3, flagged=int(flags.count_nonzero()),
                       speedup_over_host_loop=host_ms / (med / (a.steps * n_mu)))
            raw["device"].append(dev)
            left = (f"{kind:<10} {host_ms:18.1f}   {1e3 / host_ms:12.2f}   {d_host:.3e}   {d_dev:.3e}   {fc.bar(d_host):.3e}"
                    if n_mu == 1 else " " * 86)
            lines.append(f"{left}   | {n_mu:6d}   {med:10.2f} ({min(ms):.2f} - {max(ms):.2f})   {dev['us_per_step']:20.1f}   "
                         f"{dev['steps_per_s_per_point']:17.0f}   {dev['point_steps_per_s']:13.0f}   {dev['speedup_over_host_loop']:10.0f} x")
        raws.append(raw)
        print(json.dumps(raw), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n\n" + "\n".join("raw: " + json.dumps(r) for r in raws) + "\n")


if __name__ == "__main__":
    main()
