#!/usr/bin/env python3
"""The online sweeps with the GMRES reduced solver (the reference's gmres, solver="gmres") beside the default direct
solver.  Prints one JSON line:

  * the C5 hyper-reduced sweep (r = 80, 32 parameter points, 1e4 BDF2 steps by default);
  * the direct sweep (N_h = 1e5, r = 80, 32 parameter points, 200 steps by default).

For each sweep and solver: steps/s from the host clock around one synchronised sweep after a warm-up sweep of the same
shape, and (GMRES) the inner iterations per solve and unconverged systems from the ctx counters."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import ops  # noqa: E402
from romtime_amd._lib import Context  # noqa: E402
from romtime_amd.sweep import hrom_bdf_sweep, rom_bdf_sweep  # noqa: E402
from romtime_amd.testing.workloads import c5_direct, c5_hyper_reduced  # noqa: E402


def measure(nt, run):
    ctx = Context.current()
    out = {}
    traj = {}
    for solver in ("direct", "gmres"):
        run(solver)                      # warm-up: code objects, arena sizes
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        uN = run(solver)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        traj[solver] = uN.cpu().numpy()
        rec = dict(steps_per_s=nt / wall, us_per_step=1e6 * wall / nt, solves=ctx.counter("sweep_solves"))
        if solver == "gmres":
            its = ctx.counter("sweep_gmres_iterations")
            rec.update(inner_iterations=its, inner_iterations_per_solve=its / rec["solves"],
                       unconverged=ctx.counter("sweep_gmres_unconverged"))
        out[solver] = rec
    d, g = traj["direct"], traj["gmres"]
    out["rel_l2_gmres_vs_direct"] = float(np.linalg.norm(g - d) / np.linalg.norm(d))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hsteps", type=int, default=10_000, help="steps of the hyper-reduced sweep")
    ap.add_argument("--dsteps", type=int, default=200, help="steps of the direct sweep")
    ap.add_argument("--n-mu", type=int, default=32)
    ap.add_argument("--r", type=int, default=80)
    a = ap.parse_args()
    res = dict(workload="online sweeps, solver direct vs gmres (rtol = atol = 1e-10, restart 20, rom.py:36)",
               n_mu=a.n_mu, r=a.r)
    terms, _, _, _ = c5_hyper_reduced(nt=a.hsteps, n_mu=a.n_mu, r=a.r)
    hargs = (terms["mass"], terms["lin"], terms["nl"], terms["rhs"], terms["dt"])
    res["hyper_reduced"] = dict(nt=a.hsteps, **measure(a.hsteps, lambda s: hrom_bdf_sweep(*hargs, bdf2=True, solver=s)))
    fom, V, mus, d = c5_direct(nt=a.dsteps, n_mu=a.n_mu, r=a.r)
    dargs = [ops.to_device(V), d["indptr"], d["indices"], ops.to_device(d["mass"]), ops.to_device(d["terms"]),
             ops.to_device(d["term_coef"]), ops.to_device(d["tril"]), ops.to_device(d["rhs_terms"]),
             ops.to_device(d["rhs_coef"]), d["dt"]]
    res["direct"] = dict(nt=a.dsteps, N=int(V.shape[0]), **measure(a.dsteps, lambda s: rom_bdf_sweep(*dargs, bdf2=True, solver=s)))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
