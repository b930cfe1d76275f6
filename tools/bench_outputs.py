#!/usr/bin/env python3
"""Mass curves of whole trajectories: the fused kernel (``ops.trajectory_integrals`` -> rt_trajectory_integrals) beside
the only route to the same numbers without it, ``ops.gemm_nn`` over step chunks plus ``torch.pow`` and a weighted row sum,
which writes the lifted block to HBM and reads it back several times.  Prints one JSON line (``--out`` also writes it to
a file).

Default shape: config 5's, N_h = 1e5 nodes (two Gauss points per cell: 2e5 quadrature rows), nt = 1e4, k = 81 (r = 80
plus one lifting column), 32 device-resident trajectories, the density's exponent 5.000000000000001.  In one process,
alternating the two routes after a warm-up of both: device-event times of ``--reps`` calls each (median, min, max), ms
per trajectory, evaluations of f per second from the median, and the largest relative difference between the two routes'
curves."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import ops, outputs  # noqa: E402
from romtime_amd._lib import Context  # noqa: E402


def timed(fn, reps):
    """Device-event milliseconds of ``reps`` calls of fn, each between two events on the current stream."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def unfused(E, w, A, scale, fn, chunk):
    """out (n, nt) by lifting ``chunk`` steps at a time: one GEMM, the pointwise function and one weighted row sum."""
    _, c0, c1, p = fn
    n, nt, _ = A.shape
    out = torch.empty((n, nt), dtype=torch.float64, device=E.device)
    for j in range(n):
        for t0 in range(0, nt, chunk):
            t1 = min(t0 + chunk, nt)
            lifted = ops.gemm_nn(E, A[j, t0:t1].T.contiguous())          # n_pts x chunk
            lifted.mul_(c1).add_(c0).pow_(p)
            out[j, t0:t1] = w @ lifted
    return out * scale


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000, help="nodes of the mesh")
    ap.add_argument("--nt", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=81)
    ap.add_argument("--traj", type=int, default=32)
    ap.add_argument("--points", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=1000, help="steps per lifted block of the unfused route")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_outputs.py measures on the GPU only")
    N, nt, k, n = a.N, a.nt, a.k, a.traj
    gen = torch.Generator(device="cuda").manual_seed(13)
    B = torch.rand((N, k), dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0
    A = (torch.rand((n, nt, k), dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0) / k      # |u| <= 1
    scale = 1.0 + 0.2 * torch.rand((n, nt), dtype=torch.float64, device="cuda", generator=gen)
    fn = outputs.density(1.4)
    E, w = outputs.quadrature_basis(B, a.points)
    del B
    res = dict(workload="mass curves of whole trajectories: fused rt_trajectory_integrals vs gemm_nn chunks + torch.pow + sum",
               N=N, quadrature_rows=int(E.shape[0]), nt=nt, k=k, trajectories=n, exponent=fn[3], chunk=a.chunk, reps=a.reps,
               device=torch.cuda.get_device_name(0))
    fused = lambda: ops.trajectory_integrals(E, A, w, scale, fn)
    plain = lambda: unfused(E, w, A, scale, fn, a.chunk)
    o_f, o_u = fused(), plain()                                       # warm-up of both routes, and the comparison
    fused()
    info = Context.current().launch_info()
    torch.cuda.synchronize()
    res["max_rel_difference_of_the_curves"] = float(((o_f - o_u).abs() / o_u.abs()).max())
    ms_f, ms_u = [], []
    for _ in range(a.reps):                                           # alternate, so that drift hits both alike
        ms_f += timed(fused, 1)
        ms_u += timed(plain, 1)
    evals = float(E.shape[0]) * nt * n
    res["fused"] = dict(stats(ms_f), launch_info=info)
    res["fused"].update(ms_per_trajectory=res["fused"]["median_ms"] / n, G_evaluations_per_s=evals / res["fused"]["median_ms"] / 1e6)
    res["unfused"] = stats(ms_u)
    res["unfused"].update(ms_per_trajectory=res["unfused"]["median_ms"] / n, G_evaluations_per_s=evals / res["unfused"]["median_ms"] / 1e6)
    res["speedup_median"] = res["unfused"]["median_ms"] / res["fused"]["median_ms"]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
