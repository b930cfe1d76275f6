#!/usr/bin/env python3
"""Error curves of whole trajectories: the fused kernel (``ops.trajectory_errors`` -> rt_trajectory_errors) beside the
route a user had without it, ``ops.gemm_nn`` over step chunks plus torch subtraction and column norms, which writes the
lifted block to HBM and reads it back.  Prints one JSON line (``--out`` also writes it to a file).

Default shape: config 5's, N = 1e5, nt = 1e4, k = 81 (r = 80 plus one lifting column), four device-resident trajectories,
U row-major and column-major (each snapshot contiguous).  Per layout, in one process, alternating the two routes after a
warm-up of both: device-event times of ``--reps`` calls each (median, min, max), ms per trajectory, TB/s of U
(8 N nt bytes per trajectory) and TFLOP/s (2 N nt k flop per trajectory) from the median, and the largest relative
difference between the two routes' curves."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import ops  # noqa: E402
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


def unfused(B, Bt, A, U, layout, chunk):
    """err (n, nt) by lifting ``chunk`` steps at a time: one GEMM, one subtraction, one column norm per chunk."""
    n, nt, _ = A.shape
    N = B.shape[0]
    err = torch.empty((n, nt), dtype=torch.float64, device=B.device)
    for j in range(n):
        for t0 in range(0, nt, chunk):
            t1 = min(t0 + chunk, nt)
            if layout == "C":                                    # U_j is N x nt row-major: lifted block N x chunk
                lifted = ops.gemm_nn(B, A[j, t0:t1].T.contiguous())
                err[j, t0:t1] = torch.linalg.vector_norm(U[j][:, t0:t1] - lifted, dim=0)
            else:                                                # snapshots contiguous: lifted block chunk x N
                lifted = ops.gemm_nn(A[j, t0:t1], Bt)
                err[j, t0:t1] = torch.linalg.vector_norm(U[j].T[t0:t1] - lifted, dim=1)
    return err / np.sqrt(N)


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--nt", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=81)
    ap.add_argument("--traj", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=1000, help="steps per lifted block of the unfused route")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_errors.py measures on the GPU only")
    N, nt, k, n = a.N, a.nt, a.k, a.traj
    gen = torch.Generator(device="cuda").manual_seed(11)
    B = torch.randn((N, k), dtype=torch.float64, device="cuda", generator=gen) / np.sqrt(N)
    Bt = B.T.contiguous()
    A = torch.randn((n, nt, k), dtype=torch.float64, device="cuda", generator=gen)
    store = torch.randn((n, N * nt), dtype=torch.float64, device="cuda", generator=gen)       # the snapshots, either way round
    bytes_u, flop = 8.0 * N * nt, 2.0 * N * nt * k
    res = dict(workload="error curves of whole trajectories: fused rt_trajectory_errors vs gemm_nn chunks + torch",
               N=N, nt=nt, k=k, trajectories=n, chunk=a.chunk, reps=a.reps, device=torch.cuda.get_device_name(0))
    for layout in ("C", "F"):
        U = store.view(n, N, nt) if layout == "C" else store.view(n, nt, N).transpose(1, 2)
        fused = lambda: ops.trajectory_errors(B, A, U)
        plain = lambda: unfused(B, Bt, A, U, layout, a.chunk)
        e_f, e_u = fused(), plain()                                   # warm-up of both routes, and the comparison
        fused()
        info = Context.current().launch_info()
        torch.cuda.synchronize()
        diff = float(((e_f - e_u).abs() / e_u).max())
        ms_f, ms_u = [], []
        for _ in range(a.reps):                                       # alternate, so that drift hits both alike
            ms_f += timed(fused, 1)
            ms_u += timed(plain, 1)
        rec = dict(fused=stats(ms_f), unfused=stats(ms_u), launch_info=info, max_rel_difference_of_the_curves=diff)
        per = rec["fused"]["median_ms"] / n
        rec["fused"].update(ms_per_trajectory=per, TBps_of_U=bytes_u / per / 1e9, TFLOPs=flop / per / 1e9)
        rec["unfused"].update(ms_per_trajectory=rec["unfused"]["median_ms"] / n)
        rec["speedup_median"] = rec["unfused"]["median_ms"] / rec["fused"]["median_ms"]
        res["U_row_major" if layout == "C" else "U_column_major"] = rec
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
