#!/usr/bin/env python3
"""The device Jacobi eigensolver (rt_sym_jacobi_eigh) beside the host routine it replaces on the two-pass POD route
(rt_host_jacobi_eigh, unchanged code), and that route beside the default one.

Part 1: the second Gram matrices G2 = Y^T Y, Y = X W, of ``graded`` (eight decades) and ``near_cluster`` (a 1e-6
cluster, then eight decades) snapshot sets of 8192 rows at n = 128, 256, 512 and 1024, formed on the device as
``pod.pod_device(passes=2)`` forms them.  The two solvers alternate in one process after a warm-up of both; the device
solver is timed by the host clock around a call that ends synchronised (it reads a counter per sweep), the host routine
by the host clock (the copy of G2 to the host is not counted).  Sweeps: the device counts the closing sweep without
rotations, the host routine does not.

Part 2: ``pod.pod_device(X, passes=2)`` against ``pod.pod_device(X)`` (the drop rule keeps every mode above 1e-7, so
the default takes the deflated levels) on device-resident ``graded`` sets of 98304 x 128 and 100000 x 512, alternating,
ms between device events.

Writes profiles/jacobi_eig_ab.txt."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import ops, pod  # noqa: E402


def spectrum(family, n):
    if family == "graded":
        return 10.0 ** (-8.0 * np.arange(n) / (n - 1))
    return np.r_[1.0, 1.0 - 1e-6, 1.0 - 2e-6, 1.0 - 3e-6, 10.0 ** (-0.2 - 7.8 * np.arange(n - 4) / (n - 5))]


def snapshots(family, N, n, seed):
    rng = np.random.RandomState(seed)
    U, _ = np.linalg.qr(rng.standard_normal((N, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (U * spectrum(family, n)) @ V.T


def second_gram(Xd):
    n = Xd.shape[1]
    eig = pod._SmallEig(ops.gram(Xd))
    W = eig.vectors(n)
    return ops.gram(ops.gemm_nn(Xd, W.contiguous()))


def host_solve(G2h):
    t0 = time.perf_counter()
    A = G2h.copy()
    n = A.shape[0]
    W, lam = np.empty((n, n)), np.empty(n)
    sweeps = C.c_int(0)
    rc = pod._lib.load().rt_host_jacobi_eigh(A.ctypes.data, n, W.ctypes.data, lam.ctypes.data, 40, C.byref(sweeps))
    assert rc == 0
    return 1e3 * (time.perf_counter() - t0), lam, int(sweeps.value)


def device_solve(G2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lam, W, sweeps = ops.sym_jacobi_eigh(G2)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), lam.cpu().numpy(), sweeps


_LEVELS = []
_deflated = pod._pod_deflated


def _recording(*args, **kw):
    out = _deflated(*args, **kw)
    _LEVELS.append(out[-1])        # the levels the deflated route took
    return out


pod._pod_deflated = _recording


def timed_pod(Xd, passes):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = pod.pod_device(Xd, passes=passes)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--sizes", default="128,256,512,1024")
    ap.add_argument("--out", default=os.path.join("profiles", "jacobi_eig_ab.txt"))
    a = ap.parse_args()
    lines = ["second Gram matrices of 8192 x n sets: rt_sym_jacobi_eigh (device) beside rt_host_jacobi_eigh (host), alternating; "
             "ms, host clock, median (min .. max) over the repetitions; sweeps (the device's include the closing one)",
             f"{'family':>13} {'n':>5} {'device ms':>26} {'sweeps':>6} {'host ms':>30} {'sweeps':>6} {'reps d/h':>8} {'host/device':>11} "
             f"{'max |lam_d - lam_h| / lam_h':>27}"]
    for family in ("graded", "near_cluster"):
        for n in [int(v) for v in a.sizes.split(",")]:
            G2 = second_gram(ops.to_device(snapshots(family, 8192, n, a.seed)))
            G2h = G2.cpu().numpy()
            host_reps = a.reps if n <= 256 else (3 if n <= 512 else 1)
            device_solve(G2)                       # warm-up: code object, arena
            if n <= 512:
                host_solve(G2h)
            td, th = [], []
            for rep in range(a.reps):
                t, lam_d, sw_d = device_solve(G2)
                td.append(t)
                if rep < host_reps:
                    t, lam_h, sw_h = host_solve(G2h)
                    th.append(t)
            td, th = np.array(td), np.array(th)
            pos = lam_h > 0
            rel = float(np.max(np.abs(lam_d[pos] - lam_h[pos]) / lam_h[pos]))
            lines.append(f"{family:>13} {n:>5} {np.median(td):10.2f} ({td.min():.2f} .. {td.max():.2f}) {sw_d:>6} "
                         f"{np.median(th):12.2f} ({th.min():.2f} .. {th.max():.2f}) {sw_h:>6} {a.reps:>4}/{host_reps:<3} "
                         f"{np.median(th) / np.median(td):11.2f} {rel:27.2e}")
    lines.append("")
    lines.append(f"pod.pod_device(X, passes=2) beside pod.pod_device(X) (default route), graded sets on the device, {a.reps} "
                 "repetitions, alternating; ms between device events")
    lines.append(f"{'shape':>14} {'route':>12} {'median':>9} {'min':>9} {'max':>9}   r  levels")
    for N, n in ((98304, 128), (100_000, 512)):
        Xd = ops.to_device(snapshots("graded", N, n, a.seed + 1))
        routes = (("passes=2", 2), ("default", None))
        for _, passes in routes:
            timed_pod(Xd, passes)
            timed_pod(Xd, passes)
        ms, outs = {name: [] for name, _ in routes}, {}
        for _ in range(a.reps):
            for name, passes in routes:
                t, outs[name] = timed_pod(Xd, passes)
                ms[name].append(t)
        for name, _ in routes:
            v, o = np.array(ms[name]), outs[name]
            levels = str(_LEVELS[-1]) if o["passes"] == "deflate" else "-"
            lines.append(f"{N:>7} x {n:<4} {name:>12} {np.median(v):9.2f} {v.min():9.2f} {v.max():9.2f} {o['r']:>3}  {levels}")
        d, h = outs["passes=2"], outs["default"]
        lines.append(f"{N:>7} x {n:<4} max |s_passes=2 - s_default| / s_default over the kept modes = "
                     f"{float(np.max(np.abs(d['s'][:h['r']] - h['s'][:h['r']]) / h['s'][:h['r']])):.2e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
