#!/usr/bin/env python3
"""POD of snapshot sets wider than 2048 columns: the block Rayleigh-Ritz route (``pod.WIDE_EIG = "device"``,
rt_sym_eig_blocked) beside the host eigensolver (np.linalg.eigh on the n x n Gram matrix), which is the code as it stood
and so the yardstick.

Runs ``pod.pod_device(X, num=40, normalize=False)`` on device-resident stacked-bases sets (what the mu level of a tree
walk hands to ``orth``: the time-level bases of every parameter point side by side) of 1e5 x 4096 and 1e5 x 10000.  The
two routes alternate in one process after a warm-up of both; every repetition is timed by a pair of device events that
ends in a synchronise.  Writes, per shape and route, the median and the min-max spread, R and the block ranks of the
device route, the two routes' difference in ``s`` and the subspace distance of their bases.  The numbers are records:
the default of ``WIDE_EIG`` does not hang on them.

The bases are drawn from one ``rank``-dimensional space (a spectrum six decades deep) with noise at ``--noise``; the
default 0 gives sets of rank 60.  With the 1e-9 of tools/bench_wide_pod.py the orthonormalised blocks carry their noise
well above n eps lam_max and the block ranks grow with it (829 and 824 at 4096 columns); where R passes 2048 the set is
not reducible and the "device" rows time the refusal plus the host route - the status line says which it was."""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import _lib, ops, pod  # noqa: E402

ROUTES = ("host", "device")


def stacked_bases(N, blocks, cols, seed, rank=60, noise=0.0):
    rng = np.random.RandomState(seed)
    U0, _ = np.linalg.qr(rng.standard_normal((N, rank)))
    Uw = U0 * 10.0 ** (-6.0 * np.arange(rank) / (rank - 1))
    X = np.empty((N, blocks * cols))
    for b in range(blocks):
        B = Uw @ rng.standard_normal((rank, cols))
        if noise:
            B += noise * rng.standard_normal((N, cols))
        X[:, b * cols:(b + 1) * cols] = np.linalg.qr(B)[0]
    return X


def timed(Xd, route):
    pod.WIDE_EIG = route
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # a set that is not reducible is a result here
        out = pod.pod_device(Xd, num=40, normalize=False)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--noise", type=float, default=0.0)
    ap.add_argument("--columns", type=int, nargs="*", default=[4096, 10000])
    ap.add_argument("--out", default=os.path.join("profiles", "blocked_pod_ab.txt"))
    a = ap.parse_args()
    shapes = {4096: (128, 32), 10000: (250, 40)}
    lines = [f"pod.pod_device(X, num=40, normalize=False), stacked bases (seed {a.seed}, noise {a.noise:g}), {a.reps} "
             f"repetitions per route, routes alternating; ms between device events",
             f"{'shape':>15} {'route':>7} {'median':>10} {'min':>10} {'max':>10} {'spread':>10}"]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    ctx = _lib.Context.current()
    for n in a.columns:
        blocks, cols = shapes[n]
        Xd = ops.to_device(stacked_bases(a.rows, blocks, cols, a.seed, noise=a.noise))
        outs, ms = {}, {name: [] for name in ROUTES}
        for name in ROUTES:                 # warm-up: code objects, arenas, pinned buffers
            timed(Xd, name)
        refused = ctx.counter("eig_blocked_not_reducible")
        for _ in range(a.reps):
            for name in ROUTES:
                t, outs[name] = timed(Xd, name)
                ms[name].append(t)
                print(f"{a.rows} x {n} {name}: {t:.2f} ms", flush=True)
        for name in ROUTES:
            v = np.array(ms[name])
            lines.append(f"{a.rows:>7} x {n:<5} {name:>7} {np.median(v):10.2f} {v.min():10.2f} {v.max():10.2f} {v.max() - v.min():10.2f}")
        G = ops.gram(Xd)
        _, _, info = ops.sym_eig_blocked(G, 0)
        refused = ctx.counter("eig_blocked_not_reducible") - refused - (1 if info["status"] == 1 else 0)
        d, h = outs["device"], outs["host"]
        Qd, Qh = d["Q"], h["Q"]
        sub = float(torch.linalg.matrix_norm(Qd - Qh @ (Qh.T @ Qd), 2).item())
        m = min(len(d["s"]), len(h["s"]), 40)
        lines.append(f"{a.rows:>7} x {n:<5} status = {info['status']}, R = {info['resolved']}, block ranks = {info['block_ranks']}, "
                     f"device-route calls that took the host route = {refused} of {a.reps}; r = {d['r']} / {h['r']} (device / "
                     f"host), worst |s_device - s_host| / s_1 over the {m} kept = "
                     f"{float(np.max(np.abs(d['s'][:m] - h['s'][:m])) / h['s'][0]):.3e}, subspace distance of the bases = {sub:.2e}")
        flush()
        del Xd, G, outs, d, h, Qd, Qh
        torch.cuda.empty_cache()
    pod.WIDE_EIG = "host"
    print("\n".join(lines))
    flush()


if __name__ == "__main__":
    main()
