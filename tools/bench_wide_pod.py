#!/usr/bin/env python3
"""POD of snapshot sets wider than 1024 columns: the device eigensolver's wide route (1024 < n <= 2048) beside the host
eigensolver (np.linalg.eigh on the n x n Gram matrix) it replaces.

Runs ``pod.pod_device(X, num=40, normalize=False)`` on device-resident stacked-bases sets (what the mu level of a tree
walk hands to ``orth``: the time-level bases of every parameter point side by side) of 1e5 x 2000 and 1e5 x 1100.  The
two routes alternate in one process - ``pod.DEVICE_EIG_MAX_N`` is flipped between 2048 and 1024, the host route's code
being the same as before the wide route existed - after a warm-up of both; every repetition is timed by a pair of
device events that ends in a synchronise.  Prints, per shape and route, the median and the min-max spread, the two
routes' difference in ``s`` against the parity bar 2e-13 s_1 + 8 eps s_1^2 / s and the subspace distance of their
bases, and the verdict of the decision rule: the device route is the default only if its median at
1e5 x 2000 is below the host route's by more than the larger of the two spreads.

``--device-only SHAPE`` runs the device route alone (for a kernel trace of it)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import ops, pod  # noqa: E402

EPS = 2.2e-16
ROUTES = (("device", 2048), ("host", 1024))


def stacked_bases(N, blocks, cols, seed, rank=60):
    """``blocks`` orthonormal bases of ``cols`` modes each, all drawn from one ``rank``-dimensional space with a
    spectrum six decades deep plus noise at 1e-9: full numerical rank, a few dozen modes that matter."""
    rng = np.random.RandomState(seed)
    U0, _ = np.linalg.qr(rng.standard_normal((N, rank)))
    Uw = U0 * 10.0 ** (-6.0 * np.arange(rank) / (rank - 1))
    X = np.empty((N, blocks * cols))
    for b in range(blocks):
        B = Uw @ rng.standard_normal((rank, cols)) + 1e-9 * rng.standard_normal((N, cols))
        X[:, b * cols:(b + 1) * cols] = np.linalg.qr(B)[0]
    return X


def timed(Xd, limit):
    pod.DEVICE_EIG_MAX_N = limit
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = pod.pod_device(Xd, num=40, normalize=False)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "wide_eig_ab.txt"))
    ap.add_argument("--device-only", type=int, default=0, metavar="COLUMNS",
                    help="run the device route alone on the set of that many columns, three times, and print nothing else")
    a = ap.parse_args()
    shapes = {2000: (50, 40), 1100: (25, 44)}
    if a.device_only:
        Xd = ops.to_device(stacked_bases(a.rows, *shapes[a.device_only], a.seed))
        for _ in range(3):
            ms, _ = timed(Xd, 2048)
        print(f"device route, {a.rows} x {a.device_only}: {ms:.2f} ms")
        return
    lines = [f"pod.pod_device(X, num=40, normalize=False), stacked bases (seed {a.seed}), {a.reps} repetitions per route, "
             f"routes alternating; ms between device events",
             f"{'shape':>14} {'route':>7} {'median':>9} {'min':>9} {'max':>9} {'spread':>9}"]
    stats = {}
    for n, (blocks, cols) in shapes.items():
        Xd = ops.to_device(stacked_bases(a.rows, blocks, cols, a.seed))
        outs = {}
        for name, limit in ROUTES:          # warm-up: code objects, arenas, pinned buffers
            for _ in range(2):
                timed(Xd, limit)
        ms = {name: [] for name, _ in ROUTES}
        for _ in range(a.reps):
            for name, limit in ROUTES:
                t, outs[name] = timed(Xd, limit)
                ms[name].append(t)
        for name, _ in ROUTES:
            v = np.array(ms[name])
            stats[n, name] = (float(np.median(v)), float(v.max() - v.min()))
            lines.append(f"{a.rows:>7} x {n:<4} {name:>7} {np.median(v):9.2f} {v.min():9.2f} {v.max():9.2f} {v.max() - v.min():9.2f}")
        d, h = outs["device"], outs["host"]
        bar = 2e-13 * h["s"][0] + 8 * EPS * h["s"][0] ** 2 / np.maximum(h["s"], 1e-300)
        Qd, Qh = d["Q"], h["Q"]
        sub = float(torch.linalg.matrix_norm(Qd - Qh @ (Qh.T @ Qd), 2).item())
        lines.append(f"{a.rows:>7} x {n:<4} r = {d['r']} / {h['r']} (device / host), worst |s_device - s_host| / bar = "
                     f"{(np.abs(d['s'] - h['s']) / bar).max():.3f}, subspace distance of the bases = {sub:.2e}")
    pod.DEVICE_EIG_MAX_N = 2048
    (md, sd), (mh, sh) = stats[2000, "device"], stats[2000, "host"]
    met = mh - md > max(sd, sh)
    lines.append(f"decision rule at {a.rows} x 2000: host median - device median = {mh - md:.2f} ms, larger spread = "
                 f"{max(sd, sh):.2f} ms: {'met, the device route is the default' if met else 'NOT met, DEVICE_EIG_MAX_N stays 1024'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
