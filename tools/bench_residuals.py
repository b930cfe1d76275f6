#!/usr/bin/env python3
"""Full-order residual curves of reduced trajectories: the fused kernel (``ops.trajectory_residuals`` ->
rt_trajectory_residuals) beside two alternatives, all in one process:

  (i)  the same numbers composed from existing operators: ``ops.gemm_nn`` lifts one trajectory at a time (the lifted
       block of (nt + 2) x N_h doubles goes to HBM), a torch stencil forms the rows and the two sums;
  (ii) what certifying a point costs today: ``fom.fom_sweep`` of the same points (``--fom-chunk`` steps a call) plus
       ``ops.trajectory_errors`` of every block.

Default shape: N_h = 1e5, nt = 1000, r = 80, MockBurgers on a moving interval (tests/fom_cases.py), a random orthonormal
basis and random coefficients, 1 and 32 trajectories resident on the device.  Per trajectory count, after a warm-up of all
three routes, ``--reps`` calls of each in alternation, device-event times (median, min, max).  Writes a table and one JSON
line per count to ``--out`` and prints the JSON lines."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import fom as device_fom  # noqa: E402
from romtime_amd import ops  # noqa: E402
from romtime_amd._lib import Context  # noqa: E402
from tests import fom_cases as fc  # noqa: E402


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def composed(V, Vt, A, nx, tab, dt, bdf2, state_in_w):
    """(res, scale) by the header's formulas from a stored lift: one GEMM and some forty elementwise passes per trajectory."""
    n, nt, _ = A.shape
    Nh = nx + 1
    res, scale = (torch.empty((n, nt), dtype=torch.float64, device=V.device) for _ in range(2))
    node = torch.arange(Nh, dtype=torch.float64, device=V.device)[None, :]
    ramp = node / float(nx)
    two = torch.ones((nt, 1), dtype=torch.bool, device=V.device)
    two[0] = False
    two &= bool(bdf2)
    for j in range(n):
        X = torch.zeros((nt + 2, Nh), dtype=torch.float64, device=V.device)
        ops.gemm_nn(A[j], Vt, out=X[2:])
        X[:, 0] = 0.0
        X[:, -1] = 0.0
        x, un, un1 = X[2:], X[1:-1], X[:-2]
        h, alpha, c0, c1, a0, a1, a2 = (tab[:, j, q][:, None] for q in range(7))
        bdf = torch.where(two, 1.5, 1.0)
        ustar = torch.where(two, 2 * un - un1, un)
        past = torch.where(two, 2 * un - un1 / 2, un)
        w = (ustar if state_in_w else 0 * ustar) + c0 + c1 * ramp
        ae, be = (2 * w[:, :-1] + w[:, 1:]) / 6, (w[:, :-1] + 2 * w[:, 1:]) / 6
        lo = bdf * h / 6 + dt * (-alpha / h - be[:, :-1])
        di = bdf * 4 * h / 6 + dt * (2 * alpha / h + be[:, :-1] - ae[:, 1:])
        up = bdf * h / 6 + dt * (-alpha / h + ae[:, 1:])
        xs = (node * h)[:, 1:-1]
        load = h * (a0 + a1 * xs + a2 * xs * xs + a2 * h * h / 6)
        r = h / 6 * (past[:, :-2] + 4 * past[:, 1:-1] + past[:, 2:]) + dt * load
        lo[:, 0] = 0.0
        up[:, -1] = 0.0
        tl, tc, tr = lo * x[:, :-2], di * x[:, 1:-1], up * x[:, 2:]
        res[j] = torch.linalg.vector_norm(r - (tl + tc + tr), dim=1)
        scale[j] = torch.linalg.vector_norm(tl.abs() + tc.abs() + tr.abs() + r.abs(), dim=1)
    return res, scale


def certify_today(fom, mus, rec, V, A, chunk):
    """The FOM truth of every point and the error curves against it; returns the curves, or None where the sweep flags."""
    out = torch.empty(A.shape[:2], dtype=torch.float64, device=V.device)
    try:
        for first, block in device_fom.fom_sweep(fom, mus, chunk=chunk, rec=rec):
            for j in range(len(mus)):
                out[j, first:first + block.shape[1]] = ops.trajectory_errors(V, A[j, first:first + block.shape[1]], block[j].T)[0]
    except ArithmeticError:
        return None
    return out


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=99_999, help="cells: N_h = nx + 1")
    ap.add_argument("--nt", type=int, default=1000)
    ap.add_argument("--r", type=int, default=80)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fom-chunk", type=int, default=100)
    ap.add_argument("--out", default=os.path.join("profiles", "trajectory_residuals_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_residuals.py measures on the GPU only")
    nx, nt, r, Nh = a.nx, a.nt, a.r, a.nx + 1
    fom = fc.make_fom("burgers", nx, nt)
    gen = torch.Generator(device="cuda").manual_seed(0)
    V = torch.linalg.qr(torch.randn((Nh, r), dtype=torch.float64, device="cuda", generator=gen))[0].contiguous()
    Vt = V.T.contiguous()
    lines = [f"N_h = {Nh}, nt = {nt}, r = {r}, MockBurgers BDF2 on a moving interval, {torch.cuda.get_device_name(0)}; one process, all routes",
             f"warmed up, then {a.reps} calls of each in alternation, device-event times: median ms (min - max)",
             "",
             "trajectories   fused (rt_trajectory_residuals)   (i) gemm_nn lift + torch stencil   (ii) fom_sweep + trajectory_errors   (i) / fused   (ii) / fused   parity (i)"]
    raws = []
    for n in a.counts:
        mus = fc.mus_of("burgers", n)
        rec = fc.recipe(fom, mus)
        tab = ops.to_device(rec["tab"])
        A = (0.1 * torch.rand((n, nt, r), dtype=torch.float64, device="cuda", generator=gen) - 0.05).contiguous()
        args = (nx, tab, fom.dt, rec["bdf2"], rec["state_in_w"])
        routes = dict(fused=lambda: ops.trajectory_residuals(V, A, *args),
                      composed=lambda: composed(V, Vt, A, *args),
                      today=lambda: certify_today(fom, mus, rec, V, A, a.fom_chunk))
        first = {name: fn() for name, fn in routes.items()}                          # warm-up, and the parity of (i)
        routes["fused"]()
        info = Context.current().launch_info()
        torch.cuda.synchronize()
        parity = max(float(((first["fused"][q] - first["composed"][q]).abs() / first["fused"][1]).max()) for q in range(2))
        ms = {name: [] for name in routes}
        for _ in range(a.reps):
            for name, fn in routes.items():
                ms[name].append(timed_once(fn))
        med = {name: float(np.median(v)) for name, v in ms.items()}
        raw = dict(workload="full-order residual curves of reduced trajectories", N_h=Nh, nt=nt, r=r, trajectories=n, reps=a.reps,
                   fom_chunk=a.fom_chunk, device=torch.cuda.get_device_name(0), fused=dict(stats(ms["fused"]), launch_info=info),
                   composed=stats(ms["composed"]), fom_sweep_plus_errors=dict(stats(ms["today"]), flagged=first["today"] is None),
                   parity_composed=parity, us_per_step_per_trajectory_fused=1e3 * med["fused"] / (n * nt),
                   tflops_fused=2.0 * Nh * nt * r * n / (med["fused"] * 1e-3) / 1e12)
        raws.append(raw)
        print(json.dumps(raw), flush=True)
        cell = lambda k: f"{med[k]:9.2f} ({min(ms[k]):.2f} - {max(ms[k]):.2f})"
        lines.append(f"{n:12d}   {cell('fused'):>31}   {cell('composed'):>33}   {cell('today'):>35}   {med['composed'] / med['fused']:11.1f}   "
                     f"{med['today'] / med['fused']:12.1f}   {parity:.2e}")
    lines += ["", f"fused launch at {a.counts[-1]} trajectories: {raws[-1]['fused']['launch_info']}",
              "parity (i): largest |difference| / scale between the fused and the composed curves (res and scale).",
              "One run, one shape; no counters were collected, so what bounds the fused kernel is not established by this record."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("Full-order residual curves of reduced trajectories: rt_trajectory_residuals beside the routes without it\n"
                 "=========================================================================================================\n\n"
                 "tools/bench_residuals.py (defaults)\n\n" + "\n".join(lines) + "\n\n" + "\n".join("raw: " + json.dumps(x) for x in raws) + "\n")


if __name__ == "__main__":
    main()
