#!/usr/bin/env python3
"""(M)DEIM interpolation errors of whole snapshot sets: three routes to the same numbers, timed in one process.

* fused: ``ops.interpolation_errors`` (rt_interpolation_errors) on the folded basis ``Psi = basis_fom PT_U^-1``: one read
  of the snapshot block, nothing stored.  The fold (``interpolation.fold``, once per reductor) is timed separately.
* composed: what the library offered before - a row gather of the block, ``ops.dense_solve_multi`` for the thetas, two
  transposes, and ``ops.trajectory_errors`` on a copy of the block whose pinned entry holds f_0 - pin_value (against a basis
  whose pinned row is zero): a write of the block and two more reads.
* host loop: ``evaluate`` of the classes as it stands (``EVALUATE_ON = "host"``) on ``MockSolver`` (mass, MDEIM) and
  ``MockBurgers`` (trilinear, N-MDEIM with 3 states) of the same N_h and m, for ``--host-samples`` samples, beside
  ``EVALUATE_ON = "device"`` on the same samples (FOM callbacks included in both).

Shapes: N in --N, m in --m, S snapshots, every snapshot contiguous.  Both device routes are warmed up, then timed in
alternation with device events (median, min, max of ``--reps`` calls); the bytes are those the fused route must move (F once,
Psi once per 64 snapshots through L2), the flops 2 N m S.  Prints one JSON line per shape and route; ``--out`` writes
the text record."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from romtime_amd import interpolation, ops  # noqa: E402
from romtime_amd._lib import Context  # noqa: E402


def timed(fn, reps=1):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def composed(basis0, PT_U, idx_dev, Ft, pin_value):
    """err (S) from the existing operators.  ``Ft``: S x N, snapshot s in row s; ``basis0``: the basis with row 0 zeroed."""
    C = Ft.index_select(1, idx_dev)                                   # S x m gather
    theta, _ = ops.dense_solve_multi(PT_U, C.T.contiguous())          # m x S
    A = theta.T.contiguous()                                          # S x m
    U = Ft.clone()
    U[:, 0] -= pin_value                                              # (f_0 - 1) - 0 = f_0 - pinned value
    return ops.trajectory_errors(basis0, A, U.T)[0]


def device_shape(N, m, S, reps, gen):
    basis = torch.randn((N, m), dtype=torch.float64, device="cuda", generator=gen) / np.sqrt(N)   # columns of about unit norm
    idx_dev, _, _ = ops.deim_greedy(basis)
    idx = idx_dev.cpu().numpy().astype(np.int64)
    PT_U = basis[idx_dev].contiguous()
    Ft = (torch.randn((S, m), dtype=torch.float64, device="cuda", generator=gen) @ basis.T).contiguous()
    Ft += 1e-3 * torch.randn((S, N), dtype=torch.float64, device="cuda", generator=gen) / np.sqrt(N)
    Ft[:, 0] = 1.0

    class Holder:                                                     # what interpolation.fold needs of a reductor
        basis_fom, _dev_cache = basis, {}

        @staticmethod
        def _device(key, array):
            return array

    Holder.PT_U = PT_U.cpu().numpy()
    t0 = time.perf_counter()
    Psi = interpolation.fold(Holder)
    torch.cuda.synchronize()
    fold_ms = 1e3 * (time.perf_counter() - t0)
    basis0 = basis.clone()
    basis0[0] = 0.0
    fused = lambda: ops.interpolation_errors(Psi, idx, Ft.T, pin=(0, 1.0))
    plain = lambda: composed(basis0, PT_U, idx_dev, Ft, 1.0)
    e_f, e_c = fused(), plain()
    fused()
    info = Context.current().launch_info()
    torch.cuda.synchronize()
    parity = float(((e_f - e_c).abs() / e_c.abs()).max())
    ms_f, ms_c = [], []
    for _ in range(reps):
        ms_f += timed(fused)
        ms_c += timed(plain)
    bytes_f = 8.0 * N * S
    out = dict(N=N, m=m, S=S, fold_ms_first_call=fold_ms, max_rel_difference=parity, launch_info=info,
               fused=stats(ms_f), composed=stats(ms_c))
    out["fused"].update(GB_per_s_of_F=bytes_f / out["fused"]["median_ms"] / 1e6, TFLOP_per_s=2.0 * N * m * S / out["fused"]["median_ms"] / 1e9)
    out["speedup_median"] = out["composed"]["median_ms"] / out["fused"]["median_ms"]
    return out


def host_loops(nx, m, samples, gen):
    """The classes' evaluate on the mock FOMs, host loop and device route, per sample (FOM callbacks included)."""
    from romtime_amd import MatrixDiscreteEmpiricalInterpolation, MatrixDiscreteEmpiricalInterpolationNonlinear
    from romtime_amd.testing.mock import MockBurgers

    solver = MockBurgers(domain={"L0": 1.0, "nx": nx, "T": 5.0, "nt": 100}, Lt=lambda t, **mu: 1.0 + 0.1 * mu["delta"] * t)
    solver.setup()
    mu = dict(alpha_0=1.0, delta=0.4, omega=9.0)
    x = np.linspace(0.0, 1.0, nx + 1)
    states = np.stack([(1.0 + x) ** (k + 1) for k in range(3)], axis=1)
    out = {}
    for name in ("mass_mdeim", "trilinear_nmdeim"):
        if name == "mass_mdeim":
            red = MatrixDiscreteEmpiricalInterpolation(name=name, assemble=solver.assemble_mass)
            red.rows, red.cols = red.get_matrix_topology(mu=mu, t=1.0)
            per_t, ts = 1, list(np.linspace(0.1, 4.9, samples))
        else:
            red = MatrixDiscreteEmpiricalInterpolationNonlinear(name=name, assemble=solver.assemble_trilinear)
            red.rows, red.cols = red.get_matrix_topology(mu=mu, t=1.0, u_n=x)
            red.u_n = states
            per_t, ts = 3, list(np.linspace(0.1, 4.9, max(samples // 3, 1)))
        N = len(red.rows)
        basis = torch.randn((N, m), dtype=torch.float64, device="cuda", generator=gen) / np.sqrt(N)
        basis[0] = 0.0
        red.load_fom_basis(basis=basis.cpu().numpy())
        rec = dict(N=N, m=m, samples=per_t * len(ts))
        for route in ("host", "device", "host", "device"):            # the first pair warms up (resident bases, the fold)
            red.errors_rom.clear()
            red.mu_space["online"] = []
            red.EVALUATE_ON = route
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            red.evaluate(ts, mu_space=[mu])
            torch.cuda.synchronize()
            rec[route + "_ms_per_sample"] = 1e3 * (time.perf_counter() - t0) / rec["samples"]
            rec[route + "_errors"] = [float(v) for v in red.errors_rom[0][:2]]
        rec["speedup"] = rec["host_ms_per_sample"] / rec["device_ms_per_sample"]
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[100_000, 300_000])
    ap.add_argument("--m", type=int, nargs="+", default=[32, 120])
    ap.add_argument("--S", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=48)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_interpolation.py measures on the GPU only")
    gen = torch.Generator(device="cuda").manual_seed(17)
    lines = [f"device: {torch.cuda.get_device_name(0)}; S = {a.S} contiguous snapshots; {a.reps} alternating calls after a warm-up of both routes"]
    for N in a.N:
        for m in a.m:
            rec = device_shape(N, m, a.S, a.reps, gen)
            lines.append(json.dumps(dict(kind="device routes", **rec)))
            print(lines[-1], flush=True)
    for m in a.m:
        rec = host_loops(a.N[0] // 3, m, a.host_samples, gen)
        lines.append(json.dumps(dict(kind="class evaluate, host loop vs device", m=m, **rec)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
