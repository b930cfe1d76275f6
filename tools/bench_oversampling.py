#!/usr/bin/env python3
"""Oversampled (M)DEIM: what the extra entries cost and what they buy, on one commit.

  cost    ``ops.deim_oversample`` at N = 1e5 and 1e6, m = 64 -> 128, in both memory orders, beside its NumPy restatement
          (tests/oversample_cases.py); one selection step (rt_deim_oversample_step) in bytes per second beside
          ``rt_bench_copy`` of the same session; the rectangular fold at r = 80 (``ops.dense_lstsq_multi``, 128 x 64, 6400
          right-hand sides) beside the square one (``ops.dense_solve_multi``, 64 x 64).
  effect  the piston workflow of tools/bench_online_classes.py (MockBurgers, nx = 2000, nt = 500, 8 points) built with
          ``OVERSAMPLING`` 1, 1.5 and 2: entries and 1 / sigma_min(PT_U) of every reductor, its worst interpolation error
          over the points and instants (``interpolation.evaluate_closed_form``), the worst res / scale of the reduced
          trajectories (``online.residuals``) and the distance of ``solve_many`` from the full-order sweep (``fom.fom_sweep``).

Writes the record to ``--out``.  A record, not a pass criterion."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def cost(rec, rows, sizes, m, m_s):
    from romtime_amd import ops
    from tests import oversample_cases as oc

    copy = ops.bench_copy(1 << 30, 10)
    rec["copy_gbps"] = copy
    rows.append(f"rt_bench_copy, 1 GiB, read + write: {copy:8.1f} GB/s")
    rows.append("")
    rows.append("      N    m  m_s  order   device loop  NumPy loop   ratio   same picks    one step    GB/s read   of copy")
    for N in sizes:
        B = np.linalg.qr(np.random.default_rng(N).standard_normal((N, m)))[0]
        t_np = None
        for order, host in (("C", np.ascontiguousarray(B)), ("F", np.asfortranarray(B))):
            Phi = ops.to_device(host)
            idx0 = ops.deim_greedy(Phi)[0]
            ops.deim_oversample(Phi, idx0, m + 2)                                              # warm-up
            t_dev, (idx, _, margin, sigma) = timed(lambda: ops.deim_oversample(Phi, idx0, m_s))
            idx = idx.cpu().numpy()
            if t_np is None:
                t0 = time.perf_counter()
                ref = oc.oversample(B, idx[:m], m_s)[0]
                t_np = time.perf_counter() - t0
            w, g, _ = ops.oversample_direction(B[idx[:m]])
            wd = ops.to_device(w)
            taken = torch.zeros(N, dtype=torch.uint8, device=Phi.device)
            pick = torch.empty(1, dtype=torch.int64, device=Phi.device)
            top2 = torch.empty(2, dtype=torch.float64, device=Phi.device)
            ops.deim_oversample_step(Phi, wd, g, taken, pick, top2)
            t_step, _ = timed(lambda: ops.deim_oversample_step(Phi, wd, g, taken, pick, top2), reps=50)
            gbps = N * m * 8 / t_step / 1e9
            rec["runs"].append(dict(N=N, m=m, m_s=m_s, order=order, device_s=t_dev, numpy_s=t_np, same=bool(np.array_equal(idx, ref)),
                                    step_s=t_step, step_gbps=gbps, sigma_min=[float(sigma[0]), float(sigma[-1])],
                                    min_margin=float(margin.min())))
            rows.append(f"{N:8d} {m:4d} {m_s:4d}  {order:5s}  {t_dev:10.4f} s {t_np:10.4f} s {t_np / t_dev:7.1f}   {'yes' if np.array_equal(idx, ref) else 'no':10s} "
                        f"{t_step * 1e6:9.1f} us {gbps:10.1f}   {gbps / (copy / 2):7.2f}")
    rows.append("(`of copy`: against half the copy figure, the bytes per second that kernel reads)")
    rows.append("")
    r, m_f, ms_f = 80, 64, 128
    rng = np.random.default_rng(0)
    basis_rom_T = ops.to_device(rng.standard_normal((m_f, r * r)))
    rect = ops.to_device(np.linalg.qr(rng.standard_normal((ms_f, m_f)))[0])
    square = ops.to_device(np.ascontiguousarray(rect[:m_f].cpu().numpy().T))
    ops.dense_lstsq_multi(rect, basis_rom_T, trans=True)
    ops.dense_solve_multi(square, basis_rom_T)
    t_rect, _ = timed(lambda: ops.dense_lstsq_multi(rect, basis_rom_T, trans=True), reps=10)
    t_sq, _ = timed(lambda: ops.dense_solve_multi(square, basis_rom_T), reps=10)
    rec["fold"] = dict(r=r, m=m_f, m_s=ms_f, lstsq_s=t_rect, solve_s=t_sq)
    rows.append(f"fold at r = {r} ({r * r} right-hand sides): rectangular {ms_f} x {m_f} (dense_lstsq_multi, trans) {t_rect * 1e3:.3f} ms, "
                f"square {m_f} x {m_f} (dense_solve_multi) {t_sq * 1e3:.3f} ms")


def effect(rec, rows, nx, nt, n_points, factors):
    from romtime_amd import DiscreteEmpiricalInterpolation, interpolation, online
    from romtime_amd.fom import fom_sweep
    from tools.bench_online_classes import build_model

    mus = [dict(alpha_0=0.045 + 0.009 * i, delta=0.295 + 0.002 * i, omega=8.7 + 0.35 * i) for i in range(n_points)]
    kinds = dict(mdeim_Mh="mass", mdeim_Ah="stiffness", mdeim_Ch="convection", mdeim_Nh_hat="nonlinear_lifting", deim_fgh="lifting",
                 mdeim_Nh="trilinear")
    rows.append("factor  reductor            m  m_s  1/sigma_min  worst interpolation error   |  worst res/scale   solve_many vs fom_sweep")
    for factor in factors:
        DiscreteEmpiricalInterpolation.OVERSAMPLING = factor
        try:
            fom, rom = build_model(nx, nt)
        finally:
            DiscreteEmpiricalInterpolation.OVERSAMPLING = 1.0
        ts = online.times(fom)
        per = {}
        for slot, kind in kinds.items():
            red = getattr(rom, slot)
            red.OVERSAMPLING = factor
            s = np.linalg.svd(red.PT_U, compute_uv=False)
            try:
                err = interpolation.evaluate_closed_form(red, kind, fom, mus, ts[::10], funcs=rom.basis if kind == "trilinear" else None)
                worst = float(np.max(err))
            except Exception as exc:                      # a record: say what did not run and go on
                worst = float("nan")
                print(f"{slot}: interpolation errors did not run: {type(exc).__name__}: {str(exc)[:100]}", flush=True)
            per[slot] = dict(m=int(red.N), m_s=int(red.PT_U.shape[0]), inv_sigma_min=float(1.0 / s[-1]), interpolation_error=worst)
        rom.ONLINE_ON = "device"
        curves = online.residuals(rom, mus, "online")
        res = float(max(np.max(c) for c in curves.values()))
        many = rom.solve_many(mus)
        (_, block), = fom_sweep(fom, mus, check="defect")
        V = many._V
        dist = float(max((torch.linalg.norm(many.uN[j] @ V.T - block[j]) / torch.linalg.norm(block[j])).item() for j in range(len(mus))))
        rec["effect"].append(dict(factor=factor, reductors=per, worst_res_over_scale=res, solve_many_vs_fom_sweep=dist))
        for i, (slot, p) in enumerate(per.items()):
            tail = f"   |  {res:15.4e}   {dist:15.4e}" if i == 0 else ""
            rows.append(f"{factor:6.2f}  {kinds[slot]:18s} {p['m']:3d}  {p['m_s']:3d}  {p['inv_sigma_min']:11.4g}  {p['interpolation_error']:25.4e}{tail}")
        print(rows[-len(per):], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--nt", type=int, default=500)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "oversampling_ab.txt"))
    a = ap.parse_args()
    rec = dict(gpu=torch.cuda.get_device_name(0), runs=[], effect=[], nx=a.nx, nt=a.nt, points=a.points)
    cost_rows, effect_rows = [], []
    for part, fn, args in (("cost", cost, (rec, cost_rows, a.sizes, 64, 128)),
                           ("effect", effect, (rec, effect_rows, a.nx, a.nt, a.points, (1.0, 1.5, 2.0)))):
        try:
            fn(*args)
        except Exception as exc:                          # a record: say what did not run and go on
            (cost_rows if part == "cost" else effect_rows).append(f"{part} did not finish: {type(exc).__name__}: {str(exc)[:200]}")
            print(f"{part} did not finish: {type(exc).__name__}: {exc}", flush=True)
    lines = [
        "Oversampled (M)DEIM: GappyPOD+E entries and the least-squares fold",
        "==================================================================",
        "",
        f"tools/bench_oversampling.py, one {rec['gpu']}, one process.  Wall clock between two device synchronisations; the loop once",
        "after a warm-up of two steps, a single step as the mean of 50 back-to-back calls (two launches each), the folds as the",
        "mean of 10.  The device loop includes its host SVDs and its three small transfers per step.",
        "",
    ] + cost_rows + [
        "",
        f"The piston workflow (MockBurgers, nx = {a.nx}, nt = {a.nt}, {a.points} points; tools/bench_online_classes.py) at OVERSAMPLING 1, 1.5, 2.",
        "Interpolation errors: worst over the points and every tenth instant (interpolation.evaluate_closed_form; N-MDEIM over the",
        "reduced basis).  res / scale: worst over the points and steps (online.residuals).  Distance: worst relative 2-norm of",
        "V uN - U over the points, U the homogeneous full-order sweep (fom.fom_sweep, check = 'defect').",
        "",
    ] + effect_rows + ["", "raw: " + json.dumps(rec)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
