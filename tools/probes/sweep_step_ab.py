"""Both online sweeps on a fixed seeded list of small cases that between them take every route of the reduced step:
tracked solve (scalar and 16-byte loads, one tile to 25), its in-kernel LU fallback, the r > 80 route (right-hand-side kernel, plain LU,
step close), GMRES mode, eager and graph replay, BDF1 and BDF2, with and without right-hand-side terms.  Prints per case
the SHA-256 of the returned trajectory's bytes, Context.sweep_stats() and the two GMRES counters; a refactor of the step
must leave every row as it was.  Runs against the checkout it is started from (--root), so the same file serves the
parent commit's build and this one's.  --time adds the r = 96 cases over --time-steps steps, ms per step of the whole
call (median of five calls), for the speed comparison."""
import argparse
import hashlib
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--time", action="store_true")
ap.add_argument("--time-steps", type=int, default=400)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from romtime_amd._lib import Context  # noqa: E402
from romtime_amd.sweep import hrom_bdf_sweep, rom_bdf_sweep  # noqa: E402
from romtime_amd.testing.mock import AffineBurgers  # noqa: E402


def synthetic(r, nt, n_mu, seed, dead=None):
    """Random interpolation terms in the form of tests/test_kernels_gpu.py's synthetic model; ``dead``: a parameter
    point whose operator coefficients are all zero (K_N = 0: the tracked solve hands it to its LU, which reports it)."""
    rng = np.random.RandomState(seed)
    spd = lambda: (lambda a: a @ a.T + r * np.eye(r))(rng.standard_normal((r, r)))

    def matrix_term(m, base):
        cols = np.concatenate([base.reshape(-1, 1), 0.05 * rng.standard_normal((r * r, m - 1))], axis=1)
        PT_U, _ = np.linalg.qr(rng.standard_normal((m, m)))
        theta = np.concatenate([1.0 + 0.1 * rng.standard_normal((nt, n_mu, 1)), 0.1 * rng.standard_normal((nt, n_mu, m - 1))], axis=-1)
        return dict(PT_U=PT_U, basis_rom=cols, F=theta @ PT_U.T)

    mass, lin = matrix_term(4, spd()), [matrix_term(3, spd()), matrix_term(5, rng.standard_normal((r, r)))]
    PTn, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    nl = dict(PT_U=PTn, basis_rom=0.3 * rng.standard_normal((r * r, 6)), W=0.2 * rng.standard_normal((6, r)),
              C=0.1 * rng.standard_normal((nt, n_mu, 6)), S=1.0 + 0.1 * rng.standard_normal((nt, n_mu)))
    PTf, _ = np.linalg.qr(rng.standard_normal((4, 4)))
    rhs = [dict(PT_U=PTf, basis_rom=rng.standard_normal((r, 4)), F=rng.standard_normal((nt, n_mu, 4)))]
    if dead is not None:
        kill3 = np.arange(n_mu)[None, :, None] == dead
        zero = lambda term: dict(term, F=np.where(kill3, 0.0, term["F"]))
        mass, lin = zero(mass), [zero(t) for t in lin]
        nl = dict(nl, C=np.where(kill3, 0.0, nl["C"]), S=np.where(kill3[:, :, 0], 0.0, nl["S"]))
    return mass, lin, nl, rhs


def direct(r, nt, bdf2, with_rhs=True):
    fom = AffineBurgers(N=3000, nt=nt, dt=2e-3, bdf2=bdf2, seed=3)
    rng = np.random.RandomState(r)
    xs = (np.arange(fom.Nh) + 0.5) / fom.Nh
    V, _ = np.linalg.qr(np.stack([np.sin((k + 1) * np.pi * xs) for k in range(r)], axis=1) + 1e-3 * rng.standard_normal((fom.Nh, r)))
    mus = [dict(alpha=0.5 + 0.2 * i, beta=1.0 - 0.1 * i, delta=0.3 + 0.05 * i, omega=7.0 + i) for i in range(3)]
    d = fom.descriptor(mus)
    return (V, d["indptr"], d["indices"], d["mass"], d["terms"], d["term_coef"], d["tril"],
            d["rhs_terms"] if with_rhs else None, d["rhs_coef"] if with_rhs else None, d["dt"])


ctx = Context.current()


def report(name, run, graph=False):
    ctx.set_option("sweep_graph", 1 if graph else 0)
    try:
        u = run()
    finally:
        ctx.set_option("sweep_graph", 0)
    torch.cuda.synchronize()
    sha = hashlib.sha256(u.cpu().numpy().tobytes()).hexdigest()
    print(f"CASE {name:30s} sha256 {sha}  stats {ctx.sweep_stats()}  gmres_iterations {ctx.counter('sweep_gmres_iterations')}"
          f"  gmres_unconverged {ctx.counter('sweep_gmres_unconverged')}", flush=True)


for bdf2 in (True, False):
    tag = "bdf2" if bdf2 else "bdf1"
    model = synthetic(11, 9, 3, seed=3)
    report(f"hrom_r11_{tag}", lambda: hrom_bdf_sweep(*model, 1e-2, bdf2=bdf2))
    report(f"hrom_r11_{tag}_graph", lambda: hrom_bdf_sweep(*model, 1e-2, bdf2=bdf2), graph=True)
    dead = synthetic(11, 9, 3, seed=3, dead=1)
    report(f"hrom_r11_{tag}_dead", lambda: hrom_bdf_sweep(*dead, 1e-2, bdf2=bdf2))
    report(f"hrom_r11_{tag}_dead_graph", lambda: hrom_bdf_sweep(*dead, 1e-2, bdf2=bdf2), graph=True)
    big = synthetic(96, 5, 2, seed=7)
    report(f"hrom_r96_{tag}", lambda: hrom_bdf_sweep(*big, 1e-2, bdf2=bdf2))
    report(f"direct_r24_{tag}", lambda: rom_bdf_sweep(*direct(24, 40, bdf2), bdf2=bdf2))
    report(f"direct_r96_{tag}", lambda: rom_bdf_sweep(*direct(96, 6, bdf2), bdf2=bdf2))
wide = synthetic(32, 9, 3, seed=5)
report("hrom_r32_bdf2", lambda: hrom_bdf_sweep(*wide, 1e-2, bdf2=True))
report("hrom_r32_bdf2_graph", lambda: hrom_bdf_sweep(*wide, 1e-2, bdf2=True), graph=True)
report("hrom_r11_gmres", lambda: hrom_bdf_sweep(*synthetic(11, 9, 3, seed=3), 1e-2, bdf2=True, solver="gmres"))
report("hrom_r96_gmres", lambda: hrom_bdf_sweep(*synthetic(96, 5, 2, seed=7), 1e-2, bdf2=True, solver="gmres"))
report("direct_r24_gmres", lambda: rom_bdf_sweep(*direct(24, 40, True), bdf2=True, solver="gmres"))
report("direct_r24_no_rhs", lambda: rom_bdf_sweep(*direct(24, 40, True, with_rhs=False), bdf2=True))
report("direct_r96_no_rhs", lambda: rom_bdf_sweep(*direct(96, 6, True, with_rhs=False), bdf2=True))
# the tracked solve's 16-byte loads with the direct sweep's one shared M_N, its smallest (one tile) and largest (25 tiles)
# sizes, and GMRES with the Krylov basis in the global work area (r > 121 at restart 20)
report("direct_r32_bdf2", lambda: rom_bdf_sweep(*direct(32, 12, True), bdf2=True))
report("hrom_r16_bdf2", lambda: hrom_bdf_sweep(*synthetic(16, 9, 3, seed=11), 1e-2, bdf2=True))
report("hrom_r80_bdf2", lambda: hrom_bdf_sweep(*synthetic(80, 5, 2, seed=13), 1e-2, bdf2=True))
report("hrom_r128_gmres", lambda: hrom_bdf_sweep(*synthetic(128, 3, 2, seed=17), 1e-2, bdf2=True, solver="gmres"))

if args.time:
    nt = args.time_steps

    def per_step(run):
        run()
        torch.cuda.synchronize()
        out = []
        for _ in range(5):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / nt)
        return sorted(out)[2]

    for bdf2 in (True, False):
        tag = "bdf2" if bdf2 else "bdf1"
        mass, lin, nl, rhs = synthetic(96, nt, 2, seed=7)
        onto = lambda t: dict(t, F=torch.as_tensor(t["F"]).cuda()) if "F" in t else t
        hmodel = (onto(mass), [onto(t) for t in lin], nl, [onto(t) for t in rhs])
        print(f"TIME {args.label:8s} hrom_r96_{tag:5s} ms_per_step {per_step(lambda: hrom_bdf_sweep(*hmodel, 1e-2, bdf2=bdf2)):.5f}", flush=True)
        dmodel = direct(96, nt, bdf2)
        print(f"TIME {args.label:8s} direct_r96_{tag:5s} ms_per_step {per_step(lambda: rom_bdf_sweep(*dmodel, bdf2=bdf2)):.5f}", flush=True)
