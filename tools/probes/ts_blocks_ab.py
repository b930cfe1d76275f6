"""Back-projection Y (1e6 x k) = X (1e6 x 512) T on the whole chip, ms per launch over 30 launches back to back, for the
widths given (default 32 40 48: k = 32 and 48 are whole tiles, k = 40 takes the four-block remainder path).  Runs against
the checkout it is started from (--root), so the same file times the parent commit's build and this one's, alternated
by the caller; random normal data, three rounds per width."""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--k", type=int, nargs="+", default=[32, 40, 48])
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402
from romtime_amd import ops  # noqa: E402

gen = torch.Generator(device="cuda").manual_seed(0)
X = torch.randn((args.rows, 512), dtype=torch.float64, device="cuda", generator=gen)


def timeit(fn, reps=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for k in args.k:
    T = torch.randn((512, k), dtype=torch.float64, device="cuda", generator=gen)
    Y = torch.empty((args.rows, k), dtype=torch.float64, device="cuda")
    ms = [timeit(lambda: ops.gemm_nn(X, T, out=Y)) for _ in range(3)]
    gb = args.rows * (512 + k) * 8 / 1e9
    print(f"{args.label:8s} k={k:3d}  " + "  ".join(f"{m:.4f}" for m in ms) + f"  ms   best {gb / min(ms):.2f} TB/s", flush=True)
