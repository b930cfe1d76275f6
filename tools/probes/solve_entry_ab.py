"""The two stand-alone reduced solvers on fixed inputs, one line of SHA-256 hashes per case; a refactor of their kernels
must leave every line as it was.  rt_tracked_solve_batched: every call of tests/solve_cases.ladder_calls(r) (a first
call, then each rung from the inverse that call left) at the sizes where the kernel changes path, operands 16-byte
aligned (16-byte loads and stores when r is a multiple of 16) and 8 bytes off (scalar ones); hashed are x, Xinv, info
and the differences of the four sweep counters.  rt_gmres_batched: the 32 systems of tests/test_gmres_gpu.py at
restart 20 with the reference's tolerances, at sizes on both sides of one and two values per lane (64 | 65) and of the
Krylov basis in LDS or in the global work area (121 | 122); hashed are x, info and iters.  Runs against the checkout it
is started from (--root), so the same file serves the parent commit's build and this one's."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from romtime_amd import ops  # noqa: E402
from romtime_amd._lib import Context  # noqa: E402
from tests import solve_cases as sc  # noqa: E402
# The GMRES inputs are the test module's own generator (_systems) and tolerances (TOLS), on purpose: the probe hashes
# exactly what tests/test_gmres_gpu.py::test_kernel_against_scipy checks against SciPy.  Renaming them there means
# renaming them here.
from tests import test_gmres_gpu as tg  # noqa: E402

ctx = Context.current()
P = lambda t: C.c_void_p(t.data_ptr())


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def tracked(K, b, Xinv, misalign):
    B, r, _ = K.shape
    Kd, bd = sc.place(K, misalign), sc.place(b, misalign)
    Xd = sc.place(np.zeros_like(K) if Xinv is None else Xinv, misalign)
    info = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    before = ctx.sweep_stats()
    rc = ctx.lib.rt_tracked_solve_batched(ctx.handle, P(Kd), P(Xd), P(bd), r, B, int(Xinv is not None), P(info))
    assert rc == 0, rc
    after = ctx.sweep_stats()
    counters = np.array([after[k] - before[k] for k in sorted(after)], dtype=np.int64)
    return bd.cpu().numpy(), Xd.cpu().numpy(), info.cpu().numpy(), counters


for r in (1, 15, 16, 17, 48, 80):
    for misalign in (False, True):
        calls = sc.ladder_calls(r)
        out = [tracked(calls[0][0], calls[0][1], None, misalign)]
        X0 = out[0][1]
        for K, b, _route in calls[1:]:
            out.append(tracked(K, b, X0, misalign))
        counters = np.sum([o[3] for o in out], axis=0).tolist()
        print(f"CASE tracked_r{r}_{'off8' if misalign else 'aligned':8s} sha256 {sha(*[a for o in out for a in o])}"
              f"  counters {counters}", flush=True)

for r in (1, 64, 65, 121, 122, 128):
    systems = tg._systems(r, np.random.RandomState(1000 * r + 20))
    Ks, bs = np.stack([K for _, K, _ in systems]), np.stack([b for _, _, b in systems])
    x, info, iters = ops.gmres_solve(ops.to_device(Ks), ops.to_device(bs), dict(tg.TOLS["reference"], restart=20))
    x, info, iters = x.cpu().numpy(), info.cpu().numpy(), iters.cpu().numpy()
    print(f"CASE gmres_r{r:<15d} sha256 {sha(x, info, iters)}  iters {int(iters.sum())} unconverged {int((info != 0).sum())}",
          flush=True)
