"""Guarded operands and outputs for the kernel tests: NaN-poisoned memory around every operand, a canary around every
output, and integer-valued data whose products a correct kernel reproduces bit for bit.

* ``guarded_operand`` places a matrix, row- or column-major, with any leading-dimension padding, 16-byte aligned or
  offset by one element, inside a buffer of quiet NaNs.  A kernel that reads a single word outside the operand and
  cancels it with a zero from the other operand gets NaN instead of the right answer.
* ``guarded_output`` places an output view inside a buffer of NaNs with a fixed payload (the canary); ``check()``
  finds, bitwise, every word written outside the view and every word of the view left unwritten.
* ``exact_operands`` draws integers scaled by powers of two whose products and partial sums are all exact in float64:
  the NumPy product is then the exact answer, independent of summation order.
* ``project_guarded`` runs the reduced projection on such operands and such an output and asserts all of the above
  (tests/test_guarded_kernels_gpu.py, tests/test_project_truth_gpu.py).
* ``gemm_plan`` and friends restate the dispatch rules of the HIP library in Python, so that a test can assert the
  route its case takes (``Context.launch_info``): a changed threshold fails loudly instead of dropping coverage.

Plain module, not a conftest: everything here works on CPU tensors too (tests/test_guarded_helpers_cpu.py).
"""
from __future__ import annotations

import os

import numpy as np
import torch

QNAN_BITS = 0x7FF8000000000000            # the default quiet NaN
CANARY_BITS = 0x7FF8C0FFEE15BAD5           # a quiet NaN with a payload no kernel produces
GUARD = 128                                # guard rows / columns: the widest tile over-read (BT = 128 columns, KB = 16 rows)


def require_clean_env():
    """The route assertions hold for the library's defaults only: ROMTIME_* switches change routes and results."""
    bad = sorted(k for k in os.environ if k.startswith("ROMTIME_"))
    if bad:
        raise RuntimeError(f"unset {', '.join(bad)}: the guarded kernel tests assert the default dispatch routes")


def _as_bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64)


def _poisoned(numel: int, bits: int, device) -> torch.Tensor:
    buf = torch.empty(numel, dtype=torch.float64, device=device)
    _as_bits(buf).fill_(bits)
    return buf


def _start(buf: torch.Tensor, first: int, misalign: bool) -> int:
    """Element offset >= first whose address is 16-byte aligned, or 8 bytes past such an address."""
    addr = buf.data_ptr() + 8 * first
    off = first + ((addr // 8) % 2)                    # -> 16-byte aligned
    return off + (1 if misalign else 0)


def _region(shape, ld, layout):
    rows, cols = shape
    if layout == "C":
        return (ld, 1), (rows, ld)                     # strides, (outer extent, ld)
    return (1, ld), (cols, ld)


def guarded_operand(host, layout="C", ld_pad=0, misalign=False, device="cuda", guard=GUARD) -> torch.Tensor:
    """``host`` (2-D) copied into a row-major ("C") or column-major ("F") view with ld = width + ld_pad, surrounded by
    quiet NaNs: the padding of every line and ``guard`` whole lines before and after.  The base pointer is 16-byte
    aligned, or 8 bytes past that with ``misalign``.  The view keeps the whole buffer alive; ``operand_intact`` checks
    the buffer afterwards."""
    host = np.asarray(host, dtype=np.float64)
    assert host.ndim == 2 and layout in ("C", "F") and ld_pad >= 0
    rows, cols = host.shape
    width = cols if layout == "C" else rows
    ld = width + ld_pad
    strides, (outer, _) = _region(host.shape, ld, layout)
    numel = (outer + 2 * guard) * ld + 2
    buf = _poisoned(numel, QNAN_BITS, device)
    start = _start(buf, guard * ld, misalign)
    view = buf.as_strided(host.shape, strides, start)
    view.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return view


def leading_dim(view: torch.Tensor):
    """(ld, "C" | "F") of a guarded operand or output view."""
    s0, s1 = view.stride()
    if s1 == 1 and (s0 != 1 or view.shape[1] == 1):
        return s0, "C"
    return s1, "F"


def operand_intact(view: torch.Tensor, host) -> list[str]:
    """Problems with a guarded operand after a kernel ran: its values differ from ``host`` (bitwise), or a word of
    poison around it changed.  Restores nothing it did not find; empty list = intact."""
    problems = []
    got = _as_bits(view).cpu()
    want = torch.from_numpy(np.ascontiguousarray(np.asarray(host, dtype=np.float64))).view(torch.int64)
    diff = (got != want).nonzero()
    if len(diff):
        problems.append(f"{len(diff)} operand words changed, first at {tuple(diff[0].tolist())}")
    buf = torch.as_strided(view, (view.untyped_storage().nbytes() // 8,), (1,), 0)
    saved = view.clone()
    _as_bits(view).fill_(QNAN_BITS)
    try:
        bits = _as_bits(buf)
        chunk = 1 << 26
        for lo in range(0, bits.numel(), chunk):
            bad = (bits[lo:lo + chunk] != QNAN_BITS).nonzero()
            if len(bad):
                first = lo + int(bad[0]) - view.storage_offset()
                problems.append(f"{len(bad)} guard words changed in [{lo}, {lo + chunk}), first at offset {first} from the view")
    finally:
        view.copy_(saved)
    return problems


class GuardedOutput:
    """An output view of ``shape`` (row-major "C" or column-major "F", leading dimension ``ld``) inside a canary
    buffer.  ``t`` is the view; ``check()`` lists canary words changed outside it and view words left unwritten."""

    def __init__(self, shape, ld=None, layout="C", device="cuda", guard=GUARD, misalign=False, dtype=torch.float64):
        shape = tuple(int(s) for s in shape)
        if len(shape) == 1:
            shape = (1, shape[0])
            self._flat = True
        else:
            self._flat = False
        rows, cols = shape
        width = cols if layout == "C" else rows
        ld = width if ld is None else int(ld)
        assert ld >= width
        strides, (outer, _) = _region(shape, ld, layout)
        numel = (outer + 2 * guard) * ld + 2
        self.buf = _poisoned(numel, CANARY_BITS, device)
        start = _start(self.buf, guard * ld, misalign)
        self.ld, self.layout = ld, layout
        self.view2d = self.buf.as_strided(shape, strides, start)
        self.t = self.view2d[0] if self._flat else self.view2d
        if dtype == torch.int64:
            self.t = self.t.view(torch.int64)
        self.prefilled = False

    def fill(self, values):
        """Start from ``values`` instead of the canary (accumulating or in-place kernels): the view then counts as
        written whatever the kernel does to it."""
        v = torch.as_tensor(np.asarray(values, dtype=np.float64)).reshape(self.view2d.shape)
        self.view2d.copy_(v)
        self.prefilled = True
        return self

    def check(self) -> list[str]:
        bits = _as_bits(self.buf)
        mask = torch.zeros(bits.numel(), dtype=torch.bool, device=bits.device)
        mask.as_strided(self.view2d.shape, self.view2d.stride(), self.view2d.storage_offset()).fill_(True)
        problems = []
        outside = ((bits != CANARY_BITS) & ~mask).nonzero().flatten()
        if len(outside):
            rel = (outside[:4] - self.view2d.storage_offset()).tolist()
            problems.append(f"{len(outside)} words written outside the output, offsets from its start {rel}")
        if not self.prefilled:
            unwritten = (_as_bits(self.view2d) == CANARY_BITS).nonzero()
            if len(unwritten):
                problems.append(f"{len(unwritten)} output words never written, first {tuple(unwritten[0].tolist())}")
        return problems


def guarded_output(shape, ld=None, layout="C", device="cuda", **kw) -> GuardedOutput:
    return GuardedOutput(shape, ld, layout, device, **kw)


def exact_operands(rng, shape, bits, col_exponents=None, k=None, partner_bits=None):
    """Integers in [-2^bits, 2^bits] (zeros, +-1 and both ends included), column j scaled by 2^col_exponents[j].

    ``k`` terms of a contraction against a partner with integers below 2^partner_bits (default ``bits``): every partial
    sum then stays below 2^53 units of the column pair's scale, so each product, each sum in any order, and so the
    float64 result of NumPy, is exact.  Refuses a case where that does not hold."""
    rows, cols = shape
    pb = bits if partner_bits is None else partner_bits
    if k is not None:
        assert k * 2.0 ** (bits + pb) < 2.0 ** 53, f"{k} terms of {bits} x {pb} bits could reach 2^53"
    lim = 1 << bits
    v = rng.integers(-lim, lim + 1, size=shape).astype(np.float64)
    flat = v.reshape(-1)
    pick = rng.random(flat.size)
    flat[pick < 0.05] = 0.0
    flat[(pick >= 0.05) & (pick < 0.08)] = 1.0
    flat[(pick >= 0.08) & (pick < 0.11)] = -1.0
    if flat.size >= 2:
        flat[0], flat[-1] = float(lim), float(-lim)
    if col_exponents is not None:
        e = np.asarray(col_exponents)
        assert e.shape == (cols,) and np.all(np.abs(e) <= 300)
        v = np.ldexp(v, e[None, :].astype(np.int64))
    return v


def graded_exponents(rng, n, span=100):
    """Column exponents in [-span, span], the first and last columns at the two ends."""
    e = rng.integers(-span, span + 1, size=n)
    if n >= 2:
        e[0], e[-1] = -span, span
    return e


def bits_equal(got, want) -> bool:
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float64))
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float64))
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def mismatch(got, want) -> str:
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64)) if got.shape == want.shape else None
    if bad is None:
        return f"shape {got.shape} vs {want.shape}"
    i = tuple(bad[0])
    return f"{len(bad)} entries differ, first at {i}: {got[i]!r} vs {want[i]!r}"


# ---- the reduced projection on guarded buffers ---------------------------------------------------------------------------

def device_pattern(indptr, indices, device="cuda"):
    """(indptr, indices) of a CSR pattern as device tensors; indices keeps one word when the pattern has no entry, so
    that its pointer is not null."""
    ip = torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(device)
    ix = torch.zeros(max(len(indices), 1), dtype=torch.int64, device=device)
    ix[:len(indices)] = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int64))
    return ip, ix


def project_guarded(ctx, pattern, data, V, dlay="C", dpad=0, vpad=0, vmis=False, vguard=GUARD, single=False):
    """A_N[b] = V^T (A_b V) through rt_project_csr_batched (rt_project_csr with ``single``: one value vector) with V
    (N x r) and data (nnz x B) as guarded operands and the result in a guarded output.  ``pattern``: (indptr, indices),
    NumPy or ``device_pattern`` tensors.  Requires every output word written, nothing written outside the output, and
    operands and their poison intact; returns (A_N as a (B, r, r) host array, launch_info, the guarded V)."""
    import ctypes as C

    # where the view starts inside its buffer: data_ptr() of a view without elements (nnz = 0) is null
    P = lambda t: C.c_void_p(t.untyped_storage().data_ptr() + t.element_size() * t.storage_offset())
    ip, ix = pattern if isinstance(pattern[0], torch.Tensor) else device_pattern(*pattern)
    (N, r), (nnz, B) = V.shape, data.shape
    assert ip.numel() == N + 1
    Vd = guarded_operand(V, "C", vpad, vmis, guard=vguard)
    Dd = guarded_operand(data, dlay, dpad, False)
    ldd, dl = leading_dim(Dd)
    AN = guarded_output((B * r, r))
    if single:
        assert B == 1 and dl == "F"
        ctx.check(ctx.lib.rt_project_csr(ctx.handle, P(ip), P(ix), P(Dd), N, P(Vd), r + vpad, r, P(AN.t)), "rt_project_csr")
    else:
        ctx.check(ctx.lib.rt_project_csr_batched(ctx.handle, P(ip), P(ix), P(Dd), ldd, {"C": 0, "F": 1}[dl], B, N, P(Vd), r + vpad,
                                                 r, P(AN.t)), "rt_project_csr_batched")
    info = ctx.launch_info()
    torch.cuda.synchronize()
    got = AN.t.cpu().numpy().reshape(B, r, r)
    assert AN.check() == [], AN.check()
    for view, host in ((Vd, V), (Dd, data)):
        problems = operand_intact(view, host)
        assert problems == [], problems
    return got, info, Vd


# ---- the dispatch rules of the HIP library, restated (route assertions) -----------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def gemm_plan(M, Nn, K, symmetric, allow_split, cus):
    """launch_info of rt_gemm_strided (gemm_mfma.hip) for an M x Nn output over K."""
    tu = lambda e: 4 if e >= 128 else _cdiv(e, 32)
    mt, nt = tu(M), tu(Nn)
    if symmetric:
        nt = mt
    else:
        while nt > 1 and _cdiv(M, 32 * mt) * _cdiv(Nn, 32 * nt) < cus:
            nt -= 1
    skinny = not symmetric and Nn <= 64 and M >= 256
    BM, BN = (128, 16 * _cdiv(Nn, 16)) if skinny else (32 * mt, 32 * nt)
    tm, tn = _cdiv(M, BM), _cdiv(Nn, BN)
    ntiles = tm * (tm + 1) // 2 if symmetric else tm * tn
    splits = 1
    if allow_split and ntiles < 2 * cus:
        splits = (2 * cus) // ntiles
        if splits >= 8:
            splits &= ~7
        kps = max(_cdiv(K, splits), 128)
        kps = _cdiv(kps, 16) * 16
        splits = max(_cdiv(K, kps), 1)
    grid = ntiles if splits == 1 else 8 * _cdiv(splits, 8) * ntiles
    return dict(grid=grid, splits=splits, tile=(BM, BN))


def tallskinny_plan(N, n, k, cus):
    """launch_info of rt_tallskinny (tallskinny.hip), or None where it declines."""
    if k > 128 or n < 64 or N < 64 * cus:
        return None
    nt = _cdiv(k, 16)
    bm = 128 if (nt <= 4 and N >= 512 * cus) else 64
    return dict(grid=_cdiv(N, bm), splits=1, tile=(bm, 16 * nt))


def skinny_tn_plan(N, m, n, cus):
    """launch_info of rt_skinny_tn (rank_update.hip), or None where it declines."""
    if m > 16 or n > 4096 or N < 16384 or N * n < (1 << 22):
        return None
    pairs = _cdiv(n, 2)
    threads = 256 if pairs >= 256 else _cdiv(pairs, 64) * 64
    gy = _cdiv(pairs, threads)
    gx = max(min(cus * 16 // (threads // 64 * gy), N // (16 * m)), 1)
    rpw = _cdiv(_cdiv(N, gx), 8) * 8
    gx = _cdiv(N, rpw)
    return dict(grid=gx * gy, splits=gx, tile=(m, 2 * threads))


def rank_update_plan(N, n, cus):
    gy = _cdiv(n, 128)
    gx = max(min(cus * 8 // gy, _cdiv(N, 32)), 1)
    return dict(grid=gx * gy, splits=1, tile=(32, 128))


def expansion_plan(k):
    return dict(grid=_cdiv(k, 32), splits=1, tile=(64, 32))
