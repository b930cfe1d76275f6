"""The tridiagonal eigensolver (csrc/symeig.hip: rt_sym_eig_values, rt_sym_eig_values_part, rt_sym_eig_vectors) against
exact and extended-precision truth on an MI355X.  Helpers, matrices and LAPACK's figures: tests/eig_cases.py (premises:
tests/test_sym_eig_truth_cpu.py).

Two families.  ``exact``: G = H D H whose eigenvalues and eigenvectors are known exactly at every size (n = 3 ... 2048,
both sides of the one-workgroup form, of every size class, of both teams and of the wide route, every residue of
(n - 2) % 4 and % 2, k = n up to 512 and k = 1, 2, 63, 64, 65, 128 beyond, k = 1, 5, 13 at n = 66, slices passed as
``lam + first``).  ``recorded``: the graded (12 decades), clustered and singular-tail matrices of
tests/jacobi_cases.py with their long-double eigenvalues.  Every operand sits among NaNs (8 bytes off alignment at odd
n), ``lam`` and ``W`` between canaries; the route of every case is asserted from the device counters.

Measured, every product in long double on the device's output (eig_cases.measure): eigenvalues and per-vector
residuals in units of n eps lam_1, norms in eps, orthogonality |w_i . w_j| min(gap_ij / lam_1, 1) in n eps, and (exact
family) the distance of every vector from the exact one times gap_i / lam_1 in n eps.  A bar is four times the larger of
1 and LAPACK's figure on the same matrix (tests/golden/eig_lapack.json), at most 20.

Measured on an MI355X over all 114 cases (LAPACK's figure on the same matrices in brackets); no factor had to be set
from a measurement, every bar is the four-fold one:
exact family, n <= 10:     lam 0.04 ... 0.50 (0.10 ... 0.42)   res 0.08 ... 0.52 (0.17 ... 0.52)   norm 0.3 ... 1.9 (0.8 ... 2.7)
                           orth 0.07 ... 0.33 (0.02 ... 0.25)  vec 0.09 ... 0.37 (0.12 ... 0.47)
exact family, 63 ... 512:  lam 0.002 ... 0.047 (0.004 ... 0.047)  res 0.004 ... 0.062 (0.008 ... 0.069)  norm 2.2 ... 7.1 (2.6 ... 6.6)
                           orth 0.002 ... 0.019 (0.003 ... 0.025)  vec 0.002 ... 0.027 (0.002 ... 0.028)
exact family, 513 ... 2048 (k <= 128):  lam 0.001 ... 0.010 (0.001 ... 0.007)  res 0.001 ... 0.010 (0.002 ... 0.012)
                           norm 0.02 ... 8.3 (2.5 ... 5.7)  orth <= 0.001 (<= 0.002)  vec <= 0.002 (<= 0.004)
slices (130: 37 + 50, 1026: 700 + 65):  lam <= 0.019  res <= 0.024  norm 2.2 ... 8.0  orth <= 0.003  vec <= 0.007
recorded family, n = 7:    lam 0.03 ... 0.68 (0.01 ... 0.40)  res 0.07 ... 0.77 (0.01 ... 0.48)  norm 0.6 ... 1.5  orth 0.04 (0.003)
recorded family, 64 ... 512:  lam 0.003 ... 0.037 (0.005 ... 0.036)  res 0.004 ... 0.039 (0.009 ... 0.069)
                           norm 2.8 ... 8.9 (4.1 ... 9.4)  orth 0.001 ... 0.015 (0.003 ... 0.015)
Where ``pod_rules.separated`` holds (k = 1 ... 130 of the exact family) the worst distance from the exact eigenvector is
1.0e-15 ... 8.8e-13 (LAPACK: 5.7e-16 ... 2.84e-12), the largest on ``spread`` at n = 130 with all 130 vectors kept and a
smallest gap of 1.01e-4 lam_1.  n = 130 gives the same bits with "eig_one_xcd" 1 and 0 and on the team of 16.
Told apart (a hand-broken build, not committed: one inverse iteration instead of two, and the pair form of the
back-transformation reading slot 6 (blk >> 1) + 4 (blk & 1)): 32 of the 108 cases of the first three tests fail - the
wrong slot gives residuals of 6e10 ... 5e11 at every n > 1024, one iteration 6.5 ... 44 on ``res`` at n = 7, 63, 65,
130, 256, 512, 1024 and 4.7 on the 1e-6 cluster at n = 64.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import eig_cases as ec
from tests import guarded as gd
from tests import jacobi_cases as jc
from tests.guarded import guarded_operand, guarded_output

pytestmark = pytest.mark.gpu
EIG_COUNTERS = ("eig_wide_form", "eig_general_form", "eig_one_xcd", "eig_timeouts")
_ids = dict(ids=lambda c: str(c))


def P(t):
    return C.c_void_p(t.data_ptr())


def _route(n, moved, one_xcd_option=True, team_fits_an_xcd=True):
    """The hand-off form the counters must show for a solve of size n (csrc/symeig.hip): n <= 64 one workgroup (counted
    as eig_one_xcd), up to 512 the one-XCD form where the team was seen on one XCD and the general one elsewhere, up to
    1024 the 128-workgroup team in the general form, beyond it the wide route; never a time-out."""
    wide, general, one, timeouts = (moved[c] for c in EIG_COUNTERS)
    assert timeouts == 0, moved
    if n > 1024:
        assert (wide, general, one) == (1, 0, 0), moved
    elif n > 512 or (n > 64 and not (one_xcd_option and team_fits_an_xcd)):
        assert (wide, general, one) == (0, 1, 0), moved
    elif n > 64:
        assert wide == 0 and general + one == 1, moved
    else:
        assert (wide, general, one) == (0, 0, 1), moved


def _solve(G, ks, part=None, **route):
    """rt_sym_eig_values (or _part with ``part`` = (first, count)) on ``G`` among NaNs, 8 bytes off alignment at odd n,
    then rt_sym_eig_vectors for every k of ``ks`` on ``lam + first``; lam and every W between canaries.  Returns
    (lam of the computed indices, {k: W}) as host arrays after checking status, canaries, operand and route."""
    from romtime_amd._lib import Context

    ctx = Context.current()
    G = np.array(G, dtype=np.float64)      # a writable copy: the cached matrices are read-only
    n = G.shape[0]
    first, count = (0, n) if part is None else part
    Gd = guarded_operand(G, "C", 0, n % 2 == 1)
    lam = guarded_output((n,))
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    before = {c: ctx.counter(c) for c in EIG_COUNTERS}
    if part is None:
        ctx.check(ctx.lib.rt_sym_eig_values(ctx.handle, P(Gd), n, P(lam.t), P(status)), "rt_sym_eig_values")
    else:
        ctx.check(ctx.lib.rt_sym_eig_values_part(ctx.handle, P(Gd), n, first, count, P(lam.t), P(status)),
                  "rt_sym_eig_values_part")
    Ws = {}
    for k in ks:
        assert k <= count
        Ws[k] = guarded_output((n, k), misalign=n % 2 == 1)
        ctx.check(ctx.lib.rt_sym_eig_vectors(ctx.handle, n, k, P(lam.t[first:]), P(Ws[k].t)), "rt_sym_eig_vectors")
    torch.cuda.synchronize()
    moved = {c: ctx.counter(c) - before[c] for c in EIG_COUNTERS}
    assert int(status.item()) == 0, int(status.item())
    _route(n, moved, **route)
    bits = lam.t.view(torch.int64).cpu().numpy()
    assert np.all(np.r_[bits[:first], bits[first + count:]] == gd.CANARY_BITS), "written outside the slice"
    assert not np.any(bits[first:first + count] == gd.CANARY_BITS), "eigenvalues left unwritten"
    lam.prefilled = True
    assert lam.check() == [], lam.check()
    for k, W in Ws.items():
        assert W.check() == [], (k, W.check())
    assert gd.operand_intact(Gd, G) == [], gd.operand_intact(Gd, G)
    lam_h = lam.t[first:first + count].cpu().numpy()
    assert np.all(np.isfinite(lam_h)) and np.all(lam_h[:-1] >= lam_h[1:]), "lam is not non-increasing"
    return lam_h, {k: W.t.cpu().numpy() for k, W in Ws.items()}


def _hold(label, got, ref, what=""):
    print(ec.format_line("EIG-DEVICE", label + what, got, ref))
    for key in ec.FIGURES:
        if key in ref:
            assert got[key] <= ec.bar(ref[key]), (label + what, key, got[key], ec.bar(ref[key]), ref[key])


# ---- the exact family -------------------------------------------------------------------------------------------------------
def _ks(n):
    if n == 66:
        return (66, 1, 5, 13)
    return (n,) if n <= ec.FULL_K_MAX else ec.LARGE_KS


_RUNS: dict = {}


def _exact_run(spectrum, n):
    """One solve per matrix, shared by the tests below: (lam, {k: W}, {k: figures}).  A solve that failed is not run
    again: its failure is what every test that shares it reports."""
    key = (spectrum, n)
    if key not in _RUNS:
        try:
            ex = ec.exact(spectrum, n)
            lam, Ws = _solve(ex.G, _ks(n))
            figures = {}
            for k, W in Ws.items():
                cols = np.arange(k)
                figures[k] = ec.measure(ex.truth, np.arange(n), lam, cols, W, ex.apply, H=ex.vectors(cols))
            _RUNS[key] = (lam, Ws, figures)
        except Exception as failure:   # noqa: BLE001 - kept and raised again below
            _RUNS[key] = failure
    if isinstance(_RUNS[key], Exception):
        raise _RUNS[key]
    return _RUNS[key]


@pytest.mark.parametrize("spectrum,n", ec.exact_cases(), **_ids)
def test_exact_family(spectrum, n):
    """Eigenvalues, residuals, norms, gap-scaled orthogonality and gap-scaled distance from the exact eigenvectors of
    every returned column, for every k of the size, each within four times the larger of 1 and LAPACK's figure (at most
    20).  Column t does not depend on k: the k leading columns of a wider request are the same bits."""
    label = ec.exact_label(spectrum, n)
    ref = ec.lapack_reference(label)
    lam, Ws, figures = _exact_run(spectrum, n)
    widest = Ws[max(Ws)]
    for k in sorted(Ws, reverse=True):
        assert gd.bits_equal(Ws[k], widest[:, :k]), (k, gd.mismatch(Ws[k], widest[:, :k]))
    for k in sorted(Ws, reverse=True):
        _hold(label, figures[k], ref, f" k={k}")


@pytest.mark.parametrize("spectrum,n", ec.exact_cases(), **_ids)
def test_separated_vectors_are_within_the_stated_distance(spectrum, n):
    """The premise of ``pod_rules.separated``: wherever it holds for the k leading eigenvalues of the truth, every one of
    the k vectors is within 2e-12 of the exact eigenvector."""
    ex = ec.exact(spectrum, n)
    _, Ws, figures = _exact_run(spectrum, n)
    kmax = max(Ws)
    k = ec.separated_prefix(ex.truth, kmax)
    if k == 0:
        return                                  # no k at which the rule holds on this spectrum: nothing is claimed
    worst = float(figures[kmax]["vec_abs"][:k].max())
    print(f"EIG-DEVICE {ec.exact_label(spectrum, n)} separated k={k}: worst distance {worst:.2e}")
    assert worst <= ec.SEPARATED_BOUND, (k, worst)


@pytest.mark.parametrize("spectrum", ec.SPECTRA)
@pytest.mark.parametrize("n", sorted(ec.SLICES))
def test_slices(spectrum, n):
    """rt_sym_eig_values_part and its ``lam + first`` passed to rt_sym_eig_vectors: the vectors of a slice that starts
    at first > 0 are seeded differently from the full call's, so they are held to the truth, on the same bars; the
    eigenvalues are the full call's bits."""
    first, count = ec.SLICES[n]
    ex = ec.exact(spectrum, n)
    label = ec.exact_label(spectrum, n)
    lam, Ws = _solve(ex.G, (count,), part=(first, count))
    idx = np.arange(first, first + count)
    got = ec.measure(ex.truth, idx, lam, idx, Ws[count], ex.apply, H=ex.vectors(idx))
    _hold(label, got, ec.lapack_reference(label), f" slice={first}+{count}")
    full = _exact_run(spectrum, n)[0]
    assert gd.bits_equal(lam, full[first:first + count]), gd.mismatch(lam, full[first:first + count])


# ---- recorded long-double truth: deep and clustered spectra ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", jc.cases(jc.GPU_SIZES), ids=[jc.label(k, n) for k, n in jc.cases(jc.GPU_SIZES)])
def test_recorded_truth_family(kind, n):
    """The graded, clustered and singular-tail matrices of tests/jacobi_cases.py, every vector requested: eigenvalues
    (absolute), per-vector residuals and norms on every column; gap-scaled orthogonality over all pairs but those
    inside the 1e-6 cluster (an exactly repeated eigenvalue has gap 0 and weighs nothing).  Inside a cluster a vector is
    held to its residual alone."""
    G, _ = jc.matrix(kind, n)
    label = ec.recorded_label(kind, n)
    lam, Ws = _solve(G, (n,))
    skip = np.arange(ec.CLUSTER) if kind == "cluster" and n > ec.CLUSTER else ()
    got = ec.measure(jc.truth(kind, n), np.arange(n), lam, np.arange(n), Ws[n], ec.dense_apply(G), skip=skip)
    _hold(label, got, ec.lapack_reference(label))


# ---- routes ---------------------------------------------------------------------------------------------------------------------
def test_hand_off_forms_agree_on_the_truth():
    """n = 130 with the ctx option "eig_one_xcd" 1 and 0: the one-XCD hand-off (where the team was seen on one XCD) and
    the write-through form, each asserted from its counter, held to the same bars and to the same bits."""
    from romtime_amd._lib import Context

    ctx = Context.current()
    ex = ec.exact("spread", 130)
    label = ec.exact_label("spread", 130)
    ref = ec.lapack_reference(label)
    out = {}
    try:
        for option in (1, 0):
            ctx.set_option("eig_one_xcd", option)
            lam, Ws = _solve(ex.G, (130,), one_xcd_option=bool(option))
            got = ec.measure(ex.truth, np.arange(130), lam, np.arange(130), Ws[130], ex.apply, H=ex.vectors(np.arange(130)))
            _hold(label, got, ref, f" eig_one_xcd={option}")
            out[option] = (lam, Ws[130])
    finally:
        ctx.set_option("eig_one_xcd", 1)
    assert gd.bits_equal(out[1][0], out[0][0]), gd.mismatch(out[1][0], out[0][0])
    assert gd.bits_equal(out[1][1], out[0][1]), gd.mismatch(out[1][1], out[0][1])


def test_half_team_agrees_on_the_truth():
    """A ctx confined to 16 CUs (two of every XCD, "cu_limit" 16): a team of 32 would be refused there, so a solve that
    succeeds ran the team of 16 workgroups, in the general form (its counter moves on that ctx).  n = 130: the bits of
    the full team, and the same bars."""
    from romtime_amd import _lib

    ex = ec.exact("spread", 130)
    label = ec.exact_label("spread", 130)
    lam0, Ws0, _ = _exact_run("spread", 130)
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rt_stream_create_cu_range(0, 0, 2, C.byref(h)) == 0 and h.value
    masked = _lib.Context(0)
    masked.set_option("cu_limit", 16)
    st = torch.cuda.ExternalStream(h.value)
    torch.cuda.synchronize()
    try:
        with masked.use(st):
            lam, Ws = _solve(ex.G, (130,), team_fits_an_xcd=False)
        st.synchronize()
    finally:
        masked.set_option("cu_limit", 0)
    # (this stream stays: torch's allocator remembers the stream of every block handed out under it)
    got = ec.measure(ex.truth, np.arange(130), lam, np.arange(130), Ws[130], ex.apply, H=ex.vectors(np.arange(130)))
    _hold(label, got, ec.lapack_reference(label), " half team")
    assert gd.bits_equal(lam, lam0), gd.mismatch(lam, lam0)
    assert gd.bits_equal(Ws[130], Ws0[130]), gd.mismatch(Ws[130], Ws0[130])
