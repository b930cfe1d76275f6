"""rt_deim_greedy against the truth (helpers in tests/deim_cases.py; the host half is tests/test_deim_truth_cpu.py).

Every pick of the device is held to the extended-precision residual of the device's OWN sequence: |r_k[p_k]| >= (1 - 1e-9)
max|r_k|, which forces the true argmax wherever the true margin exceeds 1e-9 and lets either side of a near-tie win.
The shapes are the smallest that reach each edge of csrc/deim.hip (blocks of 8 columns, 512-row sweeps, 1024-row column
workgroups, 128-wide passes and 16 waves in the block start, m up to 1024); exact ties, power-of-two column scaling and row
permutations are bitwise statements with no tolerance.

Out of scope: a basis with an exactly zero residual column (a rank-deficient Phi).  The reference raises LinAlgError there
and what the device does is unspecified."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import deim_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from romtime_amd import ops as _ops

    return _ops


def _run(ops, Phi, want_margin=True):
    idx, PT_U, margin = ops.deim_greedy(Phi, want_margin=want_margin)
    return idx.cpu().numpy(), PT_U.cpu().numpy(), (margin.cpu().numpy() if want_margin else None)


def _greedy(ops, B, placed=None):
    """(idx, margin) of the basis ``B`` on the device, in both layouts: ``placed`` is the pair of device tensors to run
    (default: tight C and F copies).  PT_U is the gather to the last bit, the two layouts agree to the last bit, and
    leaving the margins out changes no index."""
    placed = placed or (ops.to_device(np.ascontiguousarray(B)), ops.to_device(np.asfortranarray(B)))
    out = []
    for Phi in placed:
        assert tuple(Phi.shape) == B.shape
        idx, PT_U, margin = _run(ops, Phi)
        assert idx.min() >= 0 and idx.max() < B.shape[0] and len(set(idx.tolist())) == B.shape[1], idx
        assert np.array_equal(PT_U, B[idx])
        assert np.array_equal(_run(ops, Phi, want_margin=False)[0], idx)
        out.append((idx, margin))
    assert np.array_equal(out[0][0], out[1][0]), np.nonzero(out[0][0] != out[1][0])[0][:8]
    assert np.array_equal(out[0][1], out[1][1])
    return out[0]


def _certified(B, idx, margin, label):
    cert = dc.assert_certified(B, idx, label=label)
    err = np.abs(margin - cert.margin)
    assert np.all(err <= 1e-6 * cert.margin + 1e-11), (label, np.nonzero(err > 1e-6 * cert.margin + 1e-11)[0][:8])
    return cert


@pytest.mark.parametrize("N,m", dc.RANDOM_SHAPES)
def test_random_bases_every_pick_is_the_maximum(ops, N, m):
    B = dc.basis("random", N, m)
    idx, margin = _greedy(ops, B)
    _certified(B, idx, margin, f"random-{N}x{m}")


@pytest.mark.parametrize("N,m", dc.SINE_SHAPES)
def test_sine_modes_either_side_of_a_near_tie(ops, N, m):
    """|phi(x)| = |phi(L - x)| to rounding: the second mode's two extrema are a true margin of 1e-16 (the one pick, off the
    axis, breaks the symmetry of the later residuals, whose smallest margins are some 4e-6).  The device may take either
    row; what it takes must be the maximum of the residual along ITS sequence, and so must every pick after it."""
    B = dc.basis("sine", N, m)
    idx, margin = _greedy(ops, B)
    cert = _certified(B, idx, margin, f"sine-{N}x{m}")
    assert cert.margin.min() < 1e-12          # the family does what it is here for


def test_a_near_tie_at_every_step(ops):
    """Row N - 1 - i = +-row i times (1 +- a few ulps): every step's two largest entries lie some 1e-16 apart, in different
    workgroups, and float64 rounding decides which one the device sees as larger.  Whichever it takes, the pick has to be
    the maximum of the true residual along the device's own sequence to 1e-9 - a comparison of index lists with the oracle
    means nothing here."""
    family, N, m, seed = dc.NEAR_MIRROR_CASE
    B = dc.basis(family, N, m, seed)
    idx, margin = _greedy(ops, B)
    cert = _certified(B, idx, margin, f"{family}-{N}x{m}")
    assert cert.margin.max() < 1e-12


@pytest.mark.parametrize("N,m", dc.SLICE_SHAPES)
def test_the_basis_where_it_lies(ops, N, m):
    """A column slice of a wider row-major buffer (odd leading dimension, first column 8 bytes off 16-byte alignment:
    the scalar loads of phase A, a last block of fewer than 8 columns) and a slice of a padded column-major buffer."""
    B = dc.basis("random", N, m)
    width = m + 6 + (m % 2 == 0)
    wide = np.full((N, width), 3.0)
    wide[:, 3:3 + m] = B
    row_major = ops.to_device(wide)[:, 3:3 + m]
    assert row_major.stride() == (width, 1) and width % 2 == 1 and row_major.data_ptr() % 16 == 8 and m % 8 != 0
    tall = np.full((m + 2, N + 5), 3.0)
    tall[1:1 + m, 2:2 + N] = B.T
    col_major = ops.to_device(tall)[1:1 + m, 2:2 + N].T
    assert col_major.stride() == (1, N + 5)
    idx, margin = _greedy(ops, B, placed=(row_major, col_major))
    _certified(B, idx, margin, f"slices-{N}x{m}")
    tight_idx, tight_margin = _greedy(ops, B)
    assert np.array_equal(idx, tight_idx) and np.array_equal(margin, tight_margin)


@pytest.mark.parametrize("family,N,m", dc.DUP_CASES)
def test_exact_ties_go_to_the_first_index(ops, family, N, m):
    """Row b(i) = +-row i: the device does the same fma sequence on both, so every step is an exact tie.  The pick is the
    lower row and the margin 0.0 to the last bit - through the pair merge of one thread (2i, 2i + 1), a thread's two
    halves (i, i + 512) and the workgroup partials (i, N - 1 - i)."""
    B = dc.basis(family, N, m)
    idx, margin = _greedy(ops, B)
    dc.assert_exact_ties(family, N, idx, margin)
    _certified(B, idx, margin, f"{family}-{N}x{m}")


def _oracle_margin(B):
    from oracle import romtime_oracle as oracle

    return oracle.deim_greedy(B)[2]


def test_power_of_two_column_scaling_changes_nothing(ops):
    """Every operation of the algorithm commutes with a power-of-two scaling of a column: the same indices and the same
    margins to the last bit."""
    _, N, m, seed = dc.SCALED_CASE
    B, Bs = dc.basis("random", N, m, seed), dc.basis("scaled", N, m, seed)
    assert min(_oracle_margin(B).min(), _oracle_margin(Bs).min()) > 1e-6          # precondition: no near-tie
    idx, margin = _greedy(ops, B)
    idx_s, margin_s = _greedy(ops, Bs)
    assert np.array_equal(idx_s, idx) and np.array_equal(margin_s, margin)
    _certified(Bs, idx_s, margin_s, f"scaled-{N}x{m}")


def test_row_permutation_permutes_the_indices(ops):
    """Rows meet the same arithmetic wherever they sit - workgroup, wave, lane, slot of a pair, the odd tail: the picks of
    the permuted basis are the permuted picks, the margins equal to the last bit."""
    _, N, m, seed = dc.PERMUTED_CASE
    B, Bp, perm = dc.basis("random", N, m, seed), dc.basis("permuted", N, m, seed), dc.row_permutation(N, m, seed)
    assert min(_oracle_margin(B).min(), _oracle_margin(Bp).min()) > 1e-6          # precondition: no near-tie
    idx, margin = _greedy(ops, B)
    idx_p, margin_p = _greedy(ops, Bp)
    assert np.array_equal(perm[idx_p], idx) and np.array_equal(margin_p, margin)
    _certified(Bp, idx_p, margin_p, f"permuted-{N}x{m}")


def test_the_size_limit(ops):
    """m = 1024 (N = 1040): the oracle's recorded picks (tests/golden/make_deim_limit.py; no margin below 1e-6) exactly,
    its margins to 1e-9 ((k + 2) eps S_k / max|r_k| reaches 1.6e-11 here), and - independent of the record - the
    greedy's defining property in float64: every multiplier of the LU along the device's picks is at most 1 + 1e-9."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deim_limit_1024.npz"), allow_pickle=False)
    assert (str(g["family"]), int(g["N"]), int(g["m"]), int(g["seed"])) == tuple(dc.LIMIT.values())
    B = dc.basis(**dc.LIMIT)
    print("DEIM-TRUTH limit: rebuilt basis against the recorded sample, max difference", np.abs(B[dc.LIMIT_PROBE] - g["probe"]).max())
    np.testing.assert_allclose(B[dc.LIMIT_PROBE], g["probe"], rtol=0, atol=dc.LIMIT_PROBE_ATOL)
    idx, margin = _greedy(ops, B)
    assert np.array_equal(idx, g["dofs"]), np.nonzero(idx != g["dofs"])[0][:8]
    np.testing.assert_allclose(margin, g["margin"], rtol=0, atol=1e-9)
    bound = dc.multiplier_bound(B, idx)
    print("DEIM-TRUTH limit 1040x1024 max multiplier - 1 =", bound - 1.0)
    assert bound <= 1.0 + dc.NEAR_TIE, bound


@pytest.mark.parametrize("N,m,ld,layout", [(1030, 1025, 1025, "C"), (1030, 1025, 1030, "F"), (5, 6, 6, "C"), (5, 6, 5, "F"),
                                           (40, 8, 7, "C"), (40, 8, 39, "F")],
                         ids=["m1025-C", "m1025-F", "m_gt_N-C", "m_gt_N-F", "ld_lt_m-C", "ld_lt_N-F"])
def test_bad_arguments_raise_and_write_nothing(N, m, ld, layout):
    from romtime_amd._lib import COL_MAJOR, ROW_MAJOR, Context, RomtimeHipError

    ctx = Context.current()
    Phi = torch.randn(N * m + 8, dtype=torch.float64, device="cuda")
    idx = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    PT_U = torch.full((m, m), -7.0, dtype=torch.float64, device="cuda")
    margin = torch.full((m,), -7.0, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx.lib.rt_deim_greedy(ctx.handle, P(Phi), N, m, ld, COL_MAJOR if layout == "F" else ROW_MAJOR, P(idx), P(PT_U),
                                P(margin))
    with pytest.raises(RomtimeHipError):
        ctx.check(rc, "rt_deim_greedy")
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((PT_U == -7.0).all()) and bool((margin == -7.0).all())
