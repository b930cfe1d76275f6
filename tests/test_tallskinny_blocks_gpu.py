"""The tall-skinny product's remainder columns (k % 16 in 1..12 go through four-block FP64 matrix instructions, 13..15 and 0
stay whole 16-column tiles), bit-exact inside NaN-poisoned operands and a canary-guarded output.

Operands as in test_gemm_nn_axpby_guarded: integers scaled by powers of two, every product and partial sum exact, so
X @ T from NumPy is the answer bit for bit in whatever order the instructions add.  Shapes are the smallest the kernel
accepts: 64 cus + 37 rows (one 16-row block per wave), 512 cus + 129 rows (two), three stages of the contraction (n = 96)
or a ragged one (n = 70)."""
import numpy as np
import pytest

from tests import guarded as gd
from tests.guarded import guarded_operand, guarded_output, exact_operands
from tests.test_guarded_kernels_gpu import LAY, P, _bits_for, _clean, _defaults_only, _exact, _host, ctx, cus  # noqa: F401

pytestmark = pytest.mark.gpu

_X = {}


def _x_operand(N, n):
    """The snapshot operand of (N, n), drawn once and left unchanged: (X, row exponents)."""
    if (N, n) not in _X:
        rng = np.random.default_rng(N + n)
        g = gd.graded_exponents(rng, N, 60)
        _X[N, n] = (exact_operands(rng, (n, N), _bits_for(2 * n + 2), g).T, g)
    return _X[N, n]


def _run(ctx, cus, N, n, k, bm, px=0, mis=False, pt=0, zero_cols=()):
    X, _ = _x_operand(N, n)
    rng = np.random.default_rng(1000 * n + k)
    T = exact_operands(rng, (n, k), _bits_for(2 * n + 2), gd.graded_exponents(rng, k, 60), k=n + 1)
    T[:, list(zero_cols)] = 0.0
    Xd, Td = guarded_operand(X, "C", px, mis), guarded_operand(T, "C", pt, False)
    ldx, lx = gd.leading_dim(Xd)
    Y = guarded_output((N, k), ld=k + 3)
    ctx.check(ctx.lib.rt_gemm_nn_axpby(ctx.handle, P(Xd), ldx, LAY[lx], P(Td), k + pt, N, n, k, 1.0, 0.0, P(Y.t), Y.ld, LAY["C"]),
              "rt_gemm_nn_axpby")
    plan = gd.tallskinny_plan(N, n, k, cus)
    assert plan is not None and plan["tile"][0] == bm, plan
    assert ctx.launch_info() == plan
    got, want = _host(Y.t), X @ T
    _exact(got, want)
    _clean([Y], [(Xd, X), (Td, T)])
    return got


# remainder only (1, 2, 3 groups), c = 13 (stays a padded tile), no remainder, full tiles plus each group count, more than
# four tiles
@pytest.mark.parametrize("k", [4, 8, 12, 13, 16, 20, 24, 28, 29, 40, 44, 108])
def test_one_row_block_per_wave(ctx, cus, k):
    _run(ctx, cus, 64 * cus + 37, 96, k, 64)


@pytest.mark.parametrize("k", [40, 56, 60])
def test_two_row_blocks_per_wave(ctx, cus, k):
    _run(ctx, cus, 512 * cus + 129, 96, k, 128)


GENERAL = [
    # id, n, k, X ld_pad, X misaligned, T ld_pad
    ("odd_ldx_misaligned_base", 96, 40, 1, True, 0),
    ("odd_ldt", 96, 22, 0, False, 1),
    ("odd_k_partial_group", 96, 39, 0, False, 0),
    ("ragged_stage", 70, 40, 0, False, 0),
]


@pytest.mark.parametrize("case", GENERAL, ids=[c[0] for c in GENERAL])
def test_general_loop(ctx, cus, case):
    _, n, k, px, mis, pt = case
    _run(ctx, cus, 64 * cus + 37, n, k, 64, px=px, mis=mis, pt=pt)


@pytest.mark.parametrize("k,zero_cols", [(40, (33, 36, 37, 38, 39)), (24, (16, 17, 18, 19, 23))], ids=["k40", "k24"])
def test_zero_columns_inside_the_remainder(ctx, cus, k, zero_cols):
    """Whole zero columns of T, a full group of them included, come out as the zeros NumPy gives (+0.0: the sum starts
    from +0.0 and a row of X is never all negative), bit for bit - _run compares bits."""
    got = _run(ctx, cus, 64 * cus + 37, 96, k, 64, zero_cols=zero_cols)
    assert not got[:, list(zero_cols)].view(np.int64).any()
