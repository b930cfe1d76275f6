"""The guard machinery of tests/guarded.py, on CPU tensors with NumPy stand-ins for the kernels: it must catch the bugs
the guarded GPU tests exist for."""
import numpy as np
import pytest
import torch

from tests import guarded as gd


def _host(rng, shape):
    return gd.exact_operands(rng, shape, 8, gd.graded_exponents(rng, shape[1], 40), k=64)


def _atb_reading_past_the_end(A: torch.Tensor, B: torch.Tensor, overread: bool):
    """C = A^T B; with ``overread`` every column of A also reads the word after its last row and multiplies it by a zero
    (the kind of clamped-load bug a finite padding hides)."""
    N = A.shape[0]
    C = A.T @ B
    if overread:
        past = torch.as_strided(A, (1, A.shape[1]), A.stride(), A.storage_offset() + N * A.stride(0))
        C = C + past.T @ torch.zeros((1, B.shape[1]), dtype=torch.float64)
    return C


@pytest.mark.parametrize("layout", ["C", "F"])
@pytest.mark.parametrize("ld_pad", [0, 1, 5])
@pytest.mark.parametrize("misalign", [False, True])
def test_views_have_the_intended_strides_and_offsets(layout, ld_pad, misalign):
    rng = np.random.default_rng(1)
    host = _host(rng, (37, 11))
    v = gd.guarded_operand(host, layout, ld_pad, misalign, device="cpu")
    width = 11 if layout == "C" else 37
    ld = width + ld_pad
    assert v.stride() == ((ld, 1) if layout == "C" else (1, ld))
    assert gd.leading_dim(v) == (ld, layout)
    assert v.data_ptr() % 16 == (8 if misalign else 0)
    assert v.storage_offset() >= gd.GUARD * ld                      # a whole guard band before the view
    total = v.untyped_storage().nbytes() // 8
    outer = 37 if layout == "C" else 11
    assert total - (v.storage_offset() + (outer - 1) * ld + width) >= gd.GUARD * ld   # and after it
    assert gd.bits_equal(v.numpy(), host)
    assert gd.operand_intact(v, host) == []
    # the padding of every line is poison
    if ld_pad:
        line_pad = torch.as_strided(v, (1,), (1,), v.storage_offset() + width)
        assert torch.isnan(line_pad).all()


def test_a_hidden_read_past_the_operand_is_caught():
    rng = np.random.default_rng(2)
    Ah, Bh = _host(rng, (40, 6)), _host(rng, (40, 5))
    ref = Ah.T @ Bh
    # unguarded, tightly packed: the bug is invisible (the word past the end is finite or the next column's first)
    A_plain, B_plain = torch.from_numpy(Ah.copy(order="F")).T.contiguous().T, torch.from_numpy(Bh)
    assert gd.bits_equal(_atb_reading_past_the_end(A_plain[:-1], B_plain[:-1], True).numpy(), Ah[:-1].T @ Bh[:-1])
    A = gd.guarded_operand(Ah, "F", 1, False, device="cpu")
    B = gd.guarded_operand(Bh, "C", 0, True, device="cpu")
    assert gd.bits_equal(_atb_reading_past_the_end(A, B, False).numpy(), ref)
    bad = _atb_reading_past_the_end(A, B, True).numpy()
    assert np.isnan(bad).all() and not gd.bits_equal(bad, ref)


def test_a_write_one_word_past_the_output_is_caught():
    out = gd.guarded_output((7, 5), ld=8, layout="C", device="cpu")
    out.t.copy_(torch.arange(35, dtype=torch.float64).reshape(7, 5))
    assert out.check() == []
    # one word past the last element of the view
    past = torch.as_strided(out.t, (1,), (1,), out.t.storage_offset() + 6 * 8 + 5)
    past.fill_(0.0)
    problems = out.check()
    assert len(problems) == 1 and "outside" in problems[0] and "[53]" in problems[0]


def test_a_write_into_the_line_padding_and_a_missed_word_are_caught():
    out = gd.guarded_output((6, 4), ld=9, layout="F", device="cpu")
    out.t.fill_(1.0)
    out.t[2, 3] = float("nan")                                       # a NaN result is a write, not the canary
    assert out.check() == []
    torch.as_strided(out.t, (1,), (1,), out.t.storage_offset() + 6).fill_(2.0)   # padding of column 0
    out2 = gd.guarded_output((6, 4), ld=9, layout="F", device="cpu")
    out2.t[:, :3].fill_(1.0)                                        # last column never written
    assert any("outside" in p for p in out.check())
    assert any("never written" in p and "(0, 3)" in p for p in out2.check())


def test_a_changed_operand_or_guard_is_reported():
    rng = np.random.default_rng(3)
    host = _host(rng, (9, 4))
    v = gd.guarded_operand(host, "C", 3, True, device="cpu")
    torch.as_strided(v, (1,), (1,), v.storage_offset() - 1).fill_(0.0)   # the word before the view
    assert any("guard" in p for p in gd.operand_intact(v, host))
    w = gd.guarded_operand(host, "F", 0, False, device="cpu")
    w[3, 2] = w[3, 2] * 2
    assert any("operand" in p for p in gd.operand_intact(w, host))
    assert gd.operand_intact(w, host)[0].endswith("(3, 2)")


def test_exact_operands_refuse_sums_that_could_reach_2_53():
    rng = np.random.default_rng(4)
    gd.exact_operands(rng, (4, 3), 20, k=(1 << 12) - 1)                # 2^12 * 2^40 < 2^53
    with pytest.raises(AssertionError):
        gd.exact_operands(rng, (4, 3), 20, k=1 << 13)                  # 2^13 * 2^40 = 2^53
    with pytest.raises(AssertionError):
        gd.exact_operands(rng, (4, 3), 20, k=100, partner_bits=40)


def test_exact_operands_are_graded_integers_and_their_products_exact():
    rng = np.random.default_rng(5)
    e = gd.graded_exponents(rng, 6, 200)
    A = gd.exact_operands(rng, (500, 6), 16, e, k=500)
    ints = np.ldexp(A, -e[None, :])
    assert np.array_equal(ints, np.round(ints)) and np.abs(ints).max() == 2 ** 16
    assert (ints == 0).any() and (ints == 1).any() and (ints == -1).any()
    assert e.min() == -200 and e.max() == 200
    # the float64 Gram matrix equals the exact integer one, rescaled
    G = A.T @ A
    Gi = ints.astype(object).T.dot(ints.astype(object))
    exact = np.array([[float(Gi[i, j]) * 2.0 ** int(e[i] + e[j]) for j in range(6)] for i in range(6)])
    assert gd.bits_equal(G, exact)


def test_romtime_switches_are_refused(monkeypatch):
    monkeypatch.delenv("ROMTIME_GRAM_FLAGS", raising=False)
    for k in [k for k in list(__import__("os").environ) if k.startswith("ROMTIME_")]:
        monkeypatch.delenv(k)
    gd.require_clean_env()
    monkeypatch.setenv("ROMTIME_GRAM_FLAGS", "16")
    with pytest.raises(RuntimeError, match="ROMTIME_GRAM_FLAGS"):
        gd.require_clean_env()


def test_dispatch_restatements_match_known_launches():
    # a few launches worked out by hand from the dispatchers
    assert gd.tallskinny_plan(100_000, 256, 8, 256)["tile"] == (64, 16)
    assert gd.tallskinny_plan(200_000, 256, 8, 256)["tile"] == (128, 16)
    assert gd.tallskinny_plan(1000, 256, 8, 256) is None
    assert gd.skinny_tn_plan(20_000, 8, 700, 256)["tile"] == (8, 512)
    assert gd.skinny_tn_plan(20_000, 17, 700, 256) is None
    p = gd.gemm_plan(200, 200, 100_000, True, True, 256)
    assert p["tile"] == (128, 128) and p["grid"] == 8 * -(-p["splits"] // 8) * 3
