"""tests/bf16_ref.py against hand-built cases and against torch's fp32 -> bf16 conversion (no GPU): the yardstick of
the bf16-storage tests has to be right before it can hold a kernel to anything."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_ref as R  # noqa: E402


def bits(x):
    return int(R.bf16_bits(np.float64(x)))


def test_exact_ties_go_to_even():
    # 1 + 2^-8 lies halfway between 1 (mantissa 0x00, even) and 1 + 2^-7 (0x01, odd): down
    assert bits(1.0 + 2.0 ** -8) == 0x3F80
    # 1 + 3 * 2^-8 lies halfway between 1 + 2^-7 (odd) and 1 + 2^-6 (even): up
    assert bits(1.0 + 3 * 2.0 ** -8) == 0x3F82
    # integers: 257 between 256 and 258 (spacing 2 above 256) -> 256; 259 -> 260; negative ties mirror
    assert R.rne_bf16(257.0) == 256.0 and R.rne_bf16(259.0) == 260.0 and R.rne_bf16(-259.0) == -260.0
    assert R.rne_bf16(-257.0) == -256.0
    np.testing.assert_array_equal(R.rne_bf16(np.arange(256, 1024, dtype=np.float64)),
                                  [float(torch.tensor(float(v)).bfloat16()) for v in range(256, 1024)])


def test_just_above_and_below_a_tie():
    t = 1.0 + 2.0 ** -8
    assert R.rne_bf16(t + 2.0 ** -40) == 1.0 + 2.0 ** -7      # above the tie: up
    assert R.rne_bf16(t - 2.0 ** -40) == 1.0                  # below: down
    t = 1.0 + 3 * 2.0 ** -8
    assert R.rne_bf16(t - 2.0 ** -40) == 1.0 + 2.0 ** -7
    # the double-rounding trap: fp64 just above a bf16 tie whose fp32 rounding IS the tie (fp32 then rounds to even)
    x = 1.0 + 2.0 ** -8 + 2.0 ** -30
    assert np.float32(x) == np.float32(1.0 + 2.0 ** -8)
    assert float(torch.tensor(np.float32(x)).bfloat16()) == 1.0      # fp64 -> fp32 -> bf16: rounded twice, down
    assert R.rne_bf16(x) == 1.0 + 2.0 ** -7                          # rounded once: up


def test_largest_finite_and_overflow():
    assert bits(R.BF16_MAX) == 0x7F7F and bits(-R.BF16_MAX) == 0xFF7F
    half_ulp = 2.0 ** 119
    assert R.rne_bf16(R.BF16_MAX + half_ulp * 0.999) == R.BF16_MAX          # below the tie
    assert R.rne_bf16(R.BF16_MAX + half_ulp) == np.inf                        # the tie: even neighbour is 2^128
    assert R.rne_bf16(-(R.BF16_MAX + half_ulp)) == -np.inf
    assert R.rne_bf16(1e300) == np.inf and R.rne_bf16(-1e300) == -np.inf
    assert bits(np.inf) == 0x7F80 and bits(-np.inf) == 0xFF80
    assert R.rne_bf16(3.3895e38) == R.BF16_MAX


def test_subnormals():
    assert bits(2.0 ** -133) == 0x0001 and bits(-2.0 ** -133) == 0x8001          # smallest subnormal
    assert R.rne_bf16(2.0 ** -134) == 0.0                                         # tie with 0: even (zero)
    assert bits(-2.0 ** -134) == 0x8000                                           # ... keeping the sign
    assert R.rne_bf16(2.0 ** -134 * 1.0001) == 2.0 ** -133
    assert R.rne_bf16(3 * 2.0 ** -134) == 2 * 2.0 ** -133                         # 1.5 quanta: to even (2)
    assert R.rne_bf16(5 * 2.0 ** -134) == 2 * 2.0 ** -133                         # 2.5 quanta: to even (2)
    assert bits(2.0 ** -126 - 2.0 ** -133) == 0x007F                              # largest subnormal
    assert bits(2.0 ** -126 - 2.0 ** -134) == 0x0080                              # tie with the smallest normal: even
    assert R.rne_bf16(1e-300) == 0.0


def test_nan_payloads_and_signed_zero():
    for payload in (1, 0x7, 1 << 44, 1 << 45, 0xF << 48, (1 << 52) - 1):
        for sign in (0, 1):
            u = np.array([(sign << 63) | (0x7FF << 52) | payload], dtype=np.uint64)
            x = u.view(np.float64)
            assert np.isnan(R.rne_bf16(x)).all()
            b = int(R.bf16_bits(x)[0])
            assert (b >> 15) == sign and (b & 0x7F80) == 0x7F80 and (b & 0x7F) != 0 and (b & 0x40)
            assert (b & 0x3F) == (payload >> 45) & 0x3F                            # top payload bits kept
    assert bits(0.0) == 0x0000 and bits(-0.0) == 0x8000
    assert np.signbit(R.rne_bf16(-1e-60)) and R.rne_bf16(-1e-60) == 0.0


def test_matches_torch_fp32_conversion_on_fp32_values():
    """on values exactly representable in fp32 there is one rounding either way: the helper equals torch's fp32 -> bf16
    conversion bit for bit -- random bit patterns (every exponent, subnormals included) and every tie pattern"""
    rng = np.random.default_rng(0)
    u = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    ties = (rng.integers(0, 1 << 16, 20000, dtype=np.uint64).astype(np.uint32) << 16) | 0x8000
    u = np.concatenate([u, ties, ties ^ 1, ties - 1, np.array([0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x00008000,
                                                               0x00018000, 0x80000000], np.uint32)])
    f = u.view(np.float32)
    f = f[np.isfinite(f)]
    want = torch.from_numpy(f.copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_bits(f.astype(np.float64))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(f[i].view(np.uint32))), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


def test_bracket_and_bound():
    ref = np.array([1.0, 1.0 + 2.0 ** -8, 300.0, -5.0, np.nan, R.BF16_MAX])
    d = R.fp32_sum_bound(np.abs(ref), np.array([1, 1, 10, 3, 1, 1]))
    lo, hi = R.bf16_bracket(ref, d)
    assert lo[0] == hi[0] == 1.0                                  # a small delta around a bf16 value: that value
    assert lo[1] == 1.0 and hi[1] == 1.0 + 2.0 ** -7              # around a tie: both neighbours
    assert lo[2] == hi[2] == 300.0 and lo[3] == hi[3] == -5.0
    assert np.isnan(lo[4]) and np.isnan(hi[4])
    assert lo[5] == R.BF16_MAX
    # the bound covers a real fp32 evaluation in three orders, with scales
    rng = np.random.default_rng(1)
    for k in (1, 2, 7, 100, 3000):
        t = rng.standard_normal(k) * np.exp(rng.standard_normal(k) * 3)
        c = rng.random(k) + 0.5
        exact = float(np.sum(t.astype(np.float32).astype(np.float64) * c.astype(np.float32)))
        for order in (np.arange(k), np.arange(k)[::-1], rng.permutation(k)):
            s = np.float32(0)
            for i in order:
                s = np.float32(np.float64(c[i].astype(np.float32)) * np.float64(t[i].astype(np.float32)) + np.float64(s))
            s = np.float32(s * np.float32(0.75)) + np.float32(2.5)
            d = R.fp32_sum_bound(0.75 * np.sum(np.abs(t.astype(np.float32).astype(np.float64) * c.astype(np.float32)))
                                 + 2.5, k + 1)
            assert abs(float(s) - (0.75 * exact + 2.5)) <= d


def test_spmm64_reference():
    ip = np.array([0, 2, 2, 5]); ix = np.array([0, 2, 1, 1, 0])
    H = np.array([[1.0, -2.0], [3.0, 4.0], [-5.0, 6.0]])
    rs = np.array([2.0, 1.0, 0.5]); cs = np.array([1.0, 4.0, 0.25])
    old = np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]])
    ref, asum, k = R.spmm64(ip, ix, H, rs, cs, old)
    want = np.array([[2 * (1 - 1.25) + 1, 2 * (-2 + 1.5) + 1], [2.0, 2.0], [0.5 * (12 + 12 + 1) + 3, 0.5 * (16 + 16 - 2) + 3]])
    np.testing.assert_array_equal(ref, want)
    np.testing.assert_array_equal(k[:, 0], [3, 1, 4])
    assert asum[0, 0] == 2 * (1 + 1.25) + 1


@pytest.mark.parametrize("x", [0.1, 1 / 3, 1e-40, 3e38, -7.77e-39, 65504.0])
def test_single_values_against_fractions(x):
    """one value, by exact rational arithmetic: the nearest bf16 of the fp64 value, ties to even"""
    from fractions import Fraction
    got = R.rne_bf16(x)
    fx = Fraction(x)
    e = max(Fraction(abs(x)).numerator.bit_length() - Fraction(abs(x)).denominator.bit_length(), -126)
    while Fraction(2) ** e > abs(fx):
        e -= 1
    e = max(e, -126)
    q = Fraction(2) ** (e - 7)
    r = fx / q
    lo = r.numerator // r.denominator
    rem = r - lo
    n = lo + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2) else 0)
    want = float(n * q)
    assert got == want
