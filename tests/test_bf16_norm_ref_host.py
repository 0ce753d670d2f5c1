"""tests/bf16_norm_ref.py checked on the CPU (no GPU, no library): the bit-level conversions against their definitions, the whole
restatement against float64 at shapes where every operation is exact (so the expected bits are known without any rounding argument),
against float64 with a half-ulp bound on ordinary data, and the proof that the helper pins the summation ORDER: a wrong order gives
other bits on an input built for it."""
import numpy as np
import pytest

import bf16_norm_ref as R


def test_bf16_conversions_are_the_definition():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    finite = bits[(bits & 0x7F80) != 0x7F80]
    f = R.bf16_bits_to_f32(finite)
    assert np.array_equal(R.f32_to_bf16_bits(f), finite)                          # every finite bf16 survives the round trip
    # round to nearest, ties to even: halfway between two neighbours goes to the one with an even pattern; anything past halfway goes up
    lo = finite[(finite & 0x7FFF) < 0x7F7F]                                        # (the neighbour above is finite)
    a, b = R.bf16_bits_to_f32(lo).astype(np.float64), R.bf16_bits_to_f32(lo + np.uint16(1)).astype(np.float64)
    mid = ((a + b) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (a + b) / 2)                     # the midpoint is an fp32 number
    even = np.where(lo & 1, lo + np.uint16(1), lo)
    assert np.array_equal(R.f32_to_bf16_bits(mid), even)
    toward = np.where(lo & 0x8000, np.float32(-np.inf), np.float32(np.inf)).astype(np.float32)
    up = np.nextafter(mid, toward)                                                 # one fp32 step past the midpoint, away from zero
    assert np.array_equal(R.f32_to_bf16_bits(up), lo + np.uint16(1))
    down = np.nextafter(mid, -toward)
    assert np.array_equal(R.f32_to_bf16_bits(down), lo)


@pytest.mark.parametrize("M,K", [(1, 128), (3, 4096), (2, 8192), (2, 32768)])
def test_restatement_equals_float64_where_every_operation_is_exact(M, K):
    """Row m holds +-2^e(m) in every column (random signs): ss = K 4^e exactly in any order, ss / K = 4^e, eps = 0, sqrt and the division
    are exact, inv = 2^-e, x inv = +-1, and y = +-w with w any bf16: nothing rounds, so float64 gives the expected bits."""
    rng = np.random.default_rng(K + M)
    e = rng.integers(-20, 30, size=M)
    sign = rng.choice([-1.0, 1.0], size=(M, K))
    x64 = sign * (2.0 ** e)[:, None]
    wbits = rng.integers(0x3C00, 0x4200, size=K).astype(np.uint16)               # bf16 values in [2^-7, 32), all 7 mantissa bits in use
    wbits[::3] |= 0x8000
    w64 = R.bf16_bits_to_f32(wbits).astype(np.float64)
    xbits = R.f32_to_bf16_bits_from_f64(x64)
    ss = R.sum_squares(xbits)
    assert np.array_equal(ss.astype(np.float64), K * 4.0 ** e)
    assert np.array_equal(R.inv_rms(ss, K, 0.0).astype(np.float64), 2.0 ** -e)
    y = R.rmsnorm_bf16(xbits, wbits, 0.0)
    assert np.array_equal(y, R.f32_to_bf16_bits_from_f64(sign * w64[None, :]))
    for order in R.ORDERS:                                                        # (exact sums do not depend on the order)
        assert np.array_equal(R.rmsnorm_bf16(xbits, wbits, 0.0, order), y)


def test_restatement_is_within_half_a_bf16_ulp_of_float64_on_ordinary_data():
    rng = np.random.default_rng(7)
    for M, K in [(3, 64), (5, 4096), (2, 11008)]:
        xbits = R.f32_to_bf16_bits((rng.standard_normal((M, K)) * 3).astype(np.float32))
        wbits = R.f32_to_bf16_bits((1 + 0.2 * rng.standard_normal(K)).astype(np.float32))
        y = R.bf16_bits_to_f32(R.rmsnorm_bf16(xbits, wbits, 1e-6)).astype(np.float64)
        xd, wd = R.bf16_bits_to_f32(xbits).astype(np.float64), R.bf16_bits_to_f32(wbits).astype(np.float64)
        ref = xd / np.sqrt((xd ** 2).mean(axis=1, keepdims=True) + np.float64(np.float32(1e-6))) * wd
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 7)
        # correctly rounded up to the fp32 path's noise: the sum (K roundings of relative size 2^-24 at most, far fewer in effect), the
        # division, the square root and the two products
        assert (np.abs(y - ref) <= 0.5 * ulp + 1e-6 * np.abs(ref)).all()


def test_a_wrong_summation_order_gives_other_bits():
    """One big square in front, then K - 1 small ones, each below half an ulp of the running sum: a left-to-right chain loses every one of
    them, the kernel's 256 partial sums keep them - and so do not agree with the chain.  The helper's own order must not be either of the
    two wrong ones, or the GPU test would accept a kernel that sums differently."""
    K = 4096
    x = np.full((1, K), 2.0 ** -5, dtype=np.float32)                              # squares 2^-10
    x[0, 0] = 2.0 ** 8                                                            # square 2^16: ulp 2^-7, half of it 2^-8 > 2^-10
    xbits = R.f32_to_bf16_bits(x)
    seq, ker = R.sum_squares(xbits, "sequential"), R.sum_squares(xbits, "kernel")
    assert float(seq[0]) == 2.0 ** 16                                             # the chain never moves
    exact = 2.0 ** 16 + (K - 1) * 2.0 ** -10
    # (thread 0's own chain still loses its 15 small squares behind the big one, 15 * 2^-10, and the butterfly rounds at 2^-7 steps)
    assert float(ker[0]) != float(seq[0]) and abs(float(ker[0]) - exact) <= 15 * 2.0 ** -10 + 4 * 2.0 ** -7
    # chunk-strided against chunk-consecutive threads: random data, 16 chunks per thread
    rng = np.random.default_rng(3)
    xb = R.f32_to_bf16_bits((rng.standard_normal((8, 32768)) * 2).astype(np.float32))
    a, b = R.sum_squares(xb, "kernel"), R.sum_squares(xb, "lane_major")
    assert (a != b).any()
    # ... and the two sums of the first input give two different inv_rms: what every element of y is multiplied with
    assert (R.inv_rms(ker, K, 0.0) != R.inv_rms(seq, K, 0.0)).all()
    # a sum one fp32 step apart is visible in y: some element of a long row sits close enough to a rounding boundary
    wb = R.f32_to_bf16_bits((1 + 0.2 * rng.standard_normal(32768)).astype(np.float32))
    assert (R.rmsnorm_bf16(xb, wb, 1e-6, "kernel") != R.rmsnorm_bf16(xb, wb, 1e-6, "lane_major")).any()


def test_the_helper_refuses_what_it_cannot_restate():
    with pytest.raises(AssertionError):
        R.sum_squares(R.f32_to_bf16_bits(np.full((1, 8), 2.0 ** 70, dtype=np.float32)))       # a square beyond the exact range
    with pytest.raises(AssertionError):
        R.sum_squares(np.zeros((1, 12), dtype=np.uint16))                                      # K % 8
    with pytest.raises(AssertionError):
        R.sum_squares(np.zeros((1, 32776), dtype=np.uint16))                                   # more than 16 chunks per thread
    assert R.sum_squares(np.zeros((2, 128), dtype=np.uint16)).tolist() == [0.0, 0.0]
