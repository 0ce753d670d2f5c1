"""The arithmetic contract of mixq_gemm_w8a16_bf16 / mixq_gemm_w8a16_addend_bf16 (mixq_amd/csrc/gemm_w8a16.hip compiled as
gemm_w8a16_bf16.hip; include/mixq_hip.h, "bf16 weight-only layers") restated in float64.  oracle/ has no bfloat16 W8A16, so this file is
the expectation of tests/test_gpu_w8a16_bf16.py; tests/test_w8a16_bf16_host.py checks it on its own.

    z[m, n] = ( sum_k x[m, k] * q[k, n] ) * float(scale_col[n]) (+ float(addend[m, n])) (+ float(bias[n]))
    y[m, n] = RNE_bf16( z[m, n] )

x, addend and y are bfloat16 (uint16 bit patterns here: numpy has no bfloat16), scale_col and bias float16, q int8 - every weight enters the
contraction as the integer it is.  In float64 the sum is exact for any data a test here uses (|x q| < 2^140 is far from the range's end and
53 bits hold K <= 2^16 products of 8-bit by 8-bit significands that share an exponent window of 30 binades).

Where the operands are EXACT (tests/exact.py: every term a multiple of a quantum q[m, n], the sum of absolute terms below 2^22 quanta) the
kernel's only rounding is the last one and `expect_bits` is the answer bit for bit.  For free operands the fp32 accumulation order is the
kernel's own, and `bound` derives what a correct kernel may differ by: see there."""
import numpy as np

from exact import BF16, from_bits, to_bits


def bf16_values(bits):
    """uint16 bfloat16 patterns -> float64."""
    return from_bits(np.asarray(bits, dtype=np.uint16), BF16)


def z64(xbits, qkn, scale, addend_bits=None, bias=None):
    """The exact value in front of the rounding, float64 [M, N].  xbits uint16 [M, K] (bf16), qkn int8 [K, N], scale float16 [N],
    addend_bits uint16 [M, N] (bf16) or None, bias float16 [N] or None.  The addend first, then the bias (exact in float64 either way)."""
    x = bf16_values(xbits)
    qkn = np.asarray(qkn)
    assert qkn.dtype == np.int8 and np.asarray(scale).dtype == np.float16 and (bias is None or np.asarray(bias).dtype == np.float16)
    z = (x @ qkn.astype(np.float64)) * np.asarray(scale).astype(np.float64)[None, :]
    if addend_bits is not None:
        z = z + bf16_values(addend_bits)
    if bias is not None:
        z = z + np.asarray(bias).astype(np.float64)[None, :]
    return z


def expect_bits(z):
    """uint16 [M, N]: RNE_bf16 of an exact z (a value fp32 holds: exact.to_bits asserts it), overflow to inf included."""
    return to_bits(z, BF16)


def ulp_bf16(v):
    """The spacing of bfloat16 (8-bit significand) at |v|, float64; the subnormal spacing 2^-133 below 2^-126."""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(a)) - 7)


def bound(xbits, qkn, scale, addend_bits=None, bias=None):
    """float64 [M, N]: what |y - z| may reach for a kernel that keeps the contract on FREE operands.
    The products x q are exact in fp32 (8 + 8 significand bits); the MFMA sums K of them in fp32 in an order the contract leaves free, and
    the epilogue's multiply and at most two adds round once each: |v - z| <= e = (K + 2) 2^-24 S with S = sum_k |x q| scale + |addend| + |bias|
    (the standard first-order bound gamma_n ~ n u with u = 2^-24; K <= 2^12 here, so second-order terms are below 2^-12 of it and the factor
    1.001 covers them).  Then ONE rounding to bfloat16 of v: half a bf16 ulp at |z| + e.  Nothing here comes from what the kernel gives."""
    x = np.abs(bf16_values(xbits))
    K = x.shape[1]
    S = (x @ np.abs(np.asarray(qkn).astype(np.float64))) * np.asarray(scale).astype(np.float64)[None, :]
    if addend_bits is not None:
        S = S + np.abs(bf16_values(addend_bits))
    if bias is not None:
        S = S + np.abs(np.asarray(bias).astype(np.float64))[None, :]
    e = 1.001 * (K + 2) * 2.0 ** -24 * S
    return e + 0.5 * ulp_bf16(np.abs(z64(xbits, qkn, scale, addend_bits, bias)) + e)
