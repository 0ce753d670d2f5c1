"""The arithmetic contract of mixq_rmsnorm_bf16 (mixq_amd/csrc/norm.hip, include/mixq_hip.h "bf16 RMSNorm") restated in numpy float32, bit
for bit.  oracle/ has no bfloat16, so this file is the expectation of tests/test_gpu_bf16_norm.py; tests/test_bf16_norm_ref_host.py
checks it against float64 where every operation is exact, and shows that another summation order gives other bits.

    ss   thread t of 256 takes the row's 16-byte chunks (8 elements) t, t + 256, ... element by element, ss = fmaf(v, v, ss) in fp32;
         64-lane butterfly (xor 32, 16, 8, 4, 2, 1) inside each of the four waves; (w0 + w1) + (w2 + w3)
    inv  = 1 / sqrtf(ss / K + eps)                       IEEE fp32 divide and sqrt
    y    = RNE_bf16( fp32( fp32(x * inv) * w ) )

bfloat16 travels as uint16 bit patterns (numpy has no bfloat16).  A bf16 value has an 8-bit significand, so its square is exact in fp32
while it stays a normal fp32 number: `v * v + ss` in float32 then rounds once, exactly as the fma does.  The helper refuses rows outside
that range (nonzero |x| below 2^-63 or above 2^63) instead of restating them wrongly."""
import numpy as np

NT = 256                      # threads per row
ORDERS = ("kernel", "sequential", "lane_major")


def bf16_bits_to_f32(bits):
    """uint16 bfloat16 patterns -> float32 (a shift: every bf16 is an fp32)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(f):
    """Round-to-nearest-even of finite float32 values to bfloat16, by bit operations: add 0x7fff plus the lowest kept bit, cut 16 bits."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    assert np.isfinite(f).all(), "finite values only"
    u = f.view(np.uint32).astype(np.uint64)
    u = u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))
    return (u >> np.uint64(16)).astype(np.uint16)


def f32_to_bf16_bits_from_f64(v):
    """Bits of the bfloat16 nearest (ties to even) to float64 values that are exactly representable in float32."""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    assert (f.astype(np.float64) == np.asarray(v, dtype=np.float64)).all()
    return f32_to_bf16_bits(f)


def _check_range(x):
    a = np.abs(x[x != 0])
    assert a.size == 0 or (a.min() >= 2.0 ** -63 and a.max() <= 2.0 ** 63), "a bf16 square must be an exact, normal fp32 number"


def sum_squares(xbits, order="kernel"):
    """float32 [M]: the row sums of squares in the kernel's order.  `order` = "sequential" (one left-to-right chain) and "lane_major" (each
    thread owns CONSECUTIVE chunks instead of strided ones) are deliberately wrong orders, for the test that shows the order matters."""
    assert order in ORDERS
    x = bf16_bits_to_f32(xbits)
    M, K = x.shape
    assert K % 8 == 0 and K // 8 <= 16 * NT
    _check_range(x)
    if order == "sequential":
        ss = np.zeros(M, dtype=np.float32)
        for k in range(K):
            ss = x[:, k] * x[:, k] + ss
        return ss
    nchunk = K // 8
    nch = -(-nchunk // NT)
    pad = np.zeros((M, nch * NT * 8), dtype=np.float32)          # (a chunk that is not there adds nothing: the kernel skips it, + 0 is exact)
    pad[:, :K] = x
    if order == "kernel":
        v = pad.reshape(M, nch, NT, 8)                           # chunk c = i * 256 + t
        parts = [v[:, i, :, e] for i in range(nch) for e in range(8)]
    else:
        v = pad.reshape(M, NT, nch, 8)                           # chunk c = t * nch + i
        parts = [v[:, :, i, e] for i in range(nch) for e in range(8)]
    ss = np.zeros((M, NT), dtype=np.float32)
    for p in parts:
        ss = p * p + ss                                          # exact square, one rounding: fmaf(v, v, ss)
    lanes = np.arange(64)
    w = ss.reshape(M, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lanes ^ o]
    w = w[:, :, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def inv_rms(ss, K, eps):
    ss = np.asarray(ss, dtype=np.float32)
    return (np.float32(1.0) / np.sqrt(ss / np.float32(K) + np.float32(eps))).astype(np.float32)


def rmsnorm_bf16(xbits, wbits, eps, order="kernel"):
    """uint16 [M, K]: the bfloat16 patterns mixq_rmsnorm_bf16 writes for x (uint16 [M, K]) and weight (uint16 [K])."""
    x, w = bf16_bits_to_f32(xbits), bf16_bits_to_f32(wbits)
    inv = inv_rms(sum_squares(xbits, order), x.shape[1], eps)
    assert np.isfinite(inv).all()
    t = (x * inv[:, None]).astype(np.float32)                    # first fp32 rounding
    t = (t * w[None, :]).astype(np.float32)                      # second fp32 rounding
    return f32_to_bf16_bits(t)
