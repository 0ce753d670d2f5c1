"""Operands for which the fused GEMMs' epilogue is EXACT, float64 expectations, and the checkers that hold a kernel to them bit for bit.

The contract (include/mixq_hip.h): fp32 throughout, acc * sx * sw + sum_j xo * wo + addend -> act -> + bias, and ONE
round-to-nearest-even to the 16-bit container.  A tolerance of two ulp cannot tell that from a round-toward-zero conversion, a 16-bit
intermediate or a half-precision tail.  An exact problem can: every term is an integer multiple of a per-element quantum q[m, n] and

    |acc sx sw| + sum_j |xo wo| + |addend| + |bias| < 2^22 q[m, n]

so every partial sum of every summation order is an integer below 2^22 in units of q - exactly representable in fp32, whose significand
holds 2^24 (the two spare bits are headroom for the internal alignment of the 16-bit matrix instruction that runs the tail).  The
kernel's only rounding is then the last one, and the expected output is RNE_16 of the float64 sum: no tolerance.

    sx[m] = 2^-a_m, sw[n] = 2^-b_n (exponents drawn per row / per column), q[m, n] = 2^-(a_m + b_n)
    xo, wo, addend, bias: integers times powers of two, every tail product, addend and bias a multiple of the COARSEST q

Exact.check_conditions() asserts both conditions on the data, term by term, in float64.  Host only (numpy / torch CPU), like frames.py;
tests/test_exact_host.py shows that the oracle equals these expectations bit for bit and that the checkers reject four wrong kernels.

SiLU is not exact: silu_reference() is the float64 value and a bound DERIVED from the instructions mixq_silu issues (common.h:
v * rcp(1 + exp2(-v * log2e)), v_exp_f32 and v_rcp_f32 are 1-ulp instructions), see there."""
import numpy as np
import torch

F16, BF16 = "f16", "bf16"
LIMIT = 2.0 ** 22                        # the second condition, in units of q[m, n]


# ---- 16-bit containers ----------------------------------------------------------------------------------------------------------------
def to_bits(v, dtype):
    """RNE of a float64 / float32 array to the container -> its uint16 bit patterns.  fp16: numpy's correctly rounded float64 -> float16;
    bf16: through float32 (callers pass values that fp32 holds exactly), then torch's RNE."""
    v = np.asarray(v)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(v.astype(np.float16)).view(np.uint16)
    f32 = v.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), v.astype(np.float64)), "bf16 expectation: the exact value does not fit fp32"
    return torch.from_numpy(np.ascontiguousarray(f32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


def from_bits(b, dtype):
    """uint16 bit patterns -> float64 values."""
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if dtype == F16:
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def representable(v, dtype):
    v = np.asarray(v, dtype=np.float64)
    return bool(np.array_equal(from_bits(to_bits(v, dtype), dtype), v))


def torch_dtype(dtype):
    return torch.float16 if dtype == F16 else torch.bfloat16


def as_tensor(v, dtype):
    """A float array whose values the container holds exactly -> a CPU tensor in the container."""
    assert representable(v, dtype)
    return torch.from_numpy(to_bits(v, dtype).view(np.int16).copy()).view(torch_dtype(dtype))


def all_finite_patterns(dtype):
    """Every finite bit pattern of the container once: 63 488 for fp16 (= 248 x 256), 65 280 for bf16 (= 255 x 256)."""
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    exp_all_ones = (b & 0x7C00) == 0x7C00 if dtype == F16 else (b & 0x7F80) == 0x7F80
    return b[~exp_all_ones]


def ulp16(v, dtype):
    """Spacing of the container at |v| (float64 in, float64 out), subnormal spacing below the smallest normal; above the largest finite
    value the spacing the format would have with one more exponent (what IEEE overflow rounds in)."""
    emin, p = (-14, 10) if dtype == F16 else (-126, 7)
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return np.exp2(np.maximum(e, emin) - p)


def pack_i4(q):
    """int values in [-8, 7], [R, K] -> nibble-packed uint8 [R, K / 2], low nibble = even column (include/mixq_hip.h)."""
    u = (np.asarray(q, dtype=np.int16) & 0xF).astype(np.uint8)
    return np.ascontiguousarray(u[:, 0::2] | (u[:, 1::2] << 4))


# ---- exact problems -------------------------------------------------------------------------------------------------------------------
class Exact:
    """One problem.  qx [M,K] / qw [N,K]: the LOGICAL integers (int8; within [-8, 7] for bit 4).  sx [M], sw [N], bias [N]: float16.
    xo [M,n_cap], wo [N,n_cap], addend [M,N]: float64 values the 16-bit container `dtype` holds exactly.  q [M,N]: the quantum.  acc: the
    exact contraction (int64).  main_exact = False: |acc| exceeds 2^24 and float(acc_i32) - one RNE to fp32, part of the contract - comes
    first (the long-K problem; no other term then)."""

    def __init__(self, bit, dtype, qx, qw, sx, sw, xo, wo, addend, bias, q, name, main_exact=True):
        self.bit, self.dtype, self.name, self.main_exact = bit, dtype, name, main_exact
        self.qx, self.qw = np.ascontiguousarray(qx, dtype=np.int8), np.ascontiguousarray(qw, dtype=np.int8)
        self.M, self.K, self.N = qx.shape[0], qx.shape[1], qw.shape[0]
        self.sx, self.sw, self.bias = (np.ascontiguousarray(v, dtype=np.float16) for v in (sx, sw, bias))
        self.xo, self.wo, self.addend, self.q = (np.ascontiguousarray(v, dtype=np.float64) for v in (xo, wo, addend, q))
        self.n_cap = self.xo.shape[1]
        self.acc = self.qx.astype(np.int64) @ self.qw.astype(np.int64).T
        assert np.abs(self.acc).max() < 2 ** 31
        lim = 7 if bit == 4 else 127
        assert np.abs(self.qx.astype(np.int16)).max() <= lim and self.qw.min() >= -lim - 1 and self.qw.max() <= lim
        for nm, v in (("xo", self.xo), ("wo", self.wo), ("addend", self.addend)):
            assert representable(v, dtype), f"{name}: {nm} does not fit {dtype}"

    # -- the terms, float64 --
    def main(self):
        a = self.acc.astype(np.float64) if self.main_exact else self.acc.astype(np.float32).astype(np.float64)
        return a * self.sx.astype(np.float64)[:, None] * self.sw.astype(np.float64)[None, :]

    def tail(self, n_out):
        return self.xo[:, :n_out] @ self.wo[:, :n_out].T if n_out else np.zeros((self.M, self.N))

    def tail_abs(self, n_out):
        return np.abs(self.xo[:, :n_out]) @ np.abs(self.wo[:, :n_out]).T if n_out else np.zeros((self.M, self.N))

    def addend_values(self, addend):
        """addend: None / False, True (the [M, N] matrix) or "bcast" (row 0 for every row: lda = 0)."""
        if not addend:
            return np.zeros((self.M, self.N))
        return np.broadcast_to(self.addend[:1], (self.M, self.N)) if addend == "bcast" else self.addend

    def z(self, n_out=0, addend=None, bias=False, main=True):
        z = self.main() if main else np.zeros((self.M, self.N))
        return z + self.tail(n_out) + self.addend_values(addend) + (self.bias.astype(np.float64)[None, :] if bias else 0.0)

    def expected(self, n_out=0, addend=None, bias=False, main=True):
        """(bit patterns of RNE_16(z), z)."""
        z = self.z(n_out, addend, bias, main)
        return to_bits(z, self.dtype), z

    def check_conditions(self, n_out=None, addend=True, bias=True, bcast=False):
        """The generator's own conditions on the data it made, for the LARGEST combination a test launches (fewer outlier columns, no
        addend, no bias: a subset of the same terms; bcast: the lda = 0 form, row 0 of the addend under every row, is launched too).
        (1) every term - each single tail product, not only their sum - is an integer multiple of q[m, n]; (2) the absolute terms sum
        below 2^22 q[m, n].  Returns the largest sum, in units of q."""
        n_out = self.n_cap if n_out is None else n_out
        q = self.q
        if not self.main_exact:
            assert n_out == 0 and not addend and not bias, "float(acc_i32) rounds: the long-K problem has no other term"
            return None

        def multiple(v):
            r = np.broadcast_to(v, q.shape) / q
            return bool(np.array_equal(r, np.rint(r)))

        live = (self.sx != 0)[:, None]                                          # (a zero-scale row keeps the q of its nominal exponent)
        assert np.array_equal(np.outer(self.sx.astype(np.float64), self.sw.astype(np.float64)) * live, q * live), f"{self.name}: q is not sx sw"
        assert multiple(self.main()), f"{self.name}: main term off the grid"
        for j in range(n_out):
            assert multiple(np.outer(self.xo[:, j], self.wo[:, j])), f"{self.name}: tail product {j} off the grid"
        total = np.abs(self.main()) + self.tail_abs(n_out)
        if addend:
            kinds = (True, "bcast") if bcast else (True,)
            assert all(multiple(self.addend_values(k)) for k in kinds), f"{self.name}: addend off the grid"
            total = total + np.max([np.abs(self.addend_values(k)) for k in kinds], axis=0)
        if bias:
            b = self.bias.astype(np.float64)[None, :]
            assert multiple(b), f"{self.name}: bias off the grid"
            total = total + np.abs(b)
        worst = float((total / q).max())
        assert worst < LIMIT, f"{self.name}: sum of absolute terms reaches {worst:.4g} q (limit 2^22)"
        return worst

    # -- operands as the entry points take them (host tensors) --
    def q_plain(self):
        """(q_x, q_w) plain row-major: int8 [R, K], or nibble-packed uint8 [R, K / 2]."""
        if self.bit == 8:
            return torch.from_numpy(self.qx.copy()), torch.from_numpy(self.qw.copy())
        return torch.from_numpy(pack_i4(self.qx)), torch.from_numpy(pack_i4(self.qw))


def _fit(k, dtype):
    """Integers -> the nearest-toward-zero integers with at most 11 (fp16) / 8 (bf16) significant bits."""
    bits = 11 if dtype == F16 else 8
    k = np.asarray(k, dtype=np.int64)
    s = np.maximum(0, np.floor(np.log2(np.maximum(np.abs(k), 1))).astype(np.int64) + 1 - bits)
    return np.sign(k) * ((np.abs(k) >> s) << s)


def exact_problem(bit, M, K, N, n_out, a_range=(3, 5), b_range=(6, 8), xo_exp=4, xo_max=64, wo_exp=None, wo_max=32, add_exp=None, add_max=2000,
                  bias_exp=None, bias_max=2000, q_max=None, zero_rows=(), dtype=F16, seed=0, name=None):
    """The generator of the module docstring.  Exponents are of 1/2: xo = i 2^-xo_exp (|i| <= xo_max), wo = j 2^-wo_exp (|j| <= wo_max; default
    a_min + b_min - xo_exp, so that a tail product is a multiple of the coarsest q), addend = k 2^-add_exp and bias = k 2^-bias_exp (default
    a_min + b_min).  q_max bounds |q_x|, |q_w| (default: the full range of `bit`).  zero_rows: q_x = 0 and sx = 0 (an all-zero activation
    row) while the tail, the addend and the bias stay live."""
    rng = np.random.default_rng(seed)
    a_lo, a_hi = a_range
    b_lo, b_hi = b_range
    coarse = a_lo + b_lo
    wo_exp = coarse - xo_exp if wo_exp is None else wo_exp
    add_exp = coarse if add_exp is None else add_exp
    bias_exp = coarse if bias_exp is None else bias_exp
    assert xo_exp + wo_exp <= coarse and add_exp <= coarse and bias_exp <= coarse, "a tail product, addend or bias would not be a multiple of the coarsest q"
    full = 127 if bit == 8 else 7
    q_max = full if q_max is None else q_max
    qx = rng.integers(-q_max, q_max + 1, (M, K)).astype(np.int8)
    qw = rng.integers(-min(q_max, full) - (1 if q_max == full else 0), q_max + 1, (N, K)).astype(np.int8)
    a = rng.integers(a_lo, a_hi + 1, M)
    b = rng.integers(b_lo, b_hi + 1, N)
    a[: min(M, a_hi - a_lo + 1)] = np.arange(a_lo, a_hi + 1)[:M]            # both ends of either range occur whatever the seed
    b[: min(N, b_hi - b_lo + 1)] = np.arange(b_lo, b_hi + 1)[:N]
    sx = np.exp2(-a.astype(np.float64))
    sw = np.exp2(-b.astype(np.float64))
    q = np.outer(sx, sw)
    for r in zero_rows:
        qx[r] = 0
        sx[r] = 0.0
    assert np.array_equal(sx.astype(np.float16).astype(np.float64), sx) and np.array_equal(sw.astype(np.float16).astype(np.float64), sw), "a scale does not fit fp16"
    xo = rng.integers(-xo_max, xo_max + 1, (M, n_out)) * 2.0 ** -xo_exp
    wo = rng.integers(-wo_max, wo_max + 1, (N, n_out)) * 2.0 ** -wo_exp
    addend = _fit(rng.integers(-add_max, add_max + 1, (M, N)), dtype) * 2.0 ** -add_exp
    bias = _fit(rng.integers(-bias_max, bias_max + 1, N), F16) * 2.0 ** -bias_exp
    assert representable(bias, F16), "bias does not fit fp16"
    return Exact(bit, dtype, qx, qw, sx, sw, xo, wo, addend, bias, q, name or f"exact W{bit} {dtype} {M}x{K}->{N}")


# ---- the range-edge problems (same generator, same conditions) ---------------------------------------------------------------------------
def tiny_problem(bit, M, K, N, n_out, seed=1):
    """Subnormal fp16 scale_col (2^-20 .. 2^-24), subnormal tail weights (j 2^-16), two all-zero rows with a live tail and bias.  q = 2^-30 ..
    2^-36: most outputs are fp16 subnormals, some underflow to +-0.  bias and addend are fp16 subnormals themselves (k 2^-24)."""
    qm = None if bit == 8 else 7
    return exact_problem(bit, M, K, N, n_out, a_range=(10, 12), b_range=(20, 24), xo_exp=14, xo_max=64, wo_exp=16, wo_max=32, add_exp=24, add_max=150,
                         bias_exp=24, bias_max=150, q_max=qm, zero_rows=(3, M - 2), dtype=F16, seed=seed, name=f"tiny W{bit} {M}x{K}->{N}")


def tinier_problem(bit, M, K, N, n_out, seed=2):
    """q = 2^-34 .. 2^-38 and small operands: a good share of the outputs lies below half the smallest fp16 subnormal and flushes to zero,
    hundreds of them to -0 (the sign of an underflowed nonzero z must match)."""
    return exact_problem(bit, M, K, N, n_out, a_range=(12, 14), b_range=(22, 24), xo_exp=18, xo_max=16, wo_exp=16, wo_max=16, add_exp=24, add_max=2,
                         bias_exp=24, bias_max=2, q_max=40 if bit == 8 else 7, dtype=F16, seed=seed, name=f"tinier W{bit} {M}x{K}->{N}")


def overflow_problem(bit, M, K, N, n_out, seed=3):
    """Scales around 1 (2^0 .. 2^-2), K = 512: a share of the fp16 outputs is +-inf (IEEE RNE: |z| >= 65520 -> inf).  Two planted elements
    of the main-only launch pin the threshold itself: z = 65504 exactly (the largest finite value) at [0, 0] and z = 65520 (the tie that
    rounds to inf) at [0, 1]."""
    if bit == 8:
        p = exact_problem(bit, M, K, N, n_out, a_range=(0, 2), b_range=(0, 2), xo_exp=0, xo_max=64, wo_exp=0, wo_max=32, add_exp=0, add_max=2000, bias_exp=0,
                          bias_max=2000, dtype=F16, seed=seed, name=f"overflow W{bit} {M}x{K}->{N}")
        assert p.sx[0] == 1 and p.sw[0] == 1 and p.sw[1] == 0.5
        # row 0: 65504 = 4 x 127 x 127 + 76 x 13 at q = 1;  2 x 65520 = 131040 = 8 x 127 x 127 + 124 x 16 + 24 x 1 at q = 1/2
        p.qx[0] = 0
        p.qx[0, :11] = [127] * 8 + [76, 124, 24]
        p.qw[0, :11] = [127] * 4 + [0] * 4 + [13, 0, 0]
        p.qw[1, :11] = [127] * 8 + [0, 16, 1]
    else:                                # int4 operands reach 7 x 8 x 512 only: scales of 4 .. 16 (q = 16 .. 256) bring the same share of +-inf
        p = exact_problem(bit, M, K, N, n_out, a_range=(-4, -2), b_range=(-4, -2), xo_exp=-4, xo_max=16, wo_exp=-4, wo_max=8, add_exp=-8, add_max=100,
                          bias_exp=-8, bias_max=100, dtype=F16, seed=seed, name=f"overflow W{bit} {M}x{K}->{N}")
        p.sw[3] = p.sw[2]
        p.q[:, 3] = p.q[:, 2]
        assert p.sx[2] == 4 and p.sw[2] == 4 and p.sw[3] == 4
        # row 2 at q = 16: 65504 = 16 x 4094 = 16 x (73 x 56 + 6);  65520 = 16 x 4095 = 16 x (73 x 56 + 7)
        p.qx[2] = 0
        p.qx[2, :75] = [-7] * 73 + [6, 7]
        p.qw[2, :75] = [-8] * 73 + [1, 0]
        p.qw[3, :75] = [-8] * 73 + [0, 1]
    return Exact(p.bit, p.dtype, p.qx, p.qw, p.sx, p.sw, p.xo, p.wo, p.addend, p.bias, p.q, p.name)


def long_k_problem(M, N, K=2048, seed=4):
    """int8, K = 2048, operands mostly +-127 / -128 with correlated signs: |acc| > 2^24, where float(acc_i32) rounds (RNE) before the scales.
    Expected: RNE_16(RNE_32(acc) * q).  Main term only."""
    rng = np.random.default_rng(seed)
    s = rng.choice([-1, 1], K)
    fx = np.where(rng.random((M, K)) < 0.04, -1, 1) * rng.choice([-1, 1], (M, 1))
    fw = np.where(rng.random((N, K)) < 0.04, -1, 1) * rng.choice([-1, 1], (N, 1))
    qx = (127 * s[None, :] * fx).astype(np.int8)
    sgn = s[None, :] * fw
    qw = np.where(sgn > 0, 127, -128).astype(np.int8)
    odd = rng.random((M, K)) < 0.02                                          # a few smaller operands: odd low bits in acc
    qx[odd] = (qx[odd].astype(np.int16) // 2).astype(np.int8)
    a, b = rng.integers(6, 9, M), rng.integers(6, 9, N)
    sx, sw = np.exp2(-a.astype(np.float64)), np.exp2(-b.astype(np.float64))
    p = Exact(8, F16, qx, qw, sx, sw, np.zeros((M, 0)), np.zeros((N, 0)), np.zeros((M, N)), np.zeros(N), np.outer(sx, sw), f"long K W8 {M}x{K}->{N}", main_exact=False)
    big = np.abs(p.acc) > 2 ** 24
    inexact = p.acc.astype(np.float32).astype(np.int64) != p.acc
    assert big.mean() > 0.9 and inexact.mean() > 0.25, (big.mean(), inexact.mean())
    return p


def int32_extremes(M, N, seed=5):
    """For mixq_dequant, which is handed the int32 values directly: +-(2^31 - 1), -2^31, 2^24 + 1, 2^30 + 2^6 (a tie of the fp32 rounding) and
    random values of every magnitude; scales 2^-10 x 2^-10 .. 2^-12 keep the results finite in fp16.  Returns (y32, sx, sw, q)."""
    rng = np.random.default_rng(seed)
    mag = rng.integers(0, 32, (M, N))
    y32 = (rng.integers(-2 ** 31, 2 ** 31, (M, N)) >> (31 - mag)).astype(np.int64)
    special = [2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 30 + 2 ** 6, 2 ** 30 + 3 * 2 ** 6, 2 ** 25 + 2, 2 ** 25 + 6, 0]
    y32.reshape(-1)[: len(special)] = special
    y32[-1, -len(special):] = special
    sx = np.full(M, 2.0 ** -10)
    sw = np.exp2(-rng.integers(10, 13, N).astype(np.float64))
    return y32.astype(np.int32), sx.astype(np.float16), sw.astype(np.float16), np.outer(sx, sw)


def wide_problem_bf16(bit, M, K, N, n_out, seed=6):
    """bf16 only: tail operands at 2^+-40, outputs spanning 2^-80 .. 2^80.  A row either carries the main term (its x_out is zero: the tail
    vanishes) or is an all-zero activation row (q_x = 0, sx = 0) whose output is tail + addend; q[m, n] = 2^(ex_m + ew_n) there and the
    addend is an integer multiple of it.  No bias (fp16 cannot follow the range).  Finite expected values only."""
    rng = np.random.default_rng(seed)
    base = exact_problem(bit, M, K, N, n_out, dtype=BF16, seed=seed)
    main_rows = np.arange(M) % 4 == 0
    ex = rng.integers(-40, 41, M)
    ew = rng.integers(-40, 41, N)
    ex[1], ex[2], ew[0], ew[1] = 40, -40, 40, -40                           # both corners occur: 2^80 and 2^-80
    xo = rng.integers(-64, 65, (M, n_out)) * np.exp2(ex.astype(np.float64))[:, None]
    wo = rng.integers(-32, 33, (N, n_out)) * np.exp2(ew.astype(np.float64))[:, None]
    qt = np.exp2(ex.astype(np.float64))[:, None] * np.exp2(ew.astype(np.float64))[None, :]
    addend = _fit(rng.integers(-2000, 2001, (M, N)), BF16) * qt
    qx, sx, q = base.qx.copy(), base.sx.astype(np.float64), base.q.copy()
    xo[main_rows] = 0
    addend[main_rows] = base.addend[main_rows]
    qx[~main_rows] = 0
    sx[~main_rows] = 0
    q[~main_rows] = qt[~main_rows]
    p = Exact(bit, BF16, qx, base.qw, sx, base.sw, xo, wo, addend, np.zeros(N), q, f"bf16 wide W{bit} {M}x{K}->{N}")
    return p


def w8a16_problem(M, K, N, seed=7):
    """Weight-only W8A16 by the same construction: x = i 2^-6 (|i| <= 64), full-range int8 weights [K, N], scale_col = 2^-b (b in 6 .. 8), bias
    on the coarsest quantum 2^-12.  q[m, n] = 2^-(6 + b_n).  The kernel multiplies offset-binary weights (q + 128, in 0 .. 255) and takes
    128 sum_k x back out, so the condition is put on sum_k |x| 255 scale + |bias| < 2^22 q.  Returns (x, qkn, scale, bias, z, q)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-64, 65, (M, K)) * 2.0 ** -6
    qkn = rng.integers(-128, 128, (K, N)).astype(np.int8)
    b = rng.integers(6, 9, N)
    b[:3] = [6, 7, 8]
    scale = np.exp2(-b.astype(np.float64))
    bias = _fit(rng.integers(-2000, 2001, N), F16) * 2.0 ** -12
    q = 2.0 ** -6 * scale[None, :] * np.ones((M, 1))
    acc = x @ qkn.astype(np.float64)                                          # exact: integers times 2^-6 far below 2^53
    z = acc * scale[None, :] + bias[None, :]
    r = z / q
    assert np.array_equal(r, np.rint(r)) and np.array_equal((bias[None, :] / q), np.rint(bias[None, :] / q))
    worst = float(((np.abs(x).sum(axis=1)[:, None] * 255.0 * scale[None, :] + np.abs(bias)[None, :]) / q).max())
    assert worst < LIMIT, worst
    assert representable(x, F16) and representable(scale, F16) and representable(bias, F16)
    return x.astype(np.float16), qkn, scale.astype(np.float16), bias.astype(np.float16), z, q


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def mismatches(y_bits, want_bits, z):
    """Boolean [M, N]: where y differs from the expectation bit for bit.  The one exception: where the exact z == 0 either zero sign passes
    (the sign of an exactly cancelling sum depends on the tail's summation order, which the contract leaves free).  A -0 that comes from
    the underflow of a nonzero z must match."""
    y_bits, want_bits = np.asarray(y_bits, dtype=np.uint16), np.asarray(want_bits, dtype=np.uint16)
    assert y_bits.shape == want_bits.shape == z.shape, (y_bits.shape, want_bits.shape, z.shape)
    return (y_bits != want_bits) & ~((z == 0) & ((y_bits & 0x7FFF) == 0))


def assert_exact(y_bits, want_bits, z, dtype, what):
    bad = mismatches(y_bits, want_bits, z)
    if bad.any():
        m, n = np.argwhere(bad)[0]
        got, want = from_bits(y_bits[m, n:n + 1], dtype)[0], from_bits(want_bits[m, n:n + 1], dtype)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ from RNE_16(z); first at [{m},{n}]: y {got!r} (0x{int(y_bits[m, n]):04x}) "
                             f"expected {want!r} (0x{int(want_bits[m, n]):04x}) exact z {z[m, n]!r}")


def shares(want_bits, z, dtype):
    """What an expectation exercises: the shares of elements that round away from zero, that are exact ties, that become +-inf, that are
    subnormal in the container, that flush to zero from a nonzero z, and the number of -0 among those."""
    v = from_bits(want_bits, dtype)
    fin = np.isfinite(v)
    u = ulp16(z, dtype)
    emin = -14 if dtype == F16 else -126
    with np.errstate(invalid="ignore"):
        away = fin & (np.abs(v) > np.abs(z))
        r = np.abs(z) / u
        tie = fin & (r - np.floor(r) == 0.5)
    flushed = (v == 0) & (z != 0)
    return dict(away=float(away.mean()), tie=float(tie.mean()), inf=float((~fin).mean()), subnormal=float(((np.abs(v) < 2.0 ** emin) & (v != 0)).mean()),
                flushed=float(flushed.mean()), neg_zero=int((flushed & (want_bits == 0x8000)).sum()), has_max=bool((np.abs(v) == (65504.0 if dtype == F16 else 0)).any()))


# ---- SiLU: the float64 value and a derived bound ------------------------------------------------------------------------------------------
RCP_FLUSH_FLOOR = 88.73 * 2.0 ** -126     # see silu_reference


def silu64(z):
    with np.errstate(over="ignore"):
        return z / (1.0 + np.exp(-z))


def silu_reference(z64, bias=None, mul=None, dtype=F16):
    """(ref, bound) for y = RNE_16(silu(z) + bias) and, with `mul`, y = RNE_16((silu(z) + bias) * mul); z, bias, mul float64 arrays that
    broadcast (bias / mul None: absent).

    mixq_silu (common.h) is v * v_rcp_f32(1 + v_exp_f32(-v * log2e)).  Error sources, relative to silu(v), in units of 2^-24 (half an fp32 ulp
    at most):
      - the rounded constant log2e and the rounded product -v * log2e each move the exponent by |v log2e| 2^-24, i.e. the exponential by
        |v| 2^-24 relative; d sigmoid / sigmoid = -(e / (1 + e)) de / e, at most as much: 2 |v|
      - v_exp_f32, a 1-ulp instruction: 2;  the addition 1 + e: 1;  v_rcp_f32, 1 ulp: 2;  the product v * r: 1;  spare: 2  -> 8
    so delta(v) = (2 |v| + 8) 2^-24.  The bias addition rounds once more: 2^-24 (|silu| + |bias|), and the container's RNE adds half an ulp OF
    THE RESULT:
        bound = ulp_16(ref) / 2 + delta(z) |silu(z)| + 2^-24 (|silu(z)| + |bias|)
    With a multiplier the fp32 error before the product scales with |mul|, the product rounds once (2^-24 |ref|) and the half ulp is that
    of the final value:
        bound = ulp_16(ref) / 2 + |mul| (delta(z) |silu(z)| + 2^-24 (|silu(z)| + |bias|)) + 2^-24 |ref|
    bf16 adds an absolute floor to the fp32 error (before the multiplier): v_rcp_f32 returns no subnormals - a result below 2^-126 is flushed
    to zero, as the compiler's own division lowering assumes of this instruction - so from 1 + e^-v > 2^126 (v < -87.34) on, and past
    v = -88.73, where the exponential itself overflows, the kernel returns -0 where |silu(v)| = |v| r < 88.73 x 2^-126 = 2^-119.5.  (An
    earlier form of this floor, 2^-120, counted the overflow alone; the MI355X showed the flush at v = -87.5, the one bf16 argument between
    the two thresholds whose silu exceeds 2^-120.)  fp16 arguments end at -65504 and half an fp16 ulp, 2^-25, covers the same window."""
    z = np.asarray(z64, dtype=np.float64)
    s = silu64(z)
    b = 0.0 if bias is None else np.asarray(bias, dtype=np.float64)
    inner = s + b
    pre = (2.0 * np.abs(z) + 8.0) * 2.0 ** -24 * np.abs(s) + 2.0 ** -24 * (np.abs(s) + np.abs(b))
    if dtype == BF16:
        pre = pre + RCP_FLUSH_FLOOR
    if mul is None:
        ref = inner
        bound = 0.5 * ulp16(ref, dtype) + pre
    else:
        mu = np.asarray(mul, dtype=np.float64)
        ref = inner * mu
        bound = 0.5 * ulp16(ref, dtype) + np.abs(mu) * pre + 2.0 ** -24 * np.abs(ref)
    return ref, bound


def decode_for_bound(y_bits, dtype):
    """The container's values as float64 with +-inf read as the value overflow rounded FROM: +-2^16 (fp16) / +-2^128 (bf16), the next power of
    two - IEEE overflow is RNE with one more exponent followed by the replacement of everything >= max + ulp / 2 by inf.  NaN stays NaN
    (and fails every comparison)."""
    v = from_bits(y_bits, dtype)
    top = 2.0 ** 16 if dtype == F16 else 2.0 ** 128
    return np.where(np.isinf(v), np.sign(v) * top, v)


def silu_check(y_bits, ref, bound, dtype, what):
    """Every element within its bound; returns the worst err / bound."""
    y = decode_for_bound(y_bits, dtype)
    ref, bound = np.broadcast_to(ref, y.shape), np.broadcast_to(bound, y.shape)
    err = np.abs(y - ref)
    bad = ~(err <= bound)                                                       # (NaN fails)
    if bad.any():
        i = np.argwhere(bad)
        worst = i[np.argmax(np.where(np.isnan(err[bad]), np.inf, err[bad] / bound[bad]))]
        m, n = worst
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived SiLU bound; worst at [{m},{n}]: y {y[m, n]!r} ref {ref[m, n]!r} "
                             f"|err| {err[m, n]:.6g} bound {bound[m, n]:.6g}")
    return float((err / bound).max())


def silu_mul_operands(dtype, seed=8):
    """z through ONE outlier column: xo[m, 0] = +-(1 + k / 128) (124 significands x both signs = 248 rows; seven fraction bits: exact in fp16 and
    bf16), wo[n, 0] = 2^p, p = -24 .. 7 cycling along 256 columns; z[m, n] = xo wo is exact in fp32.  The multiplier: random container
    values in +-[0.5, 2).  Returns (xo [248], wo [256], z [248, 256], mul [248, 256]) as float64."""
    rng = np.random.default_rng(seed)
    sig = 1.0 + np.arange(124) / 128.0
    xo = np.concatenate([sig, -sig])
    wo = np.exp2((np.arange(256) % 32 - 24).astype(np.float64))
    frac_bits = 10 if dtype == F16 else 7
    mant = 1.0 + rng.integers(0, 2 ** frac_bits, (248, 256)) / 2.0 ** frac_bits
    mul = mant * np.exp2(rng.integers(-1, 1, (248, 256)).astype(np.float64)) * rng.choice([-1.0, 1.0], (248, 256))
    assert representable(xo, dtype) and representable(wo, dtype) and representable(mul, dtype) and np.abs(mul).min() >= 0.5 and np.abs(mul).max() < 2
    return xo, wo, np.outer(xo, wo), mul


def silu_bias_vector(N=256):
    """A fixed fp16 bias of mixed signs and magnitudes 2^-10 .. 2^6."""
    n = np.arange(N)
    b = np.exp2((n % 17 - 10).astype(np.float64)) * (1.0 + (n % 5) / 8.0) * np.where(n % 3 == 0, -1.0, 1.0)
    assert representable(b, F16)
    return b


# ---- the configurations the GPU module launches (tests/test_exact_host.py holds every one to its conditions) --------------------------------
N_OUTS = (0, 1, 16, 17, 32, 33, 41, 129)     # the 16-column pad, the 32-column tail k-step that tail_mode skips, more than 128 columns
M_SHAPES = (72, 24)                          # a partial 128-row tile, 64-row tile and 16-row block; the small batch of decode32 and 32 x 64
N_SHAPES = (136, 140)                        # N % 8 == 0 (staged stores) with a partial N tile for every tiling; N % 8 == 4 (8-byte stores)
K_MAIN = 128
EDGE_N_OUT = 17
EDGES_F16 = ("tiny", "tinier", "overflow", "long_k")
_cache = {}


def problem(kind, bit, dtype, M, N):
    """One shared, never modified instance per configuration."""
    key = (kind, bit, dtype, M, N)
    if key not in _cache:
        if kind == "main":
            # (bf16 keeps 8 significand bits: smaller int8 operands keep the quantum within reach of its ulp, so that ties and inexact sums stay frequent)
            kw = dict(q_max=31, xo_max=16, wo_max=8, add_max=255, bias_max=255) if (dtype == BF16 and bit == 8) else {}
            p = exact_problem(bit, M, K_MAIN, N, max(N_OUTS), dtype=dtype, seed=100 * bit + M + N, **kw)
            p.check_conditions(bcast=True)
        elif kind == "tiny":
            p = tiny_problem(bit, M, K_MAIN, N, EDGE_N_OUT)
            p.check_conditions()
        elif kind == "tinier":
            p = tinier_problem(bit, M, K_MAIN, N, EDGE_N_OUT)
            p.check_conditions()
        elif kind == "overflow":
            p = overflow_problem(bit, M, 512, N, EDGE_N_OUT)
            p.check_conditions()
        elif kind == "long_k":
            assert bit == 8
            p = long_k_problem(M, N)
            p.check_conditions(0, False, False)
        elif kind == "wide":
            assert dtype == BF16
            p = wide_problem_bf16(bit, M, K_MAIN, N, EDGE_N_OUT)
            p.check_conditions(bias=False)
        else:
            raise KeyError(kind)
        _cache[key] = p
    return _cache[key]


def edge_combos(kind):
    """(n_out, addend, bias) of the launches an edge problem gets."""
    if kind == "long_k":
        return [(0, None, False)]
    if kind == "wide":
        return [(EDGE_N_OUT, None, False), (EDGE_N_OUT, True, False), (1, True, False)]
    return [(0, None, False), (EDGE_N_OUT, None, False), (EDGE_N_OUT, True, True), (EDGE_N_OUT, None, True)]
