"""The fused GEMMs' epilogue held to its contract BIT FOR BIT on operands for which every fp32 operation of the formula is exact
(tests/exact.py), at the edges of the 16-bit range, and - SiLU, which is not exact - over every finite argument against a bound derived
from the instructions' documented accuracy.  tests/test_exact_host.py shows on the CPU that the expectations are the oracle's bits and that
these comparisons reject a round-toward-zero conversion, a 16-bit tail, a 16-bit main term and a half-precision exponential.

  (a) MIXQ_ACT_NONE, every tiling of every family, outlier counts {0, 1, 16, 17, 32, 33, 41, 129} and 41 as a device-resident count below a
      NaN-poisoned capacity of 48, with and without addend, with and without bias, lda = 0 once per tiling: y == RNE_16(float64 z).
  (b) the range edges (subnormal scales and tail weights, zero rows, underflow to +-0, overflow to +-inf, |acc| > 2^24, bf16 at 2^+-80) through
      one tiling of each family and the automatic pick; int32 extremes through mixq_dequant.
  (c) W8A16 by the same construction, every configuration.
  (d) SiLU, SILU_MUL and the joint gate / up form over every finite fp16 / bf16 argument, every family that has SiLU.
Every element of every launch is compared; the only tolerance in (a) - (c) is the sign of a zero where the exact sum is zero."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact as E  # noqa: E402
from exact import BF16, F16  # noqa: E402
from mixq_amd import _capi, mixlib  # noqa: E402
from mixq_amd._capi import ACT_NONE, ACT_SILU, ACT_SILU_MUL, ACT_SILU_PAIR, FMT_F16X64, FMT_F6X128, FMT_P16X64, FMT_R6X128  # noqa: E402
from mixq_amd.fused import interleave_pair_rows  # noqa: E402
from test_gpu_bf16_gemm import BF16_FP6, BF16_INT8  # noqa: E402
from test_gpu_fp6 import F6_TILINGS  # noqa: E402
from test_gpu_parity import _skinny_id, _tiled_configs, _w8a16_real_configs, _wr_configs  # noqa: E402
from test_gpu_strides import PAIR_TILINGS  # noqa: E402

DEV = "cuda"
NAN_BITS = 0x7FC1                                          # a NaN in bf16 and in fp16: the pad columns of x_out / w_out
DEV_COUNT, DEV_CAP = 41, 48
SMALL_M = ("decode32", "wr32x64_s8_d6_l1")                 # the small-batch forms: M = 24 (decode32 takes M <= 32 only)
T0 = time.time()
WORST = {}                                                 # SiLU sweep: family -> worst err / bound


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    lib = _capi.load()
    lib.mixq_gemm_set_config(-1); lib.mixq_gemm_w8a16_set_config(-1)
    yield
    lib.mixq_gemm_set_config(-1); lib.mixq_gemm_w8a16_set_config(-1)
    for fam, w in sorted(WORST.items()):
        print(f"SiLU sweep, worst err / bound: {fam}: {w:.6f}")
    print(f"tests/test_gpu_exact.py: {time.time() - T0:.1f} s wall")


def forced(names_or_ids):
    """Iterate (id, name) over tilings, each forced through mixq_gemm_set_config while the body runs; automatic again afterwards."""
    lib, names = _capi.load(), _capi.gemm_config_names()
    try:
        for c in names_or_ids:
            cid = names.index(c) if isinstance(c, str) else c
            assert lib.mixq_gemm_set_config(cid) == 0
            yield cid, (names[cid] if cid >= 0 else "auto")
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0


def bits_of(y):
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def pad16(v):
    return (v + 15) // 16 * 16


def poisoned(vals, cap, dtype):
    """[rows, pad16(cap)] in the container: the live columns, NaN patterns in every column behind them."""
    t = torch.full((vals.shape[0], pad16(cap)), NAN_BITS, dtype=torch.int16).view(E.torch_dtype(dtype))
    if vals.shape[1]:
        t[:, :vals.shape[1]] = E.as_tensor(vals, dtype)
    return t.to(DEV)


def q_images(qx, qw, bit, fmt):
    """(q_x, q_w) on the device in the operand pair `fmt` names: 0 plain, 1 P16X64 both, 2 P16X64 activations + fragment-order weights, 6 the
    FP6 pair (4-bit)."""
    qx, qw = qx.to(DEV), qw.to(DEV)
    if fmt == 0:
        return qx, qw
    xf, wf = {1: (FMT_P16X64, FMT_P16X64), 2: (FMT_P16X64, FMT_F16X64), 6: (FMT_R6X128, FMT_F6X128)}[fmt]
    assert fmt != 6 or bit == 4
    return mixlib.PackOperand(qx, xf), mixlib.PackOperand(qw, wf)


class OnDevice:
    """An exact.Exact problem on the device: operand images per format, poisoned outlier operands per count, expectations per combination -
    each made once and left unchanged."""

    def __init__(self, p):
        self.p, self.td = p, E.torch_dtype(p.dtype)
        self._q, self._o, self._want = {}, {}, {}
        self.sx = torch.from_numpy(p.sx.copy()).reshape(-1, 1).to(DEV)
        self.sw = torch.from_numpy(p.sw.copy()).reshape(1, -1).to(DEV)
        self.bias = torch.from_numpy(p.bias.copy()).to(DEV)
        self.addend = E.as_tensor(p.addend, p.dtype).to(DEV)
        self.bcast = self.addend.as_strided((p.M, p.N), (0, 1))

    def q(self, fmt):
        if fmt not in self._q:
            self._q[fmt] = q_images(*self.p.q_plain(), self.p.bit, fmt)
        return self._q[fmt]

    def outliers(self, n_out, dev):
        key = (n_out, dev)
        if key not in self._o:
            if n_out == 0:
                self._o[key] = (None, None, 0, None)
            else:
                cap = DEV_CAP if dev else n_out
                xo, wo = poisoned(self.p.xo[:, :n_out], cap, self.p.dtype), poisoned(self.p.wo[:, :n_out], cap, self.p.dtype)
                self._o[key] = (xo, wo, cap, torch.tensor([n_out], dtype=torch.int32, device=DEV) if dev else None)
        return self._o[key]

    def want(self, n_out, addend, bias):
        key = (n_out, addend, bias)
        if key not in self._want:
            self._want[key] = self.p.expected(n_out, addend, bias)
        return self._want[key]

    def run(self, fmt, n_out, dev, addend, bias, what):
        p = self.p
        xo, wo, n_arg, n_dev = self.outliers(n_out, dev)
        qx, qw = self.q(fmt)
        a = None if not addend else (self.bcast if addend == "bcast" else self.addend)
        y = mixlib.FusedLinear(qx, qw, self.sx, self.sw, xo, wo, n_arg, self.bias if bias else None, p.M, p.N, p.K, bit=p.bit, act=ACT_NONE, n_out_dev=n_dev,
                               addend=a, dtype=self.td)
        want, z = self.want(n_out, addend, bias)
        E.assert_exact(bits_of(y), want, z, p.dtype, f"{p.name} {what} n_out={n_out} dev_count={dev} addend={addend} bias={bias}")


_dev = {}


def on_device(kind, bit, dtype, M, N):
    key = (kind, bit, dtype, M, N)
    if key not in _dev:
        _dev[key] = OnDevice(E.problem(kind, bit, dtype, M, N))
    return _dev[key]


# (n_out, device-resident count, addend, bias): 8 counts x addend on / off x bias on / off, 41 once more as a count in device memory below a
# poisoned capacity of 48, and lda = 0 (one addend row for every row)
COMBOS = [(n, False, a, b) for n in E.N_OUTS for a in (None, True) for b in (False, True)] + \
         [(DEV_COUNT, True, a, b) for a in (None, True) for b in (False, True)] + [(17, False, "bcast", True)]
assert len(COMBOS) == 37


def rows_for(name):
    return (24,) if name == "decode32" else ((72, 24) if name in SMALL_M else (72,))


def sweep_exact(bit, dtype, N, fmt, name):
    for M in rows_for(name):
        d = on_device("main", bit, dtype, M, N)
        for n_out, dev, addend, bias in COMBOS:
            d.run(fmt, n_out, dev, addend, bias, f"{name} fmt {fmt}")


# ---- (a) exact epilogue, MIXQ_ACT_NONE ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("N", E.N_SHAPES)
def test_exact_epilogue_every_lds_staged_tiling_plain_and_p16x64(N, bit):
    ran = 0
    for _, name in forced(_tiled_configs()):
        for fmt in (0, 1):
            sweep_exact(bit, F16, N, fmt, name)
            ran += 1
    assert ran == 2 * len(_tiled_configs()) >= 2


@pytest.mark.parametrize("N", E.N_SHAPES)
def test_exact_epilogue_every_weights_in_registers_tiling_int8(N):
    for _, name in forced(_wr_configs()):
        sweep_exact(8, F16, N, 2, name)


@pytest.mark.parametrize("N", E.N_SHAPES)
def test_exact_epilogue_every_weights_in_registers_tiling_int4_nibbles_and_fp6(N):
    names = _capi.gemm_config_names()
    for _, name in forced([c for c in _wr_configs() if "128x256" not in names[c]]):      # (128 x 256 has no nibble form)
        sweep_exact(4, F16, N, 2, name)
    for _, name in forced(F6_TILINGS):
        sweep_exact(4, F16, N, 6, name)


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("N", E.N_SHAPES)
def test_exact_epilogue_decode32_and_the_automatic_pick(N, bit):
    for _, name in forced([_skinny_id()]):
        for fmt in (1, 2):
            sweep_exact(bit, F16, N, fmt, name)
    for _ in forced([-1]):
        for fmt in (0, 1, 2) + ((6,) if bit == 4 else ()):
            for M in E.M_SHAPES:
                d = on_device("main", bit, F16, M, N)
                for n_out, dev, addend, bias in COMBOS:
                    d.run(fmt, n_out, dev, addend, bias, f"auto fmt {fmt}")


@pytest.mark.parametrize("bit,names", [(8, BF16_INT8), (4, BF16_FP6)])
@pytest.mark.parametrize("N", E.N_SHAPES)
def test_exact_epilogue_every_bf16_tiling(N, bit, names):
    """bf16 containers (x_out, w_out, addend, y), fp16 scales and bias, bf16 expectation."""
    fmt = 2 if bit == 8 else 6
    for _, name in forced([-1] + names):
        for M in (E.M_SHAPES if name in SMALL_M + ("auto",) else (72,)):
            d = on_device("main", bit, BF16, M, N)
            for n_out, dev, addend, bias in COMBOS:
                d.run(fmt, n_out, dev, addend, bias, f"bf16 {name}")


def dequant(y32, sx, sw, addend, lda, bias, M, N, act):
    y = torch.empty((M, N), dtype=torch.float16, device=DEV)
    _capi.call("mixq_dequant", y32.data_ptr(), y32.stride(0), sx.data_ptr(), sw.data_ptr(), None if addend is None else addend.data_ptr(), lda,
               None if bias is None else bias.data_ptr(), y.data_ptr(), N, M, N, act, mixlib._stream())
    return y


@pytest.mark.parametrize("N", E.N_SHAPES)
def test_exact_epilogue_gemm_then_dequantize(N):
    """mixq_gemm_i8 + mixq_dequant (the reference's unfused pair): no outlier tail in this form."""
    assert _capi.load().mixq_gemm_set_config(-1) == 0
    for M in E.M_SHAPES:
        d = on_device("main", 8, F16, M, N)
        p = d.p
        qx, qw = d.q(0)
        y32 = torch.empty((M, N), dtype=torch.int32, device=DEV)
        _capi.call("mixq_gemm_i8", qx.data_ptr(), qw.data_ptr(), y32.data_ptr(), N, M, N, p.K, mixlib._stream())
        assert np.array_equal(y32.cpu().numpy(), p.acc.astype(np.int32))
        for addend in (None, True, "bcast"):
            for bias in (False, True):
                a = None if not addend else d.addend
                y = dequant(y32, d.sx, d.sw, a, 0 if addend != True else N, d.bias if bias else None, M, N, ACT_NONE)  # noqa: E712
                want, z = d.want(0, addend, bias)
                E.assert_exact(bits_of(y), want, z, F16, f"{p.name} gemm + dequant addend={addend} bias={bias}")


# ---- (b) range edges ------------------------------------------------------------------------------------------------------------------------
def representatives(bit):
    """(tiling, fmt, M) of one representative per family - the first tiling of each list - and the automatic pick."""
    names = _capi.gemm_config_names()
    reps = [(_tiled_configs()[0], 0, 72), (_tiled_configs()[0], 1, 72), (_wr_configs()[0], 2, 72), (_skinny_id(), 1, 24), (_skinny_id(), 2, 24),
            (-1, 0, 72), (-1, 1, 72), (-1, 2, 72), (-1, 1, 24), (-1, 2, 24)]
    if bit == 4:
        reps += [(names.index(F6_TILINGS[0]), 6, 72), (-1, 6, 72), (-1, 6, 24)]
    return reps


# (the long-K problem is int8 only: int4 products cannot pass 2^24 at any K the kernels take)
@pytest.mark.parametrize("kind,bit", [(k, b) for k in E.EDGES_F16 for b in (8, 4) if not (k == "long_k" and b == 4)])
def test_range_edges_one_tiling_of_each_family(kind, bit):
    for cfg, fmt, M in representatives(bit):
        for _, name in forced([cfg]):
            d = on_device(kind, bit, F16, M, E.N_SHAPES[0])
            for n_out, addend, bias in E.edge_combos(kind):
                d.run(fmt, n_out, False, addend, bias, f"{name} fmt {fmt}")


@pytest.mark.parametrize("bit,names", [(8, BF16_INT8), (4, BF16_FP6)])
def test_range_edges_bf16_wide(bit, names):
    fmt = 2 if bit == 8 else 6
    for _, name in forced([names[0], -1]):
        for M in E.M_SHAPES:
            d = on_device("wide", bit, BF16, M, E.N_SHAPES[0])
            for n_out, addend, bias in E.edge_combos("wide"):
                d.run(fmt, n_out, False, addend, bias, f"bf16 {name}")


def test_range_edges_int32_extremes_through_dequant():
    M, N = 72, 136
    y32, sx, sw, q = E.int32_extremes(M, N)
    z = y32.astype(np.float32).astype(np.float64) * q                      # float(acc_i32) rounds once above 2^24: part of the contract
    y = dequant(torch.from_numpy(y32).to(DEV), torch.from_numpy(sx).to(DEV), torch.from_numpy(sw).to(DEV), None, 0, None, M, N, ACT_NONE)
    E.assert_exact(bits_of(y), E.to_bits(z, F16), z, F16, "mixq_dequant on int32 extremes")


# ---- (c) W8A16 exact ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.N_SHAPES)
@pytest.mark.parametrize("M", E.M_SHAPES)
def test_w8a16_exact_every_configuration(M, N):
    x, qkn, scale, bias, z, q = E.w8a16_problem(M, E.K_MAIN, N)
    lib, names = _capi.load(), _capi.w8a16_config_names()
    cfgs = [-1] + sorted(set(_w8a16_real_configs() + [names.index("w8a16_32x64_s8_d5_l1")] + ([names.index("w8a16_decode32")] if M <= 32 else [])))
    wp, xd, sd, bd = mixlib.PackW8A16(torch.from_numpy(qkn).to(DEV)), torch.from_numpy(x).to(DEV), torch.from_numpy(scale).to(DEV), torch.from_numpy(bias).to(DEV)
    z0 = z - bias.astype(np.float64)[None, :]
    try:
        for cfg in cfgs:
            assert lib.mixq_gemm_w8a16_set_config(cfg) == 0
            for b, zz in ((None, z0), (bd, z)):
                y = mixlib.W8A16Linear(xd, wp, sd, b, N, E.K_MAIN)
                E.assert_exact(bits_of(y), E.to_bits(zz, F16), zz, F16, f"w8a16 {names[cfg] if cfg >= 0 else 'auto'} {M}x{E.K_MAIN}->{N} bias={b is not None}")
    finally:
        lib.mixq_gemm_w8a16_set_config(-1)


# ---- (d) SiLU over every argument -------------------------------------------------------------------------------------------------------------
def silu_families(dtype):
    """(family, tiling, fmt, bit) of every kernel family that has SiLU: one tiling each and the automatic pick."""
    if dtype == BF16:
        return [("bf16 wreg int8", BF16_INT8[0], 2, 8), ("bf16 wreg FP6", BF16_FP6[0], 6, 4), ("bf16 auto int8", -1, 2, 8), ("bf16 auto FP6", -1, 6, 4)]
    t0, w0 = _tiled_configs()[0], _wr_configs()[0]
    return [("gemm.hip plain int8", t0, 0, 8), ("gemm.hip P16X64 int8", t0, 1, 8), ("gemm.hip plain int4", t0, 0, 4), ("gemm.hip P16X64 int4", t0, 1, 4),
            ("wreg int8", w0, 2, 8), ("wreg int4 nibbles", w0, 2, 4), ("wreg FP6", F6_TILINGS[0], 6, 4), ("decode32 int8", "decode32", 1, 8),
            ("decode32 int4", "decode32", 2, 4), ("auto int8", -1, 2, 8), ("auto FP6", -1, 6, 4)]


class SiluOperands:
    """q_x = 0 (an all-zero activation: the main term vanishes), random weights, power-of-two scales; rows x 256."""

    def __init__(self, rows, bit, fmt, N=256):
        K = 64 if bit == 8 else 128
        rng = np.random.default_rng(rows + bit)
        lim = 127 if bit == 8 else 7
        qx, qw = np.zeros((rows, K), np.int8), rng.integers(-lim, lim + 1, (N, K)).astype(np.int8)
        qx, qw = (torch.from_numpy(qx), torch.from_numpy(qw)) if bit == 8 else (torch.from_numpy(E.pack_i4(qx)), torch.from_numpy(E.pack_i4(qw)))
        self.rows, self.N, self.K, self.bit, self.fmt = rows, N, K, bit, fmt
        self.q = q_images(qx, qw, bit, fmt)
        self.sx = torch.full((rows, 1), 0.125, dtype=torch.float16, device=DEV)
        self.sw = torch.full((1, N), 0.125, dtype=torch.float16, device=DEV)

    def launch(self, act, dtype, xo=None, wo=None, addend=None, bias=None, chunk=None):
        """One launch over all rows, or (decode32: M <= 32) launches over row chunks of `chunk`."""
        td = E.torch_dtype(dtype)
        if chunk is None:
            return mixlib.FusedLinear(self.q[0], self.q[1], self.sx, self.sw, xo, wo, 1 if xo is not None else 0, bias, self.rows, self.N, self.K, bit=self.bit, act=act,
                                      addend=addend, dtype=td)
        out = []
        sub = silu_operands(chunk, self.bit, self.fmt)                      # (its q_x image and x_scale: `chunk` all-zero rows)
        for r in range(0, self.rows, chunk):
            out.append(mixlib.FusedLinear(sub.q[0], self.q[1], sub.sx, self.sw, None if xo is None else xo[r:r + chunk], wo, 1 if xo is not None else 0, bias, chunk,
                                          self.N, self.K, bit=self.bit, act=act, addend=None if addend is None else addend[r:r + chunk], dtype=td))
        return torch.cat(out)


_silu_ops = {}


def silu_operands(rows, bit, fmt):
    key = (rows, bit, fmt)
    if key not in _silu_ops:
        _silu_ops[key] = SiluOperands(rows, bit, fmt)
    return _silu_ops[key]


def note(family, worst):
    WORST[family] = max(WORST.get(family, 0.0), worst)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_silu_over_every_finite_argument(dtype):
    """MIXQ_ACT_SILU with q_x = 0: z IS the addend, which holds every finite bit pattern of the container once; without bias, and with a
    fixed fp16 bias of mixed signs and magnitudes 2^-10 .. 2^6."""
    pat = E.all_finite_patterns(dtype)
    rows = pat.size // 256
    assert rows * 256 == pat.size and rows == (248 if dtype == F16 else 255)
    z = E.from_bits(pat, dtype).reshape(rows, 256)
    addend = torch.from_numpy(pat.view(np.int16).reshape(rows, 256).copy()).view(E.torch_dtype(dtype)).to(DEV)
    bias_np = E.silu_bias_vector(256)
    bias = torch.from_numpy(bias_np.astype(np.float16)).to(DEV)
    refs = {False: E.silu_reference(z, None, None, dtype), True: E.silu_reference(z, bias_np[None, :], None, dtype)}
    for family, cfg, fmt, bit in silu_families(dtype):
        chunk = None
        if cfg == "decode32":
            chunk = rows // 8
            assert chunk * 8 == rows and chunk <= 32
        op = silu_operands(rows, bit, fmt)
        for _ in forced([cfg]):
            for with_bias in (False, True):
                y = op.launch(ACT_SILU, dtype, addend=addend, bias=bias if with_bias else None, chunk=chunk)
                note(f"{family} SILU", E.silu_check(bits_of(y), *refs[with_bias], dtype, f"{family} ACT_SILU bias={with_bias}"))
    if dtype == F16:                                                           # the unfused pair's second half: mixq_dequant with the SiLU epilogue
        y32 = torch.zeros((rows, 256), dtype=torch.int32, device=DEV)
        op = silu_operands(rows, 8, 0)
        for with_bias in (False, True):
            y = dequant(y32, op.sx, op.sw, addend, 256, bias if with_bias else None, rows, 256, ACT_SILU)
            note("mixq_dequant SILU", E.silu_check(bits_of(y), *refs[with_bias], dtype, f"mixq_dequant ACT_SILU bias={with_bias}"))


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_silu_mul_over_signs_significands_and_exponents(dtype):
    """MIXQ_ACT_SILU_MUL: the addend slot carries the multiplier, so z arrives through ONE outlier column (exact in fp32)."""
    xo_np, wo_np, z, mul_np = E.silu_mul_operands(dtype)
    rows = 248
    xo, wo = poisoned(xo_np[:, None], 1, dtype), poisoned(wo_np[:, None], 1, dtype)
    mul = E.as_tensor(mul_np, dtype).to(DEV)
    bias_np = E.silu_bias_vector(256)
    bias = torch.from_numpy(bias_np.astype(np.float16)).to(DEV)
    refs = {False: E.silu_reference(z, None, mul_np, dtype), True: E.silu_reference(z, bias_np[None, :], mul_np, dtype)}
    for family, cfg, fmt, bit in silu_families(dtype):
        op = silu_operands(rows, bit, fmt)
        for _ in forced([cfg]):
            for with_bias in (False, True):
                y = op.launch(ACT_SILU_MUL, dtype, xo=xo, wo=wo, addend=mul, bias=bias if with_bias else None, chunk=31 if cfg == "decode32" else None)
                note(f"{family} SILU_MUL", E.silu_check(bits_of(y), *refs[with_bias], dtype, f"{family} ACT_SILU_MUL bias={with_bias}"))


@pytest.mark.parametrize("bit", [8, 4])
def test_silu_pair_form_over_signs_significands_and_exponents(bit):
    """MIXQ_ACT_SILU_PAIR: the up rows have a zero main term and a zero tail, so up = fp16(0 + bias_up) = bias_up, a constant per column that
    fp16 holds exactly - up's designed intermediate rounding is not in play; y = (silu(z_gate) + bias_gate) * bias_up."""
    xo_np, wo_np, z, mul_np = E.silu_mul_operands(F16)
    rows, N = 248, 256
    bias_u, bias_g = mul_np[0], E.silu_bias_vector(N)
    K = 64 if bit == 8 else 128
    lim = 127 if bit == 8 else 7
    rng = np.random.default_rng(bit)
    qx, qw2 = np.zeros((rows, K), np.int8), rng.integers(-lim, lim + 1, (2 * N, K)).astype(np.int8)
    qx, qw2 = (torch.from_numpy(qx), torch.from_numpy(qw2)) if bit == 8 else (torch.from_numpy(E.pack_i4(qx)), torch.from_numpy(E.pack_i4(qw2)))
    qx, qw2 = q_images(qx, qw2, bit, 2 if bit == 8 else 6)
    sx = torch.full((rows, 1), 0.125, dtype=torch.float16, device=DEV)
    sw2 = torch.full((1, 2 * N), 0.125, dtype=torch.float16, device=DEV)
    xo = poisoned(xo_np[:, None], 1, F16)
    wo2 = poisoned(np.zeros((2 * N, 1)), 1, F16)
    wo2[:, :1] = interleave_pair_rows(torch.zeros((N, 1), dtype=torch.float16, device=DEV), E.as_tensor(wo_np[:, None], F16).to(DEV))
    bias2 = interleave_pair_rows(E.as_tensor(bias_u, F16).to(DEV), E.as_tensor(bias_g, F16).to(DEV))
    ref, bound = E.silu_reference(z, bias_g[None, :], bias_u[None, :], F16)
    tilings = [t for t in PAIR_TILINGS if bit == 8 or t != "wr128x256_s16_d3_l2"]
    for _, name in forced([-1, tilings[0]]):
        y = mixlib.FusedLinear(qx, qw2, sx, sw2, xo, wo2, 1, bias2, rows, 2 * N, K, bit=bit, act=ACT_SILU_PAIR)
        assert tuple(y.shape) == (rows, N)
        note(f"pair W{bit} {name}", E.silu_check(bits_of(y), ref, bound, F16, f"W{bit} {name} ACT_SILU_PAIR"))
