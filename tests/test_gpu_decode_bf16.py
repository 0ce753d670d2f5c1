"""The small-batch ("decode") kernel in bfloat16 on the MI355X: mixq_gemm_i8_decode_bf16 / mixq_gemm_i4_decode_bf16 (gemm_skinny_bf16.hip),
mixq_linear_forward_decode_bf16 and the layers under MixqConfig.decode_bf16.  The contract is include/mixq_hip.h, "bf16 layers", word for
word; the float64 restatement, its derived bound and the operand generators are tests/test_gpu_bf16_gemm.py's and tests/exact.py's, imported
and not restated.

Shapes: the kernel splits K over 8 waves in steps of 64 bytes, loads 4 steps at a time into one of two buffers.  int8 K in {64, 512, 704,
2368, 4608} gives per-wave step counts {0 or 1}, {1}, {1 or 2}, {4 or 5}, {9}: the empty wave, less than one group, the exact group, a
remainder after one group, both buffers plus a remainder; the nibble form takes twice those K.  N in {36, 100, 260, 1000}: a partial
32-channel block and N % 8 != 0; M in {1, 5, 17, 24, 32}.  Every value appears with outliers and without.

  1 the epilogue against float64, both kernels (and both int8 weight layouts), every element, NaN pads included
  2 bytes where bytes are owed: n_out = 0 against mixq_gemm_i8_fused_bf16 / the FP6 route of mixq_gemm_i4_fused_bf16; the two int8 layouts
    at every n_out.  With outlier columns the decode form and the `_bf16` route agree to the bound of 1 only: the tail sums 16 columns per
    v_mfma_f32_32x32x16_bf16 step where the weights-in-registers kernels sum 32 per v_mfma_f32_16x16x32_bf16 step - another fp32 order.
  3 exact operands (tests/exact.py) at M = 24, bit for bit, at the bf16 range edges, and SiLU / SILU_MUL over every finite argument
  4 store paths: strided ldy, offset y, guard frames; nothing changes after a refusal
  5 mixq_linear_forward_decode_bf16 is its two calls, byte for byte
  6 the layers: search phase, freeze, one-call route, hipGraph replay; M = 33; the flag off; MixLlamaMLP; a serving sequence with the flag
    flipped mid-life against a twin that keeps nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact as E  # noqa: E402
import frames  # noqa: E402
import test_gpu_bf16_gemm as G  # noqa: E402
import test_gpu_exact as X  # noqa: E402
import test_operator_stateful as S  # noqa: E402
from exact import BF16  # noqa: E402
from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib  # noqa: E402
from mixq_amd._capi import ACT_NONE, ACT_SILU, ACT_SILU_MUL, ACT_SILU_PAIR, FMT_F16X64, FMT_P16X64  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402
from mixq_amd.linear import kept_outlier_map  # noqa: E402
from test_gpu_stateful import on_gpu  # noqa: E402

DEV = "cuda"
BF, F16 = torch.bfloat16, torch.float16
WF16, P16 = _capi.X_PACKED | _capi.W_F16X64, _capi.X_PACKED | _capi.W_PACKED
# (int8 K, N, M): every K, N and M of the module docstring; the nibble form runs the same rows at twice the K
SHAPES = [(64, 36, 1), (512, 100, 5), (704, 260, 17), (2368, 1000, 24), (4608, 260, 32)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    _capi.load().mixq_gemm_set_config(-1)
    yield
    _capi.load().mixq_gemm_set_config(-1)


def ibits(t):
    return t.contiguous().view(torch.int16)


class DecodeProblem(G.Problem):
    """tests/test_gpu_bf16_gemm.py's Problem with the images the decode entry points read beside the ones the `_bf16` entry points read (the
    same integers): int8 P16X64 x {F16X64, P16X64}; 4-bit nibbles in P16X64 on both sides beside the FP6 pair.  `route` chooses what run()
    launches: "decode" (weights F16X64 for int8), "decode_p16" (int8: P16X64 weights) or "bf16" (the parent's entry points)."""

    def __init__(self, bit, M, K, N, seed):
        super().__init__(bit, M, K, N, seed)
        self.images = {"bf16": (self.qx_img, self.qw_img)}
        if bit == 8:
            self.images["decode"] = (self.qx_img, self.qw_img)
            self.images["decode_p16"] = (self.qx_img, mixlib.PackOperand(mixlib.UnpackOperand(self.qw_img, N), FMT_P16X64))
        else:
            self.images["decode"] = (mixlib.PackOperand(mixlib.UnpackOperand(self.qx_img, M), FMT_P16X64),
                                     mixlib.PackOperand(mixlib.UnpackOperand(self.qw_img, N), FMT_P16X64))
        self.route = "decode"

    def run(self, n, dev_count, act, bias, addend, **kw):
        self.qx_img, self.qw_img = self.images[self.route]
        if self.route != "bf16":
            kw["decode"] = True
        return super().run(n, dev_count, act, bias, addend, **kw)


_problems = {}


def problem(bit, K8, N, M):
    key = (bit, K8, N, M)
    if key not in _problems:
        _problems[key] = DecodeProblem(bit, M, K8 if bit == 8 else 2 * K8, N, seed=77 * bit + K8 + N + M)
    return _problems[key]


# ---- 1. the epilogue against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("K8,N,M", SHAPES)
def test_epilogue_of_the_decode_form_against_float64(bit, K8, N, M):
    """N_OUTS x CASES x bias x device count of tests/test_gpu_bf16_gemm.py's sweep, its reference and its derived bound."""
    p = problem(bit, K8, N, M)
    p.route = "decode"
    G.sweep(p, f"W{bit} decode {M}x{p.K}->{N}")
    if bit == 8:
        p.route = "decode_p16"
        G.sweep(p, f"W8 decode P16X64 weights {M}x{p.K}->{N}")


# ---- 2. bytes where bytes are owed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("K8,N,M", SHAPES)
def test_without_outliers_the_bytes_are_the_bf16_entry_points(bit, K8, N, M):
    """n_out = 0: the same exact accumulator and the same fp32 operations in the same order as the automatic route of mixq_gemm_i8_fused_bf16
    (the 32 x 64 tiling at these shapes); the nibble form against the FP6 route of mixq_gemm_i4_fused_bf16 - its factor 256 leaves as an
    exact 1 / 256 on x_scale (normal scales)."""
    p = problem(bit, K8, N, M)
    assert _capi.load().mixq_gemm_set_config(-1) == 0
    for act, has_add in G.CASES:
        for bias in (False, True):
            add = (p.mul if act == ACT_SILU_MUL else p.addend) if has_add else None
            p.route = "decode"
            y, _, _ = p.run(0, False, act, bias, add)
            p.route = "bf16"
            y0, _, _ = p.run(0, False, act, bias, add)
            assert torch.equal(ibits(y), ibits(y0)), f"W{bit} {M}x{p.K}->{N} act={act} addend={has_add} bias={bias}"


@pytest.mark.parametrize("K8,N,M", SHAPES)
def test_the_two_int8_weight_layouts_write_identical_bytes(K8, N, M):
    p = problem(8, K8, N, M)
    for n in G.N_OUTS:
        for act, has_add in G.CASES:
            add = (p.mul if act == ACT_SILU_MUL else p.addend) if has_add else None
            p.route = "decode"
            y, _, _ = p.run(n, n == 41, act, True, add)
            p.route = "decode_p16"
            y1, _, _ = p.run(n, n == 41, act, True, add)
            assert torch.equal(ibits(y), ibits(y1)), f"{M}x{p.K}->{N} n_out={n} act={act}"


@pytest.mark.parametrize("bit", [8, 4])
def test_with_outliers_the_two_routes_agree_to_the_bound_only(bit):
    """The decode tail sums 16 columns per 32x32x16 MFMA step, the weights-in-registers tail 32 per 16x16x32 step: another order of fp32
    additions, so bytes are not owed - both are within the derived bound of the same float64 value."""
    K8, N, M = SHAPES[3]
    p = problem(bit, K8, N, M)
    for n in (17, 41, 70):
        out = {}
        for route in ("decode", "bf16"):
            p.route = route
            y, xo, wo = p.run(n, False, ACT_NONE, True, p.addend)
            ref, bound = G.reference(p.acc, p.sx, p.sw, xo, wo, n, p.addend, p.bias, ACT_NONE)
            G.check(y, ref, bound, f"W{bit} {route} n_out={n}")
            out[route] = y
        assert bool(((out["decode"].to(torch.float64) - out["bf16"].to(torch.float64)).abs() <= 2 * bound).all())


# ---- 3. exact operands ----------------------------------------------------------------------------------------------------------------
def run_exact(d, fmt, n_out, dev, addend, bias, what):
    """tests/test_gpu_exact.py's OnDevice.run through the decode entry points."""
    p = d.p
    xo, wo, n_arg, n_dev = d.outliers(n_out, dev)
    qx, qw = d.q(fmt)
    a = None if not addend else (d.bcast if addend == "bcast" else d.addend)
    y = mixlib.FusedLinear(qx, qw, d.sx, d.sw, xo, wo, n_arg, d.bias if bias else None, p.M, p.N, p.K, bit=p.bit, act=ACT_NONE, n_out_dev=n_dev,
                           addend=a, dtype=d.td, decode=True)
    want, z = d.want(n_out, addend, bias)
    E.assert_exact(X.bits_of(y), want, z, p.dtype, f"{p.name} {what} n_out={n_out} dev_count={dev} addend={addend} bias={bias}")


@pytest.mark.parametrize("bit,fmt", [(8, 2), (8, 1), (4, 1)])
@pytest.mark.parametrize("N", E.N_SHAPES)
def test_exact_epilogue_of_the_decode_form(N, bit, fmt):
    """Operands for which every fp32 operation of the formula is exact: y == RNE_bf16(float64 z) bit for bit, every element - what a wrong
    lane map of the bf16 tail MFMA (rows, columns or the k halves swapped) cannot pass."""
    d = X.on_device("main", bit, BF16, 24, N)
    for n_out, dev, addend, bias in X.COMBOS:
        run_exact(d, fmt, n_out, dev, addend, bias, f"decode fmt {fmt}")


@pytest.mark.parametrize("bit,fmt", [(8, 2), (4, 1)])
def test_range_edges_of_the_decode_form(bit, fmt):
    d = X.on_device("wide", bit, BF16, 24, E.N_SHAPES[0])
    for n_out, addend, bias in E.edge_combos("wide"):
        run_exact(d, fmt, n_out, False, addend, bias, f"decode fmt {fmt} wide")


def silu_launch(bit, act, rows, chunk, xo=None, wo=None, addend=None, bias=None):
    """tests/test_gpu_exact.py's SiluOperands (q_x = 0: z is the addend, or arrives through one outlier column) through the decode entry
    points, `chunk` <= 32 rows per launch."""
    fmt = 2 if bit == 8 else 1
    full, sub = X.silu_operands(rows, bit, fmt), X.silu_operands(chunk, bit, fmt)
    out = []
    for r in range(0, rows, chunk):
        out.append(mixlib.FusedLinear(sub.q[0], full.q[1], sub.sx, full.sw, None if xo is None else xo[r:r + chunk], wo, 1 if xo is not None else 0, bias, chunk,
                                      full.N, full.K, bit=bit, act=act, addend=None if addend is None else addend[r:r + chunk], dtype=BF, decode=True))
    return torch.cat(out)


@pytest.mark.parametrize("bit", [8, 4])
def test_silu_of_the_decode_form_over_every_finite_argument(bit):
    pat = E.all_finite_patterns(BF16)
    rows = pat.size // 256
    assert rows == 255
    z = E.from_bits(pat, BF16).reshape(rows, 256)
    addend = torch.from_numpy(pat.view(np.int16).reshape(rows, 256).copy()).view(BF).to(DEV)
    bias_np = E.silu_bias_vector(256)
    bias = torch.from_numpy(bias_np.astype(np.float16)).to(DEV)
    for with_bias in (False, True):
        ref = E.silu_reference(z, bias_np[None, :] if with_bias else None, None, BF16)
        y = silu_launch(bit, ACT_SILU, rows, 17, addend=addend, bias=bias if with_bias else None)
        E.silu_check(X.bits_of(y), *ref, BF16, f"W{bit} decode ACT_SILU bias={with_bias}")


@pytest.mark.parametrize("bit", [8, 4])
def test_silu_mul_of_the_decode_form(bit):
    xo_np, wo_np, z, mul_np = E.silu_mul_operands(BF16)
    rows = 248
    xo, wo = X.poisoned(xo_np[:, None], 1, BF16), X.poisoned(wo_np[:, None], 1, BF16)
    mul = E.as_tensor(mul_np, BF16).to(DEV)
    bias_np = E.silu_bias_vector(256)
    bias = torch.from_numpy(bias_np.astype(np.float16)).to(DEV)
    for with_bias in (False, True):
        ref = E.silu_reference(z, bias_np[None, :] if with_bias else None, mul_np, BF16)
        y = silu_launch(bit, ACT_SILU_MUL, rows, 31, xo=xo, wo=wo, addend=mul, bias=bias if with_bias else None)
        E.silu_check(X.bits_of(y), *ref, BF16, f"W{bit} decode ACT_SILU_MUL bias={with_bias}")


# ---- 4. store paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("K8,N,M", [SHAPES[1], SHAPES[2], SHAPES[3]])
def test_decode_writes_inside_its_window(bit, K8, N, M):
    """y with a row stride above N, as a column slice of a wider buffer, on a base that is 8- but not 16-byte aligned: the window holds the
    bytes of the exact-fit launch and nothing outside it changed (N = 100, 260: N % 8 == 4; N = 1000: N % 8 == 0, a partial last block)."""
    p = problem(bit, K8, N, M)
    p.route = "decode"
    want, _, _ = p.run(41, True, ACT_SILU, True, p.addend)
    for ld, col_off, elem_off in frames.LAYOUTS(N):
        f = frames.Frame(M, N, ld, col_off, elem_off, dtype=BF, device=DEV)
        y, _, _ = p.run(41, True, ACT_SILU, True, p.addend, out=f.view)
        torch.cuda.synchronize()
        assert y.data_ptr() == f.view.data_ptr() and torch.equal(ibits(f.view), ibits(want)), (ld, col_off, elem_off)
        f.assert_untouched(f"W{bit} decode {M}x{p.K}->{N} ld {ld} col_off {col_off} elem_off {elem_off}")


@pytest.mark.parametrize("bit", [8, 4])
def test_nothing_is_written_after_a_refusal(bit):
    K8, N, M = SHAPES[2]
    p = problem(bit, K8, N, M)
    lib, names = _capi.load(), _capi.gemm_config_names()
    fn = lib.mixq_gemm_i8_decode_bf16 if bit == 8 else lib.mixq_gemm_i4_decode_bf16
    qx, qw = p.images["decode"]
    f = frames.Frame(40, N, N + 8, dtype=BF, device=DEV).freeze()

    def call(rows, act, layout=WF16 if bit == 8 else P16):
        rc = fn(qx.data_ptr(), qw.data_ptr(), p.sx.data_ptr(), p.sw.data_ptr(), None, 0, None, 0, 0, None, None, 0, None, f.view.data_ptr(), f.ld, rows, N, p.K, act,
                layout, mixlib._stream())
        torch.cuda.synchronize()
        return rc
    assert call(33, ACT_NONE) == _capi.MIXQ_ESHAPE
    f.assert_unchanged("M = 33")
    assert call(M, ACT_SILU_PAIR) == _capi.MIXQ_ESHAPE
    f.assert_unchanged("the paired act")
    assert call(M, ACT_NONE, _capi.XW_F6X128) == (_capi.MIXQ_EINVAL if bit == 8 else _capi.MIXQ_ESHAPE)
    f.assert_unchanged("an FP6 layout")
    try:
        assert lib.mixq_gemm_set_config(names.index("wr32x64_s8_d6_l1")) == 0
        assert call(M, ACT_NONE) == _capi.MIXQ_EINVAL
        f.assert_unchanged("a forced non-decode tiling")
        assert lib.mixq_gemm_set_config(names.index("decode32")) == 0
        assert call(M, ACT_NONE) == 0                                                   # ... and decode32 itself, forced, runs
        f.assert_untouched("forced decode32")
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0
    p.route = "decode"
    want, _, _ = p.run(0, False, ACT_NONE, False, None)
    assert torch.equal(ibits(f.view[:M]), ibits(want))


# ---- 5. one call = two calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit,wroute", [(8, "decode"), (8, "decode_p16"), (4, "decode")])
@pytest.mark.parametrize("quant", ["plain", "kept", "known_amax"])
def test_linear_forward_decode_bf16_is_its_two_calls(bit, wroute, quant):
    """q_x, x_scale, x_out, y (and x, whose outlier columns the pass zeroes): the `_bf16` quantise pass the block describes - plain, with a kept
    map, with a producer's row maxima - then the decode GEMM; 9 live columns below a capacity of 16 (n_dev)."""
    K8, N, M = SHAPES[2]
    p = problem(bit, K8, N, M)
    K = p.K
    qw = p.images[wroute][1]
    wfmt = mixlib.fmt_of(qw)
    layout = WF16 if wfmt == FMT_F16X64 else P16
    cols = [5, 77, 130, 131, 300, 511, 64, 2, 400]
    n, ldo = len(cols), 16
    ind = torch.zeros(ldo, dtype=torch.int32, device=DEV)
    ind[:n] = torch.tensor(cols, dtype=torch.int32)
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    cm = kept_outlier_map(ind[:n], K) if quant != "plain" else None
    x0 = G._make_x(M, K, cols, 3).to(DEV)
    _, wo = p.outliers(n)
    rows = mixlib.packed_rows(M)
    amax0 = None
    if quant == "known_amax":                                   # what a producing GEMM leaves: maxima of the bf16 bit patterns over the unmarked columns
        b = x0.view(torch.int16).int() & 0x7FFF
        b[:, cols] = 0
        amax0 = b.max(dim=1).values.to(torch.int32)

    def buffers():
        return (x0.clone(), torch.zeros(M, 1, dtype=F16, device=DEV), torch.zeros(rows, mixlib._q_row_bytes(K, bit, FMT_P16X64), dtype=torch.uint8, device=DEV),
                torch.zeros(M, ldo, dtype=BF, device=DEV), torch.zeros(M, N, dtype=BF, device=DEV), None if amax0 is None else amax0.clone())

    # two calls
    x, xs, q, xo, y, ra = buffers()
    st = mixlib._stream()
    if quant == "known_amax":
        _capi.call("mixq_quant_known_amax_bf16", x.data_ptr(), ind.data_ptr(), ldo, n_dev.data_ptr(), ra.data_ptr(), cm.data_ptr(), cm.numel(), xs.data_ptr(),
                   q.data_ptr(), xo.data_ptr(), None, M, K, K, ldo, bit, 6.0, FMT_P16X64, st)
    elif quant == "kept":
        _capi.call("mixq_quant_fused_masked_bf16", x.data_ptr(), ind.data_ptr(), ldo, n_dev.data_ptr(), cm.data_ptr(), cm.numel(), xs.data_ptr(), q.data_ptr(),
                   xo.data_ptr(), None, M, K, K, ldo, bit, 6.0, FMT_P16X64, st)
    else:
        _capi.call("mixq_quant_fused_bf16", x.data_ptr(), ind.data_ptr(), ldo, n_dev.data_ptr(), xs.data_ptr(), q.data_ptr(), xo.data_ptr(), None, M, K, K,
                   ldo, bit, 6.0, FMT_P16X64, st)
    _capi.call("mixq_gemm_i8_decode_bf16" if bit == 8 else "mixq_gemm_i4_decode_bf16", q.data_ptr(), qw.data_ptr(), xs.data_ptr(), p.sw.data_ptr(),
               xo.data_ptr(), ldo, wo.data_ptr(), wo.stride(0), ldo, n_dev.data_ptr(), None, 0, p.bias.data_ptr(), y.data_ptr(), N, M, N, K, ACT_NONE, layout, st)
    two = [t.clone() for t in (x, xs, q, xo, y)]
    # one call
    x, xs, q, xo, y, ra = buffers()
    a = _capi.LinearArgs()
    a.x, a.ldx, a.ind, a.n_cap, a.n_dev = x.data_ptr(), K, ind.data_ptr(), ldo, n_dev.data_ptr()
    a.x_scale, a.q_x, a.x_out, a.ldxo = xs.data_ptr(), q.data_ptr(), xo.data_ptr(), ldo
    a.q_w, a.scale_col, a.w_out, a.ldwo, a.bias = qw.data_ptr(), p.sw.data_ptr(), wo.data_ptr(), wo.stride(0), p.bias.data_ptr()
    a.y, a.ldy, a.M, a.N, a.K, a.bit, a.sigma, a.act, a.qfmt, a.wfmt = y.data_ptr(), N, M, N, K, bit, 6.0, ACT_NONE, FMT_P16X64, wfmt
    if cm is not None:
        a.col_mask, a.col_mask_words = cm.data_ptr(), cm.numel()
    if ra is not None:
        a.row_amax = ra.data_ptr()
    _capi.call("mixq_linear_forward_decode_bf16", C.byref(a), st)
    torch.cuda.synchronize()
    for name, t2, t1 in zip(("x", "x_scale", "q_x", "x_out", "y"), two, (x, xs, q, xo, y)):
        assert torch.equal(t2.view(torch.uint8), t1.view(torch.uint8)), name
    assert torch.equal(xo[:, :n].view(torch.int16), x0[:, cols].view(torch.int16)) and bool((y.float().abs() > 0).any())
    if ra is not None:
        assert int(ra.abs().max()) == 0                          # (the known-maximum pass cleared the producer's buffer)


# ---- 6. the layers --------------------------------------------------------------------------------------------------------------------
K_L, N_L = 512, 260
HOT = [3, 200, 411]


def make_layer(bit, config, hot=True):
    torch.manual_seed(11)
    lin = torch.nn.Linear(K_L, N_L, bias=True).to(BF)
    cache = MixLibCache(64, bit=bit, device=DEV, config=config)
    kw = {}
    if bit == 4:                                                 # (a 4-bit layer is built with its static 16-bit columns, HOT among them)
        ls = torch.ones(K_L)
        ls[HOT + [7, 90, 333]] = 20.0
        kw = {"layer_scales": ls, "fp_features_num": 6}
    return MixLinear_GEMM.from_linear(lin, bit, cache=cache, dev=DEV, **kw)


def layer_x(M, seed, hot=True):
    return G._make_x(M, K_L, HOT if hot else [], seed, 6.0e4).to(DEV)


class Spy:
    """What mixlib.FusedLinear / ForwardPlan were handed and which kept plans ran: (what, N, decode, a row maximum asked of / handed to it)."""

    def __init__(self, monkeypatch):
        self.seen = seen = []
        fused, plan_init, plan_run = mixlib.FusedLinear, mixlib.ForwardPlan.__init__, mixlib.ForwardPlan.run

        def fused_spy(*args, **kw):
            seen.append(("FusedLinear", args[9], bool(kw.get("decode")), kw.get("row_amax") is not None))
            return fused(*args, **kw)

        def init_spy(self, M, N, *args, **kw):
            seen.append(("ForwardPlan", N, bool(kw.get("decode")), False))
            return plan_init(self, M, N, *args, **kw)

        def run_spy(self, x, row_amax=None, **kw):
            seen.append(("ForwardPlan.run", self.N, self.decode, row_amax is not None))
            return plan_run(self, x, row_amax=row_amax, **kw)
        monkeypatch.setattr(mixlib, "FusedLinear", fused_spy)
        monkeypatch.setattr(mixlib.ForwardPlan, "run", run_spy)
        monkeypatch.setattr(mixlib.ForwardPlan, "__init__", init_spy)


@pytest.mark.parametrize("bit", [8, 4])
def test_layer_under_the_flag_search_freeze_one_call_and_graph_replay(bit, monkeypatch):
    """512 -> 260 at M = 8: every step of the layer's life writes the bytes of the two-call route under the flag (a twin with
    one_call_forward off), the decode form is what ran, and the result is the contract's (the float64 reference of the layer's own state).
    The 4-bit layer serves the batch from its nibble image (small_batch_m4 = 32) through mixq_gemm_i4_decode_bf16."""
    flags = dict(act_dtype=BF, decode_bf16=True, small_batch_m4=32 if bit == 4 else 0)
    spy = Spy(monkeypatch)
    layer, twin = make_layer(bit, MixqConfig(**flags)), make_layer(bit, MixqConfig(one_call_forward=False, **flags))
    M = 8
    for call in range(4):                                        # calls 0, 1: the search phase; from call 2 on the prediction is frozen
        x = layer_x(M, call)
        spy.seen.clear()
        y, y2 = layer(x.clone(), None, True), twin(x.clone(), None, True)
        torch.cuda.synchronize()
        assert torch.equal(ibits(y), ibits(y2)), call
        assert spy.seen and all(s[2] for s in spy.seen), (call, spy.seen)               # every GEMM of both layers took the decode form
        ref, bound = G._layer_reference(layer, x, bit)
        G.check(y, ref, bound, f"W{bit} layer under the flag, call {call}")
    assert layer.add_outliers is False and layer._plan is not None and layer._plan.decode is True
    assert layer._plan.fn_name == "mixq_linear_forward_decode_bf16"
    if bit == 4:
        assert mixlib.fmt_of(layer._packed_weight(M)) == FMT_P16X64                     # the nibble image
    # hipGraph: captured once on a side stream, replayed on restored inputs (the forward zeroes x's outlier columns in place)
    x3 = layer_x(M, 9)
    y_two = twin(x3.clone(), None, True)
    xg = x3.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(xg, None, True)
        xg.copy_(x3)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            yg = layer(xg, None, True)
        for _ in range(2):
            xg.copy_(x3)
            yg.zero_()
            g.replay()
            side.synchronize()
            assert torch.equal(ibits(yg), ibits(y_two))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # M = 33: the parent's route (no decode), the bytes of a layer that never heard of the flag - W8 (a 4-bit layer serves M = 33 from its FP6 image)
    spy.seen.clear()
    off = make_layer(bit, MixqConfig(act_dtype=BF))
    for call in range(3):
        off(layer_x(M, call), None, True)
    spy.seen.clear()
    x33 = layer_x(33, 5)
    y_on, y_off = layer(x33.clone(), None, True), off(x33.clone(), None, True)
    torch.cuda.synchronize()
    assert not any(s[2] for s in spy.seen), spy.seen
    assert torch.equal(layer.ind, off.ind) and torch.equal(ibits(y_on), ibits(y_off))
    # ... and at M = 8 the flag-off layer is within the contract's bound like the flag-on one (bytes are not owed: the tail's summation order)
    x8 = layer_x(M, 6)
    if bit == 8:
        y_off8 = off(x8.clone(), None, True)
        ref, bound = G._layer_reference(off, x8, bit)
        G.check(y_off8, ref, bound, "flag off")
        G.check(layer(x8.clone(), None, True), ref, bound, "flag on")
    del g


def test_flag_off_is_the_parent_and_without_outliers_the_flag_changes_no_byte(monkeypatch):
    spy = Spy(monkeypatch)
    on, off = make_layer(8, MixqConfig(act_dtype=BF, decode_bf16=True)), make_layer(8, MixqConfig(act_dtype=BF))
    for call in range(4):
        x = layer_x(8, 20 + call, hot=False) * 0.05              # (no column above sigma: the layers find no outlier)
        spy.seen.clear()
        y_off = off(x.clone(), None, True)
        assert spy.seen and not any(s[2] for s in spy.seen), spy.seen                   # flag off: never the decode form
        y_on = on(x.clone(), None, True)
        torch.cuda.synchronize()
        assert any(s[2] for s in spy.seen)
        assert int(on.ind.numel()) == 0 == int(off.ind.numel())
        assert torch.equal(ibits(y_on), ibits(y_off)), call
    # flipping the flag on the live, frozen layer takes effect at the next forward - and back
    x = layer_x(8, 30, hot=False) * 0.05
    off.config.decode_bf16 = True
    spy.seen.clear()
    y1 = off(x.clone(), None, True)
    assert spy.seen == [("ForwardPlan", N_L, True, False), ("ForwardPlan.run", N_L, True, False)] and off._plan.decode is True
    off.config.decode_bf16 = False
    y0 = off(x.clone(), None, True)
    assert spy.seen[2:] == [("ForwardPlan.run", N_L, False, False)]                     # (the plan kept under the flag-off identity)
    assert off._plan.decode is False and torch.equal(ibits(y0), ibits(y1))


def test_mlp_block_under_all_bf16_flags(monkeypatch):
    """MixLlamaMLP at M = 8 with fused_bf16, joint_gate_up_bf16, w8a16_bf16 and decode_bf16: down_proj takes the decode form by itself, still fed
    by the row maxima gate_proj's (joint) GEMM left; gate / up stay where they are; the block is within the bound of the flag-off block."""
    spy = Spy(monkeypatch)
    K, I, M = 128, 64, 8
    out, h_in = {}, {}
    for flag in (False, True):
        blk = S.make_block(8, K, I, 0, MixqConfig(decode_bf16=flag, **S.BF16_FLAGS), dev=DEV, dtype=BF)
        down = blk[1].down_proj_
        down.register_forward_pre_hook(lambda mod, args, flag=flag: h_in.__setitem__(flag, args[0].detach().clone()))
        for i in range(4):
            x = torch.randn(M, K, generator=torch.Generator().manual_seed(1000 + i)).to(BF)
            x[:, [5, 77]] *= 30
            spy.seen.clear()
            y = blk[1](blk[0](x.to(DEV)))
            torch.cuda.synchronize()
        out[flag] = (y, down)
        assert not down.add_outliers
        dec = [s for s in spy.seen if s[2]]
        runs = [s[1:] for s in spy.seen if s[0] == "ForwardPlan.run"]
        assert any(s[3] for s in spy.seen if s[0] == "FusedLinear"), spy.seen            # the GEMM in front of down_proj leaves the row maxima ...
        assert not any(s[2] and s[3] for s in spy.seen if s[0] == "FusedLinear"), spy.seen   # ... and is never the decode form (no side output there)
        if flag:
            assert (K, True, True) in runs, runs                                        # down_proj: the decode form, on the producer's row maxima
        else:
            assert not dec and (K, False, True) in runs, (dec, runs)
    assert torch.equal(ibits(h_in[False]), ibits(h_in[True]))                           # down_proj's input: the same bytes under either flag
    for flag in (False, True):
        y, down = out[flag]
        ref, bound = G._layer_reference(down, h_in[flag].reshape(-1, I), 8)
        G.check(y.reshape(M, K), ref, bound, f"MixLlamaMLP, decode_bf16={flag}")


@pytest.mark.parametrize("cls", [S.BlockMachineBf16, S.BlockMachine4Bf16], ids=lambda c: c.__name__)
def test_serving_sequence_with_the_flag_flipped_mid_life(cls):
    """In the shape of tests/test_gpu_stateful.py's fixed sequences: the block with every caching feature on against the twin that keeps
    nothing, step by step, byte for byte - the flag flipped on both (it chooses the kernel, so the twin follows it) between forwards of a live,
    frozen block; the 4-bit block serves its small batches from the nibble image while the flag is on."""
    m = on_gpu(cls)()
    try:
        m.build(1, warm=True)
        cfgs = (m.a[1].config, m.b[1].config)

        def flip(on):
            for c in cfgs:
                c.decode_bf16 = on
                if cls.BIT == 4:
                    c.small_batch_m4 = 8 if on else 0
        for on in (True, False, True):
            flip(on)
            m.forward(8, 3, False)
            m.forward(16, 4, True, res="contig")
            m.layer_on_its_own(8, 5, "down_proj_", residual=True)
            m.layer_on_its_own(2, 6, "up_proj_")
            m.forward(3, 7, False, res="strided")
            m.toggle_compaction_and_plans()
        m.forward(24, 8, False)
        flip(False)
        m.same_state_dict()
    finally:
        m.teardown()
    torch.cuda.synchronize()
