"""bfloat16 layers on the MI355X: the `_bf16` GEMM epilogue (every bf16 tiling and the automatic pick) against a float64 restatement of
its arithmetic over the operands the kernel reads, the row-maximum side output, the one-call forward against its two calls, and
MixLinear_GEMM end to end in bfloat16 (search phase, freeze, one-call route, hipGraph replay) - with an fp16 layer around it unchanged.

The restatement (include/mixq_hip.h "bf16 layers"), all in float64:
    z = acc * sx[m] * sw[n] + sum_j xo[m,j] * wo[n,j] + addend[m,n]          acc: the exact integer contraction, wo: the bf16 operand
    y = z + bias | silu(z) + bias | (silu(z') + bias) * mul   (z' without the addend: the slot carries the multiplier)
The kernel's only roundings are fp32 operations and ONE round-to-nearest-even to bf16, so the bound is derived, not tuned:
    |y - ref| <= ulp_bf16(ref) + (n_out + 8) * 2^-24 * (|acc sx sw| + sum_j |xo wo| + |addend| + |bias|)
(one bf16 ulp covers the half-ulp rounding and a flip at a tie; the second term is the fp32 accumulation slack, which only matters under
cancellation).  With SiLU the project's allowance for mixq_silu against a float64 SiLU is added - tests/test_gpu_parity.py::ulp_tol, two
fp16 ulp of |silu(z)| and at least 1e-3, restated below - and with MIXQ_ACT_SILU_MUL that allowance is multiplied by |mul|.
Every element of y is compared."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402
from mixq_amd.linear import kept_outlier_map  # noqa: E402
from mixq_amd._capi import ACT_NONE, ACT_SILU, ACT_SILU_MUL, FMT_F16X64, FMT_F6X128, FMT_P16X64, FMT_R6X128  # noqa: E402

DEV = "cuda"
BF, F16, F64 = torch.bfloat16, torch.float16, torch.float64
# the tilings with a bf16 form (gemm_wreg.hip: g_cost8 / g_cost6 + WR_SMALL)
BF16_INT8 = ["wr128x192_s16_d4_l2", "wr128x128_s16_d4_l2", "wr128x256_s16_d3_l2", "wr64x128_s16_d4_l2", "wr64x192_s16_d4_l2", "wr64x256_s16_d4_l2",
             "wr128x64_s8_d4_l1", "wr64x64_s8_d4_l1", "wr32x64_s8_d6_l1"]
BF16_FP6 = ["wr128x192_s16_d4_l2", "wr128x128_s16_d4_l2", "wr64x128_s16_d4_l2", "wr64x192_s16_d4_l2", "wr64x256_s16_d4_l2", "wr32x64_s8_d6_l1"]
N_OUTS = [0, 9, 16, 17, 32, 41, 70]
NAN_BITS = 0x7FC1                                          # a NaN in bf16 and in fp16: what the pad columns of x_out / w_out hold


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    _capi.load().mixq_gemm_set_config(-1)
    yield
    _capi.load().mixq_gemm_set_config(-1)


# ---- the float64 restatement -------------------------------------------------------------------------------------------------------
def ulp_bf16(v):
    """Spacing of bfloat16 (8 significand bits) at |v|, for a float64 tensor; the smallest normal exponent below 2^-126."""
    e = torch.floor(torch.log2(torch.clamp(v.abs(), min=2.0 ** -126)))
    return torch.exp2(e - 7)


def ulp_tol(ref):
    """tests/test_gpu_parity.py::ulp_tol restated: 2 fp16 ulp of the reference magnitude, at least 1e-3."""
    a = ref.abs()
    ulp = torch.where(a > 0, torch.exp2(torch.floor(torch.log2(torch.clamp(a, min=6e-5))) - 10), torch.full_like(a, 2.0 ** -24))
    return torch.clamp(2 * ulp, min=1e-3)


def silu64(z):
    return z * torch.sigmoid(z)


def reference(acc, sx, sw, xo, wo, n_out, addend, bias, act):
    """(ref, bound) of the module docstring; acc float64 [M,N] (exact integers), sx [M] / sw [N] / bias [N] fp16, xo [M,>=n] / wo [N,>=n] /
    addend [M,N] in the layer's 16-bit container (or None)."""
    main = acc * sx.to(F64).reshape(-1, 1) * sw.to(F64).reshape(1, -1)
    mag = main.abs()
    z = main.clone()
    if n_out:
        a, b = xo[:, :n_out].to(F64), wo[:, :n_out].to(F64)
        z += a @ b.T
        mag += a.abs() @ b.abs().T
    mul = None
    if addend is not None:
        if act == ACT_SILU_MUL:
            mul = addend.to(F64)
        else:
            z += addend.to(F64)
            mag += addend.to(F64).abs()
    bv = bias.to(F64).reshape(1, -1) if bias is not None else torch.zeros(1, z.shape[1], dtype=F64, device=z.device)
    mag += bv.abs()
    slack = (n_out + 8) * 2.0 ** -24 * mag
    if act == ACT_NONE:
        ref = z + bv
        return ref, ulp_bf16(ref) + slack
    s = silu64(z)
    if act == ACT_SILU:
        ref = s + bv
        return ref, ulp_bf16(ref) + slack + ulp_tol(s)
    ref = (s + bv) * mul
    return ref, ulp_bf16(ref) + slack + ulp_tol(s) * mul.abs()


def check(y, ref, bound, what):
    assert y.dtype == BF, what
    err = (y.to(F64) - ref).abs()
    assert bool(torch.isfinite(y.float()).all()), f"{what}: non-finite y"
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).flatten()))
        m, n = divmod(i, y.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {y.numel()} elements outside the bound; worst at [{m},{n}]: y {float(y[m, n])} ref {float(ref[m, n])} "
                             f"|err| {float(err[m, n]):.6g} bound {float(bound[m, n]):.6g}")
    return float((err / bound).max())


# ---- operands --------------------------------------------------------------------------------------------------------------------
def pack_i4(q):
    """int values in [-8, 7], [R,K] -> nibble-packed uint8 [R,K/2], low nibble = even column."""
    u = torch.where(q < 0, q + 16, q).to(torch.uint8)
    return (u[:, 0::2] | (u[:, 1::2] << 4)).contiguous()


def unpack_i4(p):
    lo, hi = (p & 15).to(torch.int16), (p >> 4).to(torch.int16)
    q = torch.stack([lo, hi], dim=-1).reshape(p.shape[0], -1)
    return torch.where(q > 7, q - 16, q)


class Problem:
    """Operands of one (bit, M, K, N) problem on the device, the packed images the bf16 GEMMs read, and the exact contraction."""

    def __init__(self, bit, M, K, N, seed, dtype=BF):
        g = torch.Generator().manual_seed(seed)
        self.bit, self.M, self.K, self.N, self.dtype = bit, M, K, N, dtype
        if bit == 8:
            qx = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int16)
            qw = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int16)
            self.qx_img = mixlib.PackOperand(qx.to(torch.int8).to(DEV), FMT_P16X64)
            self.qw_img = mixlib.PackOperand(qw.to(torch.int8).to(DEV), FMT_F16X64)
        else:
            qx = torch.randint(-7, 8, (M, K), generator=g, dtype=torch.int16)
            qw = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int16)
            self.qx_img = mixlib.PackOperand(pack_i4(qx).to(DEV), FMT_R6X128)
            self.qw_img = mixlib.PackOperand(pack_i4(qw).to(DEV), FMT_F6X128)
        self.acc = qx.to(DEV).to(F64) @ qw.to(DEV).to(F64).T
        amp = 0.02 if bit == 8 else 0.3
        self.sx = ((torch.rand(M, 1, generator=g) + 0.5) * amp).half().to(DEV)
        self.sw = ((torch.rand(1, N, generator=g) + 0.5) * amp).half().to(DEV)
        self.bias = (torch.randn(N, generator=g) * 3).half().to(DEV)
        self.addend = (torch.randn(M, N, generator=g) * 40).to(dtype).to(DEV)
        self.mul = (torch.randn(M, N, generator=g) * 1.5).to(dtype).to(DEV)
        # outlier operands for up to 80 columns: activation columns up to ~1e5 (fp16 cannot hold them), weights of ordinary size
        xo = torch.randn(M, 80, generator=g) * torch.logspace(1, 5, 80)[torch.randperm(80, generator=g)]
        if dtype == F16:
            xo = xo.clamp(-6e4, 6e4)
        self.xo_vals = xo.to(dtype).to(DEV)
        self.wo_vals = (torch.randn(N, 80, generator=g) * 0.05).to(dtype).to(DEV)

    def outliers(self, n):
        """x_out / w_out [rows, pad16(n)] holding n live columns and NaN patterns in the pad."""
        if n == 0:
            return None, None
        ld = (n + 15) // 16 * 16
        out = []
        for vals in (self.xo_vals, self.wo_vals):
            t = torch.full((vals.shape[0], ld), NAN_BITS, dtype=torch.int16, device=DEV).view(self.dtype)
            t[:, :n] = vals[:, :n]
            out.append(t)
        return out

    def run(self, n, dev_count, act, bias, addend, **kw):
        xo, wo = self.outliers(n)
        ld = 0 if xo is None else xo.shape[1]
        n_dev = torch.tensor([n], dtype=torch.int32, device=DEV) if (dev_count and n) else None
        y = mixlib.FusedLinear(self.qx_img, self.qw_img, self.sx, self.sw, xo, wo, ld if n_dev is not None else n, self.bias if bias else None, self.M, self.N,
                               self.K, bit=self.bit, act=act, n_out_dev=n_dev, addend=addend, dtype=self.dtype, **kw)
        return y, xo, wo


CASES = [(ACT_NONE, False), (ACT_NONE, True), (ACT_SILU, False), (ACT_SILU, True), (ACT_SILU_MUL, True)]   # (act, addend present)


def sweep(p, what):
    worst = 0.0
    for n in N_OUTS:
        for dev_count in (False, True):
            for act, has_add in CASES:
                for bias in (False, True):
                    add = (p.mul if act == ACT_SILU_MUL else p.addend) if has_add else None
                    y, xo, wo = p.run(n, dev_count, act, bias, add)
                    ref, bound = reference(p.acc, p.sx, p.sw, xo, wo, n, add, p.bias if bias else None, act)
                    worst = max(worst, check(y, ref, bound, f"{what} n_out={n} dev_count={dev_count} act={act} addend={has_add} bias={bias}"))
    torch.cuda.synchronize()
    print(f"{what}: worst |err| / bound = {worst:.3f}")


_problems = {}


def problem(bit, M, K, N):
    key = (bit, M, K, N)
    if key not in _problems:
        _problems[key] = Problem(bit, M, K, N, seed=1000 * bit + M + N)
    return _problems[key]


# ---- 1. the epilogue against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit,name", [(8, n) for n in BF16_INT8] + [(4, n) for n in BF16_FP6])
def test_epilogue_of_every_forced_bf16_tiling_against_float64(bit, name):
    """200 x 512 -> 1004: a partial last M tile and a partial last N tile for every tiling (N % 4 == 0, N % 64 != 0) - 1004 % 8 == 4, so y
    leaves as 8-byte pieces; and 200 x 512 -> 1000 (N % 8 == 0): the same partial tiles on the LDS-staged 16-byte panel stores, the path
    every real layer takes."""
    lib = _capi.load()
    names = _capi.gemm_config_names()
    try:
        assert lib.mixq_gemm_set_config(names.index(name)) == 0
        sweep(problem(bit, 200, 512, 1004), f"W{bit} {name}")
        sweep(problem(bit, 200, 512, 1000), f"W{bit} {name} 200x512->1000")
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("M,K,N", [(200, 512, 1004), (24, 512, 260), (300, 1024, 2052), (512, 1024, 4096)])
def test_epilogue_of_the_automatic_pick_against_float64(bit, M, K, N):
    """... and the automatic choice: a mid batch, a small batch of a narrow layer (fp16 would take gemm_skinny.hip: bf16 takes the 32 x 64
    tiling), shapes with partial tiles in both directions and an exact one."""
    assert _capi.load().mixq_gemm_set_config(-1) == 0
    sweep(problem(bit, M, K, N), f"W{bit} auto {M}x{K}->{N}")


def test_an_fp16_detour_could_not_pass():
    """The outlier operands of these tests are outside fp16: the same x_out as float16 is not finite."""
    p = problem(8, 200, 512, 1004)
    assert float(p.xo_vals.float().abs().max()) > 65504 and not bool(torch.isfinite(p.xo_vals.half().float()).all())


def test_mixed_dtypes_are_refused():
    p = problem(8, 200, 512, 1004)
    xo, wo = p.outliers(17)
    for kw in ({"x_out": xo.half()}, {"w_out": wo.half()}, {"addend": p.addend.half()}, {"out": torch.empty(p.M, p.N, dtype=F16, device=DEV)}):
        args = {"x_out": xo, "w_out": wo, "addend": None, "out": None}
        args.update(kw)
        with pytest.raises(RuntimeError, match="must be torch.bfloat16"):
            mixlib.FusedLinear(p.qx_img, p.qw_img, p.sx, p.sw, args["x_out"], args["w_out"], 17, None, p.M, p.N, p.K, addend=args["addend"], out=args["out"],
                               dtype=BF)
    with pytest.raises(RuntimeError, match="must be torch.float16"):                        # ... and the float16 default refuses bf16 tensors
        mixlib.FusedLinear(p.qx_img, p.qw_img, p.sx, p.sw, xo, wo, 17, None, p.M, p.N, p.K)


# ---- 2. the row-maximum side output ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N,masked", [(200, 512, 1024, True), (24, 512, 256, False), (300, 1024, 2048, True)])
def test_row_amax_is_the_maximum_of_the_bf16_bit_patterns_of_y(M, K, N, masked):
    """mixq_gemm_i8_fused_amax_bf16 leaves max_n (bits(y[m,n]) & 0x7fff) over the unmasked columns of the y it wrote, and
    mixq_quant_known_amax_bf16 fed with it writes the bytes mixq_quant_fused_masked_bf16 writes on that y (N is the next layer's K)."""
    p = problem(8, M, K, N)
    assert mixlib.amax_supported(M, N, K, FMT_P16X64, FMT_F16X64, dtype=BF)
    g = torch.Generator().manual_seed(5)
    ind = torch.sort(torch.randperm(N, generator=g)[:23])[0].to(torch.int32).to(DEV) if masked else None
    cm = kept_outlier_map(ind, N) if masked else None
    for act, add in ((ACT_NONE, p.addend), (ACT_SILU_MUL, p.mul), (ACT_SILU, None)):
        ra = torch.zeros(M, dtype=torch.int32, device=DEV)
        y, _, _ = p.run(41, True, act, True, add, row_amax=ra, col_mask=cm)
        bits = y.view(torch.int16).int() & 0x7FFF
        if masked:
            bits[:, ind.long()] = 0
        assert torch.equal(ra, bits.max(dim=1).values.to(torch.int32)), f"act {act}"
        # the same GEMM without the side output writes the same y
        y0, _, _ = p.run(41, True, act, True, add)
        assert torch.equal(y0.view(torch.int16), y.view(torch.int16))
        if not masked:
            continue
        # the next layer's quantise pass: known maxima against the two-pass masked form, on copies of y
        n = ind.numel()
        outs = []
        for known in (True, False):
            x = y.clone()
            xs = torch.zeros(M, 1, dtype=F16, device=DEV)
            xo = torch.zeros(M, (n + 15) // 16 * 16, dtype=BF, device=DEV)
            q = torch.zeros(mixlib.packed_rows(M), N, dtype=torch.int8, device=DEV)
            if known:
                _capi.call("mixq_quant_known_amax_bf16", x.data_ptr(), ind.data_ptr(), n, None, ra.data_ptr(), cm.data_ptr(), cm.numel(), xs.data_ptr(),
                           q.data_ptr(), xo.data_ptr(), None, M, N, x.stride(0), xo.stride(0), 8, 6.0, FMT_P16X64, mixlib._stream())
                assert int(ra.abs().max()) == 0                                            # cleared for the producer's next run
            else:
                _capi.call("mixq_quant_fused_masked_bf16", x.data_ptr(), ind.data_ptr(), n, None, cm.data_ptr(), cm.numel(), xs.data_ptr(), q.data_ptr(),
                           xo.data_ptr(), None, M, N, x.stride(0), xo.stride(0), 8, 6.0, FMT_P16X64, mixlib._stream())
            outs.append((q, xs, xo.view(torch.int16), x.view(torch.int16)))
        for a, b in zip(*outs):
            assert torch.equal(a, b)


# ---- 3. one call = two calls -----------------------------------------------------------------------------------------------------
def _make_x(M, K, cols, seed, big=6.0e4):
    """bf16 activations: inliers of ordinary size, the outlier columns `cols` with values up to `big` times larger."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 0.8
    for i, c in enumerate(cols):
        x[:, c] *= big / (1 + 3 * (i % 4))
    return x.to(BF)


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("kept", [False, True])
def test_linear_forward_bf16_is_its_two_calls(bit, kept):
    M, K, N = 200, 512, 1004
    p = problem(bit, M, K, N)
    cols = [5, 77, 130, 131, 300, 511, 64, 2, 400]
    n, ldo = len(cols), 16
    ind = torch.zeros(ldo, dtype=torch.int32, device=DEV)
    ind[:n] = torch.tensor(cols, dtype=torch.int32)
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    cm = kept_outlier_map(ind[:n], K) if kept else None
    x0 = _make_x(M, K, cols, 3).to(DEV)
    _, wo = p.outliers(n)
    qfmt, wfmt = (FMT_P16X64, FMT_F16X64) if bit == 8 else (FMT_R6X128, FMT_F6X128)
    layout = (_capi.X_PACKED | _capi.W_F16X64) if bit == 8 else _capi.XW_F6X128
    rows = mixlib.packed_rows(M)

    def buffers():
        return (x0.clone(), torch.zeros(M, 1, dtype=F16, device=DEV), torch.zeros(rows, mixlib._q_row_bytes(K, bit, qfmt), dtype=torch.uint8, device=DEV),
                torch.zeros(M, ldo, dtype=BF, device=DEV), torch.zeros(M, N, dtype=BF, device=DEV))

    # two calls
    x, xs, q, xo, y = buffers()
    if kept:
        _capi.call("mixq_quant_fused_masked_bf16", x.data_ptr(), ind.data_ptr(), ldo, n_dev.data_ptr(), cm.data_ptr(), cm.numel(), xs.data_ptr(), q.data_ptr(),
                   xo.data_ptr(), None, M, K, K, ldo, bit, 6.0, qfmt, mixlib._stream())
    else:
        _capi.call("mixq_quant_fused_bf16", x.data_ptr(), ind.data_ptr(), ldo, n_dev.data_ptr(), xs.data_ptr(), q.data_ptr(), xo.data_ptr(), None, M, K, K,
                   ldo, bit, 6.0, qfmt, mixlib._stream())
    _capi.call("mixq_gemm_i8_fused_bf16" if bit == 8 else "mixq_gemm_i4_fused_bf16", q.data_ptr(), p.qw_img.data_ptr(), xs.data_ptr(), p.sw.data_ptr(),
               xo.data_ptr(), ldo, wo.data_ptr(), wo.stride(0), ldo, n_dev.data_ptr(), None, 0, p.bias.data_ptr(), y.data_ptr(), N, M, N, K, ACT_NONE, layout,
               mixlib._stream())
    two = [t.clone() for t in (x, xs, q, xo, y)]
    # one call
    x, xs, q, xo, y = buffers()
    a = _capi.LinearArgs()
    a.x, a.ldx, a.ind, a.n_cap, a.n_dev = x.data_ptr(), K, ind.data_ptr(), ldo, n_dev.data_ptr()
    a.x_scale, a.q_x, a.x_out, a.ldxo = xs.data_ptr(), q.data_ptr(), xo.data_ptr(), ldo
    a.q_w, a.scale_col, a.w_out, a.ldwo, a.bias = p.qw_img.data_ptr(), p.sw.data_ptr(), wo.data_ptr(), wo.stride(0), p.bias.data_ptr()
    a.y, a.ldy, a.M, a.N, a.K, a.bit, a.sigma, a.act, a.qfmt, a.wfmt = y.data_ptr(), N, M, N, K, bit, 6.0, ACT_NONE, qfmt, wfmt
    if kept:
        a.col_mask, a.col_mask_words = cm.data_ptr(), cm.numel()
    _capi.call("mixq_linear_forward_bf16", C.byref(a), mixlib._stream())
    torch.cuda.synchronize()
    for name, t2, t1 in zip(("x", "x_scale", "q_x", "x_out", "y"), two, (x, xs, q, xo, y)):
        assert torch.equal(t2.view(torch.uint8), t1.view(torch.uint8)), name
    assert bool((xo.float().abs() > 65504).any())                # values float16 could not hold went through
    assert torch.equal(xo[:, :n].view(torch.int16), x0[:, cols].view(torch.int16))


# ---- 4. the layer ------------------------------------------------------------------------------------------------------------------
def _quantise64(x, ind, bit):
    """The quantise pass restated (include/mixq_hip.h, "bfloat16 activations"): x_scale = fp16(max |x| / qmax) over the non-outlier columns
    (fp32 divide), q = clamp(rint_half_even(float(x) / float(x_scale)))."""
    qmax = 127.0 if bit == 8 else 7.0
    xf = x.float().clone()
    if ind.numel():
        xf[:, ind.long()] = 0
    s = (xf.abs().max(dim=1, keepdim=True).values / qmax).half()
    q = torch.where(s.float() > 0, torch.round(xf / s.float()), torch.zeros_like(xf)).clamp(-qmax, qmax)
    return q.to(F64), s


def _layer_reference(layer, x, bit):
    """(ref, bound) of a bf16 layer's output on x from the layer's own state: q_weight, scale_col, ind, bias and the bf16 image of weight_cache."""
    ind = layer.ind
    n = int(ind.numel())
    q, s = _quantise64(x, ind, bit)
    qw = layer.q_weight
    qw = qw.to(F64) if bit == 8 else unpack_i4(qw).to(F64)
    wo = layer.weight_cache.to(BF) if n else None                 # RNE_bf16(weight_cache): one rounding of the fp16 buffer
    xo = x[:, ind.long()] if n else None
    return reference(q @ qw.T, s.reshape(-1), layer.scale_col.reshape(-1), xo, wo, n, None, layer.bias, ACT_NONE)


def _state_layout(layer):
    return {k: (tuple(v.shape), v.dtype) for k, v in layer.state_dict().items()}


def _run_layer(dtype, bit, K, N, M, bias, cols1, col2, check_against_reference):
    """The life of a layer: search phase (a new outlier column at call 2), freeze, two-call and one-call routes, hipGraph replay.
    Returns (layer, the frozen outputs' bytes)."""
    torch.manual_seed(11)
    lin = torch.nn.Linear(K, N, bias=bias).to(dtype)
    cache = MixLibCache(M, bit=bit, device=DEV, config=MixqConfig(act_dtype=dtype))
    kw = {}
    if bit == 4:
        # a 4-bit layer is built with its 128 static 16-bit columns (cols1 among them) and stops searching once it holds more than 128:
        # col2 is the one column it finds online
        rest = [c for c in torch.randperm(K, generator=torch.Generator().manual_seed(2)).tolist() if c not in cols1 + [col2]]
        ls = torch.ones(K)
        ls[cols1 + rest[:128 - len(cols1)]] = 20.0
        kw["layer_scales"] = ls
    layer = MixLinear_GEMM.from_linear(lin, bit, cache=cache, dev=DEV, **kw)
    assert layer.act_dtype is dtype and layer.scale_col.dtype == F16 and (layer.bias is None or layer.bias.dtype == F16)
    big = 6.0e4 if dtype == BF else 40.0
    n0 = int(layer.ind.numel())
    xs = [_make_x(M, K, cols1, 1, big), _make_x(M, K, cols1 + [col2], 2, big), _make_x(M, K, cols1 + [col2], 3, big), _make_x(M, K, cols1 + [col2], 4, big)]
    xs = [t.to(dtype).to(DEV) for t in xs]
    outs = []
    for call in range(3):
        x = xs[call].clone()
        y = layer(x, None, True)
        torch.cuda.synchronize()
        assert y.dtype == dtype and tuple(y.shape) == (M, N)
        want = n0 + (len(cols1) if bit == 8 else 0) + (1 if call >= 1 else 0)
        assert int(layer.ind.numel()) == want, (call, layer.ind.numel())
        if call == 1:
            assert col2 in layer.ind.tolist()
        if layer.weight_cache is not None:
            assert layer.weight_cache.dtype == F16                                        # the buffer (and the checkpoint) stay float16
            if dtype == BF:
                wo = layer._wo_ready
                assert wo.dtype == BF and torch.equal(wo.view(torch.int16), layer.weight_cache.to(BF).view(torch.int16))   # ... its image is rebuilt with it
        if check_against_reference:
            ref, bound = _layer_reference(layer, xs[call], bit)
            check(y, ref, bound, f"W{bit} layer {M}x{K}->{N} call {call}")
        outs.append(y)
    assert layer.add_outliers is False
    # frozen: the two-call route, then the one-call route, same bytes
    x3 = xs[3]
    layer.config.one_call_forward = False
    y_two = layer(x3.clone(), None, True)
    layer.config.one_call_forward = True
    y_one = layer(x3.clone(), None, True)
    torch.cuda.synchronize()
    assert layer._plan is not None and y_one.dtype == dtype
    assert torch.equal(y_two.view(torch.int16), y_one.view(torch.int16))
    if check_against_reference:
        ref, bound = _layer_reference(layer, x3, bit)
        check(y_one, ref, bound, f"W{bit} layer {M}x{K}->{N} frozen")
    # the frozen layer refuses the other container
    other = F16 if dtype == BF else BF
    with pytest.raises(RuntimeError, match="bfloat16" if dtype == BF else "float16"):
        layer(x3.clone().to(other), None, True)
    # hipGraph: captured once on a side stream, replayed three times on restored inputs (the forward zeroes x's outlier columns in place)
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
        for _ in range(3):
            xg.copy_(x3)
            yg.zero_()
            g.replay()
            side.synchronize()
            assert torch.equal(yg.view(torch.int16), y_one.view(torch.int16))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return layer, y_one.view(torch.int16).clone(), g


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("bias", [False, True])
def test_bf16_layer_end_to_end(bit, bias):
    M, K, N = 192, 512, 256
    layer, _, g = _run_layer(BF, bit, K, N, M, bias, [3, 200, 411], 77, True)
    # state_dict: keys, shapes and dtypes of an fp16 layer of the same shape and history
    layer16, _, g16 = _run_layer(F16, bit, K, N, M, bias, [3, 200, 411], 77, False)
    assert _state_layout(layer) == _state_layout(layer16)
    del g, g16


@pytest.mark.parametrize("bit", [8, 4])
def test_bf16_layer_at_the_llama_shape(bit):
    layer, _, g = _run_layer(BF, bit, 4096, 11008, 512, True, [3, 200, 411, 4000], 1777, True)
    del g


# ---- 5. fp16 untouched -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [8, 4])
def test_an_fp16_layer_gives_the_same_bytes_before_and_after_a_bf16_layer_ran(bit):
    M, K, N = 192, 512, 256
    before, y_before, g0 = _run_layer(F16, bit, K, N, M, True, [3, 200, 411], 77, False)
    x = _make_x(M, K, [3, 200, 411, 77], 9, 40.0).half().to(DEV)
    y_kept = before(x.clone(), None, True).view(torch.int16).clone()
    _, _, g1 = _run_layer(BF, bit, K, N, M, True, [3, 200, 411], 77, False)
    after, y_after, g2 = _run_layer(F16, bit, K, N, M, True, [3, 200, 411], 77, False)
    assert torch.equal(y_before, y_after)                          # a fresh fp16 layer: the same bytes
    assert torch.equal(before(x.clone(), None, True).view(torch.int16), y_kept)     # ... and the one that lived through it (kept plan, derived operands)
    assert before._wo_ready.dtype == F16 and before._plan.dtype == F16
    del g0, g1, g2
