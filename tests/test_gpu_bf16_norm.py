"""bfloat16 RMSNorm on the MI355X: mixq_rmsnorm_bf16 against the numpy float32 restatement of its contract (tests/bf16_norm_ref.py) bit for
bit, the fused norm + extract + quantise forms against the plain norm followed by mixq_quant_fused_bf16 byte for byte (every bit width,
every output format, with and without the kept outlier map), every store inside guard frames, and the modules a bfloat16 model reaches
with MixqConfig(act_dtype=torch.bfloat16, fused_bf16=True): FasterTransformerRMSNorm -> MixLlamaMLP(x, residual=r).

Shapes (the smallest that reach every dispatch arm and every partial case): M in {1, 17, 48}; K in {128, 4096, 4224, 11008, 28672} - 2, 2
(full), 4 (sparse), 8 and 16 chunks per thread, all multiples of 128; outlier counts n in {0, 1, 41, 130, 300}; a device-resident live
count below the capacity; a kept map built for another count (the fallback).  Every third row of x is scaled by 2^20, every third by 2^40:
magnitudes float16 cannot hold.  The restatement is computed once per K for 48 rows; smaller batches are its first rows (rows are
independent).

The module test compares each GEMM output with a float64 restatement over the operands the kernels actually read (the quantised image,
x_scale and outlier columns the cache holds, the layers' weights); the bound is the derived one of tests/test_gpu_bf16_gemm.py, restated:
    |y - ref| <= ulp_bf16(ref) + (n_out + 8) * 2^-24 * (|acc sx sw| + sum_j |xo wo| + |addend| + |bias|)
one bf16 ulp (the half-ulp rounding and a flip at a tie) plus the fp32 accumulation slack; with SiLU the project's allowance for mixq_silu
against a float64 SiLU is added (tests/test_gpu_parity.py::ulp_tol: two fp16 ulp of |silu(z)|, at least 1e-3), times |mul| for
MIXQ_ACT_SILU_MUL."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_norm_ref as R  # noqa: E402
from frames import Frame  # noqa: E402
from mixq_amd import FasterTransformerRMSNorm, MixLibCache, MixLinear_GEMM, MixLlamaMLP, _capi, mixlib  # noqa: E402
from mixq_amd._capi import ACT_NONE, ACT_SILU_MUL, FMT_F16X64, FMT_F6X128, FMT_P16X64, FMT_PLAIN, FMT_R6X128  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402
from mixq_amd.linear import kept_outlier_map  # noqa: E402

DEV = "cuda"
BF, F16, F64 = torch.bfloat16, torch.float16, torch.float64
EPS = 1e-5
MS = (1, 17, 48)
KS = (128, 4096, 4224, 11008, 28672)
NS = (0, 1, 41, 130, 300)
FORMATS = [(8, FMT_PLAIN), (8, FMT_P16X64), (8, FMT_F16X64), (4, FMT_PLAIN), (4, FMT_P16X64), (4, FMT_F6X128), (4, FMT_R6X128)]
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    yield


def _dev_bits(a):
    """numpy uint16 patterns -> a bfloat16 tensor on the device."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV).view(BF)


def _np_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _big_cols(K):
    return [1, K // 2 + 3, K - 2]


_data = {}


def data(K):
    """(x bits [48,K], w bits [K], expected y bits [48,K], x / w on the device): computed once per K."""
    if K not in _data:
        rng = np.random.default_rng(K)
        x = rng.standard_normal((max(MS), K)).astype(np.float32)
        x[:, _big_cols(K)] *= 30                                            # three outlier columns
        x *= (2.0 ** (20 * (np.arange(max(MS)) % 3)))[:, None].astype(np.float32)      # rows at 1, 2^20, 2^40
        xb = R.f32_to_bf16_bits(x)
        wb = R.f32_to_bf16_bits((0.5 + rng.random(K)).astype(np.float32))
        assert np.abs(R.bf16_bits_to_f32(xb)).max() >= 2.0 ** 40
        _data[K] = (xb, wb, R.rmsnorm_bf16(xb, wb, EPS), _dev_bits(xb), _dev_bits(wb))
    return _data[K]


def indices(K, n):
    """n distinct columns, unsorted: the outlier columns of the data first, then others."""
    rng = np.random.default_rng(1000 * n + K)
    big = _big_cols(K)
    rest = [c for c in rng.permutation(K).tolist() if c not in big]
    return (big + rest)[:n]


def _stream():
    return mixlib._stream()


def plain_norm(K, M):
    xb, wb, yb, x, w = data(K)
    out = torch.full((M, K), 0x7FC1, dtype=torch.int16, device=DEV).view(BF)
    _capi.call("mixq_rmsnorm_bf16", x.data_ptr(), w.data_ptr(), out.data_ptr(), M, K, K, K, EPS, _stream())
    return out


# ---- 1. the plain norm against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_plain_norm_equals_the_restatement_bit_for_bit(K):
    xb, wb, yb, x, w = data(K)
    for M in MS:
        got = _np_bits(plain_norm(K, M))
        bad = got != yb[:M]
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError(f"K={K} M={M}: {int(bad.sum())} of {got.size} elements differ; first at [{r},{c}]: got {got[r, c]:#06x} want {yb[r, c]:#06x} "
                                 f"(x {xb[r, c]:#06x} w {wb[c]:#06x})")
    # ... and through the Python surface: the suffix comes from x's dtype, x_out / out follow it, another dtype is refused by name
    out = torch.empty((max(MS), K), dtype=BF, device=DEV)
    mixlib.layernorm_forward_cuda(x, w, out, EPS)
    assert np.array_equal(_np_bits(out), yb)
    with pytest.raises(RuntimeError, match="weight must be torch.bfloat16 like x"):
        mixlib.layernorm_forward_cuda(x, w.half(), out, EPS)
    with pytest.raises(RuntimeError, match="out must be torch.bfloat16 like x"):
        mixlib.layernorm_forward_cuda(x, w, out.half(), EPS)


# ---- 2. the fused forms against plain norm + mixq_quant_fused_bf16 -------------------------------------------------------------------
def _cases(K):
    """(n, capacity, live count on the device or None, count the kept map is built for) of every outlier configuration at this K."""
    out = []
    for n in NS:
        if n >= K:
            continue
        out.append((n, n, None, n))
        if n == 41:
            out.append((41, 48, 41, 41))                                     # a device-resident live count below the capacity
            out.append((41, 48, 30, 41))                                     # ... lowered behind the map's back: the map is for another count (fallback)
    return out


def _buffers(M, K, bit, fmt, ldo):
    rows = mixlib.packed_rows(M) if fmt else M
    return {"xs": torch.full((M + 3,), 0x1234, dtype=torch.int16, device=DEV).view(F16),
            "q": torch.full((rows, mixlib._q_row_bytes(K, bit, fmt)), FILL, dtype=torch.uint8, device=DEV),
            "xo": torch.full((M, max(ldo, 1)), 0x7FC1, dtype=torch.int16, device=DEV).view(BF),
            "flag": torch.zeros(1, dtype=torch.int32, device=DEV)}


def _same(what, a, b):
    for name in a:
        if not torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)):
            d = (a[name].view(torch.uint8) != b[name].view(torch.uint8))
            raise AssertionError(f"{what}: {name} differs in {int(d.sum())} of {d.numel()} bytes; first at flat byte {int(torch.nonzero(d.flatten())[0])}")


def run_reference(K, M, bit, fmt, ind, cap, n_dev, ldo):
    """What the fused norm must equal: the plain norm's output, then mixq_quant_fused_bf16 on a copy of it (which zeroes the columns in place)."""
    b = _buffers(M, K, bit, fmt, ldo)
    b["out"] = plain_norm(K, M).clone()
    _capi.call("mixq_quant_fused_bf16", b["out"].data_ptr(), None if ind is None else ind.data_ptr(), cap, None if n_dev is None else n_dev.data_ptr(),
               b["xs"].data_ptr(), b["q"].data_ptr(), b["xo"].data_ptr() if cap else None, b["flag"].data_ptr(), M, K, K, ldo, bit, 6.0, fmt, _stream())
    return b


def run_fused(K, M, bit, fmt, ind, cap, n_dev, ldo, cmap=None, bufs=None, x=None, ldx=None, ldout=None):
    _, _, _, xd, w = data(K)
    b = bufs if bufs is not None else _buffers(M, K, bit, fmt, ldo)
    if "out" not in b:
        b["out"] = torch.full((M, K), 0x7FC1, dtype=torch.int16, device=DEV).view(BF)
    x = xd if x is None else x
    head = (x.data_ptr(), w.data_ptr(), b["out"].data_ptr(), None if ind is None else ind.data_ptr(), cap, None if n_dev is None else n_dev.data_ptr())
    tail = (b["xs"].data_ptr(), b["q"].data_ptr(), b["xo"].data_ptr() if cap else None, b["flag"].data_ptr(), M, K, K if ldx is None else ldx,
            K if ldout is None else ldout, ldo, EPS, bit, 6.0, fmt, _stream())
    if cmap is not None:
        _capi.call("mixq_rmsnorm_quant_fused_masked_bf16", *head, cmap.data_ptr(), cmap.numel(), *tail)
    else:
        _capi.call("mixq_rmsnorm_quant_fused_bf16", *head, *tail)
    return b


_flags_seen = set()


@pytest.mark.parametrize("bit,fmt", FORMATS)
@pytest.mark.parametrize("K", KS)
def test_fused_norm_equals_plain_norm_then_quant_fused(K, bit, fmt):
    for n, cap, live, map_n in _cases(K):
        cols = indices(K, n)
        ind = n_dev = cmap = None
        ldo = 0
        if n:
            ind = torch.zeros(cap, dtype=torch.int32, device=DEV)
            ind[:n] = torch.tensor(cols, dtype=torch.int32)
            ldo = (cap + 15) // 16 * 16
            cmap = kept_outlier_map(ind[:map_n], K)
            if live is not None:
                n_dev = torch.tensor([live], dtype=torch.int32, device=DEV)
        for M in MS:
            what = f"K={K} M={M} bit={bit} fmt={fmt} n={n} cap={cap} live={live}"
            ref = run_reference(K, M, bit, fmt, ind, cap, n_dev, ldo)
            got = run_fused(K, M, bit, fmt, ind, cap, n_dev, ldo)
            _same(what, ref, got)
            _flags_seen.add(int(got["flag"].item()))
            if n:
                masked = run_fused(K, M, bit, fmt, ind, cap, n_dev, ldo, cmap=cmap)
                _same(what + " masked", got, masked)
                live_n = n if live is None else live
                assert bool((got["xo"][:, live_n:].view(torch.int16) == 0).all()), what + ": pad columns of x_out are zero"
                want = torch.from_numpy(data(K)[2][:M][:, cols[:live_n]].view(np.int16)).to(DEV)
                assert torch.equal(got["xo"][:, :live_n].view(torch.int16), want), what + ": x_out holds the normalised outlier columns"
                assert bool((got["out"][:, torch.tensor(cols[:live_n], device=DEV)].view(torch.int16) == 0).all()), what
    torch.cuda.synchronize()


def test_the_misprediction_flag_was_seen_both_ways():
    """(after the sweep above) rows whose outlier columns were not all extracted raise the flag, rows with all three extracted do not."""
    if not _flags_seen:
        test_fused_norm_equals_plain_norm_then_quant_fused(128, 8, FMT_PLAIN)
    assert _flags_seen == {0, 1}, _flags_seen


def test_the_python_surface_runs_the_bf16_twins():
    K, M, n = 4224, 17, 41
    xb, wb, yb, x, w = data(K)
    ind = torch.tensor(indices(K, n), dtype=torch.int32, device=DEV)
    xs = torch.zeros((M, 1), dtype=F16, device=DEV)
    out = torch.empty((M, K), dtype=BF, device=DEV)
    ref = run_reference(K, M, 8, FMT_P16X64, ind, n, None, 48)
    for cm in (None, kept_outlier_map(ind, K)):
        q, xo = mixlib.RMSNormQuantFused(x[:M], w, out, EPS, ind, xs, 8, fmt=FMT_P16X64, col_mask=cm)
        assert xo.dtype == BF and tuple(xo.shape) == (M, n) and mixlib.fmt_of(q) == FMT_P16X64
        assert torch.equal(out.view(torch.int16), ref["out"].view(torch.int16)) and torch.equal(xo.view(torch.int16), ref["xo"][:, :n].view(torch.int16))
        assert torch.equal(xs.reshape(-1).view(torch.int16), ref["xs"][:M].view(torch.int16))
        assert torch.equal(mixlib.UnpackOperand(q, M), mixlib.UnpackOperand(mixlib.set_fmt(ref["q"].view(torch.int8), FMT_P16X64), M))
    xo8, q8 = mixlib.layernorm_forward_cuda_extract_outliers(x[:M], w, out, EPS, None, xs)
    assert xo8.dtype == BF and tuple(xo8.shape) == (M, 0)
    with pytest.raises(RuntimeError, match="weight must be torch.bfloat16 like x"):
        mixlib.RMSNormQuantFused(x[:M], w.half(), out, EPS, ind, xs, 8)
    with pytest.raises(RuntimeError, match="out must be torch.bfloat16 like x"):
        mixlib.RMSNormQuantFused(x[:M], w, out.half(), EPS, ind, xs, 8)


# ---- 3. every store inside its window ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit,fmt", [(8, FMT_PLAIN), (8, FMT_P16X64), (4, FMT_PLAIN), (4, FMT_R6X128)])
@pytest.mark.parametrize("masked", [False, True])
def test_stores_stay_inside_strided_offset_guard_framed_windows(bit, fmt, masked):
    M, n = 17, 41
    for K in (128, 4224):
        _, _, _, xd, w = data(K)
        cols = indices(K, n)
        ind = torch.tensor(cols, dtype=torch.int32, device=DEV)
        cmap = kept_outlier_map(ind, K) if masked else None
        ldo = 43                                                             # an odd row length of x_out: 2-byte stores, any alignment
        want = run_fused(K, M, bit, fmt, ind, n, None, ldo, cmap=cmap)
        rows = mixlib.packed_rows(M) if fmt else M
        qbytes = rows * mixlib._q_row_bytes(K, bit, fmt)
        # the input in a strided window too (ldx > K): it must not change
        fx = Frame(M, K, K + 8, 0, 8, BF, DEV, guard_rows=2)
        fx.view.copy_(xd[:M])
        fx.freeze()
        fo = Frame(M, K, K + 24, 8, 16, BF, DEV, guard_rows=2)               # out: a column slice of a wider buffer, 16-byte aligned rows
        fxo = Frame(M, ldo, ldo, 0, 1, BF, DEV, guard_rows=2)
        fs = Frame(1, M, M, 0, 3, F16, DEV, guard_rows=1)
        fq = Frame(1, qbytes, qbytes, 0, 16, torch.uint8, DEV, guard_rows=1)
        fq.view.fill_(FILL)
        fq.freeze()
        bufs = {"out": fo.view, "xo": fxo.view, "xs": fs.view, "q": fq.view, "flag": torch.zeros(1, dtype=torch.int32, device=DEV)}
        run_fused(K, M, bit, fmt, ind, n, None, ldo, cmap=cmap, bufs=bufs, x=fx.view, ldx=K + 8, ldout=K + 24)
        torch.cuda.synchronize()
        what = f"K={K} bit={bit} fmt={fmt} masked={masked}"
        for name, f in (("out", fo), ("x_out", fxo), ("x_scale", fs), ("q", fq)):
            f.assert_untouched(f"{what}: {name}")
        fx.assert_unchanged(f"{what}: x")
        assert torch.equal(fo.view.view(torch.int16), want["out"].view(torch.int16)), what
        assert torch.equal(fxo.view.view(torch.int16), want["xo"].view(torch.int16)), what
        assert torch.equal(fs.view.reshape(-1).view(torch.int16), want["xs"][:M].view(torch.int16)), what
        assert torch.equal(fq.view.reshape(-1), want["q"].reshape(-1)), what
        # the plain norm: strided input, framed output
        fo.reset()
        _capi.call("mixq_rmsnorm_bf16", fx.view.data_ptr(), w.data_ptr(), fo.view.data_ptr(), M, K, K + 8, K + 24, EPS, _stream())
        torch.cuda.synchronize()
        fo.assert_untouched(f"{what}: plain norm out")
        assert np.array_equal(_np_bits(fo.view), data(K)[2][:M])


# ---- 4. the modules ---------------------------------------------------------------------------------------------------------------
def ulp_bf16(v):
    e = torch.floor(torch.log2(torch.clamp(v.abs(), min=2.0 ** -126)))
    return torch.exp2(e - 7)


def ulp_tol(ref):
    """tests/test_gpu_parity.py::ulp_tol restated: 2 fp16 ulp of the reference magnitude, at least 1e-3."""
    a = ref.abs()
    ulp = torch.where(a > 0, torch.exp2(torch.floor(torch.log2(torch.clamp(a, min=6e-5))) - 10), torch.full_like(a, 2.0 ** -24))
    return torch.clamp(2 * ulp, min=1e-3)


def reference(acc, sx, sw, xo, wo, n_out, addend, bias, act):
    """(ref, bound) of the module docstring, all float64; act: ACT_NONE (addend added) or ACT_SILU_MUL (the slot carries the multiplier)."""
    main = acc * sx.to(F64).reshape(-1, 1) * sw.to(F64).reshape(1, -1)
    mag = main.abs()
    z = main.clone()
    if n_out:
        a, b = xo[:, :n_out].to(F64), wo[:, :n_out].to(F64)
        z += a @ b.T
        mag += a.abs() @ b.abs().T
    bv = bias.to(F64).reshape(1, -1) if bias is not None else torch.zeros(1, z.shape[1], dtype=F64, device=z.device)
    mag += bv.abs()
    if act == ACT_NONE:
        if addend is not None:
            z += addend.to(F64)
            mag += addend.to(F64).abs()
        ref = z + bv
        return ref, ulp_bf16(ref) + (n_out + 8) * 2.0 ** -24 * mag
    assert act == ACT_SILU_MUL
    mul = addend.to(F64)
    s = z * torch.sigmoid(z)
    ref = (s + bv) * mul
    return ref, ulp_bf16(ref) + (n_out + 8) * 2.0 ** -24 * mag + ulp_tol(s) * mul.abs()


def check(y, ref, bound, what):
    assert y.dtype == BF, what
    assert bool(torch.isfinite(y.float()).all()), f"{what}: non-finite y"
    err = (y.to(F64) - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).flatten()))
        m, c = divmod(i, y.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {y.numel()} elements outside the bound; worst at [{m},{c}]: y {float(y[m, c])} ref {float(ref[m, c])} "
                             f"|err| {float(err[m, c]):.6g} bound {float(bound[m, c]):.6g}")
    return float((err / bound).max())


def unpack_i4(p):
    lo, hi = (p & 15).to(torch.int16), (p >> 4).to(torch.int16)
    q = torch.stack([lo, hi], dim=-1).reshape(p.shape[0], -1)
    return torch.where(q > 7, q - 16, q)


def _ints(q_image, M, bit):
    """The integers of a quantised activation image, float64 [M, K]."""
    plain = mixlib.UnpackOperand(q_image, M) if mixlib.fmt_of(q_image) != FMT_PLAIN else q_image[:M]
    return plain.to(F64) if bit == 8 else unpack_i4(plain).to(F64)


def _weights(layer, bit):
    qw = layer.q_weight
    return qw.to(F64) if bit == 8 else unpack_i4(qw).to(F64)


def _gemm_reference(layer, bit, q_image, sx, xo, M, addend, act):
    n = int(layer.ind.numel())
    wo = layer.weight_cache.to(BF) if n else None                    # RNE_bf16(weight_cache): what the bf16 tail reads
    if n:
        assert xo is not None and xo.shape[1] == n and xo.dtype == BF
    acc = _ints(q_image, M, bit) @ _weights(layer, bit).T
    return reference(acc, sx.reshape(-1), layer.scale_col.reshape(-1), xo, wo, n, addend, layer.bias, act)


def _make_x(M, K, cols, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 0.8
    for i, c in enumerate(cols):
        x[:, c] *= 60.0 / (1 + (i % 3))
    if dtype == BF:
        x *= (2.0 ** (20 * (torch.arange(M) % 3))).reshape(-1, 1)        # rows at 1, 2^20, 2^40: beyond float16
    return x.to(dtype)


def run_chain(dtype, bit, check_reference):
    """The life of norm -> MixLlamaMLP(x, residual=r) at M = 48, 4096 -> 512 -> 4096: search phase (a new outlier column at call 1), the frozen
    state, fuse_down_amax on and off, one hipGraph replay.  Returns the frozen output's bits."""
    M, H, I = 48, 4096, 512
    cols1, col2 = [3, 200, 411, 4000], 1777
    torch.manual_seed(5)
    cfg = MixqConfig(act_dtype=dtype, fused_bf16=(dtype == BF))
    cache = MixLibCache(M, bit=bit, device=DEV, config=cfg)

    boost = [5, 100, 300]        # output channels of up_proj / gate_proj that are 12 times larger: down_proj's outlier columns (nothing else of
                                 # silu(gate) * up comes near sigma = 6 with these weights)

    def make(k, n_, static):
        lin = torch.nn.Linear(k, n_, bias=True)
        if n_ == I:
            lin.weight.data[boost] *= 12.0
        kw = {}
        if bit == 4:
            rest = [c for c in torch.randperm(k, generator=torch.Generator().manual_seed(2)).tolist() if c not in static + [col2]]
            ls = torch.ones(k)
            ls[static + rest[:128 - len(static)]] = 20.0
            kw["layer_scales"] = ls
        return MixLinear_GEMM.from_linear(lin.to(dtype), bit, cache=cache, dev=DEV, **kw)
    up, gate, down = make(H, I, cols1), make(H, I, cols1), make(I, H, boost)
    wn = (torch.rand(H) + 0.5).to(dtype).to(DEV)
    norm = FasterTransformerRMSNorm(wn, EPS, cache)
    assert norm.weight.dtype == dtype
    norm.next_layer = up
    mlp = MixLlamaMLP(gate, down, up, cache)
    r = (torch.randn(M, H, generator=torch.Generator().manual_seed(9)) * 3).to(dtype).to(DEV)
    xs = [_make_x(M, H, cols1 if i == 0 else cols1 + [col2], 20 + i, dtype).to(DEV) for i in range(4)]

    snap = {}

    def up_hook(mod, args, out):                                       # what up_proj's (and gate_proj's) GEMM read: kept before down_proj refills the cache
        xo = cache.activation_outliers
        snap.update(q=cache.q_xcache, sx=cache.x_scale[:M].clone(), xo=None if xo is None else xo.clone(), up=out.clone())
    hook = up.register_forward_hook(up_hook)
    silu = gate.forward_without_preconditionFusedSilu

    def silu_recorded(*a, **k):
        out = silu(*a, **k)
        # (a copy: down_proj's quantise pass zeroes its outlier columns in the tensor it is handed)
        snap.update(gate=out.clone(), handed_over=hasattr(out, "_mixq_row_amax"), asked=("amax_for" in k))
        return out
    gate.forward_without_preconditionFusedSilu = silu_recorded

    def forward(x):
        n_before = [int(v) for v in up.ind.tolist()]
        hidden = norm(x)
        if dtype == BF:
            # the norm itself, through the module: the restatement's bits with the next layer's known columns zeroed, x_out those columns
            yb = R.rmsnorm_bf16(_np_bits(x), _np_bits(wn.reshape(1, -1))[0], EPS)
            want = yb.copy()
            want[:, n_before] = 0
            assert np.array_equal(_np_bits(hidden), want), "norm output"
            if n_before:
                assert np.array_equal(_np_bits(cache.activation_outliers), yb[:, n_before]), "norm x_out"
        y = mlp(hidden, residual=r)
        torch.cuda.synchronize()
        return y

    def verify(y, what):
        assert y.dtype == dtype and tuple(y.shape) == (M, H)
        if not check_reference:
            return
        ref, bound = _gemm_reference(up, bit, snap["q"], snap["sx"], snap["xo"], M, None, ACT_NONE)
        w1 = check(snap["up"], ref, bound, f"{what}: up_proj")
        ref, bound = _gemm_reference(gate, bit, snap["q"], snap["sx"], snap["xo"], M, snap["up"], ACT_SILU_MUL)
        w2 = check(snap["gate"], ref, bound, f"{what}: gate_proj (SiLU and multiply)")
        xo = cache.activation_outliers if int(down.ind.numel()) else None
        ref, bound = _gemm_reference(down, bit, cache.q_xcache, cache.x_scale[:M], xo, M, r, ACT_NONE)
        w3 = check(y, ref, bound, f"{what}: down_proj + residual")
        print(f"{what}: worst |err| / bound  up {w1:.3f}  gate {w2:.3f}  down {w3:.3f}  (outlier columns up {up.ind.numel()} down {down.ind.numel()})")

    static = 128 if bit == 4 else 0
    for call in range(3):
        y = forward(xs[call].clone())
        verify(y, f"W{bit} {dtype} call {call}")
        want = (static if bit == 4 else len(cols1)) + (1 if call >= 1 else 0)
        assert int(up.ind.numel()) == want, (call, up.ind.numel())
        if call >= 1:
            assert col2 in up.ind.tolist()                              # the new column, seen through the norm's x_scale
        assert int(gate.ind.numel()) == want and torch.equal(gate.ind, up.ind)
    assert not up.add_outliers
    for _ in range(2):                                                  # (down_proj's own search ends two calls after it began)
        if down.add_outliers:
            forward(xs[3].clone())
    assert not down.add_outliers
    assert set(boost) <= set(down.ind.tolist())                        # down_proj carries outlier columns of its own through the hand-over
    if dtype == BF:
        assert mlp._joint_applies(cache) is False and mlp._joint is None     # the joint launch never runs under bfloat16
    # frozen: fuse_down_amax on and off give the same bytes
    cfg.fuse_down_amax = True
    forward(xs[3].clone())                                              # (settles kept plans and the hand-over buffer)
    y_on = forward(xs[3].clone())
    verify(y_on, f"W{bit} {dtype} frozen")
    if dtype == BF:
        assert snap["asked"] and snap["handed_over"] == (bit == 8)      # the row maxima left gate_proj's epilogue (int8 layers)
    cfg.fuse_down_amax = False
    y_off = forward(xs[3].clone())
    if dtype == BF:
        assert not snap["asked"] and not snap["handed_over"]
    assert torch.equal(y_on.view(torch.int16), y_off.view(torch.int16))
    cfg.fuse_down_amax = True
    hook.remove()
    gate.forward_without_preconditionFusedSilu = silu
    # one hipGraph: a single linear chain on a side stream, replayed on restored inputs
    xg, x3 = xs[3].clone(), xs[3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mlp(norm(xg), residual=r)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            yg = mlp(norm(xg), residual=r)
        xg.copy_(x3)
        yg.zero_()
        g.replay()
        side.synchronize()
        assert torch.equal(yg.view(torch.int16), y_on.view(torch.int16))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return y_on.view(torch.int16).clone(), g


@pytest.mark.parametrize("bit", [8, 4])
def test_norm_and_mlp_modules_in_bf16_with_an_fp16_model_beside(bit):
    before, g0 = run_chain(F16, bit, False)
    _, g1 = run_chain(BF, bit, True)
    after, g2 = run_chain(F16, bit, False)
    assert torch.equal(before, after)                                   # the fp16 model gives the bytes it gave before
    del g0, g1, g2


def test_without_the_flag_a_bf16_model_is_refused_on_the_device_too():
    cache = MixLibCache(48, device=DEV, config=MixqConfig(act_dtype=BF))
    with pytest.raises(NotImplementedError, match="no bfloat16 form yet"):
        FasterTransformerRMSNorm(torch.ones(128, device=DEV), EPS, cache)
