"""A `mixq_amd.mixlib`-shaped backend on top of the CPU oracle, for testing the operator's HOST logic (state machine, derived buffers,
packed images, kept argument blocks, the joint gate / up image) on machines without a GPU.  Test infrastructure: installed with
tests/conftest.py's swap_backend(mixq_amd.linear / fused / eetq, ...) by the tests only; the product never imports it.

Round 6: the FULL surface the product modules call - packed operand formats (real byte layouts of include/mixq_hip.h, so that the product's
own host-side unpacking, state_dict of a compacted layer, the joint image's row split ... run on them), capacity-padded `ind` + device
count, kept outlier maps, ForwardPlan, the row-maximum side output, ACT_SILU_PAIR - so that mixq_amd.linear / fused have ONE code shape
(no `hasattr(_backend, ...)` branches): what runs here on the CPU is the code that runs on the GPU, with the kernels swapped for the
oracle.  Tensors live on the CPU; `dev_check` accepts them (the HIP backend's raises: the product has no CPU path).

ABI 1.6: the surface of mixq_amd/mixlib.py signature for signature for everything linear.py / fused.py / eetq.py call - `dtype=` on FusedLinear,
ForwardPlan and amax_supported, `addend=` on ForwardPlan.run and W8A16Linear, PackW8A16(q, dtype), PAIR_LAUNCH_BF16, bfloat16 x / weight / out /
x_out in the quantise and norm entry points, and the same-dtype refusals of the HIP backend.  oracle/ has no bfloat16; the bf16 arithmetic is
the contract of include/mixq_hip.h ("bfloat16 activations" .. "bf16 weight-only layers") restated with what tests/ already holds:
  quantise family, detection   the header's formulas in numpy float32 (IEEE divide, RNE to fp16 for x_scale, rint half-even, clamp, an all-zero
                               row gives 0, |x| > fp16(sigma))
  norm                         tests/bf16_norm_ref.py
  weight-only                  tests/w8a16_bf16_ref.py (z64)
  GEMM epilogue                the header's z in float64 over the operands handed in (w_out is the caller's bf16 image), act / bias / the
                               SILU_MUL multiplier as written there, ONE rounding to bfloat16 (rne_bf16_bits: tests/exact.py's to_bits without
                               its detour through float32, which only holds values fp32 holds)
  ACT_SILU_PAIR                by construction the two computations of the two-launch route: up rounded to bfloat16, then gate's
                               SiLU-and-multiply on that tensor
tests/test_backend_oracle_bf16_host.py holds these branches to bf16_norm_ref, w8a16_bf16_ref and exact.py on those files' own operands;
tests/test_gpu_backend_oracle.py holds them to the kernels.  The fp16 arithmetic is the oracle's, as before."""
import threading

import numpy as np
import torch

import bf16_norm_ref as R
import exact as E
import w8a16_bf16_ref as W
from oracle import oracle as O

ACT_NONE, ACT_SILU, ACT_SILU_MUL, ACT_SILU_PAIR = 0, 1, 2, 3
FMT_PLAIN, FMT_P16X64, FMT_F16X64, FMT_F6X128, FMT_R6X128 = 0, 1, 2, 3, 4
PAIR_LAUNCH = True
PAIR_LAUNCH_BF16 = True
BF = torch.bfloat16
calls = []


def _np(t):
    return t.detach().cpu().contiguous().numpy()


# ---- bfloat16 travels as uint16 bit patterns (numpy has none) ------------------------------------------------------------------------------
def _u16(t):
    """bit patterns of a 16-bit tensor"""
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def _from_u16(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16).copy()).view(dtype)


def _f32(t):
    """float32 values of a 16-bit tensor (exact for either container)"""
    return t.detach().float().contiguous().numpy()


def _f64(t):
    return t.detach().double().contiguous().numpy()


def rne_bf16_bits(v):
    """float64 -> the bfloat16 patterns nearest to it, ties to even, overflow to inf, subnormals at 2^-133: ONE rounding of the exact value (a
    detour through float32 would round twice).  Scaling by a power of two is exact, np.rint is half-even."""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v)
    a = np.abs(np.where(fin, v, 0.0))
    _, e = np.frexp(a)                                                         # a = m 2^e, m in [0.5, 1)
    ulp = np.ldexp(1.0, np.maximum(e - 1, -126) - 7)
    r = np.rint(a / ulp) * ulp
    r = np.where(r >= 2.0 ** 128, np.inf, r)
    r = np.where(fin, np.copysign(r, v), v)
    return (np.ascontiguousarray(r.astype(np.float32)).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def _act_suffix(x, who):
    """(mixlib._act_suffix) "" for float16, "_bf16" for bfloat16; anything else is refused by name"""
    dtype = x if isinstance(x, torch.dtype) else x.dtype
    if dtype == torch.float16:
        return ""
    if dtype == torch.bfloat16:
        return "_bf16"
    raise RuntimeError(f"{who}: x must be float16 or bfloat16, got {dtype}")


def _check_same_dtype(dtype, who, **tensors):
    for name, t in tensors.items():
        if t is not None and t.dtype != dtype:
            raise RuntimeError(f"{who}: {name} must be {dtype} like the call's other 16-bit tensors (dtype={dtype}), got {t.dtype}")


def _check_norm_dtypes(x, who, **tensors):
    for name, t in tensors.items():
        if t.dtype != x.dtype:
            raise RuntimeError(f"{who}: {name} must be {x.dtype} like x, got {t.dtype}")


def _row_scale(x, bit):
    """(q plain numpy, x_scale fp16 numpy [M]) of a 2-D float16 or bfloat16 tensor.  bfloat16, the header's formulas in float32:
    x_scale = fp16(max |x| / qmax), q = clamp(rint_half_even(x / float(x_scale)), -qmax, qmax), a zero scale gives 0."""
    if x.dtype != BF:
        return O.find_row_scale(_np(x), bit)
    x32 = _f32(x)
    qmax = np.float32((1 << (bit - 1)) - 1)
    amax = np.abs(x32).max(axis=1) if x32.shape[1] else np.zeros(x32.shape[0], np.float32)
    with np.errstate(over="ignore"):
        s16 = (amax / qmax).astype(np.float16)
    s = s16.astype(np.float32)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.rint(x32 / s)
    q = np.clip(np.where(s > 0, v, np.float32(0)), -qmax, qmax).astype(np.int8)
    return (q if bit == 8 else E.pack_i4(q)), s16


def _extract_zero(x, live):
    """x_out [M, n] = x[:, live]; those columns of x zeroed IN PLACE (either container)"""
    if x.dtype != BF:
        xn = _np(x).copy()
        vals = O.extract_outliers_zero(xn, live)
        x.copy_(torch.from_numpy(xn))
        return torch.from_numpy(vals)
    cols = torch.from_numpy(np.ascontiguousarray(live, dtype=np.int64))
    vals = x[:, cols].clone()
    x[:, cols] = 0
    return vals


def dev_check(*ts):
    """(the HIP backend refuses CPU tensors here; this one takes them)"""
    for t in ts:
        if t is not None and t.is_cuda:
            raise RuntimeError("backend_oracle: a CPU stand-in; got a GPU tensor")


def set_fmt(t, fmt):
    t._mixq_fmt = fmt
    return t


def fmt_of(t):
    return getattr(t, "_mixq_fmt", FMT_PLAIN)


def packed_rows(rows):
    return (rows + 15) // 16 * 16


def kept_map_words(K):
    return (((K + 31) // 32 + 1 + 3) // 4) * 4 + ((K + 7) // 8) * 4


# ---- the packed layouts of include/mixq_hip.h, vectorised (tests/test_pack_properties.py holds the byte-by-byte restatements they are checked against)
_F6_MAG = np.array([0x00, 0x0C, 0x10, 0x12, 0x14, 0x15, 0x16, 0x17, 0x18], dtype=np.uint8)
_F6_OF_NIBBLE = np.array([(_F6_MAG[v] if v < 8 else (0x20 | _F6_MAG[16 - v])) for v in range(16)], dtype=np.uint8)
_NIBBLE_OF_F6 = np.zeros(64, dtype=np.uint8)
for _v in range(16):
    _NIBBLE_OF_F6[_F6_OF_NIBBLE[_v]] = _v
_NIBBLE_OF_F6[0x20] = 0                                   # (-0)
_SW = (-(np.arange(16) >> 2)) & 3                          # P16X64: chunk c of row r sits at c ^ _SW[r]
_P16_IDX = (np.arange(4)[None, :] ^ _SW[:, None]).reshape(1, 16, 1, 4, 1)


def _padded(q, rows16):
    a = np.zeros((rows16, q.shape[1]), dtype=np.uint8)
    a[: q.shape[0]] = q.view(np.uint8)
    return a


def _f6_fragments(q):
    """nibble-packed [R, K/2] -> FP6 code bytes [rb, r, kb, g, 24]: lane (g, r) of block (kb, rb) holds elements 32 g .. + 31 of row 16 rb + r
    as a little-endian stream of 6-bit codes."""
    R, KB = q.shape
    K = 2 * KB
    r16 = packed_rows(R)
    a = _padded(q, r16)
    nib = np.empty((r16, K), dtype=np.uint8)
    nib[:, 0::2], nib[:, 1::2] = a & 15, a >> 4
    codes = _F6_OF_NIBBLE[nib].astype(np.uint32).reshape(r16 // 16, 16, K // 128, 4, 8, 4)
    v = codes[..., 0] | (codes[..., 1] << 6) | (codes[..., 2] << 12) | (codes[..., 3] << 18)
    return np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=-1).astype(np.uint8).reshape(r16 // 16, 16, K // 128, 4, 24)


def pack_np(q, fmt):
    q = np.ascontiguousarray(q).view(np.uint8)
    R, KB = q.shape
    r16 = packed_rows(R)
    if fmt in (FMT_P16X64, FMT_F16X64):
        assert KB % 64 == 0
        t = _padded(q, r16).reshape(r16 // 16, 16, KB // 64, 4, 16)           # [rb, r, kb, c, b]
        if fmt == FMT_P16X64:
            t = np.take_along_axis(t, np.broadcast_to(_P16_IDX, t.shape[:4] + (1,)), axis=3).transpose(2, 0, 1, 3, 4)
        else:
            t = t.transpose(2, 0, 3, 1, 4)                                       # [kb, rb, c, r, b]
        return np.ascontiguousarray(t).reshape(r16, KB)
    assert fmt in (FMT_F6X128, FMT_R6X128) and KB % 64 == 0
    f = _f6_fragments(q)                                                          # [rb, r, kb, g, 24]
    if fmt == FMT_F6X128:
        a16 = f[..., :16].transpose(2, 0, 3, 1, 4).reshape(KB // 64, r16 // 16, 1024)   # byte 16 (16 g + r) + b
        a8 = f[..., 16:].transpose(2, 0, 3, 1, 4).reshape(KB // 64, r16 // 16, 512)     # 1024 + 8 (16 g + r) + b
    else:
        a16 = f[..., :16].transpose(2, 0, 1, 3, 4).reshape(KB // 64, r16 // 16, 16, 64)  # row r: 16-byte pieces g at 96 r + 16 g
        a8 = f[..., 16:].transpose(2, 0, 1, 3, 4).reshape(KB // 64, r16 // 16, 16, 32)   # ... its 8-byte pieces at 96 r + 64 + 8 g
        return np.ascontiguousarray(np.concatenate([a16, a8], axis=-1)).reshape(r16, KB * 3 // 2)
    return np.ascontiguousarray(np.concatenate([a16, a8], axis=-1)).reshape(r16, KB * 3 // 2)


def unpack_np(p, R, fmt):
    p = np.ascontiguousarray(p).view(np.uint8)
    r16 = p.shape[0]
    if fmt in (FMT_P16X64, FMT_F16X64):
        KB = p.shape[1]
        b = p.reshape(KB // 64, r16 // 16, 1024)
        if fmt == FMT_P16X64:
            t = b.reshape(KB // 64, r16 // 16, 16, 4, 16).transpose(1, 2, 0, 3, 4)   # [rb, r, kb, p, b]
            t = np.take_along_axis(t, np.broadcast_to(_P16_IDX, t.shape[:4] + (1,)), axis=3)
        else:
            t = b.reshape(KB // 64, r16 // 16, 4, 16, 16).transpose(1, 3, 0, 2, 4)
        return np.ascontiguousarray(t).reshape(r16, KB)[:R].copy()
    KB = p.shape[1] * 2 // 3
    K = 2 * KB
    b = p.reshape(KB // 64, r16 // 16, 1536)
    if fmt == FMT_F6X128:
        f = np.concatenate([b[..., :1024].reshape(KB // 64, r16 // 16, 4, 16, 16), b[..., 1024:].reshape(KB // 64, r16 // 16, 4, 16, 8)], axis=-1)
        f = f.transpose(1, 3, 0, 2, 4)                                            # [rb, r, kb, g, 24]
    else:
        rows = b.reshape(KB // 64, r16 // 16, 16, 96)
        f = np.concatenate([rows[..., :64].reshape(KB // 64, r16 // 16, 16, 4, 16), rows[..., 64:].reshape(KB // 64, r16 // 16, 16, 4, 8)], axis=-1)
        f = f.transpose(1, 2, 0, 3, 4)
    tri = f.astype(np.uint32).reshape(r16 // 16, 16, K // 128, 4, 8, 3)
    v = tri[..., 0] | (tri[..., 1] << 8) | (tri[..., 2] << 16)
    codes = np.stack([(v >> (6 * i)) & 63 for i in range(4)], axis=-1).reshape(r16, K)
    nib = _NIBBLE_OF_F6[codes]
    return (nib[:, 0::2] | (nib[:, 1::2] << 4))[:R].copy()


def PackOperand(q, fmt=FMT_P16X64):
    calls.append("PackOperand")
    if q.dim() != 2 or not q.is_contiguous() or q.element_size() != 1:
        raise RuntimeError("PackOperand: expected a contiguous 2-D int8/uint8 tensor")
    out = torch.from_numpy(pack_np(_np(q), fmt))
    return set_fmt(out.view(q.dtype), fmt)


def UnpackOperand(packed, R, fmt=None):
    calls.append("UnpackOperand")
    fmt = fmt_of(packed) if fmt is None else fmt
    if fmt not in (FMT_P16X64, FMT_F16X64, FMT_F6X128, FMT_R6X128):
        raise RuntimeError("UnpackOperand: the tensor carries no packed-format tag; pass fmt")
    return torch.from_numpy(unpack_np(_np(packed), R, fmt)).view(packed.dtype)


def _plain(t, rows):
    """plain [rows, KB] numpy view of a possibly packed operand"""
    f = fmt_of(t)
    a = _np(t)
    return unpack_np(a, rows, f).view(a.dtype) if f else a[:rows]


def _as_fmt(q_np, fmt, dtype):
    if not fmt:
        return torch.from_numpy(q_np)
    return set_fmt(torch.from_numpy(pack_np(q_np, fmt)).view(dtype), fmt)


def _want_fmt(packed, fmt):
    return fmt if fmt is not None else (FMT_P16X64 if packed else FMT_PLAIN)


# ---- reference surface ----------------------------------------------------------------------------------------------------------------
def FindRowScale(x, x_scale, M, K, bit=8):
    calls.append("FindRowScale")
    _act_suffix(x, "FindRowScale")
    if x_scale.dtype != torch.float16:
        raise RuntimeError("FindRowScale: x_scale must be float16")
    q, s = _row_scale(x.reshape(-1, K)[:M], bit)
    x_scale.reshape(-1)[0:M] = torch.from_numpy(s)
    return torch.from_numpy(q)


def FindRowScalePacked(x, x_scale, M, K, bit=8, fmt=FMT_P16X64):
    calls.append("FindRowScalePacked")
    _act_suffix(x, "FindRowScalePacked")
    q, s = _row_scale(x.reshape(-1, K)[:M], bit)
    x_scale.reshape(-1)[0:M] = torch.from_numpy(s)
    return _as_fmt(q, fmt, torch.int8 if bit == 8 else torch.uint8)


def ExtractOutliersAndSetToZeros(ind, x):
    calls.append("ExtractOutliersAndSetToZeros")
    _act_suffix(x, "ExtractOutliersAndSetToZeros")
    return _extract_zero(x, _np(ind))


def _live(ind, n_dev):
    """(live column ids, capacity) of a capacity-padded `ind` buffer + device count"""
    if ind is None or ind.numel() == 0:
        return np.zeros(0, np.int32), 0
    cap = int(ind.numel())
    n = cap if n_dev is None else min(int(n_dev.reshape(-1)[0].item()), cap)
    return _np(ind).astype(np.int32)[:n], cap


def _check_kept_map(col_mask, ind_live, K, who):
    if col_mask is None:
        return
    if col_mask.element_size() != 4 or col_mask.numel() < kept_map_words(K) or not col_mask.is_contiguous():
        raise RuntimeError(f"{who}: col_mask must be the kept outlier map of K = {K} columns ({kept_map_words(K)} int32 words)")
    m = _np(col_mask).view(np.uint32)
    W = (K + 31) // 32
    bits = np.zeros(W * 32, dtype=bool)
    bits[ind_live] = True
    want = np.packbits(bits.reshape(W, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
    if int(m[W]) == ind_live.size:                                   # (a map built for another live count is ignored by the kernels)
        assert np.array_equal(m[:W], want), f"{who}: the kept outlier map does not mark the live `ind` columns"
        keep = m[((W + 1 + 3) // 4) * 4:].view(np.uint16)[:K]
        assert np.array_equal(keep == 0, bits[:K]) and ((keep == 0) | (keep == 0xffff)).all(), f"{who}: AND-masks of the kept outlier map"


def QuantFused(x, ind, x_scale, bit, sigma, x_out=None, flag=None, n_dev=None, packed=False, fmt=None, col_mask=None):
    calls.append("QuantFused")
    fmt = _want_fmt(packed, fmt)
    _act_suffix(x, "QuantFused")
    M, K = x.shape
    if x_scale.numel() < M:
        raise RuntimeError(f"QuantFused: x_scale holds {x_scale.numel()} rows, the batch has {M} (MixLibCache.inputdim too small)")
    live, cap = _live(ind, n_dev)
    _check_kept_map(col_mask, live, K, "QuantFused")
    xo = None
    if cap:
        if x_out is not None and x_out.dtype != x.dtype:
            raise RuntimeError(f"QuantFused: x_out must be {x.dtype} like x, got {x_out.dtype}")
        vals = _extract_zero(x, live)
        xo = torch.zeros((M, (cap + 15) // 16 * 16), dtype=x.dtype) if x_out is None else x_out
        xo[:, :live.size] = vals
        xo[:, live.size:] = 0
    q, s = _row_scale(x, bit)
    x_scale.reshape(-1)[0:M] = torch.from_numpy(s)
    if flag is not None and O.mispredicted(s, sigma, bit):
        flag |= 1
    return _as_fmt(q, fmt, torch.int8 if bit == 8 else torch.uint8), (xo[:, :cap] if cap else None)


def DetectOutlierCols(x, sigma, scratch=None):
    calls.append("DetectOutlierCols")
    _act_suffix(x, "DetectOutlierCols")
    if x.dtype == BF:                                        # |x| > fp16(sigma), as for float16
        ind = np.nonzero((np.abs(_f32(x)) > np.float32(np.float16(sigma))).any(axis=0))[0].astype(np.int32)
    else:
        ind = O.find_outliers(_np(x), sigma)
    buf = torch.zeros(x.shape[1], dtype=torch.int32)
    buf[: ind.size] = torch.from_numpy(ind)
    return buf, torch.tensor([ind.size], dtype=torch.int32)


def DequantWeightCols(q_w, scale_col, ind, bit, out=None):
    calls.append("DequantWeightCols")
    if fmt_of(q_w) != FMT_PLAIN:
        raise RuntimeError("DequantWeightCols: q_w must be the plain, contiguous [N,KB] matrix")
    return torch.from_numpy(O.dequant_weight_cols(_np(q_w), _np(scale_col), _np(ind), bit))


def unpack_int4_to_fp16(q_w, ind):
    calls.append("unpack_int4_to_fp16")
    return torch.from_numpy(O.unpack_i4_cols(_np(q_w), _np(ind)))


def amax_supported(M, N, K, x_fmt, w_fmt, dtype=torch.float16):
    _act_suffix(dtype, "amax_supported")
    return x_fmt == FMT_P16X64 and w_fmt == FMT_F16X64 and M > 0 and K % 64 == 0


def _is_zero_addend(addend):
    return addend is None or getattr(addend, "_mixq_all_zero", False)


def _epilogue_bf16(qx, qw, sx, sw, xo, wo, addend, bias, act, bit):
    """include/mixq_hip.h, "bf16 layers": z = acc sx sw + sum_j xo wo (+ addend) in float64 over exact operands, y = act(z) + bias, with
    ACT_SILU_MUL (silu(z) + bias) * addend - ONE rounding to bfloat16.  qx / qw plain numpy, sx / sw / bias float16 numpy, xo / wo / addend
    float64 values of bfloat16 tensors (or None).  Returns the uint16 patterns."""
    a = (qx if bit == 8 else O.unpack_i4_all(qx)).astype(np.int64)
    b = (qw if bit == 8 else O.unpack_i4_all(qw)).astype(np.int64)
    z = (a @ b.T).astype(np.float64) * sx.astype(np.float64)[:, None] * sw.astype(np.float64)[None, :]
    if xo is not None:
        z = z + xo @ wo.T
    bv = 0.0 if bias is None else bias.astype(np.float64).reshape(1, -1)
    if act == ACT_SILU_MUL:
        return rne_bf16_bits((E.silu64(z) + bv) * addend)
    if addend is not None:
        z = z + addend
    return rne_bf16_bits((E.silu64(z) if act == ACT_SILU else z) + bv)


def FusedLinear(q_x, q_w, x_scale, scale_col, x_out, w_out, n_out, bias, M, N, K, bit=8, act=ACT_NONE, n_out_dev=None,
                addend=None, out=None, x_packed=None, w_packed=None, row_amax=None, col_mask=None, dtype=torch.float16):
    calls.append("FusedLinear")
    if x_scale.numel() < M or scale_col.numel() < N:
        raise RuntimeError("FusedLinear: x_scale / scale_col are shorter than M / N")
    xf, wf = fmt_of(q_x), fmt_of(q_w)
    if (xf in (FMT_F6X128, FMT_R6X128) or wf in (FMT_F6X128, FMT_R6X128)) and (xf != FMT_R6X128 or wf != FMT_F6X128):
        raise RuntimeError("the FP6 form of the W4A4 GEMM takes activations in R6X128 and weights in F6X128")
    if xf == FMT_F16X64:
        raise RuntimeError("F16X64 is a weight format")
    if act == ACT_SILU_PAIR and (N % 16 or not _is_zero_addend(addend)):
        raise RuntimeError("FusedLinear: ACT_SILU_PAIR needs N % 16 == 0 and takes no addend")
    bf = bool(_act_suffix(dtype, "FusedLinear"))
    _check_same_dtype(dtype, "FusedLinear", out=out)
    if bf and ((bit == 8 and (xf, wf) != (FMT_P16X64, FMT_F16X64)) or (bit == 4 and (xf, wf) != (FMT_R6X128, FMT_F6X128))):
        raise RuntimeError("FusedLinear: the bfloat16 GEMMs serve P16X64 x F16X64 (int8) and R6X128 x F6X128 (4-bit) only (MIXQ_ESHAPE)")
    qx, qw = _plain(q_x, M), _plain(q_w, N)
    n_live = n_out if n_out_dev is None else min(int(n_out_dev.reshape(-1)[0].item()), n_out)
    xo = wo = None
    if n_out and x_out is not None and w_out is not None:
        _check_same_dtype(dtype, "FusedLinear", x_out=x_out, w_out=w_out)
        if n_live:
            conv = _f64 if bf else _np
            xo, wo = np.ascontiguousarray(conv(x_out)[:, :n_live]), np.ascontiguousarray(conv(w_out)[:, :n_live])
    sx, sw = _np(x_scale.reshape(-1)[0:M]), _np(scale_col).reshape(-1)[:N]
    b = None if bias is None else _np(bias)
    if act == ACT_SILU_MUL and addend is None:
        raise RuntimeError("FusedLinear: ACT_SILU_MUL needs the multiplier in `addend`")
    add_t = None if (act == ACT_SILU_PAIR or (act != ACT_SILU_MUL and _is_zero_addend(addend))) else addend.reshape(M, -1)[:, :N]
    _check_same_dtype(dtype, "FusedLinear", addend=add_t)
    if bf:
        if act == ACT_SILU_PAIR:
            # by construction the two launches: up_proj's ACT_NONE output rounded to bfloat16, then gate_proj's SiLU-and-multiply on it
            qw_u, qw_g = O.pair_rows_split(qw)
            sw_u, sw_g = O.pair_rows_split(sw)
            wo_u, wo_g = (None, None) if wo is None else O.pair_rows_split(wo)
            b_u, b_g = (None, None) if b is None else O.pair_rows_split(b.reshape(-1))
            up16 = _epilogue_bf16(qx, qw_u, sx, sw_u, xo, wo_u, None, b_u, ACT_NONE, bit)
            ybits = _epilogue_bf16(qx, qw_g, sx, sw_g, xo, wo_g, E.from_bits(up16, E.BF16), b_g, ACT_SILU_MUL, bit)
        else:
            ybits = _epilogue_bf16(qx, qw, sx, sw, xo, wo, None if add_t is None else _f64(add_t), b, act, bit)
    elif act == ACT_SILU_PAIR:
        ybits = O.linear_fused_pair(qx, qw, sx, sw, xo=xo, wo2=wo, bias2=b, bit=bit).view(np.uint16)
    else:
        add = None if add_t is None else np.ascontiguousarray(_np(add_t))
        ybits = O.linear_fused(qx, qw, sx, sw, xo=xo, wo=wo, addend=add, bias=b, act=act, bit=bit).view(np.uint16)
    if row_amax is not None:                                 # the next layer's pre-pass maxima: |16-bit patterns| over the columns its map does not mark
        if bit != 8 or row_amax.numel() < M or row_amax.element_size() != 4:
            raise RuntimeError("FusedLinear: row_amax needs an int8 GEMM and a 4-byte buffer of at least M entries")
        mag = (ybits & 0x7fff).astype(np.int64)
        if col_mask is not None:
            cols = ybits.shape[1]
            m = _np(col_mask).view(np.uint32)
            marked = np.unpackbits(m[: (cols + 31) // 32].view(np.uint8), bitorder="little")[:cols].astype(bool)
            mag[:, marked] = 0
        cur = _np(row_amax).astype(np.int64)
        cur[:M] = np.maximum(cur[:M], mag.max(axis=1) if mag.shape[1] else 0)
        row_amax.copy_(torch.from_numpy(cur.astype(np.int32)))
    yt = _from_u16(ybits, dtype)
    if out is not None:
        out.copy_(yt)
        return out
    return yt


class ForwardPlan:
    """The kept argument block of mixq_linear_forward, as the product's ForwardPlan (mixq_amd/mixlib.py) presents it."""

    def __init__(self, M, N, K, bit, sigma, ldx, ind_buf, n, n_dev, x_scale, q_w, scale_col, w_out, bias, qfmt, act=ACT_NONE, kept_mask=None, dtype=torch.float16):
        calls.append("ForwardPlan")
        self.dtype = dtype
        _act_suffix(dtype, "ForwardPlan")
        if x_scale.numel() < M or scale_col.numel() < N:
            raise RuntimeError("ForwardPlan: x_scale / scale_col are shorter than M / N")
        self.n_cap = 0 if ind_buf is None else int(ind_buf.numel())
        if self.n_cap:
            _check_same_dtype(dtype, "ForwardPlan", w_out=w_out)
        if kept_mask is not None and (kept_mask.element_size() != 4 or kept_mask.numel() < kept_map_words(K)):
            raise RuntimeError("ForwardPlan: kept_mask must be the kept outlier map of K columns")
        self.kept_mask = kept_mask if self.n_cap else None
        self.keep = (ind_buf, n_dev, x_scale, q_w, scale_col, w_out, bias, kept_mask)
        self.M, self.N, self.K, self.bit, self.sigma, self.ldx, self.n, self.qfmt, self.act = M, N, K, bit, sigma, ldx, n, qfmt, act
        self.device = x_scale.device
        self.lock = threading.Lock()
        self.captured = False

    def run(self, x, row_amax=None, col_mask=None, addend=None):
        calls.append("ForwardPlan.run")
        name = str(self.dtype).replace("torch.", "")
        if addend is not None:
            if not isinstance(addend, torch.Tensor) or addend.device != self.device:
                raise RuntimeError(f"ForwardPlan: addend lives on {getattr(addend, 'device', type(addend).__name__)}, the plan was built for {self.device}")
            if addend.dtype != self.dtype or addend.dim() != 2 or tuple(addend.shape) != (self.M, self.N) or addend.stride(1) != 1 or (self.M > 1 and addend.stride(0) % 4):
                raise RuntimeError(f"ForwardPlan: addend must be {name} [{self.M}, {self.N}] with a contiguous last dimension and a row "
                                   f"stride that is a multiple of 4 elements (got {addend.dtype} {tuple(addend.shape)} strides {tuple(addend.stride())})")
        if x.dtype != self.dtype or x.dim() != 2 or x.shape[0] != self.M or x.shape[1] != self.K or x.stride(1) != 1 or x.stride(0) != self.ldx:
            raise RuntimeError(f"ForwardPlan: x must be {name} [{self.M}, {self.K}] with row stride {self.ldx} and a contiguous last dimension")
        ind_buf, n_dev, x_scale, q_w, scale_col, w_out, bias, _ = self.keep
        cm = col_mask if col_mask is not None else self.kept_mask
        if row_amax is not None:
            # the rows' maxima were left by the producing GEMM: what the known-maximum quantiser reads (and clears) must be what the
            # two-pass quantiser would find over the columns this layer does not extract
            live, _ = _live(ind_buf, n_dev)
            if self.dtype == BF:                             # maxima of bfloat16 bit patterns (order-preserving, as for float16)
                xa = (_u16(x) & 0x7fff).astype(np.int32)
                xa[:, live] = 0
                want = xa.max(axis=1) if xa.shape[1] else np.zeros(self.M, np.int32)
            else:
                xa = np.abs(_np(x).astype(np.float32))
                xa[:, live] = 0
                want = xa.max(axis=1).astype(np.float16).view(np.uint16).astype(np.int32) if xa.shape[1] else np.zeros(self.M, np.int32)
            assert np.array_equal(_np(row_amax)[: self.M], want), "row maxima handed over by the producer are not this input's"
            row_amax[: self.M] = 0
        q, xo = QuantFused(x, ind_buf, x_scale, self.bit, self.sigma, n_dev=n_dev, fmt=self.qfmt, col_mask=cm)
        calls.pop()
        y = FusedLinear(q, q_w, x_scale, scale_col, xo, None if w_out is None else w_out[:, : self.n_cap], self.n_cap, bias, self.M, self.N, self.K,
                        bit=self.bit, act=self.act, n_out_dev=n_dev, addend=addend, dtype=self.dtype)
        calls.pop()
        return y, q, (xo[:, : self.n] if xo is not None else None)


def layernorm_forward_cuda(x, weight, out, eps):
    calls.append("layernorm_forward_cuda")
    _act_suffix(x, "layernorm_forward_cuda")
    _check_norm_dtypes(x, "layernorm_forward_cuda", weight=weight, out=out)
    K = x.shape[-1]
    if x.dtype == BF:
        y = _from_u16(R.rmsnorm_bf16(_u16(x.reshape(-1, K)), _u16(weight.reshape(-1)), eps), BF)
    else:
        y = torch.from_numpy(O.rmsnorm(_np(x.reshape(-1, K)), _np(weight), eps))
    out.reshape(-1, K).copy_(y)
    return out


def RMSNormQuantFused(x, weight, out, eps, ind, x_scale, bit, sigma=6.0, flag=None, packed=False, fmt=None, n_dev=None, col_mask=None):
    calls.append("RMSNormQuantFused")
    bf = bool(_act_suffix(x, "RMSNormQuantFused"))
    _check_norm_dtypes(x, "RMSNormQuantFused", weight=weight, out=out)
    if bf and x_scale.dtype != torch.float16:
        raise RuntimeError(f"RMSNormQuantFused: x_scale stays float16 under a bfloat16 x, got {x_scale.dtype}")
    fmt = _want_fmt(packed, fmt)
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    if x_scale.numel() < M:
        raise RuntimeError(f"RMSNormQuantFused: x_scale holds {x_scale.numel()} rows, the batch has {M}")
    live, cap = _live(ind, n_dev)
    _check_kept_map(col_mask, live, K, "RMSNormQuantFused")
    if bf:
        # the fused forms of "bf16 RMSNorm": the plain norm, x_out = its columns `ind`, those columns zeroed, x_scale / q from the zeroed row
        yt = _from_u16(R.rmsnorm_bf16(_u16(x2), _u16(weight.reshape(-1)), eps), BF)
        xo = _extract_zero(yt, live)
        q, s = _row_scale(yt, bit)
    else:
        y, xo, q, s = O.rmsnorm_quant(_np(x2), _np(weight), eps, live, bit)
        yt, xo = torch.from_numpy(y), torch.from_numpy(xo)
    out.reshape(-1, K).copy_(yt)
    x_scale.reshape(-1)[0:M] = torch.from_numpy(s)
    if flag is not None and O.mispredicted(s, sigma, bit):
        flag |= 1
    x_out = None
    if cap:
        x_out = torch.zeros((M, (cap + 15) // 16 * 16), dtype=x.dtype)
        x_out[:, :live.size] = xo
    return _as_fmt(q, fmt, torch.int8 if bit == 8 else torch.uint8), (x_out[:, :cap] if cap else None)


def PackW8A16(q_weight_kn, dtype=torch.float16):
    calls.append("PackW8A16")
    if q_weight_kn.dtype != torch.int8 or q_weight_kn.dim() != 2 or not q_weight_kn.is_contiguous():
        raise RuntimeError("PackW8A16: expected a contiguous int8 [K,N] tensor")
    if dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"PackW8A16: dtype must be torch.float16 or torch.bfloat16, got {dtype}")
    # an IMAGE, as on the device: a copy of the checkpoint layout (the oracle reads it directly) that does not follow later writes to
    # q_weight, tagged with the container it was packed for
    out = q_weight_kn.clone()
    out._mixq_w8a16_dtype = dtype
    return out


def W8A16Linear(x, w_packed, scale_col, bias, N, K, out=None, addend=None):
    calls.append("W8A16Linear")
    bf = x.dtype == torch.bfloat16
    tag = getattr(w_packed, "_mixq_w8a16_dtype", None)
    if not bf and (x.dtype != torch.float16 or scale_col.dtype != torch.float16):
        raise RuntimeError("W8A16Linear: x and scale_col must be float16")
    if bf:
        if scale_col.dtype != torch.float16 or (bias is not None and bias.dtype != torch.float16):
            raise RuntimeError("W8A16Linear: scale_col and bias stay float16 with a bfloat16 x (include/mixq_hip.h, bf16 weight-only layers)")
        if tag != torch.bfloat16:
            raise RuntimeError("W8A16Linear: a bfloat16 x needs the weight image of PackW8A16(q_weight, torch.bfloat16) (two's-complement bytes); "
                               "this one is untagged or was packed for float16 (offset-binary)")
    elif tag == torch.bfloat16:
        raise RuntimeError("W8A16Linear: this weight image was packed for bfloat16 (PackW8A16(q_weight, torch.bfloat16)); a float16 x needs "
                           "the float16 image")
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[1] != K or scale_col.numel() != N:
        raise RuntimeError("W8A16Linear: shape mismatch")
    M, dt = x2.shape[0], x.dtype
    if out is not None and out.dtype != dt:
        raise RuntimeError(f"W8A16Linear: `out` must be {dt}, got {out.dtype}")
    if addend is not None:
        if addend.dtype != dt or addend.device != x.device:
            raise RuntimeError(f"W8A16Linear: addend must be {dt} on x's device ({x.device}), got {addend.dtype} on {addend.device}")
        if addend.dim() != 2 or tuple(addend.shape) != (M, N) or addend.stride(1) != 1 or (M > 1 and (addend.stride(0) % 4 or addend.stride(0) < N)):
            raise RuntimeError(f"W8A16Linear: addend must be [{M}, {N}] with a contiguous last dimension and a row stride that is a multiple of 4 elements "
                               f"and at least {N} (got {tuple(addend.shape)} strides {tuple(addend.stride())})")
    qkn, sc, b = _np(w_packed), _np(scale_col).reshape(-1), (None if bias is None else _np(bias).reshape(-1))
    if bf:
        # tests/w8a16_bf16_ref.py: the exact z in float64 (the addend first, then the bias), ONE rounding to bfloat16
        yt = _from_u16(rne_bf16_bits(W.z64(_u16(x2), qkn, sc, None if addend is None else _u16(addend), b)), BF)
    elif addend is None:
        yt = torch.from_numpy(O.w8a16_linear(_np(x2), qkn, sc, b))
    else:
        # mixq_gemm_w8a16_addend as the oracle's w8a16_linear states the GEMM: exact products, double accumulation, then fp32 - the scale,
        # the addend first, then the bias - and one rounding to float16
        v = ((_np(x2).astype(np.float64) @ qkn.astype(np.float64)) * sc.astype(np.float64)[None, :]).astype(np.float32)
        v = v + _np(addend).astype(np.float32)
        if b is not None:
            v = v + b.astype(np.float32)[None, :]
        with np.errstate(over="ignore"):
            yt = torch.from_numpy(v.astype(np.float16))
    if out is not None:
        out.copy_(yt)
        return out
    return yt
