"""bfloat16 activations at the quantise edge on the MI355X: the division-free quantiser is exact for every finite bf16 x, and every bf16
quantise pass (plain / masked / known-maximum / row-scale only / detection) writes the bytes the fp16 pass writes on the same values, and
the float64 restatement's bytes where fp16 cannot hold the values at all."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mixq_amd import _capi, mixlib  # noqa: E402
from mixq_amd.linear import kept_outlier_map  # noqa: E402
from mixq_amd.mixlib import FMT_F16X64, FMT_F6X128, FMT_P16X64, FMT_PLAIN, FMT_R6X128  # noqa: E402

DEV = "cuda"
FMTS = {8: [FMT_PLAIN, FMT_P16X64, FMT_F16X64], 4: [FMT_PLAIN, FMT_P16X64, FMT_F6X128, FMT_R6X128]}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    _capi.load().mixq_gemm_set_config(-1)
    yield
    _capi.load().mixq_gemm_set_config(-1)


@pytest.mark.parametrize("bit", [8, 4])
def test_quant_exact_selftest_bf16_has_no_mismatch(bit):
    """The division-free quantiser (common.h quant_exact / quant8_exact) against rint(RN(x / s)) for every finite bf16 x and every finite
    fp16 s > 0."""
    mism = torch.zeros(1, dtype=torch.int64, device=DEV)
    _capi.call("mixq_selftest_quant_exact_bf16", mism.data_ptr(), bit, None)
    torch.cuda.synchronize()
    assert int(mism.item()) == 0


def _pair(M, K, cols, seed):
    """The same values as bf16 and as fp16: every value is 0 or in fp16's normal range, so both containers hold it exactly."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 1.5
    if cols:
        x[:, cols] *= 25
    xb = x.bfloat16()
    xb[xb.abs() < 2.0 ** -14] = 0
    xh = xb.half()
    assert torch.equal(xh.bfloat16().view(torch.int16), xb.view(torch.int16))
    return xb.to(DEV), xh.to(DEV)


def _row_amax_bits(x, cols):
    """Row maxima of |x| over the non-outlier columns as the container's bit patterns (what mixq_gemm_i8_fused_amax leaves)."""
    b = x.view(torch.int16).int() & 0x7FFF
    if cols:
        b[:, cols] = 0
    return b.max(dim=1).values.to(torch.int32)


def _run(mode, x, ind, cols, bit, fmt, M, K):
    """One quantise pass; returns (q bytes, x_scale, x_out as float32 or None, x after the pass)."""
    x = x.clone()
    xs = torch.zeros(max(M, 1), 1, dtype=torch.float16, device=DEV)
    if mode == "findrow":
        q = mixlib.FindRowScalePacked(x, xs, M, K, bit, fmt)
        return q.view(torch.uint8).clone(), xs, None, x
    cm = kept_outlier_map(ind, K) if mode in ("masked", "known") else None
    if mode == "known":
        n = ind.numel()
        ldo = (n + 15) // 16 * 16
        xo = torch.empty((M, ldo), dtype=x.dtype, device=DEV)
        q = torch.empty((mixlib.packed_rows(M) if fmt else M, mixlib._q_row_bytes(K, bit, fmt)), dtype=torch.uint8, device=DEV)
        ra = _row_amax_bits(x, cols)
        sfx = "_bf16" if x.dtype == torch.bfloat16 else ""
        _capi.call("mixq_quant_known_amax" + sfx, x.data_ptr(), ind.data_ptr(), n, None, ra.data_ptr(), cm.data_ptr(), cm.numel(), xs.data_ptr(),
                   q.data_ptr(), xo.data_ptr(), None, M, K, x.stride(0), ldo, bit, 6.0, fmt, mixlib._stream())
        assert int(ra.abs().max()) == 0                           # cleared for the producer's next run
        return q, xs, xo[:, :n].float(), x
    q, xo = mixlib.QuantFused(x, ind, xs, bit, 6.0, fmt=fmt, col_mask=cm)
    return q.view(torch.uint8).clone(), xs, xo.float(), x


@pytest.mark.parametrize("mode", ["unmasked", "masked", "known", "findrow"])
@pytest.mark.parametrize("K", [4096, 11008])
@pytest.mark.parametrize("M", [1, 16, 100, 512])
def test_bf16_quantise_passes_match_fp16_on_shared_values(M, K, mode):
    cols = [] if mode == "findrow" else sorted({3, 77, 1000, 2049, K - 9, K // 3})
    xb, xh = _pair(M, K, cols, seed=M * 7 + K)
    ind = torch.tensor(cols, dtype=torch.int32, device=DEV)
    for bit in (8, 4):
        for fmt in FMTS[bit]:
            qb, sb, ob, xb2 = _run(mode, xb, ind, cols, bit, fmt, M, K)
            qh, sh, oh, xh2 = _run(mode, xh, ind, cols, bit, fmt, M, K)
            torch.cuda.synchronize()
            what = f"{mode} bit={bit} fmt={fmt}"
            assert torch.equal(sb[:M].view(torch.int16), sh[:M].view(torch.int16)), what
            assert torch.equal(_plain_q(qb, M, K, bit, fmt), _plain_q(qh, M, K, bit, fmt)), what
            if ob is not None:
                assert torch.equal(ob, oh), what
            assert torch.equal(xb2.float(), xh2.float()), what       # outlier columns zeroed in place, the rest untouched


def _plain_q(q, M, K, bit, fmt):
    """The plain [M, KB] bytes of a quantised activation in any format (rows >= M of a packed image are never written: left out)."""
    if fmt == FMT_PLAIN:
        return q[:M]
    KB = K if bit == 8 else K // 2
    out = torch.empty((M, KB), dtype=torch.uint8, device=DEV)
    _capi.call("mixq_unpack_operand", q.data_ptr(), out.data_ptr(), M, KB, fmt, mixlib._stream())
    return out


def _q_restated(x64, s, bit):
    qmax = (1 << (bit - 1)) - 1
    sd = s.astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(sd > 0, np.rint(x64 / sd), 0.0)
    return np.clip(q, -qmax, qmax).astype(np.int64)


def _restated_scale(x64, bit):
    qmax = (1 << (bit - 1)) - 1
    amax = np.abs(x64).max(axis=1)
    return (amax.astype(np.float32) / np.float32(qmax)).astype(np.float16)


@pytest.mark.parametrize("mode", ["unmasked", "masked", "known"])
@pytest.mark.parametrize("bit", [8, 4])
def test_bf16_values_fp16_cannot_hold_against_float64(bit, mode):
    """Inliers below fp16's normal range and above its precision, outlier columns of 1e5 .. 3e6: x_out carries them unchanged, the scale and
    q are the float64 restatement's - through each route that moves the outlier bit patterns (gather, the kept map's LDS row image, the
    known-maximum pass)."""
    M, K = 64, 4096
    g = torch.Generator().manual_seed(bit)
    x = torch.randn(M, K, generator=g) * 300.0
    x[:, 100:140] *= 1e-9                                     # far below fp16's smallest subnormal
    x[5] = 0                                                  # an all-zero row
    cols = [7, 900, 2222, 4000]
    x[:, cols] = torch.empty(M, len(cols)).uniform_(1e5, 3e6, generator=g) * torch.sign(torch.randn(M, len(cols), generator=g))
    x[5, cols] = 0
    xb = x.bfloat16().to(DEV)
    ind = torch.tensor(cols, dtype=torch.int32, device=DEV)
    q, xs, xo, xk = _run(mode, xb, ind, cols, bit, FMT_PLAIN, M, K)
    torch.cuda.synchronize()
    xo = xo.bfloat16()                                        # (_run widens x_out to float32: exact, and back)
    x64 = xb.double().cpu().numpy()
    assert torch.equal(xo.view(torch.int16), xb[:, cols].contiguous().view(torch.int16))
    inl = x64.copy()
    inl[:, cols] = 0
    assert np.array_equal(xk.double().cpu().numpy(), inl)
    s = _restated_scale(inl, bit)
    assert np.array_equal(xs[:, 0].cpu().numpy().view(np.uint16), s.view(np.uint16))
    assert np.isfinite(xs.float().cpu().numpy()).all()
    qr = _q_restated(inl, s, bit)
    got = q[:M].cpu().numpy().view(np.int8 if bit == 8 else np.uint8)
    if bit == 8:
        got = got.astype(np.int64)
    else:
        b = got.view(np.uint8).astype(np.int64)
        lo, hi = b & 15, b >> 4
        got = np.stack([lo, hi], axis=-1).reshape(M, K)
        got = np.where(got >= 8, got - 16, got)
    assert np.array_equal(got, qr)


def test_bf16_outlier_detection_matches_threshold():
    M, K = 100, 4096
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g)
    hot = [11, 512, 3000, 4095]
    x[7, hot] = torch.tensor([7.0, -1e5, 2e6, -6.5])
    x[x.abs() > 6.0] = 0.5
    x[7, hot] = torch.tensor([7.0, -1e5, 2e6, -6.5])
    x[8, 20] = 6.0                                            # not > sigma
    xb = x.bfloat16().to(DEV)
    ind_buf, count = mixlib.DetectOutlierCols(xb, 6.0)
    torch.cuda.synchronize()
    got = ind_buf[: int(count.item())].cpu().tolist()
    want = sorted(set(torch.nonzero(xb.float().abs() > 6.0)[:, 1].cpu().tolist()))
    assert got == want == hot


def test_bf16_extraction_moves_bf16_bits():
    M, K = 16, 4096
    xb = (torch.randn(M, K) * 1e4).bfloat16().to(DEV)
    xb[:, 9] = 3e6
    ref = xb.clone()
    ind = torch.tensor([9, 4000, 33], dtype=torch.int32, device=DEV)
    xo = mixlib.ExtractOutliersAndSetToZeros(ind, xb)
    torch.cuda.synchronize()
    assert xo.dtype == torch.bfloat16
    assert torch.equal(xo.view(torch.int16), ref[:, [9, 4000, 33]].contiguous().view(torch.int16))
    assert int(xb[:, [9, 4000, 33]].abs().max().item()) == 0
