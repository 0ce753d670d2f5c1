"""Parity of the HIP path (through the C ABI of libmixq_hip.so) against the CPU oracle on seeded inputs.

Bars (north_star): integer / byte / index results bit-exact; fp16 outputs within |d|inf <= 1e-2 of a CPU Linear over the
SAME dequantised operands (oracle.linear_dequant_ref, fp64), and within 2 fp16 ulp of the oracle's restatement of the
same fp32 formula.  Full BASELINE sizes are covered through size-independent exact properties (checksum of checksums,
sampled rows) because the scalar oracle cannot finish 46 GFLOP in seconds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_pack_properties import p16x64_reference, p16x64_unpack, packed_reference, packed_unpack  # noqa: E402
from mixq_amd.mixlib import fmt_of  # noqa: E402

DEV = "cuda"
GATE = 1e-2          # north_star: |d|inf vs CPU Linear over the same dequantised operands


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def ulp_tol(ref):
    """2 fp16 ulp of the reference magnitude, at least 1e-3."""
    a = np.abs(ref.astype(np.float32))
    ulp = np.where(a > 0, 2.0 ** (np.floor(np.log2(np.maximum(a, 6e-5))) - 10), 2.0 ** -24)
    return np.maximum(2 * ulp, 1e-3)


def make_x(M, K, seed, outlier_cols=(), scale=20.0, zero_rows=()):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K)).astype(np.float16)
    for c in outlier_cols:
        x[:, c] *= scale
    for r in zero_rows:
        x[r] = 0
    return x


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    info = _capi.device_info()          # raises unless a gfx950 device is visible and the native library is loaded
    assert "gfx950" in info
    _capi.load().mixq_gemm_set_config(-1)
    _capi.load().mixq_quant_set_config(-1)
    yield
    _capi.load().mixq_gemm_set_config(-1)
    _capi.load().mixq_quant_set_config(-1)


# ---------------------------------------------------------------------------------------------------------------
# (i) per-token scale + quantise
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(1, 64), (5, 64), (37, 1024), (64, 4096), (16, 11008), (3, 28672), (2, 40000)])
@pytest.mark.parametrize("bit", [8, 4])
def test_find_row_scale_bit_exact(M, K, bit):
    if bit == 4 and K % 16:
        pytest.skip("int4 needs K % 16 == 0")
    x = make_x(M, K, seed=M * 7 + K, zero_rows=(0,) if M > 1 else ())
    x[-1, -1] = 65504.0                                    # largest fp16
    xs = torch.zeros((M + 3, 1), dtype=torch.float16, device=DEV)
    q = mixlib.FindRowScale(t(x), xs, M, K, bit)
    qo, so = O.find_row_scale(x, bit)
    assert np.array_equal(n(q), qo)
    assert np.array_equal(bits(n(xs)[:M, 0]), bits(so))
    assert not n(xs)[M:].any(), "rows beyond M of the caller's x_scale buffer must not be touched"


@pytest.mark.parametrize("M,K,bit", [(1, 64, 8), (17, 256, 8), (40, 1024, 8), (33, 512, 4)])
@pytest.mark.parametrize("fmt", [1, 2])
def test_packed_quantise_equals_pack_of_plain(M, K, bit, fmt):
    x = make_x(M, K, seed=3)
    xs = torch.zeros((M, 1), dtype=torch.float16, device=DEV)
    qp = mixlib.FindRowScalePacked(t(x), xs, M, K, bit, fmt=fmt)
    assert fmt_of(qp) == fmt
    qo, so = O.find_row_scale(x, bit)
    KB = K if bit == 8 else K // 2
    got = packed_unpack(n(qp).reshape(-1).view(np.uint8), M, KB, fmt)
    assert np.array_equal(got, qo.view(np.uint8))
    assert np.array_equal(bits(n(xs)[:, 0]), bits(so))
    # the standalone re-tiling kernel produces the documented layout byte for byte (pad rows zero), and its inverse undoes it
    packed = mixlib.PackOperand(t(qo), fmt)
    assert np.array_equal(n(packed).reshape(-1).view(np.uint8), packed_reference(qo, fmt))
    assert np.array_equal(n(mixlib.UnpackOperand(packed, M)), qo)


# ---------------------------------------------------------------------------------------------------------------
# (ii) outlier extraction, fused quantise, detection
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,ncols", [(8, 64, 1), (32, 256, 3), (64, 4096, 41), (5, 1024, 130)])
def test_extract_and_fused_quantise(M, K, ncols):
    rng = np.random.default_rng(K + ncols)
    ind = np.sort(rng.choice(K, ncols, replace=False)).astype(np.int32)
    rng.shuffle(ind)                                       # `ind` is in discovery order, not sorted
    x = make_x(M, K, seed=11, outlier_cols=ind)
    # reference pair (k2, k1)
    x1 = t(x)
    xo1 = mixlib.ExtractOutliersAndSetToZeros(t(ind), x1)
    xz = x.copy()
    xo_ref = O.extract_outliers_zero(xz, ind)
    assert np.array_equal(bits(n(xo1)), bits(xo_ref))
    assert np.array_equal(bits(n(x1)), bits(xz)), "columns must be zeroed in the caller's tensor"
    # fused form
    for bit in (8, 4):
        x2 = t(x)
        xs = torch.zeros((M, 1), dtype=torch.float16, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        q, xo2 = mixlib.QuantFused(x2, t(ind), xs, bit, 6.0, flag=flag)
        qo, so = O.find_row_scale(xz, bit)
        assert np.array_equal(n(q), qo)
        assert np.array_equal(bits(n(xs)[:, 0]), bits(so))
        assert np.array_equal(bits(n(xo2)), bits(xo_ref))
        assert np.array_equal(bits(n(x2)), bits(xz))
        assert xo2.stride(0) % 16 == 0, "outlier matrix row stride must suit the GEMM tail"
        assert bool(flag.item()) == O.mispredicted(so, 6.0, bit)


def test_misprediction_flag_threshold():
    """flag <=> max(x_scale) > fp16(sigma/127) (linear.py:201), probed on both sides of the threshold."""
    for amax, expect in [(5.9, False), (6.0, False), (6.02, True), (100.0, True)]:
        x = np.full((4, 64), 0.5, dtype=np.float16)
        x[2, 5] = amax
        xs = torch.zeros((4, 1), dtype=torch.float16, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        mixlib.QuantFused(t(x), None, xs, 8, 6.0, flag=flag)
        so = O.find_row_scale(x, 8)[1]
        assert bool(flag.item()) == O.mispredicted(so, 6.0, 8) == expect


@pytest.mark.parametrize("M,K,cols", [(24, 256, [7, 100, 201]), (512, 4096, list(range(0, 4096, 100))), (3, 64, []),
                                       (16, 128, list(range(128)))])
def test_detect_outlier_columns(M, K, cols):
    x = make_x(M, K, seed=5, outlier_cols=cols)
    if not cols:
        x = np.clip(x, -3, 3)
    if K > 60:
        x[1, 55] = 6.0          # exactly sigma: not an outlier
    ind_buf, count = mixlib.DetectOutlierCols(t(x), 6.0)
    cnt = int(count.item())
    ref = O.find_outliers(x, 6.0)
    assert cnt == ref.size
    assert np.array_equal(n(ind_buf)[:cnt], ref)


def test_detect_matches_golden_find_outliers(golden):
    g = golden("g4_find_outliers.npz")
    ind_buf, count = mixlib.DetectOutlierCols(t(g["x"]), float(g["sigma"]))
    assert np.array_equal(n(ind_buf)[: int(count.item())], g["ind"])


# ---------------------------------------------------------------------------------------------------------------
# weight columns
# ---------------------------------------------------------------------------------------------------------------
def test_weight_column_dequant_bit_exact(golden):
    g8, g4 = golden("g2_from_linear_w8.npz"), golden("g3_from_linear_w4.npz")
    ind = np.array([0, 5, 255, 17], dtype=np.int32)
    got = mixlib.DequantWeightCols(t(g8["q_weight"]), t(g8["scale_col"]), t(ind), 8)
    assert np.array_equal(bits(n(got)), bits(O.dequant_weight_cols(g8["q_weight"], g8["scale_col"], ind, 8)))
    ind4 = np.array([511, 0, 33, 256], dtype=np.int32)
    got4 = mixlib.DequantWeightCols(t(g4["q_weight"]), t(g4["scale_col"]), t(ind4), 4)
    assert np.array_equal(bits(n(got4)), bits(O.dequant_weight_cols(g4["q_weight"], g4["scale_col"], ind4, 4)))
    raw = mixlib.unpack_int4_to_fp16(t(g4["q_weight"]), t(ind4))
    assert np.array_equal(bits(n(raw)), bits(O.unpack_i4_cols(g4["q_weight"], ind4)))


# ---------------------------------------------------------------------------------------------------------------
# (iii) integer GEMM: exact, every tile configuration, ragged shapes, both operand layouts
# ---------------------------------------------------------------------------------------------------------------
def _real_configs():
    return [i for i, name in enumerate(_capi.gemm_config_names()) if "abl" not in name]


@pytest.mark.parametrize("M,N,K", [(1, 4, 64), (33, 100, 128), (512, 256, 512), (300, 1000, 1024)])
def test_int32_gemm_exact_all_configs(M, N, K):
    rng = np.random.default_rng(M + N + K)
    qx = rng.integers(-127, 128, (M, K), dtype=np.int8)
    qw = rng.integers(-128, 128, (N, K), dtype=np.int8)
    ref = O.gemm_i8(qx, qw)
    lib = _capi.load()
    for c in _real_configs():
        assert lib.mixq_gemm_set_config(c) == 0
        y = mixlib.gemm(t(qx), t(qw), M, N, K)
        assert np.array_equal(n(y), ref), f"config {c} {_capi.gemm_config_names()[c]}"
    lib.mixq_gemm_set_config(-1)


def _fused_case(M, N, K, bit, seed, n_out, bias, addend, act):
    rng = np.random.default_rng(seed)
    ind = np.sort(rng.choice(K, n_out, replace=False)).astype(np.int32) if n_out else np.zeros(0, np.int32)
    x = make_x(M, K, seed=seed + 1, outlier_cols=ind)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
    if bit == 8:
        qw, sw = O.quant_weight_w8(w)
        wo = O.dequant_weight_cols(qw, sw, ind, 8) if n_out else None
    else:
        qw, sw, wo = O.quant_weight_w4(w, ind)            # fp columns keep their exact fp16 weights (linear.py:129)
        if not n_out:
            wo = None
    xz = x.copy()
    xo = O.extract_outliers_zero(xz, ind) if n_out else None
    qx, sx = O.find_row_scale(xz, bit)
    b = rng.standard_normal(N).astype(np.float16) if bias else None
    ad = rng.standard_normal((M, N)).astype(np.float16) if addend else None
    return dict(qx=qx, qw=qw, sx=sx, sw=sw, xo=xo, wo=wo, ind=ind, bias=b, addend=ad, act=act, bit=bit, M=M, N=N, K=K)


def _run_fused(c, packed, n_dev_cap=0):
    """packed: 0 / False plain, 1 / True P16x64, 2 = weights F16x64 (fragment order) with P16x64 activations: the operand pair of
    the weights-in-registers kernels.  n_dev_cap > 0: hand the kernel outlier operands of that CAPACITY (poison beyond the
    real count) with the count itself in device memory."""
    M, N, K, bit = c["M"], c["N"], c["K"], c["bit"]
    fmt = int(packed)
    n_out = int(c["ind"].size)
    cap = max(n_out, n_dev_cap)
    pad = (cap + 15) // 16 * 16
    xo = wo = n_dev = None
    if n_out or n_dev_cap:
        xo = torch.full((M, pad), float("nan"), dtype=torch.float16, device=DEV)
        wo = torch.full((N, pad), float("nan"), dtype=torch.float16, device=DEV)               # pad is poison
        if n_out:
            xo[:, :n_out] = t(c["xo"]); wo[:, :n_out] = t(c["wo"])
        xo, wo = xo[:, :cap], wo[:, :cap]
        if n_dev_cap:
            n_dev = torch.tensor([n_out], dtype=torch.int32, device=DEV)
    qx, qw = t(c["qx"]), t(c["qw"])
    if fmt:
        qx, qw = mixlib.PackOperand(qx, 1), mixlib.PackOperand(qw, fmt)
    sx = torch.zeros((M, 1), dtype=torch.float16, device=DEV); sx[:, 0] = t(c["sx"])
    return mixlib.FusedLinear(qx, qw, sx, t(c["sw"]), xo, wo, cap, None if c["bias"] is None else t(c["bias"]), M, N, K, bit=bit,
                              act=c["act"], addend=None if c["addend"] is None else t(c["addend"]), n_out_dev=n_dev)


@pytest.mark.parametrize("M,N,K,bit,n_out,bias,addend,act", [
    (32, 96, 256, 8, 0, False, False, 0),
    (32, 96, 256, 8, 3, True, False, 0),
    (96, 320, 1024, 8, 41, False, False, 0),
    (96, 320, 1024, 8, 17, True, True, 1),
    (130, 200, 512, 8, 128, True, False, 0),
    (7, 36, 128, 8, 5, False, True, 0),
    (64, 128, 512, 4, 128, False, False, 0),
    (40, 64, 1024, 4, 16, True, False, 1),
])
@pytest.mark.parametrize("packed", [0, 1, 2])
def test_fused_linear_vs_oracle(M, N, K, bit, n_out, bias, addend, act, packed):
    c = _fused_case(M, N, K, bit, seed=M + N + K + bit + n_out, n_out=n_out, bias=bias, addend=addend, act=act)
    y = n(_run_fused(c, packed)).astype(np.float32)
    ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], addend=c["addend"], bias=c["bias"], act=act,
                         bit=bit).astype(np.float32)
    assert np.isfinite(y).all()
    assert (np.abs(y - ref) <= ulp_tol(ref)).all(), f"max |d| = {np.abs(y - ref).max()}"
    if bit == 8 and not act and not addend:
        gate = O.linear_dequant_ref(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], ind=c["ind"], bias=c["bias"], wo=c["wo"])
        # tolerance stated by north_star: 1e-2 absolute on fp16 outputs.  fp16 cannot resolve 1e-2 above |y| = 16 (its
        # spacing there is 1.6e-2), so beyond that the bar is one fp16 ulp of the reference value.
        a = np.abs(gate)
        ulp1 = 2.0 ** (np.floor(np.log2(np.maximum(a, 1.0))) - 10)
        assert (np.abs(y - gate) <= np.maximum(GATE, ulp1)).all(), f"max |d| = {np.abs(y - gate).max()}"
        assert np.abs(y - gate)[a < 8].max() <= GATE


def test_reference_style_calls_through_the_mixlib_surface():
    """The reference's own call sequence (linear.py:187-285): k2, k1, torch.mm, int8FusedDequantize(addend), += bias."""
    c = _fused_case(64, 192, 512, 8, seed=9, n_out=9, bias=True, addend=False, act=0)
    rng = np.random.default_rng(9)
    x = make_x(64, 512, seed=10, outlier_cols=c["ind"])
    xt = t(x)
    cache = MixLibCache(64, device=DEV)
    xo = mixlib.ExtractOutliersAndSetToZeros(t(c["ind"]), xt)
    q = mixlib.FindRowScale(xt, cache.x_scale, 64, 512, 8)
    wc = t(c["wo"])
    outliers_fp16 = torch.mm(xo, wc.T)
    y = mixlib.int8FusedDequantize(q, t(c["qw"]), cache.x_scale, t(c["sw"]), outliers_fp16, 64, 192, 512)
    y += t(c["bias"])
    # the same sequence restated on the CPU: fp16 torch.mm result as the addend, then the fp16 `+= bias`
    sxh = n(cache.x_scale)[:64, 0]
    mm16 = (n(xo).astype(np.float32) @ c["wo"].astype(np.float32).T).astype(np.float16)
    ref = O.linear_fused(n(q), c["qw"], sxh, c["sw"], addend=mm16).astype(np.float32)
    ref = (ref.astype(np.float16) + c["bias"].astype(np.float16)).astype(np.float32)
    assert (np.abs(n(y).astype(np.float32) - ref) <= 2 * ulp_tol(ref)).all()
    # and against the fp64 Linear over the same operands: this flow rounds to fp16 three times (mm, dequant, bias add),
    # each worth up to half an fp16 ulp of |y| <= 8, so its own distance to the gate can reach 1.2e-2
    gate = O.linear_dequant_ref(n(q), c["qw"], sxh, c["sw"], xo=n(xo), ind=c["ind"], bias=c["bias"], wo=c["wo"])
    assert np.abs(n(y).astype(np.float64) - gate).max() <= 1.5e-2
    # no-outlier form with the cache's zeros addend, unfused pair, SiLU twin
    y0 = mixlib.int8FusedDequantize(q, t(c["qw"]), cache.x_scale, t(c["sw"]), cache.zeros, 64, 192, 512)
    y32 = mixlib.gemm(q, t(c["qw"]), 64, 192, 512)
    assert np.array_equal(n(y32), O.gemm_i8(n(q), c["qw"]))
    y1 = mixlib.dequantizeInt8(y32, cache.x_scale, t(c["sw"]), cache.zeros, 8, 64, 192)
    assert np.abs(n(y0).astype(np.float32) - n(y1).astype(np.float32)).max() <= 2e-3
    ys = mixlib.int8FusedDequantizeSilu(q, t(c["qw"]), cache.x_scale, t(c["sw"]), cache.zeros, 64, 192, 512)
    ref_s = O.linear_fused(n(q), c["qw"], n(cache.x_scale)[:64, 0], c["sw"], act=1).astype(np.float32)
    assert (np.abs(n(ys).astype(np.float32) - ref_s) <= ulp_tol(ref_s)).all()


# ---------------------------------------------------------------------------------------------------------------
# operator: the reference's recorded forward traces, now on the HIP backend
# ---------------------------------------------------------------------------------------------------------------
def _unpacked_q(cache, M, KB):
    q = n(cache.q_xcache)
    fmt = fmt_of(cache.q_xcache)
    if fmt:
        return packed_unpack(q.reshape(-1).view(np.uint8), M, KB, fmt)
    return q.view(np.uint8)


def test_operator_trace_w8_on_gpu(golden):
    g, g2 = golden("g5a_forward_w8_unfused.npz"), golden("g2_from_linear_w8.npz")
    lin = torch.nn.Linear(256, 96, bias=True).half()
    lin.weight.data.copy_(torch.from_numpy(g2["weight"]))
    lin.bias.data.copy_(torch.from_numpy(g2["bias_in"]))
    cache = MixLibCache(64, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    assert np.array_equal(n(layer.q_weight), g2["q_weight"]) and np.array_equal(bits(n(layer.scale_col)), bits(g2["scale_col"]))
    for i in range(int(g["ncalls"])):
        x = t(g[f"c{i}_x_in"])
        y = layer(x, None, True)
        assert np.array_equal(n(layer.ind), g[f"c{i}_ind"])
        assert layer.cnt == int(g[f"c{i}_cnt"]) and layer.add_outliers == bool(g[f"c{i}_add_outliers"])
        assert np.array_equal(bits(n(cache.x_scale)[:32]), bits(g[f"c{i}_x_scale"]))
        assert np.array_equal(_unpacked_q(cache, 32, 256), g[f"c{i}_q_xcache"].view(np.uint8))
        assert np.array_equal(bits(n(x)), bits(g[f"c{i}_x_after"]))
        if layer.ind.numel():
            assert np.array_equal(bits(n(layer.weight_cache)), bits(g[f"c{i}_weight_cache"]))
        assert np.abs(n(y).astype(np.float32) - g[f"c{i}_y"].astype(np.float32)).max() <= 4e-3


def test_operator_trace_w4_and_silu_on_gpu(golden):
    g = golden("g5d_forward_w4_silu.npz")
    ls = torch.from_numpy(g["layer_scales"])
    up, gate = torch.nn.Linear(512, 64, bias=False).half(), torch.nn.Linear(512, 64, bias=False).half()
    up.weight.data.copy_(torch.from_numpy(g["up_weight"]))
    gate.weight.data.copy_(torch.from_numpy(g["gate_weight"]))
    cache = MixLibCache(64, bit=4, device=DEV)
    up_q = MixLinear_GEMM.from_linear(up, 4, cache=cache, layer_scales=ls, dev=DEV)
    gate_q = MixLinear_GEMM.from_linear(gate, 4, cache=cache, layer_scales=ls, dev=DEV)
    for i in range(int(g["ncalls"])):
        x = t(g[f"c{i}_x_in"])
        y = up_q(x, cache, True)
        assert np.array_equal(n(up_q.ind), g[f"c{i}_ind"])
        assert np.array_equal(_unpacked_q(cache, 16, 256), g[f"c{i}_q_xcache"].view(np.uint8))
        assert np.abs(n(y).astype(np.float32) - g[f"c{i}_y"].astype(np.float32)).max() <= 4e-3
        ys = gate_q.forward_without_preconditionFusedSilu(t(g[f"c{i}_x_in"]), cache)
        assert np.abs(n(ys).astype(np.float32) - g[f"c{i}_y_silu"].astype(np.float32)).max() <= 4e-3


# ---------------------------------------------------------------------------------------------------------------
# BASELINE sizes through size-independent exact properties
# ---------------------------------------------------------------------------------------------------------------
LLAMA2_7B = [(4096, 4096), (4096, 11008), (4096, 12288), (11008, 4096)]
LLAMA2_70B = [(8192, 8192), (8192, 28672), (8192, 10240), (28672, 8192)]
LLAMA3_8B = [(4096, 4096), (4096, 6144), (4096, 14336), (14336, 4096)]


@pytest.mark.parametrize("K,N", sorted(set(LLAMA2_7B + LLAMA2_70B + LLAMA3_8B)))
def test_full_size_int32_checksum_and_rows(K, N):
    """M = 512 at the BASELINE shapes: (a) checksum of checksums  sum_n Y32[m,n] == x[m,:] . colsum(W)  for EVERY row
    (exact integers); (b) 4 sampled rows fully against the oracle; both operand layouts."""
    M = 512
    g = torch.Generator().manual_seed(K + N)
    qx = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int8)
    qw = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    colsum = qw.to(torch.int64).sum(dim=0)
    want_rowsum = (qx.to(torch.int64) * colsum).sum(dim=1).numpy()
    rows = [0, 137, 300, 511]
    ref_rows = O.gemm_i8(qx[rows].numpy(), qw.numpy())
    y = mixlib.gemm(qx.to(DEV), qw.to(DEV), M, N, K)
    assert np.array_equal(n(y.to(torch.int64).sum(dim=1)), want_rowsum)
    assert np.array_equal(n(y[rows]), ref_rows)
    # packed layout through the fused entry point with unit scales: fp16(acc * 2^-12) stays exact for |acc| < 2^11 * 2^12
    sx = torch.full((M, 1), 2.0 ** -6, dtype=torch.float16, device=DEV)
    sw = torch.full((1, N), 2.0 ** -6, dtype=torch.float16, device=DEV)
    want = (y.to(torch.float64) * 2.0 ** -12).to(torch.float16)
    for fmt in (1, 2):
        yp = mixlib.FusedLinear(mixlib.PackOperand(qx.to(DEV), 1), mixlib.PackOperand(qw.to(DEV), fmt), sx, sw, None, None, 0, None, M, N, K)
        assert torch.equal(yp, want), fmt


@pytest.mark.parametrize("K,N,bit", [(4096, 11008, 8), (4096, 14336, 8), (4096, 11008, 4)])
def test_full_size_operator_with_one_percent_outliers(K, N, bit):
    """BASELINE config 4 protocol: 1 % synthetic outlier columns x20, two warm-up forwards freeze `ind`
    (outlier-predict on), the third is checked on sampled rows against the CPU Linear over the dequantised operands."""
    M = 512
    torch.manual_seed(0)
    lin = torch.nn.Linear(K, N, bias=False).half()
    cols = torch.randperm(K, generator=torch.Generator().manual_seed(1))[: round(0.01 * K)]
    cache = MixLibCache(M, bit=bit, device=DEV)
    if bit == 8:
        layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    else:
        scales = torch.ones(K); scales[cols] = 20.0 + torch.arange(cols.numel()) * 1e-3     # calibration marks the same columns
        layer = MixLinear_GEMM.from_linear(lin, 4, cache=cache, layer_scales=scales, dev=DEV)
    xs = []
    for call in range(3):
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(10 + call)).half()
        x[:, cols] *= 20
        xs.append(x)
        y = layer(x.to(DEV), None, True)
    assert layer.add_outliers is False
    found = set(n(layer.ind).tolist())
    assert set(cols.tolist()) <= found
    rows = [0, 255, 511]
    x = xs[-1].numpy()[rows].copy()
    ind = n(layer.ind).astype(np.int32)
    xo = O.extract_outliers_zero(x, ind)
    qx, sx = O.find_row_scale(x, bit)
    if bit == 8:
        gate = O.linear_dequant_ref(qx, n(layer.q_weight), sx, n(layer.scale_col), xo=xo, ind=ind, wo=n(layer.weight_cache))
        assert np.abs(n(y)[rows].astype(np.float64) - gate).max() <= GATE
    ref = O.linear_fused(qx, n(layer.q_weight), sx, n(layer.scale_col), xo=xo, wo=n(layer.weight_cache), bit=bit).astype(np.float32)
    assert (np.abs(n(y)[rows].astype(np.float32) - ref) <= ulp_tol(ref)).all()


# ---------------------------------------------------------------------------------------------------------------
# RMSNorm (+ fused extract / quantise) - bit-exact against the oracle's restatement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(1, 64), (7, 512), (33, 4096), (16, 8192), (5, 11008), (3, 28672)])
def test_rmsnorm_bit_exact(M, K):
    rng = np.random.default_rng(M + K)
    x = (rng.standard_normal((M, K)) * 2.5).astype(np.float16)
    x[0] = 0
    w = (1 + 0.2 * rng.standard_normal(K)).astype(np.float16)
    out = torch.empty((M, K), dtype=torch.float16, device=DEV)
    mixlib.layernorm_forward_cuda(t(x), t(w), out, 1e-6)
    assert np.array_equal(bits(n(out)), bits(O.rmsnorm(x, w, 1e-6)))


@pytest.mark.parametrize("M,K,ncols,bit", [(8, 64, 0, 8), (32, 512, 3, 8), (64, 4096, 41, 8), (12, 8192, 128, 8), (24, 4096, 128, 4),
                                            (5, 1024, 7, 4)])
def test_rmsnorm_quant_fused_bit_exact(M, K, ncols, bit):
    rng = np.random.default_rng(K + ncols + bit)
    ind = rng.permutation(K)[:ncols].astype(np.int32)
    x = (rng.standard_normal((M, K)) * 1.5).astype(np.float16)
    x[:, ind] *= 30
    w = (1 + 0.2 * rng.standard_normal(K)).astype(np.float16)
    y_ref, xo_ref, q_ref, s_ref = O.rmsnorm_quant(x, w, 1e-5, ind, bit)
    xt = t(x)
    for packed in (0, 1, 2):
        KB = K if bit == 8 else K // 2
        if packed and KB % 64:
            continue
        out = torch.empty((M, K), dtype=torch.float16, device=DEV)
        xs = torch.zeros((M, 1), dtype=torch.float16, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        q, xo = mixlib.RMSNormQuantFused(xt, t(w), out, 1e-5, t(ind) if ncols else None, xs, bit, sigma=6.0, flag=flag, fmt=packed)
        assert np.array_equal(bits(n(xt)), bits(x)), "the norm must not modify its input"
        assert np.array_equal(bits(n(out)), bits(y_ref))
        assert np.array_equal(bits(n(xs)[:, 0]), bits(s_ref))
        got_q = packed_unpack(n(q).reshape(-1).view(np.uint8), M, KB, packed) if packed else n(q).view(np.uint8)
        assert np.array_equal(got_q, q_ref.view(np.uint8))
        if ncols:
            assert np.array_equal(bits(n(xo)), bits(xo_ref)) and xo.stride(0) % 16 == 0
        assert bool(flag.item()) == O.mispredicted(s_ref, 6.0, bit)
    # the reference-named entry points return (X_out, q_x) in that order (norm.py:25-33)
    out = torch.empty((M, K), dtype=torch.float16, device=DEV)
    xs = torch.zeros((M, 1), dtype=torch.float16, device=DEV)
    fn = mixlib.layernorm_forward_cuda_extract_outliers if bit == 8 else mixlib.layernorm_forward_cuda_extract_outliers_int4
    xo2, q2 = fn(xt, t(w), out, 1e-5, t(ind), xs)
    assert np.array_equal(n(q2).view(np.uint8), q_ref.view(np.uint8)) and tuple(xo2.shape) == (M, ncols)


def test_fused_norm_then_linear_on_gpu():
    """norm.next_layer = W_pack; W_pack(hidden) with unfused=False equals plain norm + unfused linear (attn.py:219)."""
    from mixq_amd import FasterTransformerRMSNorm
    torch.manual_seed(0)
    K, N, M = 4096, 512, 64
    lin = torch.nn.Linear(K, N, bias=False).half()
    cache, cache2 = MixLibCache(M, device=DEV), MixLibCache(M, device=DEV)
    a = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    b = MixLinear_GEMM.from_linear(lin, 8, cache=cache2, dev=DEV)
    wn = (torch.ones(K) + 0.1 * torch.randn(K)).to(DEV)
    norm = FasterTransformerRMSNorm(wn, eps=1e-6, cache=cache)
    norm.next_layer = a
    plain = FasterTransformerRMSNorm(wn, eps=1e-6)
    cols = torch.randperm(K)[:41]
    for call in range(3):
        h = torch.randn(M, K, generator=torch.Generator().manual_seed(call)).half()
        h[:, cols] *= 25
        y = a(norm(h.to(DEV)), None, False)
        y_ref = b(plain(h.to(DEV)), None, True)
        assert torch.equal(y, y_ref)
    assert torch.equal(a.ind, b.ind) and a.ind.numel() == 41 and a.add_outliers is False


def _sk_configs():
    return [i for i, name in enumerate(_capi.gemm_config_names()) if name.startswith("sk")]


@pytest.mark.parametrize("M,N,K", [(128, 128, 2560), (512, 256, 8192), (300, 1000, 4096), (512, 4096, 11008), (64, 384, 192)])
def test_stream_k_is_bit_identical_to_data_parallel(M, N, K):
    """The stream-K kernels hand int32 partial tiles between workgroups; integer addition is exact, so with
    power-of-two scales the fp16 result must equal the data-parallel kernel's bit for bit - on every launch (the flag
    words are self-resetting) and under hipGraph replay.  (128,128,2560) makes one tile with 40 contributors."""
    if not _sk_configs():
        pytest.skip("the stream-K kernels live in the tuning build (make -C mixq_amd/csrc tuning; MIXQ_TUNING_LIB=1): tools/gpu_suite.sh runs these there")
    _capi.ensure_workspace(DEV)
    g = torch.Generator().manual_seed(M + N + K)
    qx = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int8).to(DEV)
    qw = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8).to(DEV)
    qxp, qwp = mixlib.PackP16x64(qx), mixlib.PackP16x64(qw)
    sx = torch.full((M, 1), 2.0 ** -6, dtype=torch.float16, device=DEV)
    sw = torch.full((1, N), 2.0 ** -7, dtype=torch.float16, device=DEV)
    want = (mixlib.gemm(qx, qw, M, N, K).to(torch.float64) * 2.0 ** -13).to(torch.float16)
    lib = _capi.load()
    for c in _sk_configs():
        assert lib.mixq_gemm_set_config(c) == 0
        for rep in range(3):
            y = mixlib.FusedLinear(qxp, qwp, sx, sw, None, None, 0, None, M, N, K)
            assert torch.equal(y, want), f"{_capi.gemm_config_names()[c]} launch {rep}"
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = torch.empty((M, N), dtype=torch.float16, device=DEV)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(4):
                    mixlib.FusedLinear(qxp, qwp, sx, sw, None, None, 0, None, M, N, K, out=out)
            for _ in range(3):
                out.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, want)
    lib.mixq_gemm_set_config(-1)


def test_stream_k_full_epilogue_and_int4():
    """Outlier tail, bias, SiLU and the int4 expansion through the stream-K kernels against the oracle."""
    if not _sk_configs():
        pytest.skip("the stream-K kernels live in the tuning build (make -C mixq_amd/csrc tuning; MIXQ_TUNING_LIB=1): tools/gpu_suite.sh runs these there")
    _capi.ensure_workspace(DEV)
    lib = _capi.load()
    for (M, N, K, bit, n_out, bias, act) in [(96, 320, 4096, 8, 17, True, 0), (130, 200, 2048, 8, 41, False, 1), (64, 128, 4096, 4, 128, True, 0)]:
        c = _fused_case(M, N, K, bit, seed=M + K, n_out=n_out, bias=bias, addend=False, act=act)
        ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], bias=c["bias"], act=act, bit=bit).astype(np.float32)
        for cfg in _sk_configs():
            assert lib.mixq_gemm_set_config(cfg) == 0
            y = n(_run_fused(c, True)).astype(np.float32)
            assert (np.abs(y - ref) <= ulp_tol(ref)).all(), f"{_capi.gemm_config_names()[cfg]}: {np.abs(y - ref).max()}"
    lib.mixq_gemm_set_config(-1)


def test_stream_k_every_output_layout():
    """The stream-K kernels carry a copy of the GEMMs' store-path selector (N % 8, ldy % 8, y % 16): every layout of frames.LAYOUTS - a padded
    row, a column slice of a wider buffer, ld % 8 == 4, an 8-byte aligned base - against the oracle, with a guard frame around y, and
    byte-identical to the exact-fit layout (tests/test_gpu_strides.py runs the same checks on the product library's kernels)."""
    if not _sk_configs():
        pytest.skip("the stream-K kernels live in the tuning build (make -C mixq_amd/csrc tuning; MIXQ_TUNING_LIB=1): tools/gpu_suite.sh runs these there")
    from frames import GUARD_ROWS, LAYOUTS, Frame, classes_possible, store_class
    _capi.ensure_workspace(DEV)
    lib = _capi.load()
    try:
        for (M, N, K, bit, n_out, bias, addend, act) in [(200, 1000, 2048, 8, 17, True, True, 0), (200, 1004, 2048, 8, 41, False, False, 1),
                                                         (64, 256, 4096, 4, 16, True, True, 1), (1, 256, 2048, 8, 0, False, False, 0)]:
            c = _fused_case(M, N, K, bit, seed=M + K, n_out=n_out, bias=bias, addend=addend, act=act)
            ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], addend=c["addend"], bias=c["bias"], act=act, bit=bit).astype(np.float32)
            qx, qw = mixlib.PackOperand(t(c["qx"]), 1), mixlib.PackOperand(t(c["qw"]), 1)
            sx = torch.zeros((M, 1), dtype=torch.float16, device=DEV); sx[:, 0] = t(c["sx"])
            pad = (n_out + 15) // 16 * 16
            xo = wo = None
            if n_out:
                xo = torch.full((M, pad + 8), float("nan"), dtype=torch.float16, device=DEV); xo[:, :n_out] = t(c["xo"]); xo = xo[:, :n_out]
                wo = torch.full((N, pad + 32), float("nan"), dtype=torch.float16, device=DEV); wo[:, :n_out] = t(c["wo"]); wo = wo[:, :n_out]
            ad = None
            if addend:
                ad = torch.zeros((M, N + 4), dtype=torch.float16, device=DEV)[:, :N]
                ad.copy_(t(c["addend"]))
            for cfg in _sk_configs():
                assert lib.mixq_gemm_set_config(cfg) == 0
                first, ran = None, set()
                for ld, col_off, elem_off in LAYOUTS(N):
                    f = Frame(M, N, ld, col_off, elem_off, torch.float16, DEV, GUARD_ROWS)
                    cls = store_class(N, ld, f.view.data_ptr())
                    what = f"{_capi.gemm_config_names()[cfg]} {M}x{K}->{N} W{bit} ld={ld} col_off={col_off} elem_off={elem_off} [{cls}]"
                    y = mixlib.FusedLinear(qx, qw, sx, t(c["sw"]), xo, wo, n_out, None if c["bias"] is None else t(c["bias"]), M, N, K, bit=bit, act=act,
                                           addend=ad, out=f.view)
                    got = n(y).astype(np.float32)
                    assert np.isfinite(got).all(), what
                    assert (np.abs(got - ref) <= ulp_tol(ref)).all(), f"{what}: {np.abs(got - ref).max()}"
                    f.assert_untouched(what)
                    first = y.clone() if first is None else first
                    assert torch.equal(y, first), f"{what}: differs from the exact-fit layout"
                    ran.add(cls)
                assert ran == classes_possible(N)
    finally:
        lib.mixq_gemm_set_config(-1)


def test_linearity_in_the_outlier_operand():
    """Y(xo1 + xo2) - Y(0) == (Y(xo1) - Y(0)) + (Y(xo2) - Y(0)) up to fp16 rounding: the fp16 MFMA tail is additive."""
    c = _fused_case(64, 128, 256, 8, seed=4, n_out=16, bias=False, addend=False, act=0)
    base = dict(c); base["xo"] = np.zeros_like(c["xo"])
    a = dict(c); a["xo"] = (c["xo"].astype(np.float32) * 0.5).astype(np.float16)
    y0, ya, yfull = (n(_run_fused(k, True)).astype(np.float32) for k in (base, a, c))
    # three independently rounded fp16 outputs enter the identity: allow 3 ulp of the largest magnitude
    bound = 3 * 2.0 ** (np.floor(np.log2(max(np.abs(yfull).max(), 1.0))) - 10)
    assert np.abs((yfull - y0) - 2 * (ya - y0)).max() <= bound


def test_empty_and_tiny_inputs():
    xs = torch.zeros((4, 1), dtype=torch.float16, device=DEV)
    q = mixlib.FindRowScale(torch.zeros((0, 64), dtype=torch.float16, device=DEV), xs, 0, 64, 8)
    assert tuple(q.shape) == (0, 64)
    e = mixlib.ExtractOutliersAndSetToZeros(torch.zeros(0, dtype=torch.int32, device=DEV), torch.ones((3, 64), dtype=torch.float16, device=DEV))
    assert tuple(e.shape) == (3, 0)
    y = mixlib.gemm(torch.zeros((0, 64), dtype=torch.int8, device=DEV), torch.zeros((8, 64), dtype=torch.int8, device=DEV), 0, 8, 64)
    assert tuple(y.shape) == (0, 8)
    with pytest.raises(_capi.MixqError):
        mixlib.gemm(torch.zeros((4, 100), dtype=torch.int8, device=DEV), torch.zeros((8, 100), dtype=torch.int8, device=DEV), 4, 8, 100)


@pytest.mark.parametrize("w_bit", [8, 4])
def test_checkpoint_roundtrip_forward_identical(tmp_path, w_bit):
    """SURVEY.md §8f row 3 on the device: quantise a block's Linears, run, save in the reference's layout, load into a
    fresh skeleton, run again: bit-identical outputs; the fused QKV layer equals the three projections concatenated."""
    from mixq_amd import checkpoint as ck
    from test_checkpoint_host import Tiny, make_scales
    torch.manual_seed(0)
    dev = "cuda"
    model = Tiny(h=256, f=512, n=1).half().to(dev)
    cache = MixLibCache(64, bit=w_bit)
    scales = make_scales(model, 256, 512) if w_bit == 4 else None
    ck.quantize_(model, w_bit, cache, blocks=model.layers, act_scales=scales)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(48, 256, generator=g).half().to(dev)
    x[:, 17] *= 20
    att = model.layers[0].self_attn
    def run(a):
        return [m(x.clone(), unfused=True).clone() for m in (a.q_proj, a.k_proj, a.v_proj)]
    ck.save_quantized(model, str(tmp_path), {"w_bit": w_bit}, safetensors=True)      # before any forward: the 4-bit
    y1 = run(att)                                      # layers' ind / weight_cache buffers grow when a new column appears
    y1b = run(att)                                     # second call: outlier prediction frozen
    fresh = Tiny(h=256, f=512, n=1).half().to(dev)
    cache2 = MixLibCache(64, bit=w_bit)
    ck.load_quantized(fresh, str(tmp_path), cache2, blocks=fresh.layers)
    att2 = fresh.layers[0].self_attn
    y2 = run(att2)
    y2b = run(att2)
    for a, b in zip(y1 + y1b, y2 + y2b):
        assert torch.equal(a, b)
    fused = ck.fuse_qkv(att2.q_proj, att2.k_proj, att2.v_proj, MixLibCache(64, bit=w_bit))
    yf = fused(x.clone(), unfused=True)
    yf = fused(x.clone(), unfused=True)
    yq = torch.cat(y2b, dim=1)
    # same operands, same per-tile arithmetic; only the outlier set's discovery order could differ (8-bit) - it does not
    assert torch.equal(yf, yq)


# ---------------------------------------------------------------------------------------------------------------
# weight-only W8A16 (parity UNPINNED: EETQ is absent; the oracle restates the published rule)
# ---------------------------------------------------------------------------------------------------------------
def _w8a16_case(M, N, K, seed, bias):
    rng = np.random.default_rng(seed)
    q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    s = (rng.random(N) * 0.01 + 0.001).astype(np.float16)
    x = rng.standard_normal((M, K)).astype(np.float16)
    b = (rng.standard_normal(N)).astype(np.float16) if bias else None
    return q, s, x, b


@pytest.mark.parametrize("M,N,K,bias", [(1, 64, 64, False), (7, 192, 128, True), (33, 100, 256, False), (128, 128, 512, True),
                                        (300, 1000, 1024, False), (512, 1536, 4096, True), (16, 4096, 4096, False), (64, 36, 192, True)])
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4, 5, "w8a16_32x64_s8_d5_l1", "w8a16_decode32"])
def test_w8a16_linear_vs_oracle(M, N, K, bias, cfg):
    q, s, x, b = _w8a16_case(M, N, K, 7 * M + N + K, bias)
    lib = _capi.load()
    if isinstance(cfg, str):
        if cfg.endswith("decode32") and M > 32:
            pytest.skip("the in-workgroup K-split kernel takes M <= 32")
        cfg = _capi.w8a16_config_names().index(cfg)
    assert lib.mixq_gemm_w8a16_set_config(cfg) == 0
    try:
        wp = mixlib.PackW8A16(t(q))
        y = n(mixlib.W8A16Linear(t(x), wp, t(s), None if b is None else t(b), N, K))
    finally:
        lib.mixq_gemm_w8a16_set_config(-1)
    ref = O.w8a16_linear(x, q, s, b)
    d = np.abs(y.astype(np.float32) - ref.astype(np.float32))
    assert (d <= ulp_tol(ref)).all(), float(d.max())
    # the north-star gate: CPU Linear over the same dequantised operands
    gate = torch.nn.functional.linear(torch.from_numpy(x).float(), torch.from_numpy(q.astype(np.float32) * s.astype(np.float32)).t(),
                                      None if b is None else torch.from_numpy(b).float()).numpy()
    small = np.abs(gate) < 8
    assert np.abs(y.astype(np.float32) - gate)[small].max() <= GATE


def _w8a16_real_configs():
    return [i for i, nm in enumerate(_capi.w8a16_config_names()) if "abl" not in nm and "decode" not in nm]


def test_w8a16_every_tiling_every_k_step_count():
    """The weights-in-registers W8A16 kernel keeps D k-steps of weights and NSTAGE - 2 of activations in flight with hand-counted
    waits; its guarded tail takes over for the last < NSLOT + D k-steps.  Every tiling x every k-step count 1..14 and a few long
    ones, ragged M and N, against an fp32 matmul of the same dequantised operands on the device (fp32 accumulation order differs:
    tolerance 2 fp16 ulp of the row's largest output) and, exactly, against a one-hot probe that reads single weights back."""
    lib = _capi.load()
    names = _capi.w8a16_config_names()
    g = torch.Generator().manual_seed(11)
    M, N = 150, 328
    try:
        for cfg in _w8a16_real_configs():
            assert lib.mixq_gemm_w8a16_set_config(cfg) == 0
            for nk in list(range(1, 15)) + [23, 40, 67]:
                K = 64 * nk
                q = torch.randint(-128, 128, (K, N), generator=g, dtype=torch.int8).to(DEV)
                sc = (torch.rand(N, generator=g) * 0.01 + 0.001).half().to(DEV)
                x = torch.randn(M, K, generator=g).half().to(DEV)
                b = torch.randn(N, generator=g).half().to(DEV)
                y = mixlib.W8A16Linear(x, mixlib.PackW8A16(q), sc, b, N, K).float()
                ref = x.float() @ (q.float() * sc.float()) + b.float()
                tol = 2.0 ** (torch.floor(torch.log2(ref.abs().amax(dim=1, keepdim=True).clamp_min(1.0))) - 9)
                assert ((y - ref).abs() <= tol).all(), (names[cfg], nk, float((y - ref).abs().max()))
            # exact probe: x = one-hot rows, unit scales -> y[m, n] = q[k(m), n] for k spread over all k-steps
            K = 64 * 13
            q = torch.randint(-128, 128, (K, N), generator=g, dtype=torch.int8).to(DEV)
            ks = torch.arange(M) * 5 % K
            x = torch.zeros(M, K, dtype=torch.float16, device=DEV)
            x[torch.arange(M), ks] = 1
            y = mixlib.W8A16Linear(x, mixlib.PackW8A16(q), torch.ones(N, dtype=torch.float16, device=DEV), None, N, K)
            assert torch.equal(y.to(torch.int16).cpu(), q[ks.to(DEV)].to(torch.int16).cpu()), names[cfg]
    finally:
        lib.mixq_gemm_w8a16_set_config(-1)


def test_w8a16_offset_binary_conversion_is_exact():
    """One-hot activations read single weights back: every int8 value -128..127 must survive the perm / pk_add trick."""
    K, N = 256, 64
    q = np.zeros((K, N), np.int8)
    vals = np.arange(-128, 128, dtype=np.int16)
    for k in range(K):
        q[k, :] = np.roll(vals, k)[:N].astype(np.int8)
    s = np.ones(N, np.float16)
    x = np.eye(K, dtype=np.float16)[:128]                        # row m selects k = m
    y = n(mixlib.W8A16Linear(t(x), mixlib.PackW8A16(t(q)), t(s), None, N, K))
    assert np.array_equal(y.astype(np.int16), q[:128].astype(np.int16))


def test_w8a16_strided_input_and_operator_on_gpu():
    torch.manual_seed(3)
    K, N, M = 512, 320, 40
    lin = torch.nn.Linear(K, N, bias=True).half()
    cache = MixLibCache(64)
    ql = MixLinear_GEMM.from_linear(lin, bit=8, weight_only=True, cache=cache, dev=DEV, name="fc_out")
    big = torch.randn(M, K + 64, device=DEV).half()
    x = big[:, :K]                                               # row stride K + 64
    y = ql(x)
    ref = O.w8a16_linear(n(x), n(ql.q_weight), n(ql.scale_col), n(ql.bias))
    assert (np.abs(n(y).astype(np.float32) - ref.astype(np.float32)) <= ulp_tol(ref)).all()
    from mixq_amd import eetq
    y2 = eetq.w8_a16_gemm(x.reshape(2, M // 2, K), ql.q_weight, ql.scale_col)
    ref2 = O.w8a16_linear(n(x), n(ql.q_weight), n(ql.scale_col))
    assert y2.shape == (2, M // 2, N)
    assert (np.abs(n(y2).reshape(M, N).astype(np.float32) - ref2.astype(np.float32)) <= ulp_tol(ref2)).all()


def test_w8a16_full_size_linearity():
    """Metric-size shape through size-independent properties: y(x1 + x2) = y(x1) + y(x2) for inputs whose sums are exact
    in fp16, and sampled rows against the oracle."""
    M, K, N = 512, 4096, 11008
    rng = np.random.default_rng(5)
    q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    s = (rng.random(N) * 0.004 + 0.001).astype(np.float16)
    x1 = (rng.integers(-8, 9, size=(M, K)) / 8.0).astype(np.float16)
    x2 = (rng.integers(-8, 9, size=(M, K)) / 8.0).astype(np.float16)
    wp = mixlib.PackW8A16(t(q))
    ts = t(s)
    y1 = mixlib.W8A16Linear(t(x1), wp, ts, None, N, K).float()
    y2 = mixlib.W8A16Linear(t(x2), wp, ts, None, N, K).float()
    y12 = mixlib.W8A16Linear(t(x1 + x2), wp, ts, None, N, K).float()
    tol = torch.from_numpy(ulp_tol(n(y12)) + ulp_tol(n(y1)) + ulp_tol(n(y2))).to(DEV)      # one rounding each
    assert ((y12 - (y1 + y2)).abs() <= tol).all()
    rows = [0, 1, 127, 128, 300, 511]
    ref = O.w8a16_linear(x1[rows], q, s)
    assert (np.abs(n(y1)[rows] - ref.astype(np.float32)) <= ulp_tol(ref)).all()


def test_w8a16_cold_launches_have_no_stale_tile_patches():
    """Regression: the staged output tile was once read back before a wave's last ds_writes had been performed
    (raw s_barrier without lgkmcnt(0)); it showed only on cold launches of the 2-workgroups-per-CU config."""
    M, N, K = 512, 11008, 1024
    g = torch.Generator().manual_seed(0)
    q = torch.randint(-128, 128, (K, N), generator=g, dtype=torch.int8).to(DEV)
    s = (torch.rand(N, generator=g) * 0.01 + 0.001).half().to(DEV)
    wdeq = q.float() * s.float()
    lib = _capi.load()
    keep = []
    try:
        for cfg in (2, 0):
            assert lib.mixq_gemm_w8a16_set_config(cfg) == 0
            for rep in range(10):
                keep.append(torch.empty((rep + 1) * 3_000_000, dtype=torch.uint8, device=DEV))      # shift addresses
                x = torch.randn(M, K, generator=g).half().to(DEV)
                wp = mixlib.PackW8A16(q)
                y = mixlib.W8A16Linear(x, wp, s, None, N, K)
                ref = x.float() @ wdeq
                assert ((y.float() - ref).abs() <= 0.01 * ref.abs().max()).all(), (cfg, rep)
    finally:
        lib.mixq_gemm_w8a16_set_config(-1)


# ---------------------------------------------------------------------------------------------------------------
# small-batch ("decode") kernel: M <= 32, packed int8 operands (gemm_skinny.hip)
# ---------------------------------------------------------------------------------------------------------------
def _skinny_id():
    return _capi.gemm_config_names().index("decode32")


@pytest.mark.parametrize("M,N,K,n_out,bias,addend,act,bit", [
    (1, 64, 64, 0, False, False, 0, 8), (5, 100, 512, 3, True, False, 0, 8), (16, 4096, 4096, 41, False, False, 0, 8),
    (32, 1000, 1024, 128, True, True, 1, 8), (17, 36, 11008, 17, False, True, 0, 8), (32, 11008, 704, 0, True, False, 1, 8),
    (16, 128, 512, 128, False, False, 0, 4), (7, 64, 1024, 16, True, False, 1, 4), (32, 4096, 4096, 128, False, True, 0, 4),
    (1, 36, 128, 0, False, False, 0, 4),
])
def test_skinny_kernel_vs_oracle_and_tiled(M, N, K, n_out, bias, addend, act, bit):
    """Forced through the small-batch kernel (both packed operand formats): against the oracle, and bit-identical to the tiled
    kernels (same exact int32 accumulator, same epilogue arithmetic in the same order)."""
    c = _fused_case(M, N, K, bit, seed=3 * M + N + K + n_out, n_out=n_out, bias=bias, addend=addend, act=act)
    lib = _capi.load()
    try:
        assert lib.mixq_gemm_set_config(_skinny_id()) == 0
        y = n(_run_fused(c, 1))
        y_f16 = n(_run_fused(c, 2))
        assert lib.mixq_gemm_set_config(_capi.gemm_config_names().index("64x64_w2x2_s5_l1")) == 0
        y_tiled = n(_run_fused(c, 1))
        assert lib.mixq_gemm_set_config(_capi.gemm_config_names().index("wr64x64_s8_d4_l1")) == 0
        y_wr = n(_run_fused(c, 2))
    finally:
        lib.mixq_gemm_set_config(-1)
    assert np.array_equal(bits(y), bits(y_f16))
    if n_out == 0:        # (the fp16 tail of gemm_wreg.hip sums 32 outlier columns per MFMA, the others 16: equal to rounding only)
        assert np.array_equal(bits(y), bits(y_wr))
    else:
        assert (np.abs(y_wr.astype(np.float32) - y.astype(np.float32)) <= ulp_tol(y.astype(np.float32))).all()
    ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], addend=c["addend"], bias=c["bias"], act=act,
                         bit=bit).astype(np.float32)
    assert np.isfinite(y).all()
    assert (np.abs(y.astype(np.float32) - ref) <= ulp_tol(ref)).all()
    assert np.array_equal(bits(y), bits(y_tiled))


def test_skinny_is_the_automatic_choice_for_decode_and_refuses_large_batches():
    lib = _capi.load()
    c = _fused_case(8, 256, 512, 8, seed=1, n_out=5, bias=False, addend=False, act=0)
    y_auto = n(_run_fused(c, True))
    try:
        assert lib.mixq_gemm_set_config(_skinny_id()) == 0
        y_forced = n(_run_fused(c, True))
        big = _fused_case(64, 256, 512, 8, seed=2, n_out=0, bias=False, addend=False, act=0)
        with pytest.raises(_capi.MixqError):
            _run_fused(big, True)                                # M > 32: not this kernel's job
    finally:
        lib.mixq_gemm_set_config(-1)
    assert np.array_equal(bits(y_auto), bits(y_forced))


@pytest.mark.parametrize("M", [1, 16, 32])
def test_wide_layers_at_small_batch_take_the_32x64_weight_stream_tiling(M):
    """M <= 32 with fragment-order int8 weights and N >= 8192 (up / gate projections): the weights-in-registers 32 x 64 tiling is the
    automatic choice (12.4 us vs 17.4 us at 32 x 4096 -> 11008, profiles/r02_decode.txt); narrow layers and int4 stay with the
    in-workgroup K split.  Same bits as the decode kernel and as the oracle-checked tiled kernel, outlier tail and bias included."""
    lib = _capi.load()
    names = _capi.gemm_config_names()
    N, K = 8192 + 64, 640
    assert names[lib.mixq_gemm_pick_config_fmt(M, N, K, 8, 2)] == "wr32x64_s8_d6_l1"
    assert names[lib.mixq_gemm_pick_config_fmt(M, 4096, K, 8, 2)] == "decode32"
    assert names[lib.mixq_gemm_pick_config_fmt(M, N, K, 4, 2)] == "decode32"
    c = _fused_case(M, N, K, 8, seed=5 + M, n_out=41, bias=True, addend=False, act=0)
    y_auto = n(_run_fused(c, 2, n_dev_cap=48))
    try:
        assert lib.mixq_gemm_set_config(_skinny_id()) == 0
        y_dec = n(_run_fused(c, 2, n_dev_cap=48))
        assert lib.mixq_gemm_set_config(names.index("wr64x64_s8_d4_l1")) == 0
        y_t = n(_run_fused(c, 2, n_dev_cap=48))
    finally:
        lib.mixq_gemm_set_config(-1)
    assert np.array_equal(bits(y_auto), bits(y_dec)) and np.array_equal(bits(y_auto), bits(y_t))
    ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], bias=c["bias"], bit=8).astype(np.float32)
    assert (np.abs(y_auto.astype(np.float32) - ref) <= ulp_tol(ref)).all()


# ---------------------------------------------------------------------------------------------------------------
# randomized exactness / race hunting: every real tiling, odd shapes, cold allocations, repeated launches
# ---------------------------------------------------------------------------------------------------------------
def test_randomized_shapes_all_tilings_bit_exact():
    """With int8 operands and power-of-two scales acc * sx * sw is exact in fp32, so every tiling (and the decode kernel)
    must reproduce the correctly rounded int64 CPU matmul bit for bit - on freshly allocated buffers, launch after launch.  This is
    the net that would have caught the epilogue's LDS write/read race (it only showed on cold launches of the tilings
    that run several workgroups per CU)."""
    rng = np.random.default_rng(2024)
    names = _capi.gemm_config_names()
    # (stream-K and pairwise split-K forms need a registered workspace and have their own tests)
    real = [i for i, nm in enumerate(names) if "abl" not in nm and not nm.startswith("sk") and not nm.startswith("decode") and not nm.endswith(("_k2", "_pair"))]
    decode = names.index("decode32")
    lib = _capi.load()
    keep = []
    try:
        for case in range(48):
            M = int(rng.choice([1, 7, 16, 32, 33, 64, 100, 128, 200, 257, 512]))
            N = int(rng.integers(1, 400)) * 4
            K = int(rng.integers(1, 40)) * 64
            cfg = decode if (M <= 32 and case % 3 == 0) else int(rng.choice(real))
            fmt = 2 if (names[cfg].startswith("wr") or (cfg == decode and case % 2)) else 1
            qx = rng.integers(-127, 128, size=(M, K), dtype=np.int8)
            qw = rng.integers(-128, 128, size=(N, K), dtype=np.int8)
            want = (qx.astype(np.int64) @ qw.astype(np.int64).T).astype(np.float64) * 2.0 ** -14
            want16 = want.astype(np.float16)
            sx = torch.full((M, 1), 2.0 ** -7, dtype=torch.float16, device=DEV)
            sw = torch.full((1, N), 2.0 ** -7, dtype=torch.float16, device=DEV)
            assert lib.mixq_gemm_set_config(cfg) == 0
            for rep in range(3):
                keep.append(torch.empty((case * 3 + rep + 1) * 1_000_003, dtype=torch.uint8, device=DEV))   # shift addresses
                qxp, qwp = mixlib.PackOperand(t(qx), 1), mixlib.PackOperand(t(qw), fmt)
                y = n(mixlib.FusedLinear(qxp, qwp, sx, sw, None, None, 0, None, M, N, K))
                assert np.array_equal(bits(y), bits(want16)), (names[cfg], M, N, K, rep)
            if len(keep) > 24:
                del keep[:12]
    finally:
        lib.mixq_gemm_set_config(-1)


def test_randomized_quantise_family_bit_exact():
    """Random shapes, row strides, outlier sets (incl. device-side counts smaller than the capacity), both bit widths, plain
    and packed outputs, extreme values (zero rows, fp16 max, denormals): fused extract + quantise, the fused RMSNorm form and
    outlier detection against the oracle, bit for bit."""
    rng = np.random.default_rng(77)
    for case in range(60):
        bit = int(rng.choice([8, 4]))
        K = int(rng.integers(1, 48)) * 64 if rng.random() < 0.8 else int(rng.choice([8192, 11008, 16384, 28672]))
        M = int(rng.choice([1, 3, 16, 17, 64, 130]))
        ldx = K + int(rng.choice([0, 8, 64]))
        ncap = int(rng.choice([0, 1, 7, 41, 128, 200])) if K >= 256 else int(rng.choice([0, 1, 5]))
        ncap = min(ncap, K)
        packed = int(rng.choice([0, 1, 2])) if ((K if bit == 8 else K // 2) % 64 == 0) else 0
        assert _capi.load().mixq_quant_set_config(int(rng.integers(-1, 10))) == 0            # every launch geometry, same bytes
        x = rng.standard_normal((M, K)).astype(np.float16)
        ind = rng.choice(K, ncap, replace=False).astype(np.int32)
        x[:, ind] *= 20
        if case % 5 == 0:
            x[0] = 0                                            # all-zero row: scale 0, q 0
        if case % 7 == 0:                                        # fp16 max and denormals (finite: inf/nan inputs are not defined)
            free = np.setdiff1d(np.arange(K), ind)[:4]
            x[M - 1, free] = np.array([65504, -65504, 6e-8, -6e-8], dtype=np.float16)[: free.size]
        n_used = ncap if (ncap == 0 or rng.random() < 0.5) else int(rng.integers(0, ncap + 1))
        buf = torch.zeros((M, ldx), dtype=torch.float16, device=DEV)
        buf[:, :K] = t(x)
        xv = buf[:, :K]
        xs = torch.zeros((M, 1), dtype=torch.float16, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        n_dev = torch.tensor([n_used], dtype=torch.int32, device=DEV) if n_used != ncap else None
        q, xo = mixlib.QuantFused(xv, t(ind) if ncap else None, xs, bit, 6.0, flag=flag, n_dev=n_dev, fmt=packed)
        xz = x.copy()
        xo_ref = O.extract_outliers_zero(xz, ind[:n_used])
        qo, so = O.find_row_scale(xz, bit)
        KB = K if bit == 8 else K // 2
        got_q = packed_unpack(n(q).reshape(-1).view(np.uint8), M, KB, packed) if packed else n(q).view(np.uint8)
        ctx = (case, M, K, bit, ncap, n_used, packed, ldx)
        assert np.array_equal(got_q, qo.view(np.uint8)), ctx
        assert np.array_equal(bits(n(xs)[:, 0]), bits(so)), ctx
        assert np.array_equal(bits(n(xv)), bits(xz)), ctx
        if n_used:
            assert np.array_equal(bits(n(xo)[:, :n_used]), bits(xo_ref)), ctx
        assert bool(flag.item()) == O.mispredicted(so, 6.0, bit), ctx
        # detection on the (now zeroed) tensor and on the original
        ibuf, cnt = mixlib.DetectOutlierCols(t(x), 6.0)
        assert np.array_equal(n(ibuf)[: int(cnt.item())], O.find_outliers(x, 6.0)), ctx
        # fused RMSNorm + quantise over the same input
        if K <= 32768:
            w = (rng.random(K) + 0.5).astype(np.float16)
            out = torch.empty((M, K), dtype=torch.float16, device=DEV)
            xs2 = torch.zeros((M, 1), dtype=torch.float16, device=DEV)
            q2, xo2 = mixlib.RMSNormQuantFused(t(x), t(w), out, 1e-5, t(ind) if ncap else None, xs2, bit, fmt=packed)
            y_ref, xo_r, q_r, s_r = O.rmsnorm_quant(x, w, 1e-5, ind, bit)
            got2 = packed_unpack(n(q2).reshape(-1).view(np.uint8), M, KB, packed) if packed else n(q2).view(np.uint8)
            assert np.array_equal(bits(n(out)), bits(y_ref)), ctx
            assert np.array_equal(got2, q_r.view(np.uint8)), ctx
            assert np.array_equal(bits(n(xs2)[:, 0]), bits(s_r)), ctx
            if ncap:
                assert np.array_equal(bits(n(xo2)), bits(xo_r)), ctx


@pytest.mark.parametrize("bit", [8, 4])
def test_division_free_quantiser_is_exact_for_every_fp16_pair(bit):
    """The quantise kernels compute q = rint(x / s) as x * (1/s) + a tie fix-up (common.h: quant_exact).  The library's
    self-test compares it with the IEEE-division form for ALL finite fp16 x and all finite fp16 s > 0 (~2e9 pairs)."""
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    _capi.call("mixq_selftest_quant_exact", cnt.data_ptr(), bit, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 0


def test_batch_larger_than_the_cache_is_refused_not_overrun():
    """The reference silently relies on M <= MixLibCache.inputdim; here it is an error, never a buffer overrun."""
    lin = torch.nn.Linear(128, 64, bias=False).half()
    cache = MixLibCache(16)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    with pytest.raises(RuntimeError, match="x_scale holds 16 rows"):
        layer(torch.randn(32, 128, device=DEV).half(), None, True)


@pytest.mark.parametrize("M,N,K,bit,n_out,bias", [(96, 320, 1024, 8, 17, True), (16, 256, 512, 8, 5, False), (40, 64, 1024, 4, 16, False),
                                                 (512, 1536, 4096, 8, 41, False), (16, 256, 512, 8, 5, True), (130, 200, 512, 4, 32, True)])
@pytest.mark.parametrize("packed", [0, 1, 2])
def test_silu_times_multiplier_epilogue(M, N, K, bit, n_out, bias, packed):
    """MIXQ_ACT_SILU_MUL: y = (silu(dequant + outliers) + bias) * mul in the GEMM epilogue (gate_proj with up_proj's output
    as the multiplier; bias BEFORE the product as linear.py:372-373 + mlp.py:61 compute it), tiled,
    weights-in-registers and decode kernels, against the oracle."""
    c = _fused_case(M, N, K, bit, seed=M + N + K + 5, n_out=n_out, bias=bias, addend=True, act=2)
    y = n(_run_fused(c, packed)).astype(np.float32)
    ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], addend=c["addend"], bias=c["bias"], act=2,
                         bit=bit).astype(np.float32)
    assert np.isfinite(y).all()
    assert (np.abs(y - ref) <= ulp_tol(ref)).all(), float(np.abs(y - ref).max())
    # and it is what the two-step form computes, up to the extra rounding of the intermediate
    c1 = dict(c); c1["act"] = 1; c1["addend"] = None; c1["bias"] = None
    two_step = n(_run_fused(c1, packed)).astype(np.float32)
    if c["bias"] is not None:
        two_step = (two_step.astype(np.float16) + c["bias"]).astype(np.float32)        # the reference's fp16 `y1 += self.bias`
    two_step = two_step * c["addend"].astype(np.float32)
    assert (np.abs(y - two_step) <= 2 * ulp_tol(ref) + 4e-3 * np.abs(ref) + 2e-3 * np.abs(c["addend"].astype(np.float32))).all()


def test_silu_mul_needs_its_multiplier():
    c = _fused_case(8, 64, 128, 8, seed=1, n_out=0, bias=False, addend=False, act=2)
    with pytest.raises(RuntimeError):
        _run_fused(c, True)
    lib = _capi.load()
    one = torch.zeros(64, dtype=torch.int8, device=DEV)
    assert lib.mixq_gemm_i8_fused(one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), None, 0, None, 0, 0, None, None, 0,
                                  None, one.data_ptr(), 64, 4, 64, 128, 2, 0, None) == _capi.MIXQ_EINVAL


# ---------------------------------------------------------------------------------------------------------------
# round 2: the holes VERDICT r01 listed
# ---------------------------------------------------------------------------------------------------------------
def _wr_configs():
    # (the pairwise split-K form needs a workspace and 2 x tiles <= CUs: it has its own tests in test_gpu_round3.py)
    return [i for i, name in enumerate(_capi.gemm_config_names()) if name.startswith("wr") and "abl" not in name and "self" not in name and not name.endswith(("_k2", "_pair"))]


def _tiled_configs():
    return [i for i, name in enumerate(_capi.gemm_config_names())
            if "abl" not in name and not name.startswith(("sk", "wr", "decode"))]


def test_baseline_config0_batch32_full_output():
    """BASELINE config 0 on the HIP path: ONE MixQLinear 4096 -> 11008 W8A8O16 at batch 32 with 1 % (41) outlier columns,
    through the operator, the FULL output against the oracle's restatement and the north-star gate (CPU Linear over the same
    dequantised operands, |d|inf <= 1e-2)."""
    M, K, N = 32, 4096, 11008
    torch.manual_seed(0)
    lin = torch.nn.Linear(K, N, bias=False).half()
    cols = torch.randperm(K, generator=torch.Generator().manual_seed(1))[:41]
    cache = MixLibCache(M, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    qw0, sw0 = n(layer.q_weight), n(layer.scale_col)
    for call in range(3):
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(20 + call)).half()
        x[:, cols] *= 20
        y = layer(x.to(DEV), None, True)
    assert layer.add_outliers is False and set(cols.tolist()) <= set(n(layer.ind).tolist())
    ind = n(layer.ind).astype(np.int32)
    xh = x.numpy().copy()
    xo = O.extract_outliers_zero(xh, ind)
    qx, sx = O.find_row_scale(xh, 8)
    wo = n(layer.weight_cache)
    ref = O.linear_fused(qx, qw0, sx, sw0, xo=xo, wo=wo).astype(np.float32)
    got = n(y).astype(np.float32)
    assert (np.abs(got - ref) <= ulp_tol(ref)).all(), float(np.abs(got - ref).max())
    gate = O.linear_dequant_ref(qx, qw0, sx, sw0, xo=xo, ind=ind, wo=wo)
    a = np.abs(gate)
    ulp1 = 2.0 ** (np.floor(np.log2(np.maximum(a, 1.0))) - 10)
    assert (np.abs(got - gate) <= np.maximum(GATE, ulp1)).all(), float(np.abs(got - gate).max())
    assert np.abs(got - gate)[a < 8].max() <= GATE
    # the layer now holds only the packed weight image; the reference-layout q_weight it serves is still the original
    assert layer._buffers["q_weight"] is None and np.array_equal(n(layer.q_weight), qw0)


@pytest.mark.parametrize("n_out", [129, 143, 287])
@pytest.mark.parametrize("M", [16, 96])
def test_more_than_128_outlier_columns_every_kernel_family(n_out, M):
    """1 % of K = 14336 / 28672 is 143 / 287 columns and the reference only stops ADDING after > 128 (linear.py:225): the fp16
    tail's register ring changes regime there.  Tiled, stream-K, weights-in-registers and (M <= 32) decode kernels vs the oracle."""
    _capi.ensure_workspace(DEV)
    N, K = 320, 1024
    c = _fused_case(M, N, K, 8, seed=n_out + M, n_out=n_out, bias=True, addend=False, act=0)
    ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], bias=c["bias"], bit=8).astype(np.float32)
    names = _capi.gemm_config_names()
    lib = _capi.load()
    fam = [(cfg, 1) for cfg in _tiled_configs()[:6] + _sk_configs()] + [(cfg, 2) for cfg in _wr_configs()]
    if M <= 32:
        fam += [(_skinny_id(), 1), (_skinny_id(), 2)]
    try:
        for cfg, fmt in fam:
            assert lib.mixq_gemm_set_config(cfg) == 0
            y = n(_run_fused(c, fmt)).astype(np.float32)
            assert np.isfinite(y).all(), names[cfg]
            assert (np.abs(y - ref) <= ulp_tol(ref)).all(), (names[cfg], float(np.abs(y - ref).max()))
    finally:
        lib.mixq_gemm_set_config(-1)


@pytest.mark.parametrize("n_out", [1, 16, 65, 128, 129, 200, 257])
def test_int4_outlier_tail_staged_through_lds_every_tiling(n_out):
    """The int4 kernels copy the outlier tail's operands into the idle ring with the loader waves and run the tail out of LDS, in
    passes of 128 columns (gemm.hip, TAIL_LDS): one column, exactly one pass, one column more, two passes and a bit - every LDS-staged
    tiling (and the ones without loader waves, which keep the register ring), ragged M and N, against the oracle; and the device-side
    count (n_out_dev < capacity, poison behind it) must give the same bits."""
    M, N, K = 200, 328, 512
    c = _fused_case(M, N, K, 4, seed=900 + n_out, n_out=n_out, bias=True, addend=False, act=0)
    ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], bias=c["bias"], bit=4).astype(np.float32)
    names = _capi.gemm_config_names()
    lib = _capi.load()
    try:
        for cfg in _tiled_configs():
            assert lib.mixq_gemm_set_config(cfg) == 0
            y = n(_run_fused(c, 1))
            assert (np.abs(y.astype(np.float32) - ref) <= ulp_tol(ref)).all(), (names[cfg], float(np.abs(y.astype(np.float32) - ref).max()))
            y_dev = n(_run_fused(c, 1, n_dev_cap=n_out + 23))
            assert np.array_equal(bits(y), bits(y_dev)), names[cfg]
    finally:
        lib.mixq_gemm_set_config(-1)


@pytest.mark.parametrize("K,N", [(8192, 8192), (8192, 28672), (14336, 4096)])
def test_full_size_operator_70b_and_long_k_with_one_percent_outliers(K, N):
    """Operator-level forward at the Llama-2-70b shapes (and Llama-3's down projection) with 1 % outlier columns (82 / 143:
    more than 128 at K = 14336), sampled rows against the oracle and the gate."""
    M = 512
    torch.manual_seed(0)
    lin = torch.nn.Linear(K, N, bias=False).half()
    cols = torch.randperm(K, generator=torch.Generator().manual_seed(1))[: round(0.01 * K)]
    cache = MixLibCache(M, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    del lin
    for call in range(3):
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(10 + call)).half()
        x[:, cols] *= 20
        y = layer(x.to(DEV), None, True)
    assert layer.add_outliers is False and set(cols.tolist()) <= set(n(layer.ind).tolist())
    rows = [0, 255, 511]
    xh = x.numpy()[rows].copy()
    ind = n(layer.ind).astype(np.int32)
    xo = O.extract_outliers_zero(xh, ind)
    qx, sx = O.find_row_scale(xh, 8)
    qw, sw, wo = n(layer.q_weight), n(layer.scale_col), n(layer.weight_cache)
    ref = O.linear_fused(qx, qw, sx, sw, xo=xo, wo=wo).astype(np.float32)
    got = n(y)[rows].astype(np.float32)
    assert (np.abs(got - ref) <= ulp_tol(ref)).all(), float(np.abs(got - ref).max())
    gate = O.linear_dequant_ref(qx, qw, sx, sw, xo=xo, ind=ind, wo=wo)
    a = np.abs(gate)
    assert (np.abs(got - gate) <= np.maximum(GATE, 2.0 ** (np.floor(np.log2(np.maximum(a, 1.0))) - 10))).all()


@pytest.mark.parametrize("K,N", [(4096, 4096), (4096, 12288)])
def test_full_size_w4a4_operator(K, N):
    """BASELINE config 2 (W4A4O16, 128 static fp16 columns) at the q/k/v/o and fused-QKV shapes, sampled rows vs the oracle."""
    M = 512
    torch.manual_seed(0)
    lin = torch.nn.Linear(K, N, bias=False).half()
    cols = torch.randperm(K, generator=torch.Generator().manual_seed(1))[:128]
    scales = torch.ones(K); scales[cols] = 20.0 + torch.arange(128) * 1e-3
    cache = MixLibCache(M, bit=4, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 4, cache=cache, layer_scales=scales, dev=DEV)
    for call in range(3):
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(30 + call)).half()
        x[:, cols] *= 20
        y = layer(x.to(DEV), None, True)
    rows = [0, 100, 511]
    xh = x.numpy()[rows].copy()
    ind = n(layer.ind).astype(np.int32)
    xo = O.extract_outliers_zero(xh, ind)
    qx, sx = O.find_row_scale(xh, 4)
    ref = O.linear_fused(qx, n(layer.q_weight), sx, n(layer.scale_col), xo=xo, wo=n(layer.weight_cache), bit=4).astype(np.float32)
    got = n(y)[rows].astype(np.float32)
    assert (np.abs(got - ref) <= ulp_tol(ref)).all(), float(np.abs(got - ref).max())


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,bit,n_out,cap", [(96, 320, 1024, 8, 17, 32), (20, 256, 512, 8, 41, 48), (64, 128, 512, 4, 100, 128),
                                                 (130, 200, 512, 8, 0, 16), (512, 1536, 4096, 8, 41, 48)])
def test_gemm_reads_the_outlier_count_from_device_memory(M, N, K, bit, n_out, cap, fmt):
    """n_out_dev (kernel.py:108-111: the Triton kernel loads its K from memory): the operands have CAPACITY `cap`, the live count
    sits in device memory, everything beyond it is poison (NaN) and must not reach the result."""
    c = _fused_case(M, N, K, bit, seed=M + cap, n_out=n_out, bias=True, addend=False, act=0)
    ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], bias=c["bias"], bit=bit).astype(np.float32)
    y = n(_run_fused(c, fmt, n_dev_cap=cap)).astype(np.float32)
    assert np.isfinite(y).all()
    assert (np.abs(y - ref) <= ulp_tol(ref)).all(), float(np.abs(y - ref).max())
    assert np.array_equal(bits(n(_run_fused(c, fmt))), bits(n(_run_fused(c, fmt, n_dev_cap=cap))))      # same bits as the host count


def test_operator_at_prefill_batch_sizes_ragged_m():
    """M = 4099 tokens (33 M-tiles of 128, the last one 3 rows) through the operator: sampled rows against the oracle, every row against
    the first-128-row result of the same layer (rows are independent: a row's output must not depend on the batch it arrives in)."""
    M, K, N = 4099, 1024, 768
    torch.manual_seed(0)
    lin = torch.nn.Linear(K, N, bias=True).half()
    cache = MixLibCache(M, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    cols = [5, 130, 1000]
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(1)).half()
    x[:, cols] *= 25
    for _ in range(3):
        y = layer(x.clone().to(DEV), None, True)
    assert layer.add_outliers is False and set(cols) <= set(n(layer.ind).tolist())
    rows = [0, 127, 128, 2047, 4095, 4096, 4098]
    ind = n(layer.ind).astype(np.int32)
    xh = x.numpy()[rows].copy()
    xo = O.extract_outliers_zero(xh, ind)
    qx, sx = O.find_row_scale(xh, 8)
    ref = O.linear_fused(qx, n(layer.q_weight), sx, n(layer.scale_col), xo=xo, wo=n(layer.weight_cache), bias=n(layer.bias)).astype(np.float32)
    got = n(y)[rows].astype(np.float32)
    assert (np.abs(got - ref) <= ulp_tol(ref)).all(), float(np.abs(got - ref).max())
    cache2 = MixLibCache(128, device=DEV)
    y_small = layer(x[4096 - 125:4096 + 3].clone().to(DEV), cache2, True)
    assert torch.equal(y_small, y[4096 - 125:4096 + 3])


def test_module_apply_carries_the_packed_only_weights():
    """After compaction the weights exist only as the packed image, a plain attribute nn.Module.to() / .cuda() would not touch:
    _apply moves it with the module and drops every cache derived from the old tensors.  (One GPU here: the walk is exercised with
    a cloning function, and with .to() / .half() as no-ops.)"""
    M, K, N = 48, 512, 320
    torch.manual_seed(4)
    lin = torch.nn.Linear(K, N, bias=True).half()
    cache = MixLibCache(M, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(5)).half()
    x[:, [7, 300]] *= 30
    for _ in range(3):
        y0 = layer(x.clone().to(DEV), None, True)
    assert layer._buffers["q_weight"] is None and layer.ind.numel() == 2
    old = layer._wpk
    layer._apply(lambda t: t.clone())
    assert layer._wpk is not old and mixlib.fmt_of(layer._wpk) == mixlib.fmt_of(old) and torch.equal(layer._wpk, old)
    y1 = layer(x.clone().to(DEV), None, True)
    assert torch.equal(y0, y1)
    layer.to(DEV).half()
    assert torch.equal(layer(x.clone().to(DEV), None, True), y0)
    sd = layer.state_dict()
    assert sd["q_weight"].shape == (N, K) and sd["q_weight"].dtype == torch.int8


def test_operator_runs_on_the_device_count():
    """The operator hands the kernels `ind` / outlier operands of capacity pad16(n) with the count in `cache.n_dev`: after
    the search froze, lowering the DEVICE count (no host-side change, nothing re-captured) drops exactly those columns."""
    M, K, N = 64, 512, 256
    torch.manual_seed(1)
    lin = torch.nn.Linear(K, N, bias=False).half()
    cache = MixLibCache(M, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    cols = [3, 77, 200, 411, 500]
    x0 = torch.randn(M, K, generator=torch.Generator().manual_seed(2)).half()
    x0[:, cols] *= 20
    for _ in range(3):
        y = layer(x0.clone().to(DEV), None, True)
    assert n(layer.ind).tolist() == cols and cache.n_dev is layer._n_dev and int(layer._n_dev.item()) == 5
    qw, sw, wo = n(layer.q_weight), n(layer.scale_col), n(layer.weight_cache)
    def oracle_y(k):
        xh = x0.numpy().copy()
        ind = np.array(cols[:k], np.int32)
        xo = O.extract_outliers_zero(xh, ind)
        qx, sx = O.find_row_scale(xh, 8)
        return O.linear_fused(qx, qw, sx, sw, xo=xo, wo=wo[:, :k]).astype(np.float32)
    assert (np.abs(n(y).astype(np.float32) - oracle_y(5)) <= ulp_tol(oracle_y(5))).all()
    layer._n_dev.fill_(3)                                  # device-side edit only
    y3 = layer(x0.clone().to(DEV), None, True)
    assert (np.abs(n(y3).astype(np.float32) - oracle_y(3)) <= ulp_tol(oracle_y(3))).all()
    layer._n_dev.fill_(5)


def _check_trace_call(g, i, layer, cache, x, y, M, KB):
    assert np.array_equal(n(layer.ind), g[f"c{i}_ind"]), f"call {i}: ind"
    assert layer.cnt == int(g[f"c{i}_cnt"]) and layer.add_outliers == bool(g[f"c{i}_add_outliers"]), f"call {i}: state"
    assert np.array_equal(bits(n(cache.x_scale)[:M]), bits(g[f"c{i}_x_scale"])), f"call {i}: x_scale"
    assert np.array_equal(_unpacked_q(cache, M, KB), g[f"c{i}_q_xcache"].view(np.uint8)), f"call {i}: q_xcache"
    assert np.array_equal(bits(n(x)), bits(g[f"c{i}_x_after"])), f"call {i}: in-place mutation of x"
    if f"c{i}_weight_cache" in g.files and layer.ind.numel():
        assert np.array_equal(bits(n(layer.weight_cache)), bits(g[f"c{i}_weight_cache"]))
    if f"c{i}_activation_outliers" in g.files:
        assert np.array_equal(bits(n(cache.activation_outliers)), bits(g[f"c{i}_activation_outliers"]))
    assert tuple(y.shape) == g[f"c{i}_y"].shape
    assert np.abs(n(y).astype(np.float32) - g[f"c{i}_y"].astype(np.float32)).max() <= 4e-3, f"call {i}: y"


def test_operator_trace_w8_caller_filled_cache_on_gpu(golden):
    """G5b (recorded from the reference's own forward, linear.py:165-289 with unfused=False): the caller - here the reference's
    k2 + k1 pair through the mixlib surface, PLAIN layout - has filled cache.q_xcache / x_scale / activation_outliers."""
    g, g2 = golden("g5b_forward_w8_fused_cache.npz"), golden("g2_from_linear_w8.npz")
    lin = torch.nn.Linear(256, 96, bias=False).half()
    lin.weight.data.copy_(torch.from_numpy(g2["weight"]))
    cache = MixLibCache(64, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    for i in range(int(g["ncalls"])):
        x = t(g[f"c{i}_x_in"])
        inputs = x.reshape(-1, x.shape[-1])
        if layer.ind.shape[0]:
            cache.activation_outliers = mixlib.ExtractOutliersAndSetToZeros(layer.ind, inputs)
        cache.q_xcache = mixlib.FindRowScale(inputs, cache.x_scale, inputs.shape[0], 256, 8)
        y = layer(x, cache, False)
        assert tuple(y.shape) == (2, 16, 96) and cache.shape == (2, 16, 96)
        _check_trace_call(g, i, layer, cache, x, y, 32, 256)


def test_operator_trace_w8_no_outliers_on_gpu(golden):
    """G5c: activations that never cross sigma - the reference's zeros-addend path (linear.py:268-273); no scan is ever run."""
    g, g2 = golden("g5c_forward_w8_no_outliers.npz"), golden("g2_from_linear_w8.npz")
    lin = torch.nn.Linear(256, 96, bias=True).half()
    lin.weight.data.copy_(torch.from_numpy(g2["weight"]))
    lin.bias.data.copy_(torch.from_numpy(g2["bias_in"]))
    cache = MixLibCache(64, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    for i in range(int(g["ncalls"])):
        x = t(g[f"c{i}_x_in"])
        y = layer(x, None, True)
        _check_trace_call(g, i, layer, cache, x, y, 32, 256)
    assert layer.ind.numel() == 0 and layer.weight_cache is None


def test_every_wreg_tiling_full_epilogue_and_int4():
    """Every weights-in-registers tiling x {int8, int4} x {outlier tail, addend, SiLU, bias, SILU_MUL} on ragged shapes against
    the oracle, and - without outlier columns - bit-identical to the LDS-staged kernel of gemm.hip (same exact accumulator,
    same epilogue arithmetic in the same order)."""
    lib = _capi.load()
    names = _capi.gemm_config_names()
    cases = [(100, 260, 512, 8, 17, True, True, 1), (257, 1000, 1024, 8, 41, False, False, 0), (33, 36, 320, 8, 3, True, False, 2),
             (64, 128, 1024, 4, 128, False, False, 0), (130, 200, 512, 4, 16, True, True, 1), (512, 384, 256, 8, 0, False, False, 0),
             (48, 64, 64, 8, 5, True, False, 0), (70, 132, 192, 8, 0, False, True, 0)]
    try:
        for (M, N, K, bit, n_out, bias, addend, act) in cases:
            c = _fused_case(M, N, K, bit, seed=M + N + K, n_out=n_out, bias=bias, addend=addend or act == 2, act=act)
            ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=c["xo"], wo=c["wo"], addend=c["addend"], bias=c["bias"], act=act,
                                 bit=bit).astype(np.float32)
            lib.mixq_gemm_set_config(names.index("128x128_w2x2_s5_l2"))
            y_lds = n(_run_fused(c, 1))
            for cfg in _wr_configs():
                if bit == 4 and ("self" in names[cfg] or "128x256" in names[cfg]):
                    continue                                # the prefill tiles and 128 x 256 (accumulators + ring + expanded nibbles exceed the registers) have no nibble form
                assert lib.mixq_gemm_set_config(cfg) == 0
                y = n(_run_fused(c, 2))
                assert np.isfinite(y).all(), (names[cfg], M, N, K)
                d = np.abs(y.astype(np.float32) - ref)
                assert (d <= ulp_tol(ref)).all(), (names[cfg], M, N, K, bit, float(d.max()))
                if n_out == 0:     # with outlier columns the two kernels sum the fp16 tail in different MFMA shapes: equal to rounding
                    assert np.array_equal(bits(y), bits(y_lds)), (names[cfg], M, N, K, bit)
    finally:
        lib.mixq_gemm_set_config(-1)


def test_wreg_kernel_under_graph_replay_and_cold_buffers():
    """hipGraph replay of the weights-in-registers kernel (hand-counted vmcnt waits, LDS-DMA ring): 20 replays on shifted
    buffers must reproduce the exact integer result every time."""
    M, N, K = 512, 1536, 4096
    g = torch.Generator().manual_seed(7)
    qx = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int8).to(DEV)
    qw = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8).to(DEV)
    sx = torch.full((M, 1), 2.0 ** -7, dtype=torch.float16, device=DEV)
    sw = torch.full((1, N), 2.0 ** -7, dtype=torch.float16, device=DEV)
    want = ((qx.double() @ qw.double().T) * 2.0 ** -14).to(torch.float16)
    lib = _capi.load()
    keep = []
    try:
        for cfg in _wr_configs():
            assert lib.mixq_gemm_set_config(cfg) == 0
            keep.append(torch.empty((len(keep) + 1) * 2_000_003, dtype=torch.uint8, device=DEV))
            qxp, qwp = mixlib.PackOperand(qx, 1), mixlib.PackOperand(qw, 2)
            out = torch.empty((M, N), dtype=torch.float16, device=DEV)
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                mixlib.FusedLinear(qxp, qwp, sx, sw, None, None, 0, None, M, N, K, out=out)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    for _ in range(5):
                        mixlib.FusedLinear(qxp, qwp, sx, sw, None, None, 0, None, M, N, K, out=out)
                for _ in range(4):
                    out.zero_()
                    graph.replay()
                    torch.cuda.synchronize()
                    assert torch.equal(out, want), _capi.gemm_config_names()[cfg]
    finally:
        lib.mixq_gemm_set_config(-1)


@pytest.mark.parametrize("route", ["arch9", "fused"])
def test_fused_outliers_behind_the_reference_call_sequence(route):
    """mixlib.configure(fused_outliers=True): the reference's own sequence - ExtractOutliersAndSetToZeros, FindRowScale, torch.mm(activation_outliers,
    weight_cache.T), then gemm + dequantizeInt8 (linear.py:234-241) or int8FusedDequantize (:248-256) - runs the outlier product as the
    fp16 tail of the int8 GEMM.  Same bits as the native operator's kernel on the same operands; within 2 fp16 ulp of the literal
    route (which rounds the product to fp16 first); every other use of the deferred product still sees torch.mm's values."""
    M, K, N = 96, 1024, 640
    c = _fused_case(M, N, K, 8, seed=77, n_out=41, bias=False, addend=False, act=0)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).half()
    ind = torch.from_numpy(np.sort(np.random.default_rng(4).choice(K, 41, replace=False)).astype(np.int32)).to(DEV)
    x[:, ind.cpu().long()] *= 20
    q_weight, scale_col = t(c["qw"]), t(c["sw"]).reshape(1, N)
    weight_cache = (torch.randn(N, 41, generator=torch.Generator().manual_seed(5)) / 8).half().to(DEV)       # plain [N,41]: unpadded pitch
    x_scale = torch.zeros((M, 1), dtype=torch.float16, device=DEV)

    def run():
        xd = x.clone().to(DEV)
        xo = mixlib.ExtractOutliersAndSetToZeros(ind, xd)
        qx = mixlib.FindRowScale(xd, x_scale, M, K, 8)
        mm = torch.mm(xo, weight_cache.T)
        if route == "arch9":
            return mixlib.dequantizeInt8(mixlib.gemm(qx, q_weight, M, N, K), x_scale, scale_col, mm, 8, M, N), xo, mm, qx
        return mixlib.int8FusedDequantize(qx, q_weight, x_scale, scale_col, mm, M, N, K), xo, mm, qx

    y_lit, xo_lit, mm_lit, qx = run()
    assert type(mm_lit) is torch.Tensor
    prev = mixlib.configure(fused_outliers=True)
    try:
        y_f, xo_f, mm_f, _ = run()
        assert isinstance(xo_f, mixlib.OutlierActivations) and isinstance(mm_f, mixlib.PendingOutlierProduct)
        assert mm_f._mixq_done is False and tuple(mm_f.shape) == (M, N)                 # consumed by the GEMM, never computed
        assert torch.equal(xo_f.as_subclass(torch.Tensor), xo_lit)
        # the same operands through the native entry point (padded outlier operands, one fused kernel)
        wo = torch.zeros((N, 48), dtype=torch.float16, device=DEV); wo[:, :41] = weight_cache
        xo = torch.zeros((M, 48), dtype=torch.float16, device=DEV); xo[:, :41] = xo_lit
        y_nat = mixlib.FusedLinear(qx, q_weight, x_scale, scale_col, xo[:, :41], wo[:, :41], 41, None, M, N, K)
        assert torch.equal(y_f, y_nat)
        d = (y_f.float() - y_lit.float()).abs()
        assert (d <= 2 * torch.from_numpy(ulp_tol(n(y_lit).astype(np.float32))).to(DEV)).all(), float(d.max())
        # any other use of the deferred product computes it: same values as the plain torch.mm
        _, _, mm2, _ = run()
        assert torch.equal(mm2 + 0, mm_lit) and mm2._mixq_done is True
        # a product that was already looked at goes in as an ordinary addend
        _, xo3, _, qx3 = run()
        mm3 = torch.mm(xo3, weight_cache.T); _ = mm3.sum()
        y3 = mixlib.int8FusedDequantize(qx3, q_weight, x_scale, scale_col, mm3, M, N, K)
        assert torch.equal(y3, mixlib.int8FusedDequantize(qx3, q_weight, x_scale, scale_col, mm_lit, M, N, K))
    finally:
        mixlib.configure(prev)


def test_fused_prepass_behind_the_reference_call_sequence():
    """mixlib.configure(fused_outliers=True, fused_prepass=True): ExtractOutliersAndSetToZeros is deferred and FindRowScale on the same tensor
    runs the one-pass extract + zero + scale + quantise kernel.  Same q_x, x_scale, x_out and zeroed x as the two separate calls; a
    deferred extraction that FindRowScale never picks up runs as soon as its result is touched, or before the next prepass call."""
    M, K = 70, 1024
    rng = np.random.default_rng(12)
    x0 = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float16))
    ind = torch.from_numpy(np.sort(rng.choice(K, 19, replace=False)).astype(np.int32)).to(DEV)
    x0[:, ind.cpu().long()] *= 20
    xs_a = torch.zeros((M, 1), dtype=torch.float16, device=DEV)
    xs_b = torch.zeros((M, 1), dtype=torch.float16, device=DEV)
    xa = x0.clone().to(DEV)
    xo_a = mixlib.ExtractOutliersAndSetToZeros(ind, xa)
    q_a = mixlib.FindRowScale(xa, xs_a, M, K, 8)
    po = mixlib.configure(fused_outliers=True, fused_prepass=True)
    try:
        xb = x0.clone().to(DEV)
        xo_b = mixlib.ExtractOutliersAndSetToZeros(ind, xb)
        assert "_mixq_pending" in xo_b.__dict__ and torch.equal(xb.cpu(), x0)             # nothing has run yet
        q_b = mixlib.FindRowScale(xb, xs_b, M, K, 8)
        assert "_mixq_pending" not in xo_b.__dict__
        assert torch.equal(q_b, q_a) and torch.equal(xs_b, xs_a) and torch.equal(xb, xa)
        assert torch.equal(xo_b.as_subclass(torch.Tensor), xo_a)
        # never picked up: touching the result runs the extraction
        xc = x0.clone().to(DEV)
        xo_c = mixlib.ExtractOutliersAndSetToZeros(ind, xc)
        assert torch.equal(xo_c + 0, xo_a) and torch.equal(xc, xa)
        # ... also when it sits inside a sequence argument (the reference's torch.hstack((cache.activation_outliers, new)), linear.py:212)
        xf_ = x0.clone().to(DEV)
        xo_f = mixlib.ExtractOutliersAndSetToZeros(ind, xf_)
        both = torch.hstack((xo_f, xo_a))
        assert torch.equal(both[:, :19], xo_a) and torch.equal(xf_, xa) and type(both) is torch.Tensor
        # ... and so does the next prepass call, in program order
        xd, xe = x0.clone().to(DEV), x0.clone().to(DEV)
        xo_d = mixlib.ExtractOutliersAndSetToZeros(ind, xd)
        q_e = mixlib.FindRowScale(xe, xs_b, M, K, 8)                                       # another tensor: xd's extraction runs first
        assert torch.equal(xd, xa) and torch.equal(xo_d.as_subclass(torch.Tensor), xo_a)
        assert not torch.equal(q_e, q_a)                                                   # xe still had its outliers
    finally:
        mixlib.configure(po)


def test_gemm_shim_refuses_operands_that_do_not_match_m_n_k():
    """The reference's arch == 9 route calls mixlib.gemm for 4-bit layers too (linear.py:235) with nibble-packed [., K/2] operands and
    the full K: a byte GEMM over them would read past both buffers, so the shim raises instead of launching."""
    M, N, K = 32, 64, 128
    qx = torch.zeros((M, K // 2), dtype=torch.uint8, device="cuda")
    qw = torch.zeros((N, K // 2), dtype=torch.uint8, device="cuda")
    for lazy in (True, False):
        prev = mixlib.configure(lazy_gemm=lazy)
        try:
            with pytest.raises(RuntimeError, match="nibble-packed"):
                mixlib.gemm(qx, qw, M, N, K)
            with pytest.raises(RuntimeError, match="one-byte"):
                mixlib.gemm(torch.zeros((M, K), dtype=torch.int32, device="cuda"), torch.zeros((N, K), dtype=torch.int8, device="cuda"), M, N, K)
        finally:
            mixlib.configure(prev)


@pytest.mark.parametrize("lazy", [True, False])
def test_reference_arch9_route_at_the_metric_shape(lazy):
    """torch reports gfx950 as capability major 9, so the UNCHANGED reference forward takes linear.py:234-241:
    y = mixlib.gemm(q, W, M, N, K); outliers_fp16 = torch.mm(X_out, weight_cache.T); y1 = mixlib.dequantizeInt8(y, x_scale,
    scale_col, outliers_fp16, 8, M, N).  That exact sequence at 512 x 4096 -> 11008 through the mixlib surface: with the deferred
    product (one fused kernel) and with the literal pair (int32 round trip + vectorised dequantisation), against the oracle on
    sampled rows; the two forms agree bit for bit."""
    assert torch.cuda.get_device_capability()[0] == 9, "INTEGRATION.md states that gfx950 reports major 9"
    M, K, N = 512, 4096, 11008
    prev = mixlib.configure(lazy_gemm=lazy)
    try:
        torch.manual_seed(0)
        W = (torch.randn(N, K) / 64).half()
        qw_h, sw_h = O.quant_weight_w8(W.numpy())
        cols = np.sort(np.random.default_rng(1).choice(K, 41, replace=False)).astype(np.int32)
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).half()
        x[:, cols.tolist()] *= 20
        cache = MixLibCache(M, device=DEV)
        q_weight, scale_col, ind = t(qw_h), t(sw_h), t(cols)
        weight_cache = mixlib.DequantWeightCols(q_weight, scale_col, ind, 8)
        inputs = x.to(DEV)
        # --- linear.py:187-193 and :234-241, verbatim modulo `self.` ---
        cache.activation_outliers = mixlib.ExtractOutliersAndSetToZeros(ind, inputs)
        cache.q_xcache = mixlib.FindRowScale(inputs, cache.x_scale, inputs.shape[0], K, 8)
        y = mixlib.gemm(cache.q_xcache, q_weight, M, N, K)
        assert tuple(y.shape) == (M, N) and y.dtype == torch.int32
        outliers_fp16 = torch.mm(cache.activation_outliers, weight_cache.T)
        y1 = mixlib.dequantizeInt8(y, cache.x_scale, scale_col, outliers_fp16, 8, M, N)
        y0 = mixlib.dequantizeInt8(mixlib.gemm(cache.q_xcache, q_weight, M, N, K), cache.x_scale, scale_col, cache.zeros, 8, M, N)
        ys = mixlib.dequantizeInt8Silu(mixlib.gemm(cache.q_xcache, q_weight, M, N, K), cache.x_scale, scale_col, cache.zeros, 8, M, N)
        # --- checks ---
        rows = [0, 200, 511]
        qx, sx = n(cache.q_xcache)[rows], n(cache.x_scale)[rows, 0]
        mm16 = n(outliers_fp16)[rows]
        ref = O.linear_fused(qx, qw_h, sx, sw_h, addend=mm16).astype(np.float32)
        assert (np.abs(n(y1)[rows].astype(np.float32) - ref) <= ulp_tol(ref)).all()
        ref0 = O.linear_fused(qx, qw_h, sx, sw_h).astype(np.float32)
        assert (np.abs(n(y0)[rows].astype(np.float32) - ref0) <= ulp_tol(ref0)).all()
        refs = O.linear_fused(qx, qw_h, sx, sw_h, act=1).astype(np.float32)
        assert (np.abs(n(ys)[rows].astype(np.float32) - refs) <= ulp_tol(refs)).all()
        # an integer result somebody really reads is the exact product, whichever way it was produced
        y32 = mixlib.gemm(cache.q_xcache, q_weight, M, N, K)
        assert np.array_equal(n(y32[rows]), O.gemm_i8(qx, qw_h))
        test_reference_arch9_route_at_the_metric_shape.results[lazy] = (y1.clone(), y0.clone(), ys.clone())
    finally:
        mixlib.configure(prev)
    r = test_reference_arch9_route_at_the_metric_shape.results
    if len(r) == 2:
        for a, b in zip(r[True], r[False]):
            assert torch.equal(a, b)


test_reference_arch9_route_at_the_metric_shape.results = {}


def test_reference_style_norm_feeding_our_linear_layouts_do_not_leak():
    """the reference's own fused norm (norm.py:24-33) run through the mixlib shim returns a PLAIN q; a previous
    layer's packed activation must not make the next linear misread it.  The layout travels with the tensor: down_proj
    (unfused=True, packed) then a reference-style norm + linear(unfused=False) equals the all-native path."""
    torch.manual_seed(0)
    K, N, M = 512, 256, 48
    lin_a, lin_b = torch.nn.Linear(K, N, bias=False).half(), torch.nn.Linear(K, K, bias=False).half()
    cache, cache2 = MixLibCache(M, device=DEV), MixLibCache(M, device=DEV)
    nxt, nxt_ref = (MixLinear_GEMM.from_linear(lin_a, 8, cache=c, dev=DEV) for c in (cache, cache2))
    down, down_ref = (MixLinear_GEMM.from_linear(lin_b, 8, cache=c, dev=DEV) for c in (cache, cache2))
    wn = (torch.ones(K) + 0.1 * torch.randn(K)).half().to(DEV)
    cols = [5, 300]
    for call in range(3):
        h = torch.randn(M, K, generator=torch.Generator().manual_seed(call)).half()
        h[:, cols] *= 25
        # layer i: a native unfused linear leaves a PACKED q_xcache in the shared cache
        h1 = down(h.to(DEV).clone(), None, True)
        # layer i+1, reference style: norm.py:18-33 against the shim, then W_pack(x) with unfused=False
        out = torch.empty_like(h1)
        cache.activation_outliers, cache.q_xcache = mixlib.layernorm_forward_cuda_extract_outliers(h1, wn, out, 1e-6, nxt.ind, cache.x_scale)
        y = nxt(out, cache, False)
        # all-native twin
        h1r = down_ref(h.to(DEV).clone(), None, True)
        outr = torch.empty_like(h1r)
        mixlib.layernorm_forward_cuda(h1r, wn, outr, 1e-6)
        yr = nxt_ref(outr, None, True)
        assert torch.equal(h1, h1r) and torch.equal(y, yr), call


def test_shim_argument_checks_and_broadcast_addend():
    c = _fused_case(16, 64, 128, 8, seed=3, n_out=0, bias=False, addend=False, act=0)
    row = (np.arange(64) / 8).astype(np.float16)
    bro = t(row).reshape(1, 64).expand(16, 64)                          # a REAL stride-0 addend: must be added, not dropped
    y = mixlib.int8FusedDequantize(t(c["qx"]), t(c["qw"]), t(c["sx"]).reshape(-1, 1), t(c["sw"]), bro, 16, 64, 128)
    c2 = dict(c); c2["addend"] = np.broadcast_to(row, (16, 64)).copy()
    ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], addend=c2["addend"]).astype(np.float32)
    assert (np.abs(n(y).astype(np.float32) - ref) <= ulp_tol(ref)).all()
    x = torch.randn(8, 64, device=DEV).half()
    xs = torch.zeros(8, 1, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="int32"):
        mixlib.QuantFused(x, torch.tensor([1, 2], device=DEV), xs, 8, 6.0)                     # int64 ind
    with pytest.raises(RuntimeError, match="int32"):
        mixlib.ExtractOutliersAndSetToZeros(torch.tensor([1, 2], device=DEV), x)
    with pytest.raises(RuntimeError, match="contiguous"):
        mixlib.DequantWeightCols(torch.zeros(8, 128, dtype=torch.int8, device=DEV)[:, ::2], xs.reshape(-1), torch.tensor([0], dtype=torch.int32, device=DEV), 8)


def test_packed_only_weights_state_dict_and_memory():
    """After the outlier search froze, a layer keeps ONLY its packed weight image (the first round kept both, 2x
    the reference's weight memory).  state_dict still emits the reference layout, loading it back re-packs, q_weight reads
    the original matrix, new outlier columns can still be dequantised, and the forward is unchanged."""
    torch.manual_seed(0)
    K, N, M = 512, 384, 32
    lin = torch.nn.Linear(K, N, bias=True).half()
    cache = MixLibCache(M, device=DEV)
    layer = MixLinear_GEMM.from_linear(lin, 8, cache=cache, dev=DEV)
    q0 = layer.q_weight.clone()
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(1)).half()
    x[:, 9] *= 30
    ys = [layer(x.clone().to(DEV), None, True) for _ in range(3)]
    assert layer._buffers["q_weight"] is None and layer._wpk is not None
    assert torch.equal(layer.q_weight, q0)
    sd = layer.state_dict()
    assert torch.equal(sd["q_weight"], q0) and sd["q_weight"].dtype == torch.int8 and tuple(sd["q_weight"].shape) == (N, K)
    twin = MixLinear_GEMM(K, N, True, DEV, bit=8, cache=MixLibCache(M, device=DEV))
    twin.load_state_dict(sd)
    for _ in range(3):
        y2 = twin(x.clone().to(DEV), None, True)
    assert torch.equal(y2, ys[-1])
    layer.load_state_dict(sd)                                           # loading into a compacted layer re-creates, then re-packs
    assert torch.equal(layer(x.clone().to(DEV), None, True), ys[-1])
    assert layer._buffers["q_weight"] is None
    got = mixlib.DequantWeightCols(layer.q_weight, layer.scale_col, torch.tensor([3, 500], dtype=torch.int32, device=DEV), 8)
    assert np.array_equal(bits(n(got)), bits(O.dequant_weight_cols(n(q0), n(layer.scale_col), np.array([3, 500], np.int32), 8)))


def test_wreg_every_k_step_count_every_tiling():
    """The weights-in-registers k loop is unrolled by the ring depth with hand-counted vmcnt waits and a guarded tail: every number
    of k-steps from 1 to 24 (and a few long ones) through every tiling, int8 and int4, exact against the integer product."""
    lib = _capi.load()
    names = _capi.gemm_config_names()
    rng = np.random.default_rng(11)
    M, N = 80, 136
    sx = torch.full((M, 1), 2.0 ** -7, dtype=torch.float16, device=DEV)
    sw = torch.full((1, N), 2.0 ** -7, dtype=torch.float16, device=DEV)
    try:
        for nk in list(range(1, 25)) + [31, 47, 64, 65]:
            K = 64 * nk
            qx = rng.integers(-127, 128, size=(M, K), dtype=np.int8)
            qw = rng.integers(-128, 128, size=(N, K), dtype=np.int8)
            want16 = ((qx.astype(np.int64) @ qw.astype(np.int64).T).astype(np.float64) * 2.0 ** -14).astype(np.float16)
            qxp, qwp = mixlib.PackOperand(t(qx), 1), mixlib.PackOperand(t(qw), 2)
            # int4: K/2 bytes per row hold K nibbles; the same byte images read as nibble pairs give another exact problem
            lo = lambda b: np.where((b & 0xF) >= 8, (b & 0xF).astype(np.int64) - 16, (b & 0xF).astype(np.int64))
            hi = lambda b: np.where((b >> 4) >= 8, (b >> 4).astype(np.int64) - 16, (b >> 4).astype(np.int64))
            bx, bw = qx.view(np.uint8), qw.view(np.uint8)
            want4 = ((lo(bx) @ lo(bw).T + hi(bx) @ hi(bw).T).astype(np.float64) * 2.0 ** -6).astype(np.float16)
            sx4 = torch.full((M, 1), 2.0 ** -3, dtype=torch.float16, device=DEV)
            sw4 = torch.full((1, N), 2.0 ** -3, dtype=torch.float16, device=DEV)
            for cfg in _wr_configs():
                assert lib.mixq_gemm_set_config(cfg) == 0
                y = n(mixlib.FusedLinear(qxp, qwp, sx, sw, None, None, 0, None, M, N, K))
                assert np.array_equal(bits(y), bits(want16)), (names[cfg], nk, "int8")
                if "self" in names[cfg] or "128x256" in names[cfg]:
                    continue                                # (no nibble form of the prefill tiles, nor of 128 x 256: registers)
                y4 = n(_i4_call(qxp, qwp, sx4, sw4, M, N, K))
                assert np.array_equal(bits(y4), bits(want4)), (names[cfg], nk, "int4")
    finally:
        lib.mixq_gemm_set_config(-1)


def _i4_call(qxp, qwp, sx4, sw4, M, N, K):
    """The packed int8 images re-read as nibble-packed int4 operands of logical depth 2K (the tag travels with the view)."""
    a, b = qxp.view(torch.uint8), qwp.view(torch.uint8)
    mixlib.set_fmt(a, 1); mixlib.set_fmt(b, 2)
    return mixlib.FusedLinear(a, b, sx4, sw4, None, None, 0, None, M, N, 2 * K, bit=4)


def test_packed_operands_behind_the_reference_call_sequence():
    """mixlib.configure(packed_operands=True): the reference's own sequence (linear.py:187-193, :234-283) with q_xcache an opaque
    P16X64 handle of the reference's shape and the plain weight re-tiled (once) into fragment order - the native kernels behind
    unchanged reference code.  Results equal the plain-operand run bit for bit; a consumer that really reads the integers
    (PendingGemmI32 materialised) still gets the exact product."""
    M, K, N = 100, 512, 384
    c = _fused_case(M, N, K, 8, seed=21, n_out=7, bias=False, addend=False, act=0)
    x = make_x(M, K, seed=22, outlier_cols=c["ind"])
    q_weight, scale_col, ind = t(c["qw"]), t(c["sw"]), t(c["ind"])
    wc = t(c["wo"])
    def ref_sequence():
        cache = MixLibCache(M, device=DEV)
        inputs = t(x)
        cache.activation_outliers = mixlib.ExtractOutliersAndSetToZeros(ind, inputs)
        cache.q_xcache = mixlib.FindRowScale(inputs, cache.x_scale, M, K, 8)
        assert tuple(cache.q_xcache.shape) == (M, K)
        mm = torch.mm(cache.activation_outliers, wc.T)
        y_a = mixlib.int8FusedDequantize(cache.q_xcache, q_weight, cache.x_scale, scale_col, mm, M, N, K)                  # arch != 9
        y_b = mixlib.dequantizeInt8(mixlib.gemm(cache.q_xcache, q_weight, M, N, K), cache.x_scale, scale_col, mm, 8, M, N)   # arch == 9
        y32 = mixlib.gemm(cache.q_xcache, q_weight, M, N, K)
        return y_a, y_b, n(y32), cache.q_xcache
    plain = ref_sequence()
    prev = mixlib.configure(packed_operands=True)
    try:
        fast = ref_sequence()
        assert fmt_of(fast[3]) == 1 and fmt_of(plain[3]) == 0
    finally:
        mixlib.configure(prev)
    assert torch.equal(plain[0], fast[0]) and torch.equal(plain[1], fast[1]) and torch.equal(plain[0], plain[1])
    assert np.array_equal(plain[2], fast[2]) and np.array_equal(fast[2], O.gemm_i8(n(plain[3]), c["qw"]))


# ---------------------------------------------------------------------------------------------------------------
# the bench line's contract (what the driver parses)
# ---------------------------------------------------------------------------------------------------------------
def test_bench_line_contract_on_the_gpu():
    """`python bench.py --steps 20 --warmup 5 --full` prints ONE JSON line with the fields the driver reads: metric / value / unit / n_gpus /
    steps / warmup / ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload, a `roofline` object for the
    dominant kernel (measured live: achieved = algorithmic flops / its launch time) and a `cpu_baseline` object; value is consistent
    with ms_per_step, and the self-check against the dequantised Linear is inside the 1e-2 gate."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "20", "--warmup", "5", "--full"], capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in out, key
    assert out["n_gpus"] == 1 and out["steps"] == 20 and out["warmup"] == 5 and out["higher_is_better"] is True
    assert out["unit"] == "TFLOPS" and out["dtype"] == "int8" and out["data"] == "synthetic" and out["vs_baseline"] is None
    assert "workload" in out["config"] and out["config"]["M"] == 512 and out["config"]["K"] == 4096 and out["config"]["N"] == 11008
    flops = 2.0 * 512 * 4096 * 11008
    assert out["value"] == pytest.approx(flops / (out["ms_per_step"] * 1e-3) / 1e12, rel=1e-3)
    rf = out["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == pytest.approx(5033.0)
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-3) and 0.2 < rf["frac"] < 0.6
    assert rf["achieved"] == pytest.approx(flops / (rf["us_per_launch"] * 1e-6) / 1e12, rel=1e-3)
    assert rf["us_per_launch"] * 1e-3 < out["ms_per_step"]                              # the kernel is part of the step
    assert rf["traffic"] is None or (rf["traffic"] > rf["algorithmic_bytes_per_launch"] * 0.9 and "traffic_source" in rf)
    cb = out["cpu_baseline"]
    assert cb["unit"] == "TFLOPS" and cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("reference", "port") and cb["sample"]
    assert out["max_abs_err_vs_dequant_linear"] <= 1e-2
    # secondary timings: the reference's eager protocol and the cold-weights rotation, both slower than or equal to the
    # graph figure, neither absurd
    tm = out["timing"]
    assert tm["eager_ms_per_step"] >= 0.9 * out["ms_per_step"] and tm["eager_ms_per_step"] < 20 * out["ms_per_step"]
    assert tm["cold_weights_ms_per_step"] >= 0.9 * out["ms_per_step"] and tm["cold_weights_ms_per_step"] < 3 * out["ms_per_step"]
    assert "layer copies" in tm["cold_weights_protocol"]


def test_bench_collectives_over_rccl_single_rank():
    """The N-GPU bench's only collectives - the barriers around the timed region and one all_gather of {elapsed, FLOPs} - through
    the real RCCL backend ("nccl" on ROCm) in a 1-rank group on this GPU: process-group creation after set_device, barrier with
    device_ids, the gather on a CUDA tensor.  (The N-rank launch path itself is rehearsed on CPU over gloo, tests/test_dist_gloo.py.)"""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import os, sys, torch
        sys.path.insert(0, %r)
        import bench
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(bench.free_port()))
        torch.cuda.set_device(0)
        import torch.distributed as dist
        dist.init_process_group(backend="nccl", rank=0, world_size=1)
        dev = torch.device("cuda", 0)
        bench.barrier(1, dev)
        mx, tot, per = bench.gather_counters(0.25, 3.0e9, 1, dev, per_rank=True)
        bench.barrier(1, dev)
        assert (mx, tot, per) == (0.25, 3.0e9, [0.25]), (mx, tot, per)
        dist.destroy_process_group()
        print("rccl ok")
    """ % root)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "rccl ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
