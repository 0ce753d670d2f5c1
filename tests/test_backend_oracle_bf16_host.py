"""The bfloat16 branches of tests/backend_oracle.py (ABI 1.6) against what tests/ already holds, on those files' own operands: the one
rounding against exact.to_bits and the hand-picked ties of tests/test_w8a16_bf16_host.py, FusedLinear against the exact problems of
tests/exact.py bit for bit, W8A16Linear against w8a16_bf16_ref.expect_bits on exact.w8a16_problem, the norm against bf16_norm_ref, the
quantise family against the C oracle on values both containers hold - and ACT_SILU_PAIR against the two launches it stands for.  Host only.
tests/test_gpu_backend_oracle.py holds the same branches to the kernels."""
import numpy as np
import pytest
import torch

import backend_oracle as B
import bf16_norm_ref as R
import exact as E
import w8a16_bf16_ref as W
from exact import BF16
from oracle import oracle as O

BF, F16 = torch.bfloat16, torch.float16


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def bf(v):
    """float64 values bfloat16 holds exactly -> a bfloat16 tensor"""
    return E.as_tensor(np.asarray(v, dtype=np.float64), BF16)


# ---- the one rounding ----------------------------------------------------------------------------------------------------------------------
def test_rne_bf16_bits_is_one_rounding_of_the_float64_value():
    u = 2.0 ** -7
    cases = [(1.0 + u / 2, 0x3F80), (1.0 + 3 * u / 2, 0x3F82), (1.0 + 5 * u / 2, 0x3F82), (-(1.0 + u / 2), 0xBF80), (-(1.0 + 3 * u / 2), 0xBF82),
             (1.0 + u / 2 + 2.0 ** -23, 0x3F81), (1.0 + u / 2 - 2.0 ** -23, 0x3F80), (255.0, 0x437F), (255.5, 0x4380), (256.5, 0x4380), (257.0, 0x4380),
             (259.0, 0x4382), (2.0 ** 128 - 2.0 ** 120, 0x7F7F), (2.0 ** 128 - 2.0 ** 119, 0x7F80), (-(2.0 ** 128 - 2.0 ** 119), 0xFF80),
             (2.0 ** 128 - 2.0 ** 119 - 2.0 ** 104, 0x7F7F), (2.0 ** -134, 0x0000), (3 * 2.0 ** -134, 0x0002), (0.0, 0x0000), (-0.0, 0x8000),
             # what a detour through float32 gets wrong: just above the tie by less than half an fp32 ulp
             (1.0 + u / 2 + 2.0 ** -30, 0x3F81), (-(1.0 + u / 2 + 2.0 ** -30), 0xBF81), (np.inf, 0x7F80), (-np.inf, 0xFF80), (1e300, 0x7F80)]
    got = B.rne_bf16_bits(np.array([c[0] for c in cases]))
    assert [int(g) for g in got] == [c[1] for c in cases], [(c[0], hex(int(g))) for c, g in zip(cases, got) if g != c[1]]
    assert (B.rne_bf16_bits(np.array([np.nan])) & 0x7FFF) > 0x7F80
    # ... and exact.to_bits on everything float32 holds: every finite bf16 pattern plus fp32 values between them
    rng = np.random.default_rng(0)
    v = E.from_bits(E.all_finite_patterns(BF16), BF16)
    v = np.concatenate([v, (v * (1.0 + rng.integers(-2 ** 15, 2 ** 15, v.size) * 2.0 ** -23)).astype(np.float32).astype(np.float64)])
    assert np.array_equal(B.rne_bf16_bits(v), E.to_bits(v, BF16))


# ---- the GEMM epilogue on the exact problems of tests/exact.py ----------------------------------------------------------------------------
def _operands(p):
    qx, qw = p.q_plain()
    fx, fw = (B.FMT_P16X64, B.FMT_F16X64) if p.bit == 8 else (B.FMT_R6X128, B.FMT_F6X128)
    sx = torch.from_numpy(p.sx.copy()).reshape(-1, 1)
    return B.PackOperand(qx, fx), B.PackOperand(qw, fw), sx, torch.from_numpy(p.sw.copy()).reshape(1, -1)


def _pad(v, dtype):
    """[R, n] float64 -> a [R, pad16(n)] tensor with NaN patterns in the pad (masked: include/mixq_hip.h)"""
    n = v.shape[1]
    t = torch.full((v.shape[0], (n + 15) // 16 * 16), 0x7FC1, dtype=torch.int16).view(dtype)
    t[:, :n] = E.as_tensor(v, BF16 if dtype == BF else E.F16)
    return t


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("kind", ["main", "wide"])
def test_fused_linear_in_bfloat16_equals_the_exact_expectation(bit, kind):
    M, N = E.M_SHAPES[1], E.N_SHAPES[0]
    p = E.problem(kind, bit, BF16, M, N)
    qx, qw, sx, sw = _operands(p)
    combos = [(0, None, False), (1, True, False), (17, None, False), (17, True, False)] + ([(41, True, True), (16, None, True)] if kind == "main" else [])
    for n_out, addend, bias in combos:
        want, z = p.expected(n_out, addend, bias)
        xo, wo = (_pad(p.xo[:, :n_out], BF), _pad(p.wo[:, :n_out], BF)) if n_out else (None, None)
        for dev_count in (False, True):
            cap = xo.shape[1] if (dev_count and n_out) else n_out
            n_dev = torch.tensor([n_out], dtype=torch.int32) if (dev_count and n_out) else None
            y = B.FusedLinear(qx, qw, sx, sw, None if xo is None else xo[:, :cap], None if wo is None else wo[:, :cap], cap,
                              torch.from_numpy(p.bias.copy()) if bias else None, M, N, p.K, bit=bit, n_out_dev=n_dev,
                              addend=bf(p.addend) if addend else None, dtype=BF)
            assert y.dtype == BF
            E.assert_exact(bits(y), want, z, BF16, f"{p.name} n_out={n_out} addend={addend} bias={bias} dev_count={dev_count}")


@pytest.mark.parametrize("bit", [8, 4])
def test_silu_forms_and_the_pair_in_bfloat16(bit):
    """SiLU within exact.silu_reference's bound of the float64 value (the oracle IS that value rounded once: half an ulp); ACT_SILU_PAIR
    byte for byte the two launches - up_proj's output, then gate_proj's SiLU-and-multiply on it - and its row maxima theirs."""
    M, N, n_out = 24, 64, 17
    p = E.exact_problem(bit, M, 128, 2 * N, n_out, dtype=BF16, seed=9, **(dict(q_max=31, xo_max=16, wo_max=8) if bit == 8 else {}))
    qx, qw2, sx, sw2 = _operands(p)
    xo, wo2, b2 = _pad(p.xo, BF), _pad(p.wo, BF), torch.from_numpy(p.bias.copy())
    plain_w = B.UnpackOperand(qw2, 2 * N)
    halves = []
    for rows in O.pair_rows_split(np.arange(2 * N)):
        idx = torch.from_numpy(rows)
        halves.append((B.PackOperand(plain_w[idx].contiguous(), B.fmt_of(qw2)), sw2[:, idx], wo2[idx], b2[idx], rows))
    (wu, su, wou, bu, ru), (wg, sg, wog, bg, rg) = halves
    up = B.FusedLinear(qx, wu, sx, su, xo[:, :n_out], wou[:, :n_out], n_out, bu, M, N, 128, bit=bit, dtype=BF)
    amax2 = torch.zeros(M, dtype=torch.int32)
    kw2 = {"row_amax": amax2} if bit == 8 else {}
    two = B.FusedLinear(qx, wg, sx, sg, xo[:, :n_out], wog[:, :n_out], n_out, bg, M, N, 128, bit=bit, act=B.ACT_SILU_MUL, addend=up, dtype=BF, **kw2)
    amax1 = torch.zeros(M, dtype=torch.int32)
    kw1 = {"row_amax": amax1} if bit == 8 else {}
    one = B.FusedLinear(qx, qw2, sx, sw2, xo[:, :n_out], wo2[:, :n_out], n_out, b2, M, 2 * N, 128, bit=bit, act=B.ACT_SILU_PAIR, dtype=BF, **kw1)
    assert tuple(one.shape) == (M, N) and np.array_equal(bits(one), bits(two)) and torch.equal(amax1, amax2)
    if bit == 8:
        assert np.array_equal(amax1.numpy(), (bits(one) & 0x7FFF).astype(np.int32).max(axis=1))      # maxima of bfloat16 bit patterns
    z = p.z(n_out)
    ref, bound = E.silu_reference(z[:, rg], p.bias.astype(np.float64)[rg], E.from_bits(bits(up), BF16), BF16)
    assert E.silu_check(bits(two), ref, bound, BF16, "SILU_MUL") <= 1.0
    y = B.FusedLinear(qx, wg, sx, sg, xo[:, :n_out], wog[:, :n_out], n_out, bg, M, N, 128, bit=bit, act=B.ACT_SILU, dtype=BF)
    ref, bound = E.silu_reference(z[:, rg], p.bias.astype(np.float64)[rg], None, BF16)
    assert E.silu_check(bits(y), ref, bound, BF16, "SILU") <= 1.0


def test_mixed_containers_and_unserved_layouts_are_refused_as_the_hip_backend_refuses_them():
    p = E.problem("main", 8, BF16, E.M_SHAPES[1], E.N_SHAPES[0])
    qx, qw, sx, sw = _operands(p)
    args = (qx, qw, sx, sw)
    xo, wo = _pad(p.xo[:, :16], BF), _pad(p.wo[:, :16], BF)
    with pytest.raises(RuntimeError, match="w_out must be torch.bfloat16 like the call's other 16-bit tensors"):
        B.FusedLinear(*args, xo, wo.half(), 16, None, p.M, p.N, p.K, dtype=BF)
    with pytest.raises(RuntimeError, match="addend must be torch.float16 like"):
        B.FusedLinear(*args, None, None, 0, None, p.M, p.N, p.K, addend=bf(p.addend))
    with pytest.raises(RuntimeError, match="out must be torch.bfloat16"):
        B.FusedLinear(*args, None, None, 0, None, p.M, p.N, p.K, dtype=BF, out=torch.empty((p.M, p.N), dtype=F16))
    with pytest.raises(RuntimeError, match="x must be float16 or bfloat16, got torch.float32"):
        B.FusedLinear(*args, None, None, 0, None, p.M, p.N, p.K, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="bfloat16 GEMMs serve"):
        B.FusedLinear(qx, B.PackOperand(p.q_plain()[1], B.FMT_P16X64), sx, sw, None, None, 0, None, p.M, p.N, p.K, dtype=BF)
    with pytest.raises(RuntimeError, match="x must be float16 or bfloat16"):
        B.amax_supported(16, 64, 128, B.FMT_P16X64, B.FMT_F16X64, dtype=torch.float32)
    assert B.amax_supported(1, 64, 128, B.FMT_P16X64, B.FMT_F16X64, dtype=BF) and B.PAIR_LAUNCH_BF16 is True
    x = torch.zeros((4, 128), dtype=BF)
    with pytest.raises(RuntimeError, match="weight must be torch.bfloat16 like x"):
        B.layernorm_forward_cuda(x, torch.ones(128, dtype=F16), torch.empty_like(x), 1e-6)
    with pytest.raises(RuntimeError, match="out must be torch.bfloat16 like x"):
        B.RMSNormQuantFused(x, torch.ones(128, dtype=BF), torch.empty((4, 128), dtype=F16), 1e-6, None, torch.zeros(4, dtype=F16), 8)
    with pytest.raises(RuntimeError, match="x_out must be torch.bfloat16 like x"):
        B.QuantFused(x, torch.tensor([3], dtype=torch.int32), torch.zeros(4, dtype=F16), 8, 6.0, x_out=torch.zeros((4, 16), dtype=F16))
    plan = B.ForwardPlan(4, 64, 128, 8, 6.0, 128, None, 0, None, torch.zeros((4, 1), dtype=F16), qw, torch.ones((1, 64), dtype=F16), None, None, B.FMT_P16X64, dtype=BF)
    with pytest.raises(RuntimeError, match=r"x must be bfloat16 \[4, 128\]"):
        plan.run(x.half())
    with pytest.raises(RuntimeError, match=r"addend must be bfloat16 \[4, 64\]"):
        plan.run(x, addend=torch.zeros((4, 64), dtype=F16))


# ---- weight-only -------------------------------------------------------------------------------------------------------------------------
def test_w8a16_linear_in_bfloat16_equals_the_reference_on_the_exact_operands_and_fp16_with_an_addend_too():
    M, N = E.M_SHAPES[1], E.N_SHAPES[1]
    x, qkn, scale, bias, z, q = E.w8a16_problem(M, E.K_MAIN, N)
    add = E._fit(np.random.default_rng(2000 + M + N).integers(-2000, 2001, (M, N)), BF16) * 2.0 ** -12      # (fits both containers)
    qt, st, bt = torch.from_numpy(qkn.copy()), torch.from_numpy(scale.copy()), torch.from_numpy(bias.copy())
    xb = bf(x.astype(np.float64))
    img = B.PackW8A16(qt, BF)
    assert img is not qt and img.data_ptr() != qt.data_ptr() and img._mixq_w8a16_dtype == BF          # an image: later writes to q_weight do not reach it
    for a in (None, add):
        za = z if a is None else z + a
        y = B.W8A16Linear(xb, img, st, bt, N, E.K_MAIN, addend=None if a is None else bf(a))
        assert y.dtype == BF
        E.assert_exact(bits(y), W.expect_bits(za), za, BF16, f"bf16 W8A16 addend={a is not None}")
        y = B.W8A16Linear(torch.from_numpy(x.copy()), B.PackW8A16(qt), st, bt, N, E.K_MAIN, addend=None if a is None else E.as_tensor(a, E.F16))
        E.assert_exact(bits(y), E.to_bits(za, E.F16), za, E.F16, f"fp16 W8A16 addend={a is not None}")
    with pytest.raises(RuntimeError, match="needs the weight image of PackW8A16"):
        B.W8A16Linear(xb, B.PackW8A16(qt), st, bt, N, E.K_MAIN)
    with pytest.raises(RuntimeError, match="packed for bfloat16"):
        B.W8A16Linear(xb.half(), img, st, bt, N, E.K_MAIN)
    with pytest.raises(RuntimeError, match="addend must be torch.bfloat16 on x's device"):
        B.W8A16Linear(xb, img, st, bt, N, E.K_MAIN, addend=torch.zeros((M, N), dtype=F16))


# ---- norm and the quantise family -----------------------------------------------------------------------------------------------------
def _norm_data(M, K, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[:, [1, K // 2 + 3, K - 2]] *= 30
    x *= (2.0 ** (20 * (np.arange(M) % 3)))[:, None].astype(np.float32)                # rows at 1, 2^20, 2^40: beyond float16
    return R.f32_to_bf16_bits(x), R.f32_to_bf16_bits((0.5 + rng.random(K)).astype(np.float32))


@pytest.mark.parametrize("bit", [8, 4])
def test_norm_forms_in_bfloat16(bit):
    M, K, eps = 5, 256, 1e-5
    xb, wb = _norm_data(M, K)
    x, w = B._from_u16(xb, BF), B._from_u16(wb, BF)
    want = R.rmsnorm_bf16(xb, wb, eps)
    out = torch.empty_like(x)
    B.layernorm_forward_cuda(x.reshape(1, M, K), w, out.reshape(1, M, K), eps)
    assert np.array_equal(bits(out), want)
    # the fused form: the plain norm, then QuantFused on its output (x_out its columns `ind`, those zeroed, x_scale / q from the zeroed row)
    ind = torch.tensor([K - 2, 1, 77], dtype=torch.int32)
    fmt = B.FMT_P16X64 if bit == 8 else B.FMT_R6X128
    xs, xs2, flag, flag2 = torch.zeros((M, 1), dtype=F16), torch.zeros((M, 1), dtype=F16), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    q, xo = B.RMSNormQuantFused(x, w, out, eps, ind, xs, bit, flag=flag, fmt=fmt)
    ref = B._from_u16(want, BF)
    q2, xo2 = B.QuantFused(ref, ind, xs2, bit, 6.0, flag=flag2, fmt=fmt)
    assert xo.dtype == BF and torch.equal(q, q2) and np.array_equal(bits(xo), bits(xo2)) and np.array_equal(bits(out), bits(ref)) and torch.equal(xs, xs2)
    assert np.array_equal(bits(xo), want[:, ind.numpy()]) and not bits(out)[:, ind.numpy()].any() and int(flag) == int(flag2) == 1   # (column K/2+3 stayed in)


@pytest.mark.parametrize("bit", [8, 4])
def test_quantise_family_in_bfloat16_is_the_headers_formula(bit):
    """On values both containers hold (8 significant bits inside float16's range) the bfloat16 branch must equal the C oracle's float16 one -
    the same formula on the same numbers - and on rows beyond float16 the float64 restatement of the header."""
    rng = np.random.default_rng(4)
    M, K = 7, 128
    v = rng.integers(-255, 256, (M, K)) * np.exp2(rng.integers(-12, 6, (M, K)).astype(np.float64))
    v[2] = 0                                                                             # an all-zero row: scale 0, q 0
    v[:, [5, 77]] *= 16
    v[0, 5] = 65280.0                                                                     # (the largest value both containers hold)
    assert E.representable(v, BF16) and E.representable(v, E.F16)
    xb, xh = bf(v), E.as_tensor(v, E.F16)
    sb, sh = torch.zeros((M, 1), dtype=F16), torch.zeros((M, 1), dtype=F16)
    assert torch.equal(B.FindRowScale(xb, sb, M, K, bit), B.FindRowScale(xh, sh, M, K, bit)) and torch.equal(sb, sh) and float(sb[2]) == 0
    for fmt in ((B.FMT_P16X64, B.FMT_F16X64) if bit == 8 else (B.FMT_P16X64, B.FMT_R6X128)):
        assert torch.equal(B.FindRowScalePacked(xb, sb, M, K, bit, fmt=fmt), B.FindRowScalePacked(xh, sh, M, K, bit, fmt=fmt))
    ib, cb = B.DetectOutlierCols(xb, 6.0)
    ih, ch = B.DetectOutlierCols(xh, 6.0)
    assert torch.equal(ib, ih) and torch.equal(cb, ch) and int(cb) > 2
    ind = torch.tensor([77, 5, 100], dtype=torch.int32)
    for n_dev in (None, torch.tensor([2], dtype=torch.int32)):
        a, b = xb.clone(), xh.clone()
        fb, fh = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        qb, ob = B.QuantFused(a, ind, sb, bit, 6.0, flag=fb, n_dev=n_dev)
        qh, oh = B.QuantFused(b, ind, sh, bit, 6.0, flag=fh, n_dev=n_dev)
        assert ob.dtype == BF and torch.equal(qb, qh) and torch.equal(sb, sh) and torch.equal(ob.double(), oh.double()) and torch.equal(a.double(), b.double())
        assert torch.equal(fb, fh)
    a, b = xb.clone(), xh.clone()
    assert torch.equal(B.ExtractOutliersAndSetToZeros(ind, a).double(), B.ExtractOutliersAndSetToZeros(ind, b).double()) and torch.equal(a.double(), b.double())
    # values beyond float16 (x_scale stays float16: the row's maximum / qmax must fit it, so the factor stays below qmax)
    qmax = 127 if bit == 8 else 7
    up = 2.0 ** (6 if bit == 8 else 2)
    big = bf(v * up)
    assert float(big.abs().max()) > 65504
    q = B.FindRowScale(big, sb, M, K, bit)
    s64 = (np.abs(v * up).max(axis=1).astype(np.float32) / np.float32(qmax)).astype(np.float16).astype(np.float64)
    assert np.array_equal(sb.reshape(-1).double().numpy(), s64)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.clip(np.where(s64[:, None] > 0, np.rint((v * up).astype(np.float32) / s64[:, None].astype(np.float32)), 0), -qmax, qmax).astype(np.int8)
    assert np.array_equal(q.numpy(), want if bit == 8 else E.pack_i4(want))
