"""bfloat16 weight-only W8A16 layers on the MI355X: mixq_gemm_w8a16_bf16 / mixq_gemm_w8a16_addend_bf16 (gemm_w8a16.hip compiled as
gemm_w8a16_bf16.hip) from the kernel up to MixLinear_GEMM, eetq.w8_a16_gemm and MixGPTJMLP.  The expectation is the float64 restatement of
tests/w8a16_bf16_ref.py (oracle/ has no bfloat16 W8A16).

  (1) exact operands, every product tiling and the automatic choice, bias / addend in every combination: bit for bit RNE_bf16(z)
  (2) every int8 value survives the conversion: one-hot activations read single weights back, -128 included
  (3) every k-step count 1 .. 14, 23, 40, 67 on ragged M and N against an fp32 device matmul of the same operands (2 bf16 ulp of the row's
      largest output: the accumulation order differs), and the one-hot probe over 13 k-steps
  (4) the range: a result far above fp16's 65504 is finite; the largest finite bfloat16 stays, the tie above it becomes inf
  (5) y and the addend as windows of guard frames: nothing outside the window is read into the result or written
  (6) the operator: from_linear under MixqConfig(act_dtype=bfloat16, w8a16_bf16=True), residual=, eetq.w8_a16_gemm, MixGPTJMLP, a checkpoint
  (7) an fp16 weight-only layer before and after a bf16 one in the same process: the same bytes"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact as E  # noqa: E402
import w8a16_bf16_ref as R  # noqa: E402
from exact import BF16  # noqa: E402
from frames import Frame  # noqa: E402
from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, eetq, mixlib  # noqa: E402
from mixq_amd import checkpoint as ck  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402
from test_gpu_residual import addend_layouts  # noqa: E402

DEV = "cuda"
H, BF = torch.float16, torch.bfloat16
NAN_BF16 = 0x7FC0                                          # a quiet NaN in bfloat16


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    lib = _capi.load()
    lib.mixq_gemm_w8a16_set_config(-1)
    yield
    lib.mixq_gemm_w8a16_set_config(-1)


def bits_of(y):
    assert y.dtype == BF
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def bf(v):
    """float64 values that bfloat16 holds exactly -> a device tensor."""
    return E.as_tensor(np.asarray(v, dtype=np.float64), BF16).to(DEV)


def tilings():
    """The automatic choice and the nine product tilings (no ablation form, not the K-split kernel: it has no bf16 form)."""
    names = _capi.w8a16_config_names()
    return [-1] + [i for i, nm in enumerate(names) if "abl" not in nm and "decode" not in nm]


def forced(cfgs):
    lib, names = _capi.load(), _capi.w8a16_config_names()
    try:
        for c in cfgs:
            assert lib.mixq_gemm_w8a16_set_config(c) == 0
            yield c, (names[c] if c >= 0 else "auto")
    finally:
        assert lib.mixq_gemm_w8a16_set_config(-1) == 0


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------------
_exact = {}


def exact_problem(M, N):
    """E.w8a16_problem with x re-encoded as bfloat16 (i 2^-6, |i| <= 64: representable) and a bf16 addend i 2^-12, |i| <= 2000 cut to 8
    significant bits.  The exactness conditions are asserted on the data: every z / q an integer, the sum of absolute terms below 2^22 q
    (the weights enter as q, |q| <= 128).  One shared instance per shape, left unchanged."""
    if (M, N) not in _exact:
        x, qkn, scale, bias, z, q = E.w8a16_problem(M, E.K_MAIN, N)
        x64 = x.astype(np.float64)
        assert E.representable(x64, BF16)
        rng = np.random.default_rng(2000 + M + N)
        add = E._fit(rng.integers(-2000, 2001, (M, N)), BF16) * 2.0 ** -12
        assert E.representable(add, BF16)
        b64 = bias.astype(np.float64)
        for zz in (z, z + add):
            assert np.array_equal(zz / q, np.rint(zz / q))
        worst = float(((np.abs(x64).sum(axis=1)[:, None] * 128.0 * scale.astype(np.float64)[None, :] + np.abs(b64)[None, :] + np.abs(add)) / q).max())
        assert worst < E.LIMIT, worst
        xb, ab = E.to_bits(x64, BF16), E.to_bits(add, BF16)
        assert np.array_equal(R.z64(xb, qkn, scale, ab, bias), z + add) and np.array_equal(R.z64(xb, qkn, scale), z - b64[None, :])
        dev = dict(w=mixlib.PackW8A16(torch.from_numpy(qkn).to(DEV), BF), x=bf(x64), s=torch.from_numpy(scale).to(DEV),
                   b=torch.from_numpy(bias).to(DEV), a=bf(add))
        _exact[(M, N)] = (dev, z - b64[None, :], add, b64, worst)
    return _exact[(M, N)]


@pytest.mark.parametrize("N", E.N_SHAPES)
@pytest.mark.parametrize("M", E.M_SHAPES)
def test_w8a16_bf16_exact_every_tiling(M, N):
    d, z0, add, b64, worst = exact_problem(M, N)
    K = E.K_MAIN
    sh = E.shares(R.expect_bits(z0 + add + b64[None, :]), z0 + add + b64[None, :], BF16)
    print(f"w8a16 bf16 {M}x{K}->{N}: worst sum of absolute terms {worst:.4g} q (limit 2^22 = {E.LIMIT:.4g}); ties {sh['tie']:.3f}, round away {sh['away']:.3f}")
    for cfg, name in forced(tilings()):
        for b, zb in ((None, z0), (d["b"], z0 + b64[None, :])):
            for a, zz in ((None, zb), (d["a"], zb + add)):
                kw = {} if a is None else {"addend": a}
                y = mixlib.W8A16Linear(d["x"], d["w"], d["s"], b, N, K, **kw)
                assert y.dtype == BF and tuple(y.shape) == (M, N)
                E.assert_exact(bits_of(y), R.expect_bits(zz), zz, BF16, f"w8a16 bf16 {name} {M}x{K}->{N} bias={b is not None} addend={a is not None}")
            # addend=None is the call without the argument
            assert same(mixlib.W8A16Linear(d["x"], d["w"], d["s"], b, N, K, addend=None), mixlib.W8A16Linear(d["x"], d["w"], d["s"], b, N, K)), name


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------------
def test_w8a16_bf16_every_int8_value_survives_the_conversion():
    """One-hot activations read single weights back: every int8 value -128 .. 127 must come out of the sign-extending byte conversion as
    itself, on every tiling.  Compared as integers."""
    K, N = 256, 64
    q = np.zeros((K, N), np.int8)
    vals = np.arange(-128, 128, dtype=np.int16)
    for k in range(K):
        q[k, :] = np.roll(vals, 2 * k)[:N].astype(np.int8)           # (a step of 2: the 128 rows read back hold every one of the 256 values)
    assert set(q[:128].reshape(-1).tolist()) == set(range(-128, 128))
    x = torch.eye(K, device=DEV)[:128].bfloat16().contiguous()                      # row m selects k = m
    wp = mixlib.PackW8A16(torch.from_numpy(q).to(DEV), BF)
    s = torch.ones(N, dtype=H, device=DEV)
    for cfg, name in forced(tilings()):
        y = mixlib.W8A16Linear(x, wp, s, None, N, K)
        assert np.array_equal(y.float().cpu().numpy().astype(np.int16), q[:128].astype(np.int16)), name


# ---- (3) ---------------------------------------------------------------------------------------------------------------------------------
def test_w8a16_bf16_every_tiling_every_k_step_count():
    """The sweep of tests/test_gpu_parity.py::test_w8a16_every_tiling_every_k_step_count on the bf16 kernels: ragged M and N, k-step counts
    that end in every position of the unrolled loop and its guarded tail.  Reference: an fp32 device matmul over the same bf16 x and the
    dequantised weights; tolerance 2 bf16 ulp of the row's largest output, 2^(floor(log2 max) - 6) - the fp16 test's rule with bfloat16's
    8-bit significand."""
    names = _capi.w8a16_config_names()
    g = torch.Generator().manual_seed(11)
    M, N = 150, 328
    cases = []
    for nk in list(range(1, 15)) + [23, 40, 67]:                 # operands and references once, shared by the tilings
        K = 64 * nk
        q = torch.randint(-128, 128, (K, N), generator=g, dtype=torch.int8).to(DEV)
        sc = (torch.rand(N, generator=g) * 0.01 + 0.001).half().to(DEV)
        x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
        b = torch.randn(N, generator=g).half().to(DEV)
        ref = x.float() @ (q.float() * sc.float()) + b.float()
        tol = 2.0 ** (torch.floor(torch.log2(ref.abs().amax(dim=1, keepdim=True).clamp_min(1.0))) - 6)
        cases.append((nk, K, x, mixlib.PackW8A16(q, BF), sc, b, ref, tol))
    K1 = 64 * 13
    q1 = torch.randint(-128, 128, (K1, N), generator=g, dtype=torch.int8).to(DEV)
    ks = torch.arange(M) * 5 % K1
    x1 = torch.zeros(M, K1, dtype=BF, device=DEV)
    x1[torch.arange(M), ks] = 1
    w1, s1 = mixlib.PackW8A16(q1, BF), torch.ones(N, dtype=H, device=DEV)
    want1 = q1[ks.to(DEV)].to(torch.int16).cpu()
    for cfg, name in forced(tilings()[1:]):
        for nk, K, x, wp, sc, b, ref, tol in cases:
            y = mixlib.W8A16Linear(x, wp, sc, b, N, K).float()
            assert ((y - ref).abs() <= tol).all(), (names[cfg], nk, float((y - ref).abs().max()))
        # exact probe: one-hot rows, unit scales -> y[m, n] = q[k(m), n] for k spread over all 13 k-steps
        y = mixlib.W8A16Linear(x1, w1, s1, None, N, K1)
        assert torch.equal(y.float().to(torch.int16).cpu(), want1), names[cfg]


# ---- (4) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", E.M_SHAPES)
def test_w8a16_bf16_range(M):
    """bfloat16 has fp32's exponent range: 3 * 2^100 is a finite output (fp16 ends at 65504).  acc s + addend = 2^128 - 2^120 exactly, the
    largest finite bfloat16, stays finite; = 2^128 - 2^119 exactly, the tie above it, becomes inf (RNE, nothing saturates).  The bias is
    fp16 (at most 65504) and cannot reach that quantum (2^119): the second variant puts acc s + addend + bias on the highest binade edge
    it can decide - 2^17 - 2^9 stays, the tie 2^17 - 2^8 rounds up to 2^17."""
    N, K = 136, 64
    s = torch.ones(N, dtype=H, device=DEV)
    cfgs = [-1, 0]

    def run(x0, q01, fill_q, add01, bias01):
        x = np.zeros((M, K))
        x[:, 0] = x0
        qkn = np.zeros((K, N), dtype=np.int8)
        qkn[0, :] = fill_q
        qkn[0, 0], qkn[0, 1] = q01
        add = bias = None
        if add01 is not None:
            add = np.zeros((M, N))
            add[:, :2] = add01
        if bias01 is not None:
            bias = np.zeros(N)
            bias[:2] = bias01
        zz = x @ qkn.astype(np.float64) + (0.0 if add is None else add) + (0.0 if bias is None else bias[None, :])
        w = mixlib.PackW8A16(torch.from_numpy(qkn).to(DEV), BF)
        out = []
        for cfg, name in forced(cfgs):
            kw = {} if add is None else {"addend": bf(add)}
            y = mixlib.W8A16Linear(bf(x), w, s, None if bias is None else E.as_tensor(bias, E.F16).to(DEV), N, K, **kw)
            E.assert_exact(bits_of(y), R.expect_bits(zz), zz, BF16, f"w8a16 bf16 range {name} M={M}")
            out.append((name, zz, y.float().cpu()))
        return out

    for name, zz, y in run(2.0 ** 100, (3, -3), 1, None, None):
        assert zz[0, 0] == 3 * 2.0 ** 100 and bool(torch.isfinite(y).all()) and bool((y[:, 0] == 3 * 2.0 ** 100).all()) and bool((y[:, 1] == -3 * 2.0 ** 100).all()), name
        assert float(y[:, 0].min()) > 65504.0 * 2.0 ** 80
    for name, zz, y in run(2.0 ** 119, (126, 127), 1, 3 * 2.0 ** 126, None):
        assert zz[0, 0] == 2.0 ** 128 - 2.0 ** 120 and zz[0, 1] == 2.0 ** 128 - 2.0 ** 119
        assert bool((y[:, 0] == 2.0 ** 128 - 2.0 ** 120).all()) and bool(torch.isinf(y[:, 1]).all()) and bool(torch.isfinite(y[:, 2:]).all()), name
    for name, zz, y in run(2.0 ** 8, (126, 127), 1, 2.0 ** 16, 2.0 ** 15):
        assert zz[0, 0] == 2.0 ** 17 - 2.0 ** 9 and zz[0, 1] == 2.0 ** 17 - 2.0 ** 8
        assert bool((y[:, 0] == 2.0 ** 17 - 2.0 ** 9).all()) and bool((y[:, 1] == 2.0 ** 17).all()), name


# ---- (5) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.N_SHAPES)
def test_w8a16_bf16_windows_in_guard_frames(N):
    """y and the addend as strided, offset windows (the layouts of tests/test_gpu_residual.py::addend_layouts: the 8-byte-not-16-byte aligned
    bases put y on the narrow store path).  Every element of the addend's frame outside its window is a NaN - a read of one poisons the
    output; nothing outside y's window is written; the inputs are unchanged."""
    M, K = E.M_SHAPES[0], E.K_MAIN
    d, z0, add, b64, _ = exact_problem(M, N)
    lays = []
    for ld, co, eo in addend_layouts(N):
        fa = Frame(M, N, ld, co, eo, BF, DEV, guard_rows=8)
        fa.raw.fill_(NAN_BF16)                                  # every element outside the window is a NaN
        fa.view.copy_(d["a"])
        assert fa.view.data_ptr() % 8 == 0 and (co + eo != 4 or fa.view.data_ptr() % 16 == 8)
        lays.append(((ld, co, eo), fa.freeze(), Frame(M, N, ld, co, eo, BF, DEV)))
    xs, ws = d["x"].clone(), d["w"].clone()
    for cfg, name in forced(tilings()):
        want = mixlib.W8A16Linear(d["x"], d["w"], d["s"], d["b"], N, K, addend=d["a"])
        want0 = mixlib.W8A16Linear(d["x"], d["w"], d["s"], d["b"], N, K)
        assert bool(torch.isfinite(want).all())
        for lay, fa, fy in lays:
            what = f"w8a16 bf16 {name} {M}x{K}->{N} ld={lay[0]} col_off={lay[1]} elem_off={lay[2]}"
            fy.reset()
            y = mixlib.W8A16Linear(d["x"], d["w"], d["s"], d["b"], N, K, out=fy.view, addend=fa.view)
            torch.cuda.synchronize()
            assert y.data_ptr() == fy.view.data_ptr() and bool(torch.isfinite(y).all()), what
            assert same(y, want), what
            fy.assert_untouched(what)
            fa.assert_unchanged(what)
            fy.reset()
            y = mixlib.W8A16Linear(d["x"], d["w"], d["s"], d["b"], N, K, out=fy.view)
            torch.cuda.synchronize()
            assert same(y, want0), what + " (no addend)"
            fy.assert_untouched(what + " (no addend)")
    assert torch.equal(xs.view(torch.int16), d["x"].view(torch.int16)) and torch.equal(ws, d["w"])
    fy = lays[0][2]
    with pytest.raises(RuntimeError, match="alias"):
        mixlib.W8A16Linear(d["x"], d["w"], d["s"], d["b"], N, K, out=fy.view, addend=fy.view)


# ---- (6) the operator ---------------------------------------------------------------------------------------------------------------------
CFG = dict(act_dtype=BF, w8a16_bf16=True)


def within_bound(y, xb, qkn, scale, addend=None, bias=None, what=""):
    """|y - z| <= the bound tests/w8a16_bf16_ref.py derives (fp32 accumulation in a free order, then one rounding to bfloat16)."""
    u16 = lambda t: t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    xbits, abits = u16(xb), None if addend is None else u16(addend)
    q, s, b = qkn.cpu().numpy(), scale.cpu().numpy(), None if bias is None else bias.cpu().numpy()
    z, tol = R.z64(xbits, q, s, abits, b), R.bound(xbits, q, s, abits, b)
    err = np.abs(R.bf16_values(bits_of(y)) - z)
    print(f"{what}: max |y - z| / bound = {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), (what, float((err / tol).max()))


def test_w8a16_bf16_operator():
    torch.manual_seed(3)
    K, N, M = 512, 320, 40
    lin = torch.nn.Linear(K, N, bias=True).bfloat16()
    cache = MixLibCache(64, device=DEV, config=MixqConfig(**CFG))
    ql = MixLinear_GEMM.from_linear(lin, bit=8, weight_only=True, cache=cache, dev=DEV, name="fc_out")
    assert ql.scale_col.dtype == H and ql.bias.dtype == H and ql.q_weight.dtype == torch.int8
    big = torch.randn(M, K + 64, device=DEV).bfloat16()
    x = big[:, :K]                                               # row stride K + 64
    y = ql(x)
    assert y.dtype == BF and tuple(y.shape) == (M, N)
    xc = x.contiguous()
    within_bound(y, xc, ql.q_weight, ql.scale_col, bias=ql.bias, what="operator, strided x, bias")
    assert ql._wpk_key[-1] is BF and getattr(ql._wpk, "_mixq_w8a16_dtype", None) is BF
    # residual= reaches the addend of the GEMM's epilogue: one rounding
    res = (torch.randn(M, N, device=DEV) * 4).bfloat16()
    yr = ql(x, residual=res)
    within_bound(yr, xc, ql.q_weight, ql.scale_col, addend=res, bias=ql.bias, what="operator, residual")
    assert same(yr, mixlib.W8A16Linear(xc, ql._wpk, ql.scale_col, ql.bias, N, K, addend=res))
    assert not same(yr, (y.float() + res.float()).bfloat16())   # (two roundings give other bits somewhere in 12800 elements)
    with pytest.raises(RuntimeError, match="residual must be bfloat16"):
        ql(x, residual=res.half())
    # the EETQ-named surface on a 3-D x, no bias
    y2 = eetq.w8_a16_gemm(x.reshape(2, M // 2, K), ql.q_weight, ql.scale_col)
    assert y2.shape == (2, M // 2, N) and y2.dtype == BF
    within_bound(y2.reshape(M, N), xc, ql.q_weight, ql.scale_col, what="eetq.w8_a16_gemm, 3-D x")
    assert same(eetq.w8_a16_gemm(xc, ql.q_weight, ql.scale_col, ql.bias), y)
    # one dtype per layer: fp16 x into the bf16 layer is refused, and bf16 x into an fp16 one
    with pytest.raises(RuntimeError, match="x must be bfloat16"):
        ql(x.half())
    l16 = MixLinear_GEMM.from_linear(torch.nn.Linear(K, N).half(), bit=8, weight_only=True, cache=MixLibCache(64, device=DEV), dev=DEV)
    with pytest.raises(RuntimeError, match="x must be float16"):
        l16(xc)
    # an image packed for the other container is refused, not read as wrong numbers
    with pytest.raises(RuntimeError, match="packed for float16"):
        mixlib.W8A16Linear(xc, mixlib.PackW8A16(ql.q_weight), ql.scale_col, None, N, K)
    with pytest.raises(RuntimeError, match="packed for float16"):
        mixlib.W8A16Linear(xc, ql._wpk.clone(), ql.scale_col, None, N, K)                       # (untagged)
    with pytest.raises(RuntimeError, match="packed for bfloat16"):
        mixlib.W8A16Linear(xc.half(), ql._wpk, ql.scale_col, None, N, K)
    with pytest.raises(RuntimeError, match="stay float16"):
        mixlib.W8A16Linear(xc, ql._wpk, ql.scale_col.bfloat16(), None, N, K)
    with pytest.raises(RuntimeError, match="`out` must be torch.bfloat16"):
        mixlib.W8A16Linear(xc, ql._wpk, ql.scale_col, None, N, K, out=torch.empty(M, N, dtype=H, device=DEV))


class _GptjMlp(torch.nn.Module):
    def __init__(self, K, I):
        super().__init__()
        self.fc_in, self.fc_out = torch.nn.Linear(K, I), torch.nn.Linear(I, K)


class _GptjCfg:
    activation_function, resid_pdrop = "gelu_new", 0.0


def test_gptj_mlp_in_bfloat16_and_its_checkpoint(tmp_path):
    """MixGPTJMLP with fc_in W8A8 and fc_out weight-only, both bfloat16 (hidden 256 -> 1024): equal, bit for bit, to the same layer calls
    written out; saved and loaded again the block reproduces y bit for bit (the checkpoint is the fp16 layer's: plain int8 q_weight).
    fc_in takes its quantised activations from the fused norm in front of the block, as in a model (fused_bf16: the bf16 norm)."""
    from mixq_amd import FasterTransformerRMSNorm, MixGPTJMLP
    from transformers.activations import ACT2FN
    torch.manual_seed(11)
    K, I, M = 256, 1024, 48
    src = _GptjMlp(K, I).bfloat16()
    x = torch.randn(M, K).bfloat16().to(DEV)
    x[:, [5, 77]] *= 30

    def built(cache):
        m = _GptjMlp(K, I).bfloat16()
        m.load_state_dict(src.state_dict())
        done = ck.quantize_(m, 8, cache, arch="GPTJForCausalLM", dev=DEV)
        assert done == {"fc_in": (8, False), "fc_out": (8, True)}
        return m

    new_cache = lambda: MixLibCache(64, device=DEV, config=MixqConfig(fused_bf16=True, **CFG))

    def normed(first, cache):
        norm = FasterTransformerRMSNorm(torch.ones(K, dtype=BF, device=DEV), cache=cache)
        norm.next_layer = first
        return norm(x.clone())

    cache, cache2 = new_cache(), new_cache()
    m, m2 = built(cache), built(cache2)
    g = MixGPTJMLP(m, _GptjCfg(), cache).eval()
    for _ in range(3):                                           # call 0 finds fc_in's outlier columns, later calls run its frozen forward
        y = g(normed(m.fc_in, cache))
        ref = m2.fc_out(ACT2FN["gelu_new"](m2.fc_in(normed(m2.fc_in, cache2), cache2)), cache2)
    torch.cuda.synchronize()
    assert y.dtype == BF and tuple(y.shape) == (M, K) and bool(torch.isfinite(y).all())
    assert same(y, ref)
    dense = src.float()
    xf = x.float().cpu()
    want = dense.fc_out(ACT2FN["gelu_new"](dense.fc_in(xf / torch.sqrt((xf ** 2).mean(dim=-1, keepdim=True) + 1e-6))))
    assert (y.float().cpu() - want).abs().max() < 0.05 * want.abs().max() + 0.05
    # the checkpoint round trip
    ck.save_quantized(m, str(tmp_path), {"w_bit": 8})
    fresh = _GptjMlp(K, I).bfloat16()
    cache3 = new_cache()
    ck.load_quantized(fresh, str(tmp_path), cache3, arch="GPTJForCausalLM", dev=DEV)
    assert fresh.fc_out.weight_only and fresh.fc_out.act_dtype is BF and torch.equal(fresh.fc_out.q_weight, m.fc_out.q_weight)
    g3 = MixGPTJMLP(fresh, _GptjCfg(), cache3).eval()
    for _ in range(3):
        y3 = g3(normed(fresh.fc_in, cache3))
    assert same(y3, y)


# ---- (7) ---------------------------------------------------------------------------------------------------------------------------------
def test_fp16_weight_only_layer_is_untouched_by_a_bf16_one():
    """The pack cache keys (the layer's `_wpk_key`, eetq's `_packed`) carry the container and the images are tagged: an fp16 layer and the
    EETQ-named call on the SAME q_weight give, after a bf16 layer and a bf16 call ran, the bytes they gave before."""
    torch.manual_seed(7)
    K, N, M = 256, 136, 40
    lin = torch.nn.Linear(K, N, bias=True)
    l16 = MixLinear_GEMM.from_linear(lin.half(), bit=8, weight_only=True, cache=MixLibCache(64, device=DEV), dev=DEV)
    x16 = torch.randn(M, K, device=DEV).half()
    before = l16(x16).clone()
    e_before = eetq.w8_a16_gemm(x16, l16.q_weight, l16.scale_col, l16.bias).clone()
    assert same(before, e_before) and before.dtype == H
    lbf = MixLinear_GEMM.from_linear(lin.bfloat16(), bit=8, weight_only=True, cache=MixLibCache(64, device=DEV, config=MixqConfig(**CFG)), dev=DEV)
    xbf = x16.bfloat16()
    ybf = lbf(xbf)
    e_bf = eetq.w8_a16_gemm(xbf, l16.q_weight, l16.scale_col, l16.bias)          # the fp16 layer's q_weight tensor, the other container
    assert ybf.dtype == BF and e_bf.dtype == BF
    within_bound(e_bf, xbf, l16.q_weight, l16.scale_col, bias=l16.bias, what="eetq bf16 on the fp16 layer's q_weight")
    assert same(l16(x16), before) and same(eetq.w8_a16_gemm(x16, l16.q_weight, l16.scale_col, l16.bias), e_before)
    assert same(mixlib.W8A16Linear(x16, mixlib.PackW8A16(l16.q_weight), l16.scale_col, l16.bias, N, K), before)     # a fresh fp16 image: the same bytes
    assert getattr(l16._wpk, "_mixq_w8a16_dtype", None) is H and len(l16._wpk_key) == 3                          # the fp16 layer's key is what it was
    assert same(lbf(xbf), ybf) and same(eetq.w8_a16_gemm(xbf, l16.q_weight, l16.scale_col, l16.bias), e_bf)
