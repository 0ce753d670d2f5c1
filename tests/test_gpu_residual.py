"""The residual add in the GEMM epilogue on the MI355X: `residual=` of MixLinear_GEMM / MixLlamaMLP, `addend=` of ForwardPlan.run and
W8A16Linear, and the new device code behind mixq_gemm_w8a16_addend.

  (a) W8A16 with an addend, exact operands, every configuration: bit for bit RNE_16 of the float64 sum (tests/exact.py)
  (b) the addend as a strided, offset window of a NaN-filled frame: nothing outside rows < M / columns < N reaches the output
  (c) the range edge: 65504 stays finite, 65520 becomes inf - through the addend, and through addend + bias
  (d) the operator, int8 and 4-bit, fp16 and bf16: search phase and frozen, one call and two calls, against FusedLinear(addend=) bit for bit
      and against the oracle (fp16: tests/test_gpu_parity.py::ulp_tol; bf16, which the oracle does not speak: the float64 restatement and
      bound of tests/test_gpu_bf16_gemm.py), and a plan that alternates between calls with and without a residual
  (e) a shape the automatic choice splits along N   (f) MixLlamaMLP   (g) hipGraph replay   (h) a weight-only layer through the operator"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact as E  # noqa: E402
from exact import F16  # noqa: E402
from frames import Frame  # noqa: E402
from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib  # noqa: E402
from mixq_amd import linear as linmod  # noqa: E402
from mixq_amd._capi import ACT_NONE  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_gpu_bf16_gemm import _quantise64, check as check_bf16, reference as reference_bf16, unpack_i4  # noqa: E402
from test_gpu_pair import _block  # noqa: E402
from test_gpu_parity import _w8a16_real_configs, n, ulp_tol  # noqa: E402

DEV = "cuda"
H, BF = torch.float16, torch.bfloat16
NAN16 = 0x7E00                                             # a quiet NaN in fp16


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    lib = _capi.load()
    lib.mixq_gemm_set_config(-1); lib.mixq_gemm_w8a16_set_config(-1)
    yield
    lib.mixq_gemm_set_config(-1); lib.mixq_gemm_w8a16_set_config(-1)


def bits_of(y):
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- W8A16: generators ------------------------------------------------------------------------------------------------------------------
_w8 = {}


def w8a16_addend_problem(M, N):
    """E.w8a16_problem plus an addend i 2^-12, |i| <= 2000 (fp16-representable, on every element's quantum 2^-12 .. 2^-14).  Asserts the
    exactness conditions on the data: every z / q an integer, (sum |x| 255 scale + |bias| + |addend|) / q < 2^22.  One shared instance."""
    if (M, N) not in _w8:
        x, qkn, scale, bias, z, q = E.w8a16_problem(M, E.K_MAIN, N)
        rng = np.random.default_rng(1000 + M + N)
        add = E._fit(rng.integers(-2000, 2001, (M, N)), F16) * 2.0 ** -12
        assert E.representable(add, F16) and np.abs(add).max() <= 2000 * 2.0 ** -12
        za = z + add                                          # (z holds the bias)
        r = za / q
        assert np.array_equal(r, np.rint(r)) and np.array_equal(add / q, np.rint(add / q))
        s64, b64 = scale.astype(np.float64), bias.astype(np.float64)
        worst = float(((np.abs(x.astype(np.float64)).sum(axis=1)[:, None] * 255.0 * s64[None, :] + np.abs(b64)[None, :] + np.abs(add)) / q).max())
        assert worst < E.LIMIT, worst
        dev = dict(w=mixlib.PackW8A16(torch.from_numpy(qkn).to(DEV)), x=torch.from_numpy(x).to(DEV), s=torch.from_numpy(scale).to(DEV),
                   b=torch.from_numpy(bias).to(DEV), a=E.as_tensor(add, F16).to(DEV))
        _w8[(M, N)] = (dev, z, add, b64, worst)
    return _w8[(M, N)]


def w8a16_configs(M):
    names = _capi.w8a16_config_names()
    return [-1] + sorted(set(_w8a16_real_configs() + [names.index("w8a16_32x64_s8_d5_l1")] + ([names.index("w8a16_decode32")] if M <= 32 else [])))


def forced_w8a16(cfgs):
    lib, names = _capi.load(), _capi.w8a16_config_names()
    try:
        for c in cfgs:
            assert lib.mixq_gemm_w8a16_set_config(c) == 0
            yield c, (names[c] if c >= 0 else "auto")
    finally:
        assert lib.mixq_gemm_w8a16_set_config(-1) == 0


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.N_SHAPES)
@pytest.mark.parametrize("M", E.M_SHAPES)
def test_w8a16_addend_exact_every_configuration(M, N):
    d, z, add, b64, worst = w8a16_addend_problem(M, N)
    print(f"w8a16 addend {M}x{E.K_MAIN}->{N}: worst sum of absolute terms {worst:.4g} q (limit 2^22 = {E.LIMIT:.4g})")
    K = E.K_MAIN
    for cfg, name in forced_w8a16(w8a16_configs(M)):
        for b, zz in ((None, z - b64[None, :] + add), (d["b"], z + add)):
            y = mixlib.W8A16Linear(d["x"], d["w"], d["s"], b, N, K, addend=d["a"])
            E.assert_exact(bits_of(y), E.to_bits(zz, F16), zz, F16, f"w8a16 + addend {name} {M}x{K}->{N} bias={b is not None}")
            # addend=None is the call without the argument
            assert same(mixlib.W8A16Linear(d["x"], d["w"], d["s"], b, N, K, addend=None), mixlib.W8A16Linear(d["x"], d["w"], d["s"], b, N, K)), name


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------
def addend_layouts(N):
    """(lda, column offset, element offset) of the addend windows: lda in {N, N + 4, N + 24}, a column offset of 4 and an element offset of 4 - each
    an 8-byte-but-not-16-byte aligned base - alone and together (16-byte aligned again)."""
    return [(N, 0, 0), (N, 0, 4), (N + 4, 0, 0), (N + 4, 4, 0), (N + 24, 4, 0), (N + 24, 0, 4), (N + 24, 4, 4)]


@pytest.mark.parametrize("N", E.N_SHAPES)
@pytest.mark.parametrize("M", E.M_SHAPES)
def test_w8a16_addend_window_in_a_nan_frame(M, N):
    d, z, add, b64, _ = w8a16_addend_problem(M, N)
    K = E.K_MAIN
    frames = []
    for lda, co, eo in addend_layouts(N):
        f = Frame(M, N, lda, co, eo, H, DEV, guard_rows=8)
        f.raw.fill_(NAN16)                                   # every element outside the window is a NaN: a read of one poisons the output
        f.view.copy_(d["a"])
        assert f.view.data_ptr() % 8 == 0 and (co + eo != 4 or f.view.data_ptr() % 16 == 8)
        frames.append(((lda, co, eo), f.freeze()))
    fy = Frame(M, N, N + 8, 0, 4, H, DEV)                    # y in a frame of its own (8-byte aligned base: direct stores)
    for cfg, name in forced_w8a16(w8a16_configs(M)):
        want = mixlib.W8A16Linear(d["x"], d["w"], d["s"], d["b"], N, K, addend=d["a"])
        assert bool(torch.isfinite(want).all())
        for lay, f in frames:
            fy.reset()
            y = mixlib.W8A16Linear(d["x"], d["w"], d["s"], d["b"], N, K, out=fy.view, addend=f.view)
            torch.cuda.synchronize()
            what = f"w8a16 + addend {name} {M}x{K}->{N} lda={lay[0]} col_off={lay[1]} elem_off={lay[2]}"
            assert bool(torch.isfinite(y).all()), what
            assert same(y, want), what
            fy.assert_untouched(what)
            f.assert_unchanged(what)                          # (an input: read only)
    with pytest.raises(RuntimeError, match="alias"):
        mixlib.W8A16Linear(d["x"], d["w"], d["s"], d["b"], N, K, out=fy.view, addend=fy.view)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", E.M_SHAPES)
def test_w8a16_addend_range_edge(M):
    """acc s + addend (+ bias) = 65504 exactly stays finite; = 65520 exactly, the tie below 65536, becomes inf (RNE, nothing saturates)."""
    N, K = 136, 64
    x = np.zeros((M, K), dtype=np.float16)
    x[:, 0] = 1.0
    qkn = np.zeros((K, N), dtype=np.int8)
    qkn[0, :] = 3
    qkn[0, 0], qkn[0, 1] = 64, 80                             # acc s = 64 / 80 in columns 0 / 1 (scale 1)
    scale = np.ones(N, dtype=np.float16)
    w, xd, sd = mixlib.PackW8A16(torch.from_numpy(qkn).to(DEV)), torch.from_numpy(x).to(DEV), torch.from_numpy(scale).to(DEV)
    for add01, bias01 in ((65440.0, None), (32.0, 65408.0)):
        add = np.full((M, N), 0.5)
        add[:, :2] = add01
        bias = None
        if bias01 is not None:
            bias = np.zeros(N)
            bias[:2] = bias01
        zz = x.astype(np.float64) @ qkn.astype(np.float64) + add + (0.0 if bias is None else bias[None, :])
        assert zz[0, 0] == 65504.0 and zz[0, 1] == 65520.0 and E.representable(add, F16)
        bd = None if bias is None else E.as_tensor(bias, F16).to(DEV)
        cfgs = [-1] + ([_capi.w8a16_config_names().index("w8a16_decode32")] if M <= 32 else [0])
        for cfg, name in forced_w8a16(cfgs):
            y = mixlib.W8A16Linear(xd, w, sd, bd, N, K, addend=E.as_tensor(add, F16).to(DEV))
            what = f"w8a16 range edge {name} M={M} through {'the addend' if bias is None else 'addend + bias'}"
            E.assert_exact(bits_of(y), E.to_bits(zz, F16), zz, F16, what)
            yc = y.float().cpu()
            assert bool((yc[:, 0] == 65504.0).all()) and bool(torch.isinf(yc[:, 1]).all()) and bool(torch.isfinite(yc[:, 2:]).all()), what


# ---- (d) the operator --------------------------------------------------------------------------------------------------------------------
K_OP, N_OP = 256, 136
COLS = [3, 17, 29, 31, 64, 65, 100, 127, 128, 129, 150, 177, 200, 222, 240, 254, 255]        # 17 planted outlier columns


def make_layer(bit, dtype, M, N=N_OP, K=K_OP, bias=True, seed=11):
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, N, bias=bias).to(dtype)
    cache = MixLibCache(M, bit=bit, device=DEV, config=MixqConfig(act_dtype=dtype))
    kw = {}
    if bit == 4:                                             # 128 static 16-bit columns, the planted ones among them
        rest = [c for c in torch.randperm(K, generator=torch.Generator().manual_seed(2)).tolist() if c not in COLS]
        ls = torch.ones(K)
        ls[COLS + rest[:128 - len(COLS)]] = 20.0
        kw["layer_scales"] = ls
    return MixLinear_GEMM.from_linear(lin, bit, cache=cache, dev=DEV, **kw)


def make_xs(M, dtype, count, K=K_OP, cols=COLS):
    g = torch.Generator().manual_seed(5)
    xs = []
    for _ in range(count):
        x = torch.randn(M, K, generator=g)
        x[:, cols] *= 20.0
        xs.append(x.to(dtype).to(DEV))
    return xs


def make_res(M, N, dtype, seed):
    return torch.randn(M, N, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


class Spy:
    """Records how MixLinear_GEMM._gemm calls FusedLinear (the layer's backend is the mixlib module: the attribute is looked up per call)."""

    def __init__(self, monkeypatch):
        self.calls, orig = [], mixlib.FusedLinear

        def spy(*a, **k):
            self.calls.append((a, dict(k)))
            return orig(*a, **k)
        self.orig = orig
        monkeypatch.setattr(mixlib, "FusedLinear", spy)

    def replay_last(self, addend):
        a, k = self.calls[-1]
        assert k.get("addend") is None
        k = dict(k, addend=addend)
        return self.orig(*a, **k)


def operator_reference(layer, x, r, bit, dtype):
    """fp16: the oracle's fused linear on the oracle's own quantisation of x, with the residual as its addend, and parity's 2-ulp tolerance.
    bf16: the float64 restatement and its derived bound (tests/test_gpu_bf16_gemm.py)."""
    ind = layer.ind
    if dtype == BF:
        q, s = _quantise64(x, ind, bit)
        qw = layer.q_weight
        qw = qw.to(torch.float64) if bit == 8 else unpack_i4(qw).to(torch.float64)
        nn_ = int(ind.numel())
        wo = layer.weight_cache.to(BF) if nn_ else None
        xo = x[:, ind.long()] if nn_ else None
        return reference_bf16(q @ qw.T, s.reshape(-1), layer.scale_col.reshape(-1), xo, wo, nn_, r, layer.bias, ACT_NONE)
    xh = n(x).copy()
    indh = n(ind).astype(np.int32)
    xo = O.extract_outliers_zero(xh, indh)
    qx, sx = O.find_row_scale(xh, bit)
    ref = O.linear_fused(qx, n(layer.q_weight), sx, n(layer.scale_col), xo=xo, wo=n(layer.weight_cache), addend=n(r),
                         bias=None if layer.bias is None else n(layer.bias), bit=bit)
    return ref, None


def check_operator(y, layer, x, r, bit, dtype, what):
    ref, bound = operator_reference(layer, x, r, bit, dtype)
    if dtype == BF:
        check_bf16(y, ref, bound, what)
    else:
        err = np.abs(n(y).astype(np.float64) - ref.astype(np.float64))
        tol = ulp_tol(ref)
        assert (err <= tol).all(), f"{what}: max err / tol {float((err / tol).max()):.3f}"


@pytest.mark.parametrize("M", [24, 72])
@pytest.mark.parametrize("dtype", [H, BF], ids=["f16", "bf16"])
@pytest.mark.parametrize("bit", [8, 4])
def test_operator_residual_is_the_gemm_addend_on_every_route(bit, dtype, M, monkeypatch):
    A, B = make_layer(bit, dtype, M), make_layer(bit, dtype, M)              # A runs with a residual; B, its twin, without - and is recorded
    B.config.one_call_forward = False
    spy = Spy(monkeypatch)
    xs = make_xs(M, dtype, 6)
    rs = [make_res(M, N_OP, dtype, 40 + i) for i in range(6)]
    what = f"W{bit} {str(dtype).replace('torch.', '')} {M}x{K_OP}->{N_OP}"
    # search phase (calls 0 and 1), then frozen (call 2: A's first one-call forward)
    for call in range(3):
        searching = A.add_outliers
        r_before = rs[call].clone()
        ya = A(xs[call].clone(), None, True, residual=rs[call])
        n_spied = len(spy.calls)
        B(xs[call].clone(), None, True)
        assert len(spy.calls) == n_spied + 1
        want = spy.replay_last(rs[call])
        torch.cuda.synchronize()
        assert ya.dtype == dtype and ya.data_ptr() != rs[call].data_ptr() and same(rs[call], r_before), f"{what} call {call}: the residual is read only"
        assert same(ya, want), f"{what} call {call} ({'search' if searching else 'frozen'}): layer(residual=) != FusedLinear(addend=)"
        assert torch.equal(A.ind, B.ind) and A.cnt == B.cnt and A.add_outliers == B.add_outliers, f"{what} call {call}: the outlier search changed"
        assert same(A.cache.x_scale[:M], B.cache.x_scale[:M]), f"{what} call {call}: x_scale"
        check_operator(ya, A, xs[call], rs[call], bit, dtype, f"{what} call {call}")
    assert not A.add_outliers and A._plan is not None and sorted(set(COLS) - set(A.ind.tolist())) == []
    # frozen: one call == two calls == FusedLinear(addend=)
    x, r = xs[3], rs[3]
    y_one = A(x.clone(), None, True, residual=r)
    A.config.one_call_forward = False
    y_two = A(x.clone(), None, True, residual=r)
    A.config.one_call_forward = True
    B(x.clone(), None, True)
    want = spy.replay_last(r)
    assert same(y_one, y_two) and same(y_one, want), f"{what} frozen"
    check_operator(y_one, A, x, r, bit, dtype, f"{what} frozen")
    # the SAME kept argument block, with and without a residual in turn: each call its own result (no stale pointer)
    plan = A._plan
    y0 = B(x.clone(), None, True)
    seq = [(r, want), (None, y0), (rs[4], None), (None, y0), (r, want)]
    for i, (ri, wi) in enumerate(seq):
        yi = A(x.clone(), None, True) if ri is None else A(x.clone(), None, True, residual=ri)
        if wi is None:
            B(x.clone(), None, True)
            wi = spy.replay_last(ri)
        assert A._plan is plan and same(yi, wi), f"{what} alternating call {i}"
    assert int(plan.args.lda) == N_OP and plan.args.addend is not None
    A(x.clone(), None, True)
    assert plan.args.addend is None and int(plan.args.lda) == 0
    # a misaligned base (8-byte pieces need 8 bytes) goes through a copy, a residual in another container is refused
    wide = torch.zeros((M, N_OP + 8), dtype=dtype, device=DEV)
    wide[:, 2:2 + N_OP] = r
    assert wide[:, 2:2 + N_OP].data_ptr() % 8 == 4
    assert same(A(x.clone(), None, True, residual=wide[:, 2:2 + N_OP]), want)
    with pytest.raises(RuntimeError, match="residual must be"):
        A(x.clone(), None, True, residual=r.to(BF if dtype == H else H))
    with pytest.raises(RuntimeError, match="residual must have shape"):
        A(x.clone(), None, True, residual=r[:, :-4])


# ---- (e) the N split -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [H, BF], ids=["f16", "bf16"])
def test_residual_through_the_n_split(dtype):
    M, N, K = 2048, 8200, 128
    plan = _capi.gemm_split_plan(M, N, K, 8, 2, bf16=dtype == BF)
    if plan is None:
        pytest.skip(f"the automatic choice no longer splits {M}x{K}->{N}: nothing to compare")
    assert 0 < plan[0] < N
    lib = _capi.load()
    torch.manual_seed(3)
    cache = MixLibCache(M, device=DEV, config=MixqConfig(act_dtype=dtype))
    layer = MixLinear_GEMM.from_linear(torch.nn.Linear(K, N, bias=True).to(dtype), 8, cache=cache, dev=DEV)
    xs = make_xs(M, dtype, 3, K=K, cols=[5, 77])
    for x in xs:
        layer(x.clone(), None, True)
    assert not layer.add_outliers
    r = make_res(M, N, dtype, 8)
    outs = []
    try:
        for cfg in (-2, -1):                                  # -2: the automatic tiling as ONE launch (the split's first tiling over every column)
            assert lib.mixq_gemm_set_config(cfg) == 0
            outs.append(layer(xs[2].clone(), None, True, residual=r))
            torch.cuda.synchronize()
    finally:
        lib.mixq_gemm_set_config(-1)
    assert same(outs[0], outs[1])
    assert not same(outs[1], layer(xs[2].clone(), None, True))


# ---- (f) MixLlamaMLP ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amax", [True, False], ids=["amax", "noamax"])
@pytest.mark.parametrize("joint", [True, False], ids=["joint", "two_launch"])
def test_mlp_block_residual(joint, amax):
    M, Hd, F = 72, 256, 512
    inner, norm, cache, xs = _block(M, Hd, F, True)
    up, gate, down = inner.up_proj_, inner.gate_proj_, inner.down_proj_
    inner.config.joint_gate_up, inner.config.fuse_down_amax = joint, amax
    for x in xs[:3]:
        inner(norm(x.clone().to(DEV)))                                       # freeze every layer's outlier search
    assert not up.add_outliers and not down.add_outliers
    x = xs[3].to(DEV)
    # |r| <= 1.25: the bound below (the issue's: ulp_tol + 1/2 ulp of the two-step value) then holds for ANY block output z - the two-step
    # form carries the half ulp of fp16(z); for |z| < 2.5 that is below ulp_tol's floor of 1e-3, and beyond it |z + r| >= |z| / 2, so two
    # ulp of the reference cover it.  (A residual that cancels a large z would put the first rounding's error on a small reference.)
    r = (make_res(M, Hd, H, 21).float() * 0.25).clamp(-1.25, 1.25).half()
    r_before = r.clone()
    y = inner(norm(x.clone()), residual=r)
    assert (inner._joint is not None) == joint, "the route that was asked for did not run"
    assert same(r, r_before) and y.data_ptr() != r.data_ptr()
    # the three layers by hand (mlp.py:57-70), the residual handed to down_proj
    xn = norm(x.clone())
    extra = {"amax_for": down} if amax else {}
    g_out = gate.forward_without_preconditionFusedSilu(xn, cache, mul=up(xn, cache), **extra)
    by_hand = down(g_out, None, True, residual=r)
    assert same(y, by_hand)
    # against the block without a residual, added afterwards: the second rounding is at most half an ulp away
    y0 = inner(norm(x.clone()))
    ref = (y0.float() + r.float()).half().float().cpu().numpy()
    err = np.abs(n(y).astype(np.float64) - ref.astype(np.float64))
    half_ulp = 0.5 * E.ulp16(ref.astype(np.float64), F16)
    assert (err <= ulp_tol(ref) + half_ulp).all(), float((err / (ulp_tol(ref) + half_ulp)).max())
    assert not same(y, y0)


# ---- (g) hipGraph ------------------------------------------------------------------------------------------------------------------------------
def test_residual_under_graph_replay_reads_the_buffers_new_contents():
    M = 72
    layer = make_layer(8, H, M)
    xs = make_xs(M, H, 4)
    for x in xs[:3]:
        layer(x.clone(), None, True)
    assert not layer.add_outliers
    x3, r1, r2 = xs[3], make_res(M, N_OP, H, 31), make_res(M, N_OP, H, 32)
    xg, rg = x3.clone(), r1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(xg, None, True, residual=rg)
        xg.copy_(x3)                                          # (the forward zeroes x's outlier columns in place)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            yg = layer(xg, None, True, residual=rg)
        for rnew in (r2, r1, r2):
            xg.copy_(x3)
            rg.copy_(rnew)
            yg.zero_()
            g.replay()
            side.synchronize()
            got = yg.clone()
            assert same(got, layer(x3.clone(), None, True, residual=rnew))
    torch.cuda.synchronize()
    assert not same(layer(x3.clone(), None, True, residual=r1), layer(x3.clone(), None, True, residual=r2))


# ---- (h) a weight-only layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [24, 72])
def test_weight_only_layer_residual(M):
    K, N = 256, 136
    torch.manual_seed(4)
    cache = MixLibCache(M, device=DEV)
    layer = MixLinear_GEMM.from_linear(torch.nn.Linear(K, N, bias=True).half(), 8, weight_only=True, cache=cache, dev=DEV)
    x = torch.randn(2, M // 2, K, generator=torch.Generator().manual_seed(6)).half().to(DEV)
    r = make_res(M, N, H, 7).reshape(2, M // 2, N)
    y = layer(x, residual=r)
    assert tuple(y.shape) == (2, M // 2, N)
    want = mixlib.W8A16Linear(x.reshape(M, K), layer._wpk, layer.scale_col, layer.bias, N, K, addend=r.reshape(M, N))
    assert same(y.reshape(M, N), want)
    y0 = layer(x)
    assert same(y0.reshape(M, N), mixlib.W8A16Linear(x.reshape(M, K), layer._wpk, layer.scale_col, layer.bias, N, K))
    err = (y.float() - (y0.float() + r.float())).abs().max()
    assert float(err) <= 2e-2 and not same(y, y0)
    with pytest.raises(RuntimeError, match="residual must be float16"):
        layer(x, residual=r.bfloat16())
