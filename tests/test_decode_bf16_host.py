"""The small-batch ("decode") kernel in bfloat16 (ABI 1.7), host side (no GPU needed): mixq_gemm_i8_decode_bf16, mixq_gemm_i4_decode_bf16,
mixq_gemm_decode_pick_bf16 and mixq_linear_forward_decode_bf16 are declared, exported and bound; `MixqConfig.decode_bf16` is an opt-in outside
key(); the pick query answers 1 exactly where the fp16 plan names "decode32"; every refusal of include/mixq_hip.h's list is answered with fake
pointers, before any launch; and MixLinear_GEMM hands `decode=True` to its backend exactly where the ONE predicate of linear.py holds, on
both routes (two calls: FusedLinear; one call: ForwardPlan) - seen by a recording backend on top of tests/backend_oracle.py."""
import ctypes as C
import re

import pytest
import torch
from conftest import swap_backend

import backend_oracle
import mixq_amd.linear as L
from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib
from mixq_amd.config import MixqConfig

NEW = ("mixq_gemm_i8_decode_bf16", "mixq_gemm_i4_decode_bf16", "mixq_gemm_decode_pick_bf16", "mixq_linear_forward_decode_bf16")
EINVAL, ESHAPE = _capi.MIXQ_EINVAL, _capi.MIXQ_ESHAPE
WF16, P16, F6 = _capi.X_PACKED | _capi.W_F16X64, _capi.X_PACKED | _capi.W_PACKED, _capi.XW_F6X128
BF = torch.bfloat16


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/mixq_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_four_symbols_are_declared_exported_and_bound():
    lib = _capi.load()
    assert _header_params("mixq_gemm_i8_decode_bf16") == _header_params("mixq_gemm_i8_fused_bf16")
    assert _header_params("mixq_gemm_i4_decode_bf16") == _header_params("mixq_gemm_i4_fused_bf16")
    assert _header_params("mixq_gemm_decode_pick_bf16") == ["int M", "int N", "int K", "int bit", "int layout"]
    assert _header_params("mixq_linear_forward_decode_bf16") == _header_params("mixq_linear_forward_bf16")
    for name in NEW:
        assert name in _capi.header_symbols() and name in _capi.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _capi.SIGNATURES[name] and len(fn.argtypes) == len(_header_params(name))
    assert lib.mixq_version() == 1003                       # the number stays: callers probe for the symbols
    assert "bf16 small-batch form (ABI 1.7)" in open(_capi.HEADER_PATH).read()


def test_decode_bf16_is_an_opt_in_outside_the_key():
    assert MixqConfig().decode_bf16 is False
    on = MixqConfig(act_dtype=BF, decode_bf16=True)
    assert on.decode_bf16 is True and on.key() == MixqConfig(act_dtype=BF).key()       # a route over images that already exist
    assert MixqConfig(decode_bf16=True).key() == MixqConfig().key()
    assert on.copy(decode_bf16=False).decode_bf16 is False


GRID_M, GRID_N, GRID_K = (1, 16, 32, 33), (4, 36, 4096, 8188, 8192, 11008), (64, 4096)


def test_decode_pick_is_where_the_fp16_plan_names_decode32():
    """mixq_gemm_decode_pick_bf16 over M x N x K x (both int8 layouts, nibbles) against the fp16 planner's own answer for the same problem,
    mixq_gemm_pick_config_fmt (asked by weight FORMAT: F16X64, P16X64).  The grid crosses every term of the rule: M = 32 | 33, N = 8188 |
    8192 (the wide-layer exception of the fragment-order int8 image only), K = 64 with nibbles (32 bytes: no whole k-step)."""
    lib = _capi.load()
    q, names = lib.mixq_gemm_decode_pick_bf16, _capi.gemm_config_names()
    ones = 0
    for M in GRID_M:
        for N in GRID_N:
            for K in GRID_K:
                for bit, layout, fmt in ((8, WF16, _capi.FMT_F16X64), (8, P16, _capi.FMT_P16X64), (4, P16, _capi.FMT_P16X64)):
                    cfg = lib.mixq_gemm_pick_config_fmt(M, N, K, bit, fmt)
                    assert cfg >= 0
                    want = 1 if names[cfg] == "decode32" else 0
                    if bit == 4 and N >= 8192:
                        # narrowed by measurement (profiles/decode_bf16.txt): at 4096 -> 11008 the nibble stream is 11 - 14 % slower than the
                        # FP6 tiling a bf16 layer runs otherwise (fp16's plan compares it with another kernel); N = 4096 is 25 - 36 % faster
                        assert want == 1 or M > 32 or K == 64
                        want = 0
                    assert q(M, N, K, bit, layout) == want, (M, N, K, bit, layout)
                    ones += want
    assert 0 < ones < len(GRID_M) * len(GRID_N) * len(GRID_K) * 3
    # the terms, spelled out
    assert q(32, 4096, 4096, 8, WF16) == 1 and q(33, 4096, 4096, 8, WF16) == 0
    assert q(16, 8188, 4096, 8, WF16) == 1 and q(16, 8192, 4096, 8, WF16) == 0 and q(16, 11008, 4096, 8, WF16) == 0
    assert q(16, 8192, 4096, 8, P16) == 1                                              # (the exception is the fragment-order int8 image's)
    assert q(16, 8188, 4096, 4, P16) == 1 and q(16, 8192, 4096, 4, P16) == 0 and q(16, 11008, 4096, 4, P16) == 0   # (nibbles: narrowed by measurement)
    assert q(16, 4096, 64, 4, P16) == 0 and q(16, 4096, 128, 4, P16) == 1
    # layouts the decode entry points do not read: never the route
    for layout in (0, _capi.X_PACKED, _capi.W_PACKED):
        assert q(16, 4096, 4096, 8, layout) == 0 and q(16, 4096, 4096, 4, layout) == 0
    assert q(16, 4096, 4096, 4, F6) == 0 and q(16, 4096, 4096, 4, WF16) == 0
    # bad arguments
    for args in ((0, 64, 64, 8, WF16), (16, 0, 64, 8, WF16), (16, 64, 0, 8, WF16), (16, 64, 64, 5, WF16), (16, 64, 64, 8, 64), (16, 64, 64, 8, F6),
                 (16, 64, 64, 8, P16 | _capi.W_F16X64), (16, 64, 64, 8, _capi.W_F16X64)):
        assert q(*args) == EINVAL, args
    assert mixlib.decode_pick(16, 4096, 4096, 8, _capi.FMT_P16X64, _capi.FMT_F16X64) is True
    assert mixlib.decode_pick(16, 4096, 4096, 4, _capi.FMT_R6X128, _capi.FMT_F6X128) is False
    assert mixlib.decode_pick(16, 4096, 4096, 8, _capi.FMT_PLAIN, _capi.FMT_PLAIN) is False


def test_argument_validation_without_device():
    """Every refusal comes before any launch: fake pointers are never dereferenced."""
    lib = _capi.load()
    one = C.c_void_p(16)
    i8, i4 = lib.mixq_gemm_i8_decode_bf16, lib.mixq_gemm_i4_decode_bf16
    p4, p8, p17 = C.c_void_p(20), C.c_void_p(24), C.c_void_p(17)
    assert lib.mixq_gemm_set_config(-1) == 0

    def fused(fn, layout, M=0, y=one, addend=None, bias=None, x_out=None, w_out=None, n_out=0, lda=64, ld=16, act=0, K=128, N=64, ldy=64, q_x=one):
        return fn(q_x, one, one, one, x_out, ld, w_out, ld, n_out, None, addend, lda, bias, y, ldy, M, N, K, act, layout, None)
    served = ((i8, WF16), (i8, P16), (i4, P16))
    for fn, layout in served:
        assert fused(fn, layout) == 0                                                                       # M = 0
        assert fused(fn, layout, y=p8, addend=p8, bias=C.c_void_p(18), x_out=one, w_out=one, n_out=3) == 0   # 8 / 8 / 2 / 16 / 16: the contract
        assert fused(fn, layout, M=33) == ESHAPE and fused(fn, layout, M=33, q_x=None) == ESHAPE             # (said ahead of the NULL operand)
        assert fused(fn, layout, M=4, act=_capi.ACT_SILU_PAIR) == ESHAPE and fused(fn, layout, act=_capi.ACT_SILU_PAIR) == ESHAPE
        for M in (0, 4):                                                                                    # every alignment refusal
            assert fused(fn, layout, M, y=p4) == EINVAL
            assert fused(fn, layout, M, y=C.c_void_p(18)) == EINVAL
            assert fused(fn, layout, M, addend=p4) == EINVAL
            assert fused(fn, layout, M, addend=p4, lda=0) == EINVAL
            assert fused(fn, layout, M, bias=p17) == EINVAL
            assert fused(fn, layout, M, x_out=p8, w_out=one, n_out=3) == EINVAL
            assert fused(fn, layout, M, x_out=one, w_out=p8, n_out=3) == EINVAL
        assert fused(fn, layout, x_out=p8, w_out=p8, n_out=0) == 0                                          # (no outlier columns: not read)
        # validate_fused's other checks, in its order
        assert fused(fn, layout, M=4, q_x=None) == EINVAL and fused(fn, layout, M=-1) == EINVAL and fused(fn, layout, n_out=-1) == EINVAL
        assert fused(fn, layout, M=4, act=7) == EINVAL and fused(fn, layout, M=4, act=_capi.ACT_SILU_MUL) == EINVAL
        assert fused(fn, layout, M=4, K=96) == ESHAPE and fused(fn, layout, M=4, N=62) == ESHAPE and fused(fn, layout, M=4, ldy=60) == ESHAPE
        assert fused(fn, layout, M=4, act=_capi.ACT_SILU_MUL, ldy=62) == EINVAL                              # no multiplier before a bad ldy
        assert fused(fn, layout, M=4, addend=one, lda=32) == EINVAL
        assert fused(fn, layout, M=4, x_out=one, w_out=one, n_out=3, ld=8) == ESHAPE                         # below the padded width of 16
        assert fused(fn, layout, M=4, K=96, y=p4) == ESHAPE                                                  # a bad K before a misaligned y
    assert fused(i4, P16, M=4, K=64) == ESHAPE and fused(i4, P16, M=4, K=192) == ESHAPE                      # nibbles: K % 128
    # layouts: an FP6 layout and every other one the kernel does not read are unserved shapes; unknown bits (and FP6 codes at the int8 entry,
    # as at every int8 entry point) bad arguments
    assert fused(i4, F6) == ESHAPE and fused(i4, F6, M=4) == ESHAPE and fused(i4, WF16, M=4) == ESHAPE
    for layout in (0, _capi.X_PACKED, _capi.W_PACKED, P16 | _capi.W_F16X64, _capi.W_F16X64):
        assert fused(i8, layout, M=4) == ESHAPE and fused(i4, layout, M=4) == ESHAPE, layout
    assert fused(i8, 64) == EINVAL and fused(i4, 64) == EINVAL and fused(i8, F6) == EINVAL
    # a forced configuration: only decode32 itself runs here, and the refusal comes ahead of the M == 0 early-out
    names = _capi.gemm_config_names()
    try:
        for cfg, name in enumerate(names):
            assert lib.mixq_gemm_set_config(cfg) == 0
            for fn, layout in served:
                assert fused(fn, layout) == (0 if name == "decode32" else EINVAL), name
                assert fused(fn, layout, K=96) == ESHAPE                                                    # (the shape checks still come first)
        assert lib.mixq_gemm_set_config(0) == 0
        assert fused(i8, WF16, M=4) == EINVAL
        assert lib.mixq_gemm_set_config(-2) == 0 and fused(i8, WF16) == 0                                   # (the automatic values run)
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0
    # the one-call forward checks its block before it launches anything
    fwd = lib.mixq_linear_forward_decode_bf16
    assert fwd(None, None) == EINVAL
    blk = _capi.LinearArgs()
    blk.bit = 3
    assert fwd(C.byref(blk), None) == EINVAL
    for bit, wfmt in ((8, _capi.FMT_F16X64), (8, _capi.FMT_P16X64), (4, _capi.FMT_P16X64)):
        def block(M, wfmt=wfmt, qfmt=_capi.FMT_P16X64):
            blk = _capi.LinearArgs()
            blk.x = blk.x_scale = blk.q_x = blk.q_w = blk.scale_col = blk.y = blk.ind = blk.x_out = blk.w_out = blk.addend = blk.bias = 16
            blk.ldx, blk.ldy, blk.lda, blk.ldxo, blk.ldwo, blk.n_cap = 128, 64, 64, 16, 16, 3
            blk.M, blk.N, blk.K, blk.bit, blk.sigma, blk.qfmt, blk.wfmt = M, 64, 128, bit, 6.0, qfmt, wfmt
            return blk
        assert fwd(C.byref(block(0)), None) == 0                                    # the aligned positive control: every check runs, nothing is launched
        assert fwd(C.byref(block(33)), None) == ESHAPE
        for other in (_capi.FMT_PLAIN, _capi.FMT_F6X128) + ((_capi.FMT_F16X64,) if bit == 4 else ()):
            assert fwd(C.byref(block(4, wfmt=other)), None) == ESHAPE, (bit, other)
        assert fwd(C.byref(block(4, qfmt=_capi.FMT_PLAIN)), None) == ESHAPE
        paired = block(4)
        paired.act = _capi.ACT_SILU_PAIR
        assert fwd(C.byref(paired), None) == ESHAPE
        for field, value in (("y", 20), ("addend", 20), ("bias", 17), ("x_out", 24), ("w_out", 24)):        # the five misaligned fields
            for M in (0, 4):
                blk = block(M)
                setattr(blk, field, value)
                assert fwd(C.byref(blk), None) == EINVAL, (field, M)


# ---- routing: what MixLinear_GEMM hands its backend --------------------------------------------------------------------------------------
class Recorder:
    """tests/backend_oracle.py with the two GEMM-side calls recorded instead of computed (the GEMM is not what these tests are about: y is
    zeros) and the product's decode_pick, which asks the library and needs no device.  Neither FusedLinear nor ForwardPlan of this backend
    knows a `decode` argument unless it is handed one: a call that passes it where the predicate does not hold shows up in `seen`."""

    def __init__(self):
        rec = self
        self.seen = []                                       # (what, M, N, kwargs the call carried beyond the oracle backend's own)

        class Plan(backend_oracle.ForwardPlan):
            def __init__(self, M, N, *args, **kw):
                rec.seen.append(("ForwardPlan", M, N, "decode" in kw, kw.get("decode")))
                kw.pop("decode", None)
                super().__init__(M, N, *args, **kw)

            def run(self, x, row_amax=None, col_mask=None, addend=None):
                ind_buf, n_dev, x_scale = self.keep[:3]
                q, xo = backend_oracle.QuantFused(x, ind_buf, x_scale, self.bit, self.sigma, n_dev=n_dev, fmt=self.qfmt, col_mask=col_mask or self.kept_mask)
                return torch.zeros(self.M, self.N, dtype=self.dtype), q, (xo[:, : self.n] if xo is not None else None)
        self.ForwardPlan = Plan

    def FusedLinear(self, q_x, q_w, x_scale, scale_col, x_out, w_out, n_out, bias, M, N, K, **kw):
        self.seen.append(("FusedLinear", M, N, "decode" in kw, kw.get("decode")))
        return torch.zeros(M, N, dtype=kw.get("dtype", torch.float16))

    decode_pick = staticmethod(mixlib.decode_pick)

    def __getattr__(self, name):
        return getattr(backend_oracle, name)


@pytest.fixture()
def recorder():
    rec = Recorder()
    prev = swap_backend(L, rec)
    yield rec
    swap_backend(L, prev)


_linears = {}


def _layer(K, N, config, frozen, weight_only=False):
    if (K, N) not in _linears:
        torch.manual_seed(K + N)
        _linears[(K, N)] = torch.nn.Linear(K, N, bias=False).to(torch.float16)
    cache = MixLibCache(64, device="cpu", config=config)
    layer = MixLinear_GEMM.from_linear(_linears[(K, N)], 8, weight_only=weight_only, cache=cache, dev="cpu")
    if frozen:
        layer.add_outliers = False
    else:
        cache.stop = 1000                                    # (the search phase lasts the test)
    return layer, cache


def _x(M, K, dtype):
    return (torch.randn(M, K, generator=torch.Generator().manual_seed(M)) * 0.5).to(dtype)


def _decode_flags(rec, what):
    return [(s[3], s[4]) for s in rec.seen if s[0] == what]


def test_flag_off_never_passes_decode(recorder):
    for one_call in (False, True):
        layer, cache = _layer(4096, 4096, MixqConfig(act_dtype=BF, one_call_forward=one_call), frozen=True)
        for M in (1, 32, 33):
            layer(_x(M, 4096, BF), None, True)
    assert recorder.seen and all(s[3] is False for s in recorder.seen), recorder.seen
    assert {s[0] for s in recorder.seen} == {"FusedLinear", "ForwardPlan"}


def test_flag_on_passes_decode_where_the_predicate_holds_on_both_routes(recorder):
    on = MixqConfig(act_dtype=BF, decode_bf16=True)
    # the two-call route (a layer in its search phase, and a frozen one with one_call_forward off) and the one-call route
    for config, frozen, what in ((on, False, "FusedLinear"), (on.copy(one_call_forward=False), True, "FusedLinear"), (on, True, "ForwardPlan")):
        layer, cache = _layer(4096, 4096, config, frozen)
        for M, want in ((1, True), (8, True), (32, True), (33, False)):
            recorder.seen.clear()
            layer(_x(M, 4096, BF), None, True)
            assert _decode_flags(recorder, what) == [(want, True if want else None)], (what, M, recorder.seen)
            assert len(recorder.seen) == 1


def test_flag_on_does_not_pass_decode_where_it_does_not_hold(recorder):
    on = MixqConfig(act_dtype=BF, decode_bf16=True)
    # a wide int8 layer (fragment-order weights, N >= 8192): both configurations take the 32 x 64 tiling
    for frozen in (False, True):
        layer, cache = _layer(4096, 11008, on, frozen)
        layer(_x(8, 4096, BF), None, True)
    # a row maximum asked of this GEMM (gate_proj handing down_proj its maxima: the side output lives in the weights-in-registers kernels)
    layer, cache = _layer(4096, 4096, on, frozen=False)
    layer(_x(8, 4096, BF), None, True)
    assert recorder.seen[-1][3] is True
    layer._gemm(cache, 8, _capi.ACT_SILU, row_amax=torch.zeros(16, dtype=torch.int32), col_mask=None)
    assert recorder.seen[-1][3] is False
    before = len(recorder.seen)
    assert [s[3] for s in recorder.seen[:before - 2]] == [False, False]
    # an fp16 model: the flag has no effect (fp16 takes the kernel by itself, inside mixq_gemm_i8_fused)
    for frozen in (False, True):
        layer, cache = _layer(4096, 4096, MixqConfig(decode_bf16=True), frozen)
        layer(_x(8, 4096, torch.float16), None, True)
    assert len(recorder.seen) == before + 2 and all(s[3] is False for s in recorder.seen[before:])
    # a weight-only layer never reaches either call
    prev = swap_backend(__import__("mixq_amd.eetq", fromlist=["eetq"]), backend_oracle)
    try:
        layer, cache = _layer(4096, 4096, on.copy(w8a16_bf16=True), frozen=False, weight_only=True)
        assert layer._decode_applies(8, None) is False
        layer(_x(8, 4096, BF), None, True)
    finally:
        swap_backend(__import__("mixq_amd.eetq", fromlist=["eetq"]), prev)
    assert len(recorder.seen) == before + 2


def test_flipping_the_flag_on_a_frozen_layer_changes_the_next_forward(recorder):
    config = MixqConfig(act_dtype=BF)
    layer, cache = _layer(4096, 4096, config, frozen=True)
    x = _x(8, 4096, BF)
    layer(x.clone(), None, True)
    layer(x.clone(), None, True)                             # (the kept plan: no second build)
    assert _decode_flags(recorder, "ForwardPlan") == [(False, None)]
    config.decode_bf16 = True
    layer(x.clone(), None, True)
    assert _decode_flags(recorder, "ForwardPlan") == [(False, None), (True, True)]
    config.decode_bf16 = False
    layer(x.clone(), None, True)                             # back: the first plan again, kept under its own identity
    layer(x.clone(), None, True)
    assert _decode_flags(recorder, "ForwardPlan") == [(False, None), (True, True)]


def test_a_library_without_the_symbols_is_a_runtime_error_naming_them(monkeypatch):
    class Old:
        """A library of an earlier ABI minor: everything but the ABI 1.7 entry points."""
        def __getattr__(self, name):
            if name in NEW:
                raise AttributeError(name)
            return getattr(_capi.load(), name)
    old = Old()
    monkeypatch.setattr(mixlib._capi, "load", lambda: old)
    for name in NEW:
        with pytest.raises(RuntimeError, match=name):
            mixlib._decode_bf16_entry(name)
    with pytest.raises(RuntimeError, match="mixq_gemm_decode_pick_bf16"):
        mixlib.decode_pick(8, 4096, 4096, 8, _capi.FMT_P16X64, _capi.FMT_F16X64)
    t = torch.zeros(16, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="mixq_gemm_i8_decode_bf16"):
        mixlib.FusedLinear(t, t, t, t, None, None, 0, None, 8, 64, 64, dtype=BF, decode=True)
    with pytest.raises(RuntimeError, match="mixq_gemm_i4_decode_bf16"):
        mixlib.FusedLinear(t, t, t, t, None, None, 0, None, 8, 64, 128, bit=4, dtype=BF, decode=True)
    with pytest.raises(RuntimeError, match="mixq_linear_forward_decode_bf16"):
        mixlib.ForwardPlan(8, 64, 64, 8, 6.0, 64, None, 0, None, t, t, t, None, None, _capi.FMT_P16X64, dtype=BF, decode=True)


def test_decode_with_what_the_kernel_does_not_serve_says_why():
    t = torch.zeros(16, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="decode=True.*row-maximum"):
        mixlib.FusedLinear(t, t, t, t, None, None, 0, None, 8, 64, 64, dtype=BF, decode=True, row_amax=torch.zeros(16, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="decode=True.*ACT_SILU_PAIR"):
        mixlib.FusedLinear(t, t, t, t, None, None, 0, None, 8, 64, 64, act=_capi.ACT_SILU_PAIR, dtype=BF, decode=True)
    with pytest.raises(RuntimeError, match="decode=True.*float16"):
        mixlib.FusedLinear(t, t, t, t, None, None, 0, None, 8, 64, 64, decode=True)
    with pytest.raises(RuntimeError, match="decode=True.*float16"):
        mixlib.ForwardPlan(8, 64, 64, 8, 6.0, 64, None, 0, None, t, t, t, None, None, _capi.FMT_P16X64, decode=True)
    with pytest.raises(RuntimeError, match="decode=True.*ACT_SILU_PAIR"):
        mixlib.ForwardPlan(8, 64, 64, 8, 6.0, 64, None, 0, None, t, t, t, None, None, _capi.FMT_P16X64, act=_capi.ACT_SILU_PAIR, dtype=BF, decode=True)


def test_a_backend_without_the_query_never_sees_decode():
    """tests/backend_oracle.py as it is has no decode_pick: with the flag on, a layer on it runs as with the flag off."""
    prev = swap_backend(L, backend_oracle)
    try:
        assert not hasattr(backend_oracle, "decode_pick")
        layer, cache = _layer(512, 64, MixqConfig(act_dtype=BF, decode_bf16=True), frozen=False)
        assert layer._decode_applies(8, layer._packed_weight(8)) is False
        y = layer(_x(8, 512, BF), None, True)                # (FusedLinear of the oracle backend takes no `decode` argument: it was not handed one)
        assert y.dtype == BF and tuple(y.shape) == (8, 64)
    finally:
        swap_backend(L, prev)


def test_a_4bit_layer_serves_from_the_nibble_image_only_where_the_form_is_picked(recorder):
    """small_batch_m4 in a bfloat16 model: with decode_bf16 the nibble image serves M <= 32 of a narrow layer; a wide layer (N >= 8192, where
    the FP6 tiling measured faster) and larger batches keep the FP6 image.  Without the flag the combination is what it was."""
    for N, M, flag, want in ((4096, 8, True, True), (8192, 8, True, False), (4096, 33, True, False), (4096, 8, False, True), (8192, 8, False, True)):
        cache = MixLibCache(64, bit=4, device="cpu", config=MixqConfig(act_dtype=BF, decode_bf16=flag, small_batch_m4=64))
        layer = MixLinear_GEMM(128, N, False, "cpu", 4, cache=cache)
        assert layer._small_batch_image(M) is want, (N, M, flag)
    cache = MixLibCache(64, bit=4, device="cpu", config=MixqConfig(decode_bf16=True, small_batch_m4=64))       # float16: the flag does nothing
    assert MixLinear_GEMM(128, 8192, False, "cpu", 4, cache=cache)._small_batch_image(8) is True
