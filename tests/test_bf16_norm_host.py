"""The bfloat16 RMSNorm entry points and the opt-in that lets a bfloat16 model reach them, host side (no GPU): mixq_rmsnorm_bf16,
mixq_rmsnorm_quant_fused_bf16 and mixq_rmsnorm_quant_fused_masked_bf16 are declared, exported and bound with their fp16 twins' parameter
lists; they answer bad arguments before any launch with their twins' codes; `MixqConfig.fused_bf16` is off by default, no part of key(),
and is what lets FasterTransformerRMSNorm and MixLlamaMLP construct under a bfloat16 config - without it they refuse as before; the joint
gate / up launch stays float16 only."""
import ctypes as C
import re

import pytest
import torch

from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib
from mixq_amd.config import MixqConfig
from mixq_amd.fused import FasterTransformerRMSNorm, MixLlamaMLP

TWINS = ["mixq_rmsnorm", "mixq_rmsnorm_quant_fused", "mixq_rmsnorm_quant_fused_masked"]
EINVAL, ESHAPE, OK = _capi.MIXQ_EINVAL, _capi.MIXQ_ESHAPE, _capi.MIXQ_OK
P = C.c_void_p(4096)                                     # never dereferenced: every call below ends before a launch


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/mixq_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", TWINS)
def test_bf16_norm_twin_is_declared_exported_and_bound(name):
    assert name + "_bf16" in _capi.header_symbols()
    assert _header_params(name + "_bf16") == _header_params(name)
    assert _capi.SIGNATURES[name + "_bf16"] == _capi.SIGNATURES[name]
    fn = getattr(_capi.load(), name + "_bf16")
    assert fn.argtypes == _capi.SIGNATURES[name] and fn.restype is C.c_int


def _plain(fn, x=P, w=P, out=P, M=4, K=128, ldx=None, ldout=None):
    return fn(x, w, out, M, K, K if ldx is None else ldx, K if ldout is None else ldout, 1e-6, None)


def _fused(fn, masked, x=P, w=P, out=P, ind=None, n=0, x_scale=P, q=P, x_out=None, M=4, K=128, ldxo=0, bit=8, qfmt=0, col_mask=None, map_words=0):
    head = (x, w, out, ind, n, None) + ((col_mask, map_words) if masked else ())
    return fn(*head, x_scale, q, x_out, None, M, K, K, K, ldxo, 1e-6, bit, 6.0, qfmt, None)


@pytest.mark.parametrize("sfx", ["", "_bf16"])
def test_plain_norm_answers_bad_arguments_before_any_launch(sfx):
    fn = getattr(_capi.load(), "mixq_rmsnorm" + sfx)
    for slot in ("x", "w", "out"):
        assert _plain(fn, **{slot: None}) == EINVAL
    assert _plain(fn, K=0) == EINVAL and _plain(fn, M=-1) == EINVAL
    assert _plain(fn, K=132) == ESHAPE                                       # K % 8
    assert _plain(fn, ldx=120) == ESHAPE and _plain(fn, ldout=132) == ESHAPE # a stride below K, a stride that is no multiple of 8
    assert _plain(fn, K=32776) == ESHAPE                                     # 4097 chunks: more than 16 per thread
    assert _plain(fn, M=0) == OK and _plain(fn, M=0, x=None, w=None, out=None) == OK


@pytest.mark.parametrize("sfx", ["", "_bf16"])
@pytest.mark.parametrize("masked", [False, True])
def test_fused_norm_answers_bad_arguments_before_any_launch(sfx, masked):
    fn = getattr(_capi.load(), "mixq_rmsnorm_quant_fused" + ("_masked" if masked else "") + sfx)
    words = _capi.load().mixq_kept_map_words(128)
    f = lambda **kw: _fused(fn, masked, **kw)
    for slot in ("x", "w", "out", "x_scale", "q"):
        assert f(**{slot: None}) == EINVAL                                   # NULL operands
    for bit in (0, 5, 16):
        assert f(bit=bit) == EINVAL
    assert f(qfmt=7) == EINVAL
    assert f(bit=8, qfmt=_capi.FMT_F6X128) == EINVAL and f(bit=8, qfmt=_capi.FMT_R6X128) == EINVAL      # FP6 codes are the 4-bit form's
    # outlier columns need their operands
    good_map = dict(col_mask=P, map_words=words) if masked else {}
    assert f(n=3, ind=None, x_out=P, ldxo=16, **good_map) == EINVAL
    assert f(n=3, ind=P, x_out=None, ldxo=16, **good_map) == EINVAL
    assert f(n=3, ind=P, x_out=P, ldxo=2, **good_map) == EINVAL
    assert f(K=132) == ESHAPE                                                # K % 8
    assert f(K=136, bit=4) == ESHAPE                                         # 4-bit: K % 16
    # a packed format needs whole 64-byte blocks of a row: K % 64, for nibbles and FP6 codes K / 2 % 64
    for qfmt in (_capi.FMT_P16X64, _capi.FMT_F16X64):
        assert f(K=96, qfmt=qfmt) == ESHAPE and f(K=192, bit=4, qfmt=qfmt) == ESHAPE
    for qfmt in (_capi.FMT_F6X128, _capi.FMT_R6X128):
        assert f(K=192, bit=4, qfmt=qfmt) == ESHAPE
    assert f(K=32776) == ESHAPE and f(K=32784, bit=4) == ESHAPE              # more than 16 chunks per thread
    if masked:                                                               # the kept map: present, long enough, 16-byte aligned
        assert f(n=3, ind=P, x_out=P, ldxo=16, col_mask=None, map_words=words) == EINVAL
        assert f(n=3, ind=P, x_out=P, ldxo=16, col_mask=P, map_words=words - 1) == EINVAL
        assert f(n=3, ind=P, x_out=P, ldxo=16, col_mask=C.c_void_p(4096 + 8), map_words=words) == EINVAL
        assert f(n=3, ind=P, x_out=P, ldxo=16, col_mask=C.c_void_p(4096 + 8), map_words=words, M=0) == EINVAL   # (answered ahead of the early-out)
        assert f(n=0, col_mask=None, map_words=0, M=0) == OK                 # (no outlier columns: no map needed)
    assert f(M=0) == OK and f(M=0, x=None, w=None, out=None, x_scale=None, q=None) == OK
    assert f(M=0, n=3, ind=P, x_out=P, ldxo=16, **good_map) == OK
    for bit, qfmt, K in ((8, _capi.FMT_P16X64, 128), (8, _capi.FMT_F16X64, 128), (4, _capi.FMT_P16X64, 128), (4, _capi.FMT_F6X128, 128), (4, _capi.FMT_R6X128, 256)):
        assert f(M=0, bit=bit, qfmt=qfmt, K=K) == OK


def test_fused_bf16_is_an_opt_in_and_no_part_of_the_key():
    assert MixqConfig().fused_bf16 is False
    on = MixqConfig(act_dtype=torch.bfloat16, fused_bf16=True)
    assert on.fused_bf16 is True and on.copy().fused_bf16 is True
    assert on.key() == MixqConfig(act_dtype=torch.bfloat16).key()            # it selects no GEMM plan
    assert MixqConfig(fused_bf16=True).key() == MixqConfig().key()
    assert on.key() != MixqConfig().key()                                    # (act_dtype still is)


def _mlp_layers(cache, bit=8):
    return (MixLinear_GEMM(128, 256, False, "cpu", bit, cache=cache), MixLinear_GEMM(256, 128, False, "cpu", bit, cache=cache),
            MixLinear_GEMM(128, 256, False, "cpu", bit, cache=cache))


def test_fused_modules_construct_under_bf16_only_with_the_flag():
    off = MixLibCache(8, device="cpu", config=MixqConfig(act_dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="MixLlamaMLP has no bfloat16 form yet"):
        MixLlamaMLP(*_mlp_layers(off), off)
    with pytest.raises(NotImplementedError, match="FasterTransformerRMSNorm has no bfloat16 form yet"):
        FasterTransformerRMSNorm(torch.ones(128), cache=off)
    on = MixLibCache(8, device="cpu", config=MixqConfig(act_dtype=torch.bfloat16, fused_bf16=True))
    mlp = MixLlamaMLP(*_mlp_layers(on), on)
    assert mlp.config.fused_bf16 and mlp.up_proj_.act_dtype is torch.bfloat16
    assert mlp._joint_applies(on) is False                                   # the joint gate / up launch stays float16 only
    w = (1 + 0.01 * torch.arange(128)).to(torch.bfloat16)
    norm = FasterTransformerRMSNorm(w, cache=on)
    assert norm.weight.dtype == torch.bfloat16 and torch.equal(norm.weight, w)           # the checkpoint's bf16 weight, unrounded
    # float16 models: what they were
    fp = MixLibCache(8, device="cpu")
    assert FasterTransformerRMSNorm(w, cache=fp).weight.dtype == torch.float16
    assert FasterTransformerRMSNorm(w).weight.dtype == torch.float16
    MixLlamaMLP(*_mlp_layers(fp), fp)


def test_norm_without_a_cache_derives_its_bf16_operand_once_and_checks_x():
    on = MixLibCache(8, device="cpu", config=MixqConfig(act_dtype=torch.bfloat16, fused_bf16=True))
    w = 1 + 0.01 * torch.arange(128, dtype=torch.float32)
    norm = FasterTransformerRMSNorm(w)                                       # no cache: float16 is stored ...
    assert norm.weight.dtype == torch.float16
    a = norm._operand(torch.bfloat16)                                        # ... and the bf16 operand derived from it
    assert a.dtype == torch.bfloat16 and torch.equal(a, w.half().to(torch.bfloat16))
    assert norm._operand(torch.bfloat16) is a and norm._operand(torch.float16) is norm.weight
    norm.weight = (w * 2).half()
    assert norm._operand(torch.bfloat16) is not a
    # the model's dtype comes from the next layer when there is no cache; x of another dtype is refused by name, before anything runs
    norm.next_layer = MixLinear_GEMM(128, 64, False, "cpu", 8, cache=on)
    with pytest.raises(RuntimeError, match=r"x must be bfloat16 .*got torch\.float16"):
        norm(torch.zeros(2, 128, dtype=torch.float16))
    off_layer = MixLinear_GEMM(128, 64, False, "cpu", 8, cache=MixLibCache(8, device="cpu", config=MixqConfig(act_dtype=torch.bfloat16)))
    norm.next_layer = off_layer
    with pytest.raises(NotImplementedError, match="bfloat16"):               # a next layer whose config has not opted in: refused at forward, as before
        norm(torch.zeros(2, 128, dtype=torch.bfloat16))
    fp_norm = FasterTransformerRMSNorm(w, cache=MixLibCache(8, device="cpu"))
    with pytest.raises(RuntimeError, match=r"x must be float16 .*got torch\.bfloat16"):
        fp_norm(torch.zeros(2, 128, dtype=torch.bfloat16))


def test_mixlib_norm_functions_name_the_argument_of_another_dtype():
    x = torch.zeros(2, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"RMSNormQuantFused: weight must be torch\.bfloat16 like x, got torch\.float16"):
        mixlib._check_norm_dtypes(x, "RMSNormQuantFused", weight=x.half(), out=x)
    with pytest.raises(RuntimeError, match=r"layernorm_forward_cuda: out must be torch\.bfloat16 like x, got torch\.float16"):
        mixlib._check_norm_dtypes(x, "layernorm_forward_cuda", weight=x, out=x.half())
    with pytest.raises(RuntimeError, match=r"weight must be torch\.float16 like x"):
        mixlib._check_norm_dtypes(x.half(), "layernorm_forward_cuda", weight=x, out=x.half())
    mixlib._check_norm_dtypes(x, "f", weight=x, out=x)
    assert mixlib._act_suffix(x, "f") == "_bf16" and mixlib._act_suffix(x.half(), "f") == ""
