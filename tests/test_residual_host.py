"""The residual add in the GEMM epilogue, host side (no GPU): the new entry point mixq_gemm_w8a16_addend is exported, bound and declared with
the same arity; its argument checks answer before any launch, in the order of mixq_gemm_w8a16's own (sizes and NULL operands, strides,
pointers); and `MixLinear_GEMM.forward(..., residual=)` refuses what it documents, naming the argument."""
import ctypes as C
import inspect
import re

import pytest
import torch

from mixq_amd import MixLibCache, MixLinear_GEMM, MixLlamaMLP, _capi, mixlib

NAME = "mixq_gemm_w8a16_addend"


def test_new_symbol_is_exported_bound_and_matches_the_header():
    lib = _capi.load()
    assert NAME in _capi.header_symbols()
    fn = getattr(lib, NAME)
    assert fn.argtypes == _capi.SIGNATURES[NAME] and fn.restype is C.c_int
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", txt)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(_capi.SIGNATURES[NAME]) == 13
    # the argument list of mixq_gemm_w8a16 with (addend, lda) in front of the bias
    base = re.search(r"\bint\s+mixq_gemm_w8a16\s*\(([^)]*)\)", txt).group(1)
    base = [p.strip() for p in base.split(",")]
    assert params[:4] == base[:4] and params[4:6] == ["const uint16_t* addend", "int lda"] and params[6:] == base[4:]
    assert lib.mixq_version() == 1003


def test_argument_checks_answer_before_any_launch():
    lib = _capi.load()
    f, g = getattr(lib, NAME), lib.mixq_gemm_w8a16
    one = C.c_void_p(4096)                                   # never dereferenced: every call below ends before a launch
    odd = C.c_void_p(4100)                                   # 4-byte aligned, not 8
    assert f(one, 128, one, one, one, 64, None, one, 64, 0, 64, 128, None) == 0                       # M == 0, everything in order
    assert f(one, 128, one, one, None, 0, None, one, 64, 0, 64, 128, None) == 0                       # ... and without an addend (lda ignored)
    for M in (0, 4):
        assert f(one, 128, one, one, one, 60, None, one, 64, M, 64, 128, None) == _capi.MIXQ_ESHAPE   # lda < N
        assert f(one, 128, one, one, one, 66, None, one, 64, M, 64, 128, None) == _capi.MIXQ_ESHAPE   # lda % 4
        assert f(one, 128, one, one, odd, 64, None, one, 64, M, 64, 128, None) == _capi.MIXQ_EINVAL   # base 4-byte aligned
        assert f(one, 128, one, one, odd, 60, None, one, 64, M, 64, 128, None) == _capi.MIXQ_ESHAPE   # both: the stride is checked first
    # a fault of the arguments that were always there, together with a bad addend: what mixq_gemm_w8a16 answers for it
    for bad in ((odd, 64), (one, 60), (odd, 66)):
        want = g(one, 128, one, one, None, one, 64, 4, 64, 100, None)
        assert want == _capi.MIXQ_ESHAPE and f(one, 128, one, one, bad[0], bad[1], None, one, 64, 4, 64, 100, None) == want      # K % 64
    assert f(None, 128, one, one, odd, 60, None, one, 64, 4, 64, 128, None) == g(None, 128, one, one, None, one, 64, 4, 64, 128, None) == _capi.MIXQ_EINVAL
    assert f(one, 128, one, one, one, 64, None, C.c_void_p(20), 64, 4, 64, 128, None) == _capi.MIXQ_EINVAL                         # y alignment, as ever


def _layer(weight_only=False, N=64):
    cache = MixLibCache(8, device="cpu")
    return MixLinear_GEMM(128, N, False, "cpu", bit=8, weight_only=weight_only, cache=cache)


@pytest.mark.parametrize("weight_only", [False, True])
def test_forward_refuses_a_residual_that_is_not_what_it_documents(weight_only):
    layer = _layer(weight_only)
    x = torch.zeros((2, 2, 128), dtype=torch.float16)
    good = torch.zeros((2, 2, 64), dtype=torch.float16)
    with pytest.raises(RuntimeError, match=r"residual must be float16 .*got torch\.float32"):
        layer(x, None, True, residual=good.float())
    with pytest.raises(RuntimeError, match=r"residual must be float16 .*got torch\.bfloat16"):
        layer(x, None, True, residual=good.bfloat16())
    with pytest.raises(RuntimeError, match=r"residual must have shape \(2, 2, 64\).*got \(4, 64\)"):
        layer(x, None, True, residual=good.reshape(4, 64))
    with pytest.raises(RuntimeError, match=r"residual must have shape \(2, 2, 64\).*got \(2, 2, 128\)"):
        layer(x, None, True, residual=x)
    with pytest.raises(RuntimeError, match=r"residual must be a GPU \(HIP\) tensor on x's device"):
        layer(x, None, True, residual=good)                   # (a CPU tensor: the product has no CPU path)
    with pytest.raises(RuntimeError, match=r"residual must be a float16 tensor"):
        layer(x, None, True, residual=1.0)


def test_a_bf16_layer_wants_a_bf16_residual():
    from mixq_amd.config import MixqConfig
    cache = MixLibCache(8, device="cpu", config=MixqConfig(act_dtype=torch.bfloat16))
    layer = MixLinear_GEMM(128, 64, False, "cpu", bit=8, cache=cache)
    x = torch.zeros((4, 128), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"residual must be bfloat16 .*got torch\.float16"):
        layer(x, None, True, residual=torch.zeros((4, 64), dtype=torch.float16))


def test_the_python_surfaces_take_the_new_argument_and_default_to_none():
    for fn, name in ((MixLinear_GEMM.forward, "residual"), (MixLlamaMLP.forward, "residual"), (mixlib.ForwardPlan.run, "addend"), (mixlib.W8A16Linear, "addend")):
        p = inspect.signature(fn).parameters
        assert name in p and p[name].default is None, (fn, name)
    # the reference's positional orders are what they were
    assert list(inspect.signature(MixLinear_GEMM.forward).parameters)[:4] == ["self", "x", "cache", "unfused"]
    assert list(inspect.signature(mixlib.W8A16Linear).parameters)[:7] == ["x", "w_packed", "scale_col", "bias", "N", "K", "out"]
    assert list(inspect.signature(mixlib.ForwardPlan.run).parameters)[:4] == ["self", "x", "row_amax", "col_mask"]
