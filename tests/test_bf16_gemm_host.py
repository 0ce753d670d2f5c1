"""bfloat16 layers, host side (no GPU needed): the `_bf16` GEMM entry points and the one-call forward are declared, exported and bound
with their fp16 twins' argument lists (ABI 1.2), they answer bad arguments, unserved layouts and forced tilings without a bf16 form
before any launch, `MixqConfig.act_dtype` is part of a plan's identity, what bfloat16 does not serve is refused at construction, and the
ISA tripwire sees the 15 bf16 instantiations of gemm_wreg.hip."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from mixq_amd import _capi
from mixq_amd.config import MixqConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = ["mixq_gemm_i8_fused", "mixq_gemm_i4_fused", "mixq_gemm_i8_fused_amax", "mixq_gemm_amax_supported", "mixq_linear_forward"]
# the tilings with a bf16 form, by name (gemm_wreg.hip: g_cost8 + WR_SMALL for int8, g_cost6 + WR_SMALL for the FP6 form)
BF16_INT8 = ["wr128x192_s16_d4_l2", "wr128x128_s16_d4_l2", "wr128x256_s16_d3_l2", "wr64x128_s16_d4_l2", "wr64x192_s16_d4_l2", "wr64x256_s16_d4_l2",
             "wr128x64_s8_d4_l1", "wr64x64_s8_d4_l1", "wr32x64_s8_d6_l1"]
BF16_FP6 = ["wr128x192_s16_d4_l2", "wr128x128_s16_d4_l2", "wr64x128_s16_d4_l2", "wr64x192_s16_d4_l2", "wr64x256_s16_d4_l2", "wr32x64_s8_d6_l1"]


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/mixq_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", TWINS)
def test_bf16_gemm_twin_is_declared_exported_and_bound(name):
    assert _header_params(name + "_bf16") == _header_params(name)
    assert _capi.SIGNATURES[name + "_bf16"] == _capi.SIGNATURES[name]
    fn = getattr(_capi.load(), name + "_bf16")
    assert fn.argtypes == _capi.SIGNATURES[name]


def test_abi_version_is_1_2():
    assert _capi.load().mixq_version() >= 1002


def _gemm_args(fake, layout, q_x=None, K=128, act=0, addend=None):
    """Argument list of mixq_gemm_i8_fused / mixq_gemm_i4_fused for a 64 x K -> 64 problem without outlier columns."""
    return (fake if q_x is None else q_x, fake, fake, fake, None, 0, None, 0, 0, None, addend, 0, None, fake, 64, 64, 64, K, act, layout, None)


def _amax_args(fake, layout, row_amax):
    """... of mixq_gemm_i8_fused_amax: row_amax and col_mask stand between the layout and the stream."""
    return _gemm_args(fake, layout)[:-1] + (row_amax, None, None)


def test_bf16_gemms_answer_bad_arguments_and_unserved_layouts_before_any_launch():
    lib = _capi.load()
    fake = C.c_void_p(16)                                   # never dereferenced: every call below fails its argument checks first
    EINVAL, ESHAPE = _capi.MIXQ_EINVAL, _capi.MIXQ_ESHAPE
    wf16, f6 = _capi.X_PACKED | _capi.W_F16X64, _capi.XW_F6X128
    assert lib.mixq_gemm_set_config(-1) == 0
    # NULL operands
    for fn, layout in ((lib.mixq_gemm_i8_fused_bf16, wf16), (lib.mixq_gemm_i4_fused_bf16, f6)):
        a = list(_gemm_args(fake, layout))
        for slot in (0, 1, 2, 3, 13):                       # q_x, q_w, x_scale, scale_col, y
            b = list(a)
            b[slot] = None
            assert fn(*b) == EINVAL
    assert lib.mixq_gemm_i8_fused_amax_bf16(*_amax_args(fake, wf16, None)) == EINVAL        # the side output needs its buffer
    assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, wf16, act=_capi.ACT_SILU_MUL)) == EINVAL       # ... the multiplier its tensor
    assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, 64)) == EINVAL                                  # an unknown layout bit
    assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, f6)) == EINVAL                                  # FP6 codes are the 4-bit form's
    # layouts the bf16 forms do not serve: plain, P16X64 (either operand), nibble-packed int4, the paired gate / up epilogue
    for layout in (0, _capi.X_PACKED, _capi.W_PACKED, _capi.X_PACKED | _capi.W_PACKED):
        assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, layout)) == ESHAPE
        assert lib.mixq_gemm_i4_fused_bf16(*_gemm_args(fake, layout)) == ESHAPE
        assert lib.mixq_gemm_i8_fused_amax_bf16(*_amax_args(fake, layout, fake)) == ESHAPE
        assert lib.mixq_gemm_amax_supported_bf16(64, 64, 128, layout) == 0
    assert lib.mixq_gemm_i4_fused_bf16(*_gemm_args(fake, wf16)) == ESHAPE
    assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, wf16, act=_capi.ACT_SILU_PAIR)) == ESHAPE
    assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, wf16, K=96)) == ESHAPE                           # K % 64
    # coincident faults, the earlier check answers: the paired act is refused before the layout is looked at (and before its addend, which fp16
    # calls a bad argument); the missing multiplier before a bad K
    for layout in (0, _capi.X_PACKED | _capi.W_PACKED, wf16):
        assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, layout, act=_capi.ACT_SILU_PAIR, addend=fake)) == ESHAPE
    assert lib.mixq_gemm_i8_fused(*_gemm_args(fake, wf16, act=_capi.ACT_SILU_PAIR, addend=fake)) == EINVAL
    assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, wf16, K=96, act=_capi.ACT_SILU_MUL)) == EINVAL
    assert lib.mixq_gemm_amax_supported_bf16(8, 64, 128, wf16) == 1                                      # every batch size, small ones included
    assert lib.mixq_gemm_amax_supported_bf16(64, 64, 96, wf16) == 0
    # the one-call forward: NULL block, and a weight layout the bf16 GEMMs do not read - said before the quantise pass is launched
    assert lib.mixq_linear_forward_bf16(None, None) == EINVAL
    for wfmt, qfmt in ((_capi.FMT_PLAIN, _capi.FMT_PLAIN), (_capi.FMT_P16X64, _capi.FMT_P16X64)):
        a = _capi.LinearArgs()
        a.x = a.x_scale = a.q_x = a.q_w = a.scale_col = a.y = 16
        a.ldx, a.ldy, a.M, a.N, a.K, a.bit, a.sigma, a.qfmt, a.wfmt = 128, 64, 64, 64, 128, 8, 6.0, qfmt, wfmt
        assert lib.mixq_linear_forward_bf16(C.byref(a), None) == ESHAPE


def test_a_forced_tiling_without_a_bf16_form_answers_einval():
    lib = _capi.load()
    fake = C.c_void_p(16)
    names = _capi.gemm_config_names()
    wf16, f6 = _capi.X_PACKED | _capi.W_F16X64, _capi.XW_F6X128
    assert set(BF16_INT8) <= set(names) and set(BF16_FP6) <= set(names)
    try:
        for cfg, name in enumerate(names):
            assert lib.mixq_gemm_set_config(cfg) == 0
            # (NULL q_x: a configuration that HAS a bf16 form gets as far as the pointer check and no further - nothing is launched)
            if name not in BF16_INT8:
                assert lib.mixq_gemm_i8_fused_bf16(*_gemm_args(fake, wf16)) == _capi.MIXQ_EINVAL, name
            if name not in BF16_FP6:
                assert lib.mixq_gemm_i4_fused_bf16(*_gemm_args(fake, f6)) == _capi.MIXQ_EINVAL, name
            if name not in BF16_INT8:                           # ... ahead of the M == 0 early-out, where fp16 answers MIXQ_OK
                empty = list(_gemm_args(fake, wf16))
                empty[15] = 0
                assert lib.mixq_gemm_i8_fused_bf16(*empty) == _capi.MIXQ_EINVAL and lib.mixq_gemm_i8_fused(*empty) == 0, name
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0


def test_act_dtype_is_a_config_switch_and_part_of_the_key():
    assert MixqConfig().act_dtype is torch.float16
    assert MixqConfig(act_dtype=torch.bfloat16).act_dtype is torch.bfloat16
    assert MixqConfig().key() != MixqConfig(act_dtype=torch.bfloat16).key()
    assert MixqConfig().copy(act_dtype=torch.bfloat16).key() == MixqConfig(act_dtype=torch.bfloat16).key()
    with pytest.raises(ValueError, match="act_dtype"):
        MixqConfig(act_dtype=torch.float32)


class _Cache:
    """What a layer's constructor reads of a MixLibCache (mixq_amd/cache.py allocates on the device)."""
    def __init__(self, config):
        self.config = config
        self.sigma = torch.tensor([[6.0]], dtype=torch.float16)
        self.stop = 2


def test_what_bfloat16_does_not_serve_is_refused_at_construction():
    from mixq_amd import MixLinear_GEMM
    from mixq_amd.fused import FasterTransformerRMSNorm, MixLlamaMLP
    bf = _Cache(MixqConfig(act_dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="weight_only"):
        MixLinear_GEMM(128, 64, False, "cpu", 8, weight_only=True, cache=bf)
    with pytest.raises(ValueError, match="in_features % 64"):
        MixLinear_GEMM(96, 64, False, "cpu", 8, cache=bf)
    up, gate, down = (MixLinear_GEMM(128, 256, False, "cpu", 8, cache=bf), MixLinear_GEMM(128, 256, False, "cpu", 8, cache=bf),
                      MixLinear_GEMM(256, 128, False, "cpu", 8, cache=bf))
    assert up.act_dtype is torch.bfloat16 and up.scale_col.dtype == torch.float16          # the scales stay float16
    with pytest.raises(NotImplementedError, match="bfloat16"):
        MixLlamaMLP(gate, down, up, bf)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        FasterTransformerRMSNorm(torch.ones(128), cache=bf)
    # ... and the float16 default builds all of them as before
    fp = _Cache(MixqConfig())
    MixLinear_GEMM(128, 64, False, "cpu", 8, weight_only=True, cache=fp)
    l16 = [MixLinear_GEMM(128, 256, False, "cpu", 8, cache=fp), MixLinear_GEMM(256, 128, False, "cpu", 8, cache=fp), MixLinear_GEMM(128, 256, False, "cpu", 8, cache=fp)]
    MixLlamaMLP(*l16, fp)
    FasterTransformerRMSNorm(torch.ones(128), cache=fp)
    assert l16[0].act_dtype is torch.float16


def test_tripwire_tool_checks_the_15_bf16_instantiations():
    """tools/check_wreg_asm.py prints the bf16 kernels' lines with a leading `bf16 ` tag (tests/test_wreg_asm_tripwire.py counts the lines that
    start with `MB=`): nine int8 and six FP6 forms, each with no compiler copy or spill of an in-flight ring register."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_wreg_asm.py"), "gemm_wreg.hip"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("bf16 ")]
    assert len(lines) == 15 and len(set(l.split(":")[0] for l in lines)) == 15, r.stdout[-3000:]
    assert all(l.startswith("bf16 MB=") and "suspicious 0" in l and l.split(":")[0].endswith("ABL=0") for l in lines), lines
    assert sum(" Q=0 " in l for l in lines) == 9 and sum(" Q=3 " in l for l in lines) == 6, lines
    fp16 = [l for l in r.stdout.splitlines() if l.startswith("MB=")]
    assert len([l for l in fp16 if " Q=3 " in l]) == 10                 # the fp16 lines are what they were
