"""The joint gate / up launch in bfloat16 (ABI 1.5), host side (no GPU needed): mixq_gemm_i8_pair_bf16, mixq_gemm_i4_pair_bf16 and
mixq_gemm_pair_supported_bf16 are declared, exported and bound; every refusal of include/mixq_hip.h's list is answered with fake pointers,
before any launch; `MixqConfig.joint_gate_up_bf16` is an opt-in outside key(), and MixLlamaMLP._joint_applies needs all three flags;
mixlib.FusedLinear names the symbol a library without the entry points lacks; the ISA tripwire sees the nine instantiations of
gemm_wreg_bf16_pair.hip.  The `_bf16` entry points keep refusing MIXQ_ACT_SILU_PAIR (tests/test_bf16_gemm_host.py pins that)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from mixq_amd import _capi, mixlib
from mixq_amd.config import MixqConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mixq_gemm_i8_pair_bf16", "mixq_gemm_i4_pair_bf16", "mixq_gemm_pair_supported_bf16")
# the tilings with the paired epilogue's bf16 form, by name (gemm_wreg.hip's g_wr rows 0, 5, 7, 8, 14; 128 x 256 has no FP6 form)
PAIR_INT8 = ["wr128x192_s16_d4_l2", "wr128x256_s16_d3_l2", "wr64x192_s16_d4_l2", "wr64x256_s16_d4_l2", "wr32x64_s8_d6_l1"]
PAIR_FP6 = [n for n in PAIR_INT8 if n != "wr128x256_s16_d3_l2"]
EINVAL, ESHAPE = _capi.MIXQ_EINVAL, _capi.MIXQ_ESHAPE
WF16, F6 = _capi.X_PACKED | _capi.W_F16X64, _capi.XW_F6X128
P16 = _capi.X_PACKED | _capi.W_PACKED


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/mixq_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_three_symbols_are_declared_exported_and_bound():
    lib = _capi.load()
    fused, amax = _header_params("mixq_gemm_i8_fused"), _header_params("mixq_gemm_i8_fused_amax")
    drop = ("const uint16_t* addend", "int lda", "int act")
    # mixq_gemm_i8_fused's list without the addend, its stride and the act; the int8 one ends with mixq_gemm_i8_fused_amax's optional pair
    assert _header_params("mixq_gemm_i8_pair_bf16") == [a for a in amax if a not in drop]
    assert _header_params("mixq_gemm_i4_pair_bf16") == [a.replace("int8_t", "uint8_t") for a in fused if a not in drop]
    assert _header_params("mixq_gemm_pair_supported_bf16") == ["int M", "int N", "int K", "int bit", "int layout"]
    for name in NEW:
        assert name in _capi.header_symbols() and name in _capi.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _capi.SIGNATURES[name] and len(fn.argtypes) == len(_header_params(name))
    assert lib.mixq_version() == 1003                       # the number stays: callers probe for the symbols
    assert "ABI 1.5" in open(_capi.HEADER_PATH).read()
    assert mixlib.PAIR_LAUNCH_BF16 is True


def _i8(fake, layout, M=64, N=128, K=128, ldy=64, row_amax=None, col_mask=None, n_out=0, x_out=None, w_out=None, ld=0, **slots):
    a = dict(q_x=fake, q_w=fake, x_scale=fake, scale_col=fake, y=fake)
    a.update(slots)
    return (a["q_x"], a["q_w"], a["x_scale"], a["scale_col"], x_out, ld, w_out, ld, n_out, None, None, a["y"], ldy, M, N, K, layout, row_amax, col_mask, None)


def _i4(fake, layout, **kw):
    a = _i8(fake, layout, **kw)
    return a[:17] + (None,)


def test_refusals_in_the_documented_order_before_any_launch():
    lib = _capi.load()
    fake, p8 = C.c_void_p(4096), C.c_void_p(4096 + 8)       # never dereferenced: every call below ends in its argument checks (or at M == 0)
    i8, i4 = lib.mixq_gemm_i8_pair_bf16, lib.mixq_gemm_i4_pair_bf16
    assert lib.mixq_gemm_set_config(-1) == 0
    # MIXQ_EINVAL: NULL operands
    for fn, args, layout in ((i8, _i8, WF16), (i4, _i4, F6)):
        for slot in ("q_x", "q_w", "x_scale", "scale_col", "y"):
            assert fn(*args(fake, layout, **{slot: None})) == EINVAL, slot
    # ... unknown layout bits, FP6 codes at the int8 entry, row_amax beside a layout without the side output
    assert i8(*_i8(fake, 64)) == EINVAL and i4(*_i4(fake, 64)) == EINVAL
    assert i8(*_i8(fake, F6)) == EINVAL
    for layout in (0, _capi.X_PACKED, _capi.W_PACKED, P16, F6):
        assert i8(*_i8(fake, layout, row_amax=fake)) == EINVAL, layout
    # ... sizes
    assert i8(*_i8(fake, WF16, M=-1)) == EINVAL and i8(*_i8(fake, WF16, K=0)) == EINVAL and i8(*_i8(fake, WF16, n_out=-1)) == EINVAL
    # MIXQ_ESHAPE: layouts the form does not serve (plain, P16X64 on either side, nibble-packed int4, the other width's layout)
    for layout in (0, _capi.X_PACKED, _capi.W_PACKED, P16):
        assert i8(*_i8(fake, layout)) == ESHAPE and i4(*_i4(fake, layout)) == ESHAPE, layout
    assert i4(*_i4(fake, WF16)) == ESHAPE
    # ... K and N the form does not serve, ldy, the outlier strides
    assert i8(*_i8(fake, WF16, K=96)) == ESHAPE and i4(*_i4(fake, F6, K=192)) == ESHAPE and i4(*_i4(fake, F6, K=64)) == ESHAPE
    assert i8(*_i8(fake, WF16, N=136)) == ESHAPE and i4(*_i4(fake, F6, N=136)) == ESHAPE              # N % 16 (interleaved rows)
    assert i8(*_i8(fake, WF16, ldy=60)) == ESHAPE and i8(*_i8(fake, WF16, ldy=66)) == ESHAPE          # ldy < N / 2, ldy % 4
    assert i8(*_i8(fake, WF16, n_out=3, x_out=fake, w_out=fake, ld=8)) == ESHAPE                     # below the padded width of 16
    # coincident faults, the earlier check answers: a NULL operand before a bad K; a bad K before a misaligned y
    assert i8(*_i8(fake, WF16, K=96, q_x=None)) == EINVAL
    assert i8(*_i8(fake, WF16, K=96, y=C.c_void_p(4100))) == ESHAPE
    # MIXQ_EINVAL: pointer alignment (y 8 bytes, x_out / w_out 16 bytes)
    assert i8(*_i8(fake, WF16, y=C.c_void_p(4100))) == EINVAL
    assert i8(*_i8(fake, WF16, n_out=3, x_out=p8, w_out=fake, ld=16)) == EINVAL
    # M == 0: every check still runs, nothing is launched, null operands are fine
    assert i8(*_i8(fake, WF16, M=0)) == 0 and i8(*_i8(fake, WF16, M=0, row_amax=fake, col_mask=fake)) == 0
    assert i8(*_i8(fake, WF16, M=0, q_x=None, q_w=None, y=None)) == 0
    assert i4(*_i4(fake, F6, M=0)) == 0
    assert i8(*_i8(fake, WF16, M=0, K=96)) == ESHAPE and i8(*_i8(fake, P16, M=0)) == ESHAPE


def test_a_forced_tiling_without_a_paired_bf16_form_answers_einval():
    lib = _capi.load()
    fake = C.c_void_p(4096)
    names = _capi.gemm_config_names()
    assert set(PAIR_INT8) <= set(names)
    try:
        for cfg, name in enumerate(names):
            assert lib.mixq_gemm_set_config(cfg) == 0
            # (the empty problem: a configuration that HAS the form answers MIXQ_OK without a launch, any other is refused ahead of M == 0)
            assert lib.mixq_gemm_i8_pair_bf16(*_i8(fake, WF16, M=0)) == (0 if name in PAIR_INT8 else EINVAL), name
            assert lib.mixq_gemm_i4_pair_bf16(*_i4(fake, F6, M=0)) == (0 if name in PAIR_FP6 else EINVAL), name
            if name not in PAIR_INT8:
                assert lib.mixq_gemm_i8_pair_bf16(*_i8(fake, WF16)) == EINVAL, name
            assert lib.mixq_gemm_i8_pair_bf16(*_i8(fake, WF16, M=0, K=96)) == ESHAPE                  # (the shape checks still come first)
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0


def test_pair_supported_query():
    q = _capi.load().mixq_gemm_pair_supported_bf16
    assert q(64, 128, 128, 8, WF16) == 1                    # 64 x 128 -> 2 x 64, the int8 layout
    assert q(64, 128, 128, 4, F6) == 1 and q(8, 128, 128, 8, WF16) == 1 and q(512, 22016, 4096, 8, WF16) == 1
    assert q(64, 128, 96, 8, WF16) == 0                     # K % 64
    assert q(64, 128, 128, 8, P16) == 0                     # a P16X64 layout
    assert q(64, 128, 128, 8, 0) == 0 and q(64, 128, 128, 8, F6) == 0 and q(64, 128, 128, 4, WF16) == 0 and q(64, 128, 192, 4, F6) == 0
    assert q(64, 136, 128, 8, WF16) == 0 and q(0, 128, 128, 8, WF16) == 0 and q(64, 128, 128, 5, WF16) == 0


def test_the_bf16_entry_points_still_refuse_the_paired_act():
    lib = _capi.load()
    fake = C.c_void_p(16)
    args = (fake, fake, fake, fake, None, 0, None, 0, 0, None, None, 0, None, fake, 64, 64, 64, 128, _capi.ACT_SILU_PAIR, WF16, None)
    assert lib.mixq_gemm_i8_fused_bf16(*args) == ESHAPE
    assert lib.mixq_gemm_i4_fused_bf16(*(args[:19] + (F6, None))) == ESHAPE


def test_joint_gate_up_bf16_is_an_opt_in_outside_the_key():
    assert MixqConfig().joint_gate_up_bf16 is False
    on = MixqConfig(act_dtype=torch.bfloat16, fused_bf16=True, joint_gate_up_bf16=True)
    assert on.joint_gate_up_bf16 is True and on.joint_gate_up is True
    assert on.key() == MixqConfig(act_dtype=torch.bfloat16).key()                     # not part of a plan's / joint image's identity
    assert MixqConfig(joint_gate_up_bf16=True).key() == MixqConfig().key()
    assert on.copy(joint_gate_up_bf16=False).joint_gate_up_bf16 is False


class _Cache:
    """What the modules read of a MixLibCache on the host (as tests/test_bf16_norm_host.py)."""
    def __init__(self, config):
        self.config = config
        self.sigma = torch.tensor([[6.0]], dtype=torch.float16)
        self.stop = 2
        self.q_xcache = mixlib.set_fmt(torch.zeros(16, 128, dtype=torch.int8), _capi.FMT_P16X64)


def _frozen_block(config):
    from mixq_amd import MixLinear_GEMM
    from mixq_amd.fused import MixLlamaMLP
    cache = _Cache(config)
    up, gate, down = (MixLinear_GEMM(128, 256, False, "cpu", 8, cache=cache), MixLinear_GEMM(128, 256, False, "cpu", 8, cache=cache),
                      MixLinear_GEMM(256, 128, False, "cpu", 8, cache=cache))
    up.add_outliers = gate.add_outliers = False             # both predictions frozen, no outlier columns
    return MixLlamaMLP(gate, down, up, cache), cache


def test_joint_applies_needs_all_three_flags_and_frozen_layers():
    bf = torch.bfloat16
    mlp, cache = _frozen_block(MixqConfig(act_dtype=bf, fused_bf16=True, joint_gate_up_bf16=True))
    assert mlp._joint_applies(cache) is True
    mlp.up_proj_.add_outliers = True                        # up_proj's search still running
    assert mlp._joint_applies(cache) is False
    mlp.up_proj_.add_outliers = False
    for off in ("joint_gate_up_bf16", "joint_gate_up", "fused_bf16"):
        setattr(mlp.config, off, False)
        assert mlp._joint_applies(cache) is False, off
        setattr(mlp.config, off, True)
    assert mlp._joint_applies(cache) is True
    # the default flags of a bf16 block (pinned: tests/test_bf16_norm_host.py) and the fp16 block, which never needed the switch
    mlp, cache = _frozen_block(MixqConfig(act_dtype=bf, fused_bf16=True))
    assert mlp._joint_applies(cache) is False
    mlp, cache = _frozen_block(MixqConfig())
    assert mlp._joint_applies(cache) is True
    mlp, cache = _frozen_block(MixqConfig(joint_gate_up_bf16=True, joint_gate_up=False))
    assert mlp._joint_applies(cache) is False


def test_fused_linear_names_the_symbol_a_library_lacks(monkeypatch):
    class Old:
        """A library of an earlier ABI minor: everything but the ABI 1.5 entry points."""
        def __getattr__(self, name):
            if name in NEW:
                raise AttributeError(name)
            return getattr(_capi.load(), name)
    old = Old()
    monkeypatch.setattr(mixlib._capi, "load", lambda: old)
    with pytest.raises(RuntimeError, match="mixq_gemm_i8_pair_bf16"):
        mixlib._pair_bf16_entry("mixq_gemm_i8_pair_bf16")
    with pytest.raises(RuntimeError, match="mixq_gemm_i4_pair_bf16"):
        mixlib._pair_bf16_entry("mixq_gemm_i4_pair_bf16")


def test_tripwire_tool_checks_the_nine_paired_bf16_instantiations():
    """tools/check_wreg_asm.py gemm_wreg_bf16_pair.hip: five int8 and four FP6 forms, all ABL=90, none with a compiler copy or spill of an
    in-flight ring register - and only these: the unit is listed under its own file name alone."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_wreg_asm.py"), "gemm_wreg_bf16_pair.hip"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    lines = [l for l in r.stdout.splitlines() if "MB=" in l]
    assert len(lines) == 9 and len(set(l.split(":")[0] for l in lines)) == 9, r.stdout[-3000:]
    assert all(l.startswith("bf16 MB=") and l.split(":")[0].endswith("ABL=90") and "suspicious 0" in l for l in lines), lines
    assert sum(" Q=0 " in l for l in lines) == 5 and sum(" Q=3 " in l for l in lines) == 4, lines
    assert not any("scratch" in l for l in lines), lines                                # (no scratch access inside the counted region)
