"""bfloat16 weight-only W8A16 layers, host side (no GPU needed): the three entry points of ABI 1.6 are declared, exported and bound with
their fp16 twins' argument lists, answer bad arguments and a forced configuration without a bf16 form before any launch,
`MixqConfig.w8a16_bf16` opens the constructor, `from_linear` quantises a bf16 Linear from its fp32 image, the GPT-J policy builds fc_out
under the flag, the float64 restatement the GPU tests compare against rounds ties to even, and the ISA tripwire sees the 18 new kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact as E  # noqa: E402
import w8a16_bf16_ref as R  # noqa: E402
from exact import BF16  # noqa: E402
from mixq_amd import MixLibCache, MixLinear_GEMM, _capi  # noqa: E402
from mixq_amd import checkpoint as ck  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = ["mixq_pack_w8a16", "mixq_gemm_w8a16", "mixq_gemm_w8a16_addend"]
PRODUCT_TILINGS = ["w8a16_128x192_s8_d3_l2", "w8a16_128x128_s8_d4_l2", "w8a16_64x128_s12_d4_l2", "w8a16_64x256_s12_d3_l2", "w8a16_64x192_s12_d4_l2",
                   "w8a16_64x64_s8_d4_l1", "w8a16_128x192_s8_d4_l2", "w8a16_128x192_s6_d3_l1", "w8a16_32x64_s8_d5_l1"]


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/mixq_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", TWINS)
def test_bf16_w8a16_twin_is_declared_exported_and_bound(name):
    assert _header_params(name + "_bf16") == _header_params(name)
    assert _capi.SIGNATURES[name + "_bf16"] == _capi.SIGNATURES[name]
    assert name + "_bf16" in _capi.header_symbols()
    fn = getattr(_capi.load(), name + "_bf16")
    assert fn.argtypes == _capi.SIGNATURES[name]


def test_abi_version_stays_1003_callers_probe_for_the_symbols():
    lib = _capi.load()
    assert lib.mixq_version() == 1003
    assert all(hasattr(lib, n + "_bf16") for n in TWINS)


def test_bf16_w8a16_entry_points_answer_bad_arguments_before_any_launch():
    """The refusals of tests/test_capi_symbols.py:92-101, entry point by entry point, the fp16 twin beside it."""
    lib = _capi.load()
    one = C.c_void_p(16)                                      # a non-null dummy pointer; never dereferenced on these paths
    EINVAL, ESHAPE = _capi.MIXQ_EINVAL, _capi.MIXQ_ESHAPE
    assert lib.mixq_gemm_w8a16_set_config(-1) == 0
    for pack in (lib.mixq_pack_w8a16_bf16, lib.mixq_pack_w8a16):
        assert pack(one, one, 100, 64, None) == ESHAPE                                            # K % 64
        assert pack(None, one, 64, 64, None) == EINVAL
        assert pack(one, None, 64, 64, None) == EINVAL
        assert pack(one, one, 0, 64, None) == EINVAL and pack(one, one, 64, 0, None) == EINVAL
    for gemm in (lib.mixq_gemm_w8a16_bf16, lib.mixq_gemm_w8a16):
        assert gemm(one, 128, one, one, None, one, 64, 4, 64, 100, None) == ESHAPE                # K % 64
        assert gemm(one, 128, one, one, None, one, 64, 4, 62, 128, None) == ESHAPE                # N % 4
        assert gemm(one, 100, one, one, None, one, 64, 4, 64, 128, None) == ESHAPE                # ldx < K
        assert gemm(one, 132, one, one, None, one, 64, 4, 64, 128, None) == ESHAPE                # ldx % 8
        assert gemm(one, 128, one, one, None, one, 60, 4, 64, 128, None) == ESHAPE                # ldy < N
        assert gemm(one, 128, one, one, None, one, 66, 4, 64, 128, None) == ESHAPE                # ldy % 4
        assert gemm(C.c_void_p(8), 128, one, one, None, one, 64, 4, 64, 128, None) == EINVAL      # x alignment
        assert gemm(one, 128, one, one, None, C.c_void_p(20), 64, 4, 64, 128, None) == EINVAL     # y alignment (8 bytes)
        for slot in (0, 2, 3, 5):                                                                 # x, w_packed, scale_col, y
            a = [one, 128, one, one, None, one, 64, 4, 64, 128, None]
            a[slot] = None
            assert gemm(*a) == EINVAL
        assert gemm(one, 128, one, one, None, one, 64, -1, 64, 128, None) == EINVAL
        assert gemm(one, 128, one, one, None, one, 64, 0, 64, 128, None) == 0                     # M = 0
        assert gemm(one, 100, one, one, None, one, 64, 0, 64, 128, None) == ESHAPE                # ... runs every check
    for gemm in (lib.mixq_gemm_w8a16_addend_bf16, lib.mixq_gemm_w8a16_addend):
        assert gemm(one, 128, one, one, one, 64, None, one, 64, 0, 64, 128, None) == 0
        assert gemm(one, 128, one, one, None, 0, None, one, 64, 0, 64, 128, None) == 0            # no addend: lda is not looked at
        assert gemm(one, 128, one, one, one, 60, None, one, 64, 0, 64, 128, None) == ESHAPE       # lda < N
        assert gemm(one, 128, one, one, one, 66, None, one, 64, 0, 64, 128, None) == ESHAPE       # lda % 4
        assert gemm(one, 128, one, one, C.c_void_p(20), 64, None, one, 64, 4, 64, 128, None) == EINVAL   # addend alignment (8 bytes)
        assert gemm(one, 128, one, one, one, 64, None, one, 64, 4, 64, 100, None) == ESHAPE       # K % 64
        assert gemm(one, 128, one, one, C.c_void_p(20), 60, None, one, 64, 4, 64, 128, None) == ESHAPE   # strides are answered before pointers


def test_a_forced_decode32_answers_einval_from_the_bf16_entry_points():
    """The in-workgroup K-split kernel has no bf16 form: MIXQ_EINVAL before anything is launched, ahead of the M == 0 early-out (where fp16
    answers MIXQ_OK); every product tiling has one and gets as far as the empty problem's MIXQ_OK."""
    lib = _capi.load()
    one = C.c_void_p(16)
    names = _capi.w8a16_config_names()
    assert names[:9] == PRODUCT_TILINGS and names[-1] == "w8a16_decode32"
    try:
        assert lib.mixq_gemm_w8a16_set_config(names.index("w8a16_decode32")) == 0
        for M in (0, 4, 64):
            assert lib.mixq_gemm_w8a16_bf16(one, 128, one, one, None, one, 64, M, 64, 128, None) == _capi.MIXQ_EINVAL
            assert lib.mixq_gemm_w8a16_addend_bf16(one, 128, one, one, one, 64, None, one, 64, M, 64, 128, None) == _capi.MIXQ_EINVAL
        assert lib.mixq_gemm_w8a16(one, 128, one, one, None, one, 64, 0, 64, 128, None) == 0
        # the shape checks still come first
        assert lib.mixq_gemm_w8a16_bf16(one, 128, one, one, None, one, 64, 0, 64, 100, None) == _capi.MIXQ_ESHAPE
        for c in range(9):
            assert lib.mixq_gemm_w8a16_set_config(c) == 0
            assert lib.mixq_gemm_w8a16_bf16(one, 128, one, one, None, one, 64, 0, 64, 128, None) == 0, names[c]
            assert lib.mixq_gemm_w8a16_addend_bf16(one, 128, one, one, one, 64, None, one, 64, 0, 64, 128, None) == 0, names[c]
    finally:
        assert lib.mixq_gemm_w8a16_set_config(-1) == 0


def test_w8a16_bf16_is_an_opt_in_switch_outside_the_key():
    assert MixqConfig().w8a16_bf16 is False
    assert MixqConfig(act_dtype=torch.bfloat16).w8a16_bf16 is False
    on = MixqConfig(act_dtype=torch.bfloat16, w8a16_bf16=True)
    assert on.w8a16_bf16 is True and on.key() == MixqConfig(act_dtype=torch.bfloat16).key()
    assert MixqConfig(w8a16_bf16=True).key() == MixqConfig().key()
    assert on.copy(w8a16_bf16=False).w8a16_bf16 is False


class _Cache:
    """What a layer's constructor reads of a MixLibCache."""
    def __init__(self, config):
        self.config = config
        self.sigma = torch.tensor([[6.0]], dtype=torch.float16)
        self.stop = 2


def test_the_flag_opens_the_constructor_and_the_refusal_names_it():
    with pytest.raises(ValueError, match="weight_only") as ei:
        MixLinear_GEMM(128, 64, False, "cpu", 8, weight_only=True, cache=_Cache(MixqConfig(act_dtype=torch.bfloat16)))
    assert "w8a16_bf16" in str(ei.value)
    layer = MixLinear_GEMM(128, 64, True, "cpu", 8, weight_only=True, cache=_Cache(MixqConfig(act_dtype=torch.bfloat16, w8a16_bf16=True)))
    assert layer.weight_only and layer.act_dtype is torch.bfloat16
    assert layer.q_weight.shape == (128, 64) and layer.q_weight.dtype == torch.int8          # the buffers are the fp16 layer's
    assert layer.scale_col.dtype == torch.float16 and layer.bias.dtype == torch.float16
    # without act_dtype=bfloat16 the switch does nothing
    l16 = MixLinear_GEMM(128, 64, True, "cpu", 8, weight_only=True, cache=_Cache(MixqConfig(w8a16_bf16=True)))
    assert l16.act_dtype is torch.float16


def test_from_linear_quantises_a_bf16_linear_from_its_fp32_image():
    """scale_col = fp16(colabsmax / 128) with the quotient in fp32 - ONE rounding - and q from the same fp32 quotient.  Columns: full-range
    values, a column whose scale is an fp16 subnormal that the rounding moves (colabsmax = 1.9921875 * 2^-12: scale 255 * 2^-26 = 63.75 subnormal
    quanta of 2^-24 -> 64), an all-zero column.
    (colabsmax of bf16 weights is a bf16 value and / 128 a power of two, so the fp32 quotient is itself a bf16 value: going through bfloat16
    on the way to float16, as `quant_weights(...)[1].half()` does, happens to give the same scale for every bf16 weight.  The layer no longer
    depends on that coincidence; this test pins the contract, the one-rounding value.)"""
    torch.manual_seed(5)
    K, N = 128, 8
    lin = nn.Linear(K, N, bias=True).bfloat16()
    with torch.no_grad():
        lin.weight[1].mul_(2.0 ** -12)
        lin.weight[1, 7] = 1.9921875 * 2.0 ** -12
        lin.weight[1].clamp_(-1.9921875 * 2.0 ** -12, 1.9921875 * 2.0 ** -12)
        lin.weight[2].zero_()
        lin.weight[3, 5] = -3.0
    cache = MixLibCache(16, device="cpu", config=MixqConfig(act_dtype=torch.bfloat16, w8a16_bf16=True))
    layer = MixLinear_GEMM.from_linear(lin, 8, weight_only=True, cache=cache, dev="cpu", name="fc_out")
    w32 = lin.weight.data.float().t().contiguous()                       # [K, N], every value exact
    scale32 = w32.abs().amax(dim=0) * np.float32(1.0 / 128.0)
    assert scale32.dtype == torch.float32
    want = scale32.to(torch.float16)
    assert torch.equal(layer.scale_col, want)
    assert float(want[1]) == 64 * 2.0 ** -24 and float(scale32[1]) == 255 * 2.0 ** -26 and float(want[2]) == 0.0
    qd = torch.where(scale32 > 0, w32 / scale32, torch.zeros_like(w32))
    qd = (torch.sign(qd) * torch.floor(qd.abs() + 0.5)).clamp(-128, 127).to(torch.int8)
    assert torch.equal(layer.q_weight, qd)
    assert int(layer.q_weight[5, 3]) == -128 and int(layer.q_weight.max()) == 127 and not layer.q_weight[:, 2].any()
    assert torch.equal(layer.bias, lin.bias.data.half())
    # an fp16 Linear takes the path it always took
    lin16 = nn.Linear(K, N, bias=False).half()
    from mixq_amd import eetq
    q16, s16 = eetq.quant_weights(lin16.weight.data.t().contiguous(), torch.int8, False)
    l16 = MixLinear_GEMM.from_linear(lin16, 8, weight_only=True, cache=MixLibCache(16, device="cpu"), dev="cpu")
    assert torch.equal(l16.q_weight, q16) and torch.equal(l16.scale_col, s16.half())


class GptjMlp(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc_in, self.fc_out = nn.Linear(128, 256), nn.Linear(256, 128)


def test_gptj_policy_builds_fc_out_in_bfloat16_under_the_flag(tmp_path):
    assert ck.layer_policy("mlp.fc_out", 8, "GPTJForCausalLM") == (8, True)
    torch.manual_seed(2)
    m = GptjMlp().bfloat16()
    with pytest.raises(ValueError, match="weight_only"):
        ck.quantize_(GptjMlp().bfloat16(), 8, MixLibCache(64, device="cpu", config=MixqConfig(act_dtype=torch.bfloat16)), arch="GPTJForCausalLM")
    cfg = MixqConfig(act_dtype=torch.bfloat16, w8a16_bf16=True)
    done = ck.quantize_(m, 8, MixLibCache(64, device="cpu", config=cfg), arch="GPTJForCausalLM")
    assert done == {"fc_in": (8, False), "fc_out": (8, True)}
    assert m.fc_out.weight_only and m.fc_out.act_dtype is torch.bfloat16 and m.fc_out.q_weight.shape == (256, 128)
    ck.save_quantized(m, str(tmp_path), {"w_bit": 8})
    fresh = GptjMlp().bfloat16()
    ck.load_quantized(fresh, str(tmp_path), MixLibCache(64, device="cpu", config=cfg), arch="GPTJForCausalLM")
    assert fresh.fc_out.weight_only and fresh.fc_out.act_dtype is torch.bfloat16 and not fresh.fc_in.weight_only
    sd, sd2 = m.state_dict(), fresh.state_dict()
    assert sd.keys() == sd2.keys()
    for k, v in sd.items():
        assert torch.equal(v, sd2[k]) and v.dtype == sd2[k].dtype, k
    assert sd["fc_out.q_weight"].dtype == torch.int8 and sd["fc_out.scale_col"].dtype == torch.float16      # the checkpoint is the fp16 layer's
    with pytest.raises(ValueError, match="weight_only"):                                                     # ... and the default still refuses on load
        ck.load_quantized(GptjMlp().bfloat16(), str(tmp_path), MixLibCache(64, device="cpu", config=MixqConfig(act_dtype=torch.bfloat16)),
                          arch="GPTJForCausalLM")


def test_reference_rounds_to_nearest_even_on_hand_picked_ties():
    """bf16 keeps 8 significand bits: at 1.0 the spacing is 2^-7.  Ties go to the even neighbour, in both directions and for both signs;
    the largest finite value 2^128 - 2^120 survives, the tie 2^128 - 2^119 above it becomes inf; the smallest subnormal's half flushes to 0."""
    u = 2.0 ** -7
    cases = [(1.0 + u / 2, 0x3F80), (1.0 + 3 * u / 2, 0x3F82), (1.0 + 5 * u / 2, 0x3F82), (-(1.0 + u / 2), 0xBF80), (-(1.0 + 3 * u / 2), 0xBF82),
             (1.0 + u / 2 + 2.0 ** -23, 0x3F81), (1.0 + u / 2 - 2.0 ** -23, 0x3F80), (255.0, 0x437F), (255.5, 0x4380), (256.5, 0x4380), (257.0, 0x4380),
             (259.0, 0x4382), (2.0 ** 128 - 2.0 ** 120, 0x7F7F), (2.0 ** 128 - 2.0 ** 119, 0x7F80), (-(2.0 ** 128 - 2.0 ** 119), 0xFF80),
             (2.0 ** 128 - 2.0 ** 119 - 2.0 ** 104, 0x7F7F), (2.0 ** -134, 0x0000), (3 * 2.0 ** -134, 0x0002), (0.0, 0x0000)]
    z = np.array([[c[0] for c in cases]], dtype=np.float64)
    want = np.array([[c[1] for c in cases]], dtype=np.uint16)
    got = R.expect_bits(z)
    assert np.array_equal(got, want), [(c[0], hex(int(g))) for c, g in zip(cases, got[0]) if g != c[1]]
    # z64: the weights are the integers they are (-128 included), the addend first, then the bias; bf16 x far above fp16's range
    xbits = E.to_bits(np.array([[1.0, 2.0 ** 20, -0.5, 0.0]]), BF16)
    qkn = np.array([[-128, 1], [1, 0], [127, -1], [5, 5]], dtype=np.int8)
    scale = np.array([0.5, 2.0], dtype=np.float16)
    add = E.to_bits(np.array([[3.0, -1.0]]), BF16)
    bias = np.array([0.25, 0.125], dtype=np.float16)
    z = R.z64(xbits, qkn, scale, add, bias)
    assert z[0, 0] == (-128.0 + 2.0 ** 20 - 63.5) * 0.5 + 3.0 + 0.25 and z[0, 1] == (1.0 + 0.5) * 2.0 - 1.0 + 0.125
    assert np.array_equal(R.z64(xbits, qkn, scale), (R.bf16_values(xbits) @ qkn.astype(np.float64)) * np.array([0.5, 2.0]))
    assert R.ulp_bf16(1.0) == 2.0 ** -7 and R.ulp_bf16(255.0) == 1.0 and R.ulp_bf16(0.0) == 2.0 ** -133
    b = R.bound(xbits, qkn, scale, add, bias)
    assert b.shape == (1, 2) and (b >= 0.5 * R.ulp_bf16(z)).all() and b[0, 1] < 2.0 ** -6


def test_exact_w8a16_operands_meet_the_conditions_in_bfloat16():
    """The GPU test's operands: x of E.w8a16_problem re-encoded as bf16 (i 2^-6, |i| <= 64: representable) and a bf16 addend on the
    quantum 2^-12; every z / q an integer, the sum of absolute terms below 2^22 q; ties and round-away shares say the rounding is exercised."""
    for M in E.M_SHAPES:
        for N in E.N_SHAPES:
            x, qkn, scale, bias, z, q = E.w8a16_problem(M, E.K_MAIN, N)
            assert E.representable(x.astype(np.float64), BF16)
            rng = np.random.default_rng(2000 + M + N)
            add = E._fit(rng.integers(-2000, 2001, (M, N)), BF16) * 2.0 ** -12
            assert E.representable(add, BF16)
            za = z + add
            assert np.array_equal(za / q, np.rint(za / q))
            worst = float(((np.abs(x.astype(np.float64)).sum(axis=1)[:, None] * 128.0 * scale.astype(np.float64)[None, :]
                            + np.abs(bias.astype(np.float64))[None, :] + np.abs(add)) / q).max())
            assert worst < E.LIMIT
            assert np.array_equal(R.z64(E.to_bits(x.astype(np.float64), BF16), qkn, scale, E.to_bits(add, BF16), bias), za)
            sh = E.shares(R.expect_bits(za), za, BF16)
            assert sh["tie"] > 0.005 and 0.3 < sh["away"] < 0.7 and sh["inf"] == 0.0, sh


def test_tripwire_tool_checks_the_18_bf16_w8a16_kernels():
    """tools/check_wreg_asm.py gemm_w8a16_bf16.hip: nine tilings x (plain, addend), lines tagged `bf16 `, none with a compiler copy or spill
    of an in-flight weight-ring register, no scratch access inside the counted region - and only these under that name."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_wreg_asm.py"), "gemm_w8a16_bf16.hip"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    lines = [l for l in r.stdout.splitlines() if "MB=" in l]
    assert len(lines) == 18 and len(set(l.split(":")[0] for l in lines)) == 18, r.stdout[-3000:]
    assert all(l.startswith("bf16 w8a16 MB=") and "suspicious 0" in l and " ABL=0 " in l for l in lines), lines
    assert all(re.search(r"ring registers [1-9]", l) for l in lines), lines              # (the check found the ring it is about)
    assert sum(l.split(":")[0].endswith("ADD=1") for l in lines) == 9
    assert not any("scratch" in l for l in lines), lines
    assert not any(l.startswith("MB=") for l in r.stdout.splitlines())                  # the gemm_wreg.hip listing is untouched
