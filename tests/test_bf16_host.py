"""bfloat16 activations at the quantise edge, host side: the `_bf16` twins are declared, exported and bound with their fp16 twins'
argument lists, the ABI version says so, the dispatch of mixlib picks them by dtype, and they reject bad arguments before touching a
device (no GPU needed)."""
import ctypes as C
import re

import pytest
import torch

from mixq_amd import _capi, mixlib

TWINS = ["mixq_find_row_scale", "mixq_extract_outliers_zero", "mixq_quant_fused", "mixq_quant_fused_masked", "mixq_detect_outlier_cols",
         "mixq_quant_known_amax", "mixq_selftest_quant_exact"]


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/mixq_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", TWINS)
def test_bf16_twin_is_declared_with_the_fp16_argument_list(name):
    assert _header_params(name + "_bf16") == _header_params(name)


@pytest.mark.parametrize("name", TWINS)
def test_bf16_twin_is_exported_and_bound(name):
    lib = _capi.load()
    assert _capi.SIGNATURES[name + "_bf16"] == _capi.SIGNATURES[name]
    fn = getattr(lib, name + "_bf16")
    assert fn.argtypes == _capi.SIGNATURES[name]


def test_abi_version_is_bumped_for_the_new_entry_points():
    assert _capi.load().mixq_version() >= 1001


def test_bf16_entry_points_reject_bad_arguments_before_the_device():
    lib = _capi.load()
    fake = C.c_void_p(16)                                   # never dereferenced: every call below fails its argument checks first
    EINVAL, ESHAPE = _capi.MIXQ_EINVAL, _capi.MIXQ_ESHAPE
    assert lib.mixq_selftest_quant_exact_bf16(None, 8, None) == EINVAL
    assert lib.mixq_selftest_quant_exact_bf16(fake, 5, None) == EINVAL
    # bad bit, bad format, null pointers, shapes
    assert lib.mixq_find_row_scale_bf16(fake, fake, fake, 4, 64, 64, 5, 0, None) == EINVAL
    assert lib.mixq_find_row_scale_bf16(fake, fake, fake, 4, 128, 128, 8, 7, None) == EINVAL
    assert lib.mixq_find_row_scale_bf16(fake, fake, fake, 4, 128, 128, 8, _capi.FMT_F6X128, None) == EINVAL   # FP6 codes: 4-bit only
    assert lib.mixq_find_row_scale_bf16(None, fake, fake, 4, 64, 64, 8, 0, None) == EINVAL
    assert lib.mixq_find_row_scale_bf16(fake, fake, fake, 4, 60, 64, 8, 0, None) == ESHAPE
    for fn in (lib.mixq_quant_fused_bf16,):
        assert fn(fake, fake, 2, None, fake, fake, fake, None, 4, 64, 64, 16, 3, 6.0, 0, None) == EINVAL
        assert fn(fake, None, 2, None, fake, fake, fake, None, 4, 64, 64, 16, 8, 6.0, 0, None) == EINVAL     # n > 0 without ind
        assert fn(None, fake, 0, None, fake, fake, None, None, 4, 64, 64, 0, 8, 6.0, 0, None) == EINVAL
    # the masked form needs a kept map in this library's layout when it has columns
    assert lib.mixq_quant_fused_masked_bf16(fake, fake, 2, None, None, 0, fake, fake, fake, None, 4, 64, 64, 16, 8, 6.0, 0, None) == EINVAL
    assert lib.mixq_quant_known_amax_bf16(fake, fake, 0, None, None, None, 0, fake, fake, None, None, 4, 64, 64, 0, 8, 6.0, 0, None) == EINVAL
    assert lib.mixq_quant_known_amax_bf16(fake, fake, 0, None, fake, None, 0, fake, fake, None, None, 4, 64, 64, 0, 4, 6.0, 9, None) == EINVAL
    assert lib.mixq_detect_outlier_cols_bf16(None, 6.0, fake, fake, fake, 4, 64, 64, None) == EINVAL
    assert lib.mixq_detect_outlier_cols_bf16(fake, 6.0, fake, fake, fake, 4, 60, 64, None) == ESHAPE
    assert lib.mixq_extract_outliers_zero_bf16(fake, None, 2, fake, 4, 64, 64, 16, None) == EINVAL


def test_bf16_has_no_forced_test_geometry_below_5():
    """bf16 quantise passes exist for the geometries the automatic choice returns (5 .. 9); a forced test geometry 0 .. 4 answers
    MIXQ_EINVAL before any launch."""
    lib = _capi.load()
    fake = C.c_void_p(16)
    try:
        for cfg in range(5):
            assert lib.mixq_quant_set_config(cfg) == 0
            assert lib.mixq_quant_fused_bf16(fake, None, 0, None, fake, fake, None, None, 4, 64, 64, 0, 8, 6.0, 0, None) == _capi.MIXQ_EINVAL
            assert lib.mixq_find_row_scale_bf16(fake, fake, fake, 4, 64, 64, 8, 0, None) == _capi.MIXQ_EINVAL
    finally:
        assert lib.mixq_quant_set_config(-1) == 0


def test_mixlib_picks_the_entry_point_by_dtype():
    assert mixlib._act_suffix(torch.empty(2, 8, dtype=torch.float16), "t") == ""
    assert mixlib._act_suffix(torch.empty(2, 8, dtype=torch.bfloat16), "t") == "_bf16"
    for dt in (torch.float32, torch.int16):
        with pytest.raises(RuntimeError, match="float16 or bfloat16"):
            mixlib._act_suffix(torch.empty(2, 8, dtype=dt), "t")
