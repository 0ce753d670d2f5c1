"""The C-ABI shared library loads (no GPU needed) and exports every symbol include/mixq_hip.h declares; the ctypes
signature table mirrors the header; argument validation is exercised where it needs no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mixq_amd import _capi


def test_library_is_built_in_tree():
    assert os.path.exists(_capi.LIB_PATH), "run __graft_entry__.build() first"
    assert os.path.dirname(_capi.LIB_PATH).endswith("mixq_amd")


def test_every_header_symbol_is_exported_and_bound():
    lib = _capi.load()
    declared = _capi.header_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mixq_hip.h but not exported"
    assert set(declared) == set(_capi.SIGNATURES) - set(_capi.TUNING_ONLY), "ctypes table and header disagree"
    assert set(_capi.header_symbols(tuning=True)) == set(_capi.SIGNATURES)       # ... and with the tuning library's section


def test_header_arity_matches_ctypes_table():
    txt = open(_capi.HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for m in re.finditer(r"\b(?:int|long long)\s+(mixq_\w+)\s*\(([^)]*)\)\s*;", txt):
        name, args = m.group(1), m.group(2).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert n == len(_capi.SIGNATURES[name]), f"{name}: header has {n} parameters, ctypes table {len(_capi.SIGNATURES[name])}"


def test_linear_args_block_matches_the_header():
    """struct mixq_linear_args: the ctypes mirror has the header's fields in the header's order with matching C types."""
    txt = open(_capi.HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef struct mixq_linear_args \{(.*?)\} mixq_linear_args;", txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "ptr" if "*" in decl else ("float" if decl.startswith("float") else "int")
        names = [v.strip().lstrip("*").strip() for v in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
        fields += [(nm, kind) for nm in names]
    want = {"ptr": C.c_void_p, "int": C.c_int, "float": C.c_float}
    assert [(nm, want[k]) for nm, k in fields] == list(_capi.LinearArgs._fields_)
    assert C.sizeof(_capi.LinearArgs) >= 8 * 14 + 4 * 13


def test_code_object_is_gfx950():
    """The fat binary carries gfx950 code objects and nothing for another GPU (read from the bundle's own entry ids; running
    llvm-objdump --offloading would unpack the bundle next to the library)."""
    blob = open(_capi.LIB_PATH, "rb").read()
    targets = set(re.findall(rb"hipv4-amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", blob))
    assert targets == {b"gfx950"}, targets


def test_version_and_config_table():
    lib = _capi.load()
    assert lib.mixq_version() >= 1000
    names = _capi.gemm_config_names()
    assert len(names) == lib.mixq_gemm_num_configs() and len(set(names)) == len(names)
    assert lib.mixq_gemm_set_config(len(names)) == _capi.MIXQ_EINVAL
    assert lib.mixq_gemm_set_config(-1) == 0
    c = lib.mixq_gemm_pick_config(512, 11008, 4096, 8)
    assert 0 <= c < len(names)
    assert lib.mixq_gemm_pick_config(0, 1, 1, 8) == _capi.MIXQ_EINVAL


def test_argument_validation_without_device():
    """Bad arguments are rejected before anything touches the GPU."""
    lib = _capi.load()
    one = C.c_void_p(16)   # a non-null dummy pointer; never dereferenced on these paths
    assert lib.mixq_find_row_scale(None, one, one, 4, 64, 64, 8, 0, None) == _capi.MIXQ_EINVAL
    assert lib.mixq_find_row_scale(one, one, one, 4, 64, 64, 5, 0, None) == _capi.MIXQ_EINVAL      # bit
    assert lib.mixq_find_row_scale(one, one, one, 4, 60, 64, 8, 0, None) == _capi.MIXQ_ESHAPE      # K % 8
    assert lib.mixq_find_row_scale(one, one, one, 4, 72, 72, 8, 1, None) == _capi.MIXQ_ESHAPE      # packed needs K % 64
    assert lib.mixq_find_row_scale(one, one, one, 0, 64, 64, 8, 0, None) == 0                      # empty input is fine
    assert lib.mixq_gemm_i8_fused(one, one, one, one, None, 0, None, 0, 0, None, None, 0, None, one, 64, 4, 64, 100, 0, 0,
                                  None) == _capi.MIXQ_ESHAPE                                        # K % 64
    assert lib.mixq_gemm_i8_fused(one, one, one, one, None, 0, None, 0, 0, None, None, 0, None, one, 64, 4, 64, 128, 7, 0,
                                  None) == _capi.MIXQ_EINVAL                                        # act
    assert lib.mixq_gemm_i8_fused(one, one, one, one, None, 0, None, 0, 0, None, None, 0, None, one, 64, 0, 64, 128, 0, 0,
                                  None) == 0                                                        # M = 0
    assert lib.mixq_pack_p16x64(one, one, 4, 100, None) == _capi.MIXQ_ESHAPE
    assert lib.mixq_extract_outliers_zero(one, None, 3, one, 4, 64, 64, 3, None) == _capi.MIXQ_EINVAL
    # weight-only W8A16
    assert lib.mixq_pack_w8a16(one, one, 100, 64, None) == _capi.MIXQ_ESHAPE                        # K % 64
    assert lib.mixq_pack_w8a16(None, one, 64, 64, None) == _capi.MIXQ_EINVAL
    assert lib.mixq_gemm_w8a16(one, 128, one, one, None, one, 64, 4, 64, 100, None) == _capi.MIXQ_ESHAPE      # K % 64
    assert lib.mixq_gemm_w8a16(one, 128, one, one, None, one, 64, 4, 62, 128, None) == _capi.MIXQ_ESHAPE      # N % 4
    assert lib.mixq_gemm_w8a16(one, 100, one, one, None, one, 64, 4, 64, 128, None) == _capi.MIXQ_ESHAPE      # ldx < K
    assert lib.mixq_gemm_w8a16(C.c_void_p(8), 128, one, one, None, one, 64, 4, 64, 128, None) == _capi.MIXQ_EINVAL  # x alignment
    assert lib.mixq_gemm_w8a16(one, 128, one, one, None, C.c_void_p(20), 64, 4, 64, 128, None) == _capi.MIXQ_EINVAL   # y alignment (8 bytes)
    assert lib.mixq_gemm_w8a16(one, 128, one, one, None, one, 64, 0, 64, 128, None) == 0                      # M = 0
    assert lib.mixq_gemm_w8a16_set_config(99) == _capi.MIXQ_EINVAL and lib.mixq_gemm_w8a16_set_config(-1) == 0
    # pointer alignment of the fused GEMMs, fp16 and bf16 (include/mixq_hip.h, "Alignment and strides"): y and addend 8 bytes, x_out and w_out
    # 16 bytes, bias 2 bytes - answered before any launch (M = 0 runs every argument check and launches nothing)
    wf16 = _capi.X_PACKED | _capi.W_F16X64
    p4, p8, p17 = C.c_void_p(20), C.c_void_p(24), C.c_void_p(17)

    def fused(fn, layout, M=0, y=one, addend=None, bias=None, x_out=None, w_out=None, n_out=0, lda=64, ld=16):
        return fn(one, one, one, one, x_out, ld, w_out, ld, n_out, None, addend, lda, bias, y, 64, M, 64, 128, 0, layout, None)
    for fn, layout in ((lib.mixq_gemm_i8_fused, 0), (lib.mixq_gemm_i8_fused, wf16), (lib.mixq_gemm_i4_fused, 0), (lib.mixq_gemm_i4_fused, _capi.XW_F6X128),
                       (lib.mixq_gemm_i8_fused_bf16, wf16), (lib.mixq_gemm_i4_fused_bf16, _capi.XW_F6X128)):
        assert fused(fn, layout) == 0
        assert fused(fn, layout, y=p8, addend=p8, bias=C.c_void_p(18), x_out=one, w_out=one, n_out=3) == 0     # 8 / 8 / 2 / 16 / 16: the contract
        for M in (0, 4):
            assert fused(fn, layout, M, y=p4) == _capi.MIXQ_EINVAL
            assert fused(fn, layout, M, y=C.c_void_p(18)) == _capi.MIXQ_EINVAL
            assert fused(fn, layout, M, addend=p4) == _capi.MIXQ_EINVAL
            assert fused(fn, layout, M, addend=p4, lda=0) == _capi.MIXQ_EINVAL
            assert fused(fn, layout, M, bias=p17) == _capi.MIXQ_EINVAL
            assert fused(fn, layout, M, x_out=p8, w_out=one, n_out=3) == _capi.MIXQ_EINVAL
            assert fused(fn, layout, M, x_out=one, w_out=p8, n_out=3) == _capi.MIXQ_EINVAL
        assert fused(fn, layout, x_out=p8, w_out=p8, n_out=0) == 0                                            # (no outlier columns: not read)
    for fn in (lib.mixq_gemm_i8_fused_amax, lib.mixq_gemm_i8_fused_amax_bf16):
        amax = lambda y, addend: fn(one, one, one, one, None, 0, None, 0, 0, None, addend, 64, None, y, 64, 0, 64, 128, 0, wf16, one, None, None)
        assert amax(one, None) == 0 and amax(p4, None) == _capi.MIXQ_EINVAL and amax(one, p4) == _capi.MIXQ_EINVAL
    # coincident faults: the order of the checks is part of the behaviour, the earlier one answers (fp16 and bf16 differ where their kernels do)
    EINVAL, ESHAPE = _capi.MIXQ_EINVAL, _capi.MIXQ_ESHAPE
    i8, i8bf, i4, i4bf = lib.mixq_gemm_i8_fused, lib.mixq_gemm_i8_fused_bf16, lib.mixq_gemm_i4_fused, lib.mixq_gemm_i4_fused_bf16

    def call(fn, layout, M=4, act=0, addend=None, ldy=64):
        return fn(one, one, one, one, None, 0, None, 0, 0, None, addend, 64, None, one, ldy, M, 64, 128, act, layout, None)
    for fn, layout in ((i8, 0), (i8, wf16), (i4, _capi.XW_F6X128), (i8bf, wf16), (i4bf, _capi.XW_F6X128)):
        assert call(fn, layout, act=_capi.ACT_SILU_MUL, ldy=62) == EINVAL          # no multiplier (EINVAL) and a bad ldy (ESHAPE)
        assert call(fn, layout, act=_capi.ACT_SILU_MUL, ldy=62, M=0) == EINVAL
    assert call(i8, wf16, act=_capi.ACT_SILU_PAIR, addend=one) == EINVAL           # the paired form takes no addend ...
    assert call(i8bf, wf16, act=_capi.ACT_SILU_PAIR, addend=one) == ESHAPE         # ... and does not exist in bf16: said first there
    assert call(i8bf, _capi.X_PACKED | _capi.W_PACKED, act=_capi.ACT_SILU_PAIR) == ESHAPE      # (paired act AND a layout bf16 does not serve)
    assert call(i8bf, 64, act=_capi.ACT_SILU_PAIR) == EINVAL                       # (an unknown layout bit is answered before the act)
    both_w = _capi.X_PACKED | _capi.W_PACKED | _capi.W_F16X64
    assert call(i8, both_w) == EINVAL and call(i8bf, both_w) == ESHAPE             # two weight formats at once: fp16 a bad argument, bf16 an unserved layout
    assert call(i8, _capi.W_F16X64) == EINVAL and call(i8bf, _capi.W_F16X64) == ESHAPE
    # a forced tiling without a bf16 form (config 0: an LDS-staged tiling) and an empty problem: bf16 refuses the configuration before the
    # M == 0 early-out, fp16 - whose forced-configuration answers belong to the route - returns MIXQ_OK for the empty problem
    try:
        assert lib.mixq_gemm_set_config(0) == 0
        assert call(i8bf, wf16, M=0) == EINVAL and call(i4bf, _capi.XW_F6X128, M=0) == EINVAL
        assert call(i8, wf16, M=0) == 0 and call(i4, _capi.XW_F6X128, M=0) == 0
        assert call(i4, _capi.XW_F6X128, M=4) == EINVAL                            # (FP6 codes: only the weights-in-registers kernels read them)
        assert call(i8bf, wf16, M=0, ldy=62) == ESHAPE                             # (the shape checks still come first)
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0
    dq = lambda y32=one, addend=None, bias=None, y=one, M=0: lib.mixq_dequant(y32, 64, one, one, addend, 64, bias, y, 64, M, 64, 0, None)
    assert dq() == 0 and dq(y=p8, addend=p8, y32=p4) == 0
    for M in (0, 4):
        assert dq(y=p4, M=M) == dq(addend=p4, M=M) == dq(y32=C.c_void_p(18), M=M) == dq(bias=p17, M=M) == _capi.MIXQ_EINVAL
    # mixq_gemm_i8 writes four int32 as one 16-byte store: y32 16-byte aligned
    assert lib.mixq_gemm_i8(one, one, one, 64, 0, 64, 128, None) == 0
    for M in (0, 4):
        assert lib.mixq_gemm_i8(one, one, p8, 64, M, 64, 128, None) == lib.mixq_gemm_i8(one, one, p4, 64, M, 64, 128, None) == _capi.MIXQ_EINVAL
    # the one-call forward checks its block before it launches anything
    assert lib.mixq_linear_forward(None, None) == _capi.MIXQ_EINVAL
    blk = _capi.LinearArgs()
    blk.bit = 3
    assert lib.mixq_linear_forward(C.byref(blk), None) == _capi.MIXQ_EINVAL
    for fwd, wfmt, qfmt in ((lib.mixq_linear_forward, _capi.FMT_P16X64, _capi.FMT_P16X64), (lib.mixq_linear_forward, _capi.FMT_F16X64, _capi.FMT_P16X64),
                            (lib.mixq_linear_forward_bf16, _capi.FMT_F16X64, _capi.FMT_P16X64)):
        def block(M):
            blk = _capi.LinearArgs()
            blk.x = blk.x_scale = blk.q_x = blk.q_w = blk.scale_col = blk.y = blk.ind = blk.x_out = blk.w_out = blk.addend = blk.bias = 16
            blk.ldx, blk.ldy, blk.lda, blk.ldxo, blk.ldwo, blk.n_cap = 128, 64, 64, 16, 16, 3
            blk.M, blk.N, blk.K, blk.bit, blk.sigma, blk.qfmt, blk.wfmt = M, 64, 128, 8, 6.0, qfmt, wfmt
            return blk
        # the positive control: with every pointer aligned the block passes every argument check of the forward, of its quantise pass and of its
        # GEMM (M = 0: all checks run, nothing is launched) - so the MIXQ_EINVAL below is the alignment check's and nothing earlier
        assert fwd(C.byref(block(0)), None) == 0
        for field, value in (("y", 20), ("addend", 20), ("bias", 17), ("x_out", 24), ("w_out", 24)):        # ... the GEMM's alignment included: M > 0, no pass runs
            for M in (0, 4):
                blk = block(M)
                setattr(blk, field, value)
                assert fwd(C.byref(blk), None) == _capi.MIXQ_EINVAL, (field, M)


def test_bf16_split_plan_is_exported_and_follows_the_fp16_plan_where_every_tiling_has_a_bf16_form():
    """mixq_gemm_pick_split_bf16: the `_bf16` entry points' own N-split decision.  Every tiling the cost model prices has a bf16 form today, so
    at shapes outside fp16's small-batch and long-K exceptions the two plans agree; bad arguments answer MIXQ_EINVAL."""
    lib = _capi.load()
    n1, c2 = C.c_int(0), C.c_int(-1)
    assert lib.mixq_gemm_pick_split_bf16(0, 64, 64, 8, 2, C.byref(n1), C.byref(c2)) == _capi.MIXQ_EINVAL
    assert lib.mixq_gemm_pick_split_bf16(64, 64, 64, 8, 2, None, C.byref(c2)) == _capi.MIXQ_EINVAL
    assert lib.mixq_gemm_pick_split_bf16(512, 4096, 4096, 8, _capi.FMT_P16X64, C.byref(n1), C.byref(c2)) == 0     # a layout the bf16 GEMMs do not read
    for M, N, K, bit, fmt in ((2048, 8200, 128, 8, 2), (1024, 9224, 256, 4, 3), (4096, 11008, 4096, 8, 2), (512, 4096, 4096, 8, 2)):
        assert _capi.gemm_split_plan(M, N, K, bit, fmt, bf16=True) == _capi.gemm_split_plan(M, N, K, bit, fmt), (M, N, K, bit)
    assert _capi.gemm_split_plan(2048, 8200, 128, 8, 2, bf16=True) is not None


def test_product_library_ships_no_tuning_variants():
    """The product .so exports no configuration whose output is wrong by design (the ablation forms), no trace stamps, no K rotation
    and no quantise probes: those live in the -DMIXQ_TUNING build only (engineering #8)."""
    assert os.path.basename(_capi.LIB_PATH) == "libmixq_hip.so"
    lib = _capi.load()
    assert all("abl" not in nm for nm in _capi.gemm_config_names()), _capi.gemm_config_names()
    assert all("abl" not in nm for nm in _capi.w8a16_config_names())
    for name in _capi.TUNING_ONLY:                                          # trace stamps / tile-order knob: not even an entry point
        assert not hasattr(lib, name), name
    assert lib.mixq_quant_set_config(100) == _capi.MIXQ_EINVAL and lib.mixq_quant_set_config(-1) == 0
    blob = open(_capi.LIB_PATH, "rb").read()
    assert b"abl3_mfma" not in blob and b"abl1_noW" not in blob


def test_forced_configuration_round_trips():
    lib = _capi.load()
    names = _capi.gemm_config_names()
    assert lib.mixq_gemm_set_config(len(names) - 1) == 0 and lib.mixq_gemm_set_config(-1) == 0
    assert lib.mixq_quant_set_config(9) == 0 and lib.mixq_quant_set_config(10) == _capi.MIXQ_EINVAL and lib.mixq_quant_set_config(-1) == 0


def test_forced_rebuild_of_one_object(tmp_path):
    """`make -B` on one object (the forced-rebuild path of __graft_entry__.build(force=True), on the smallest source): hipcc cross-
    compiles gfx950 from the tracked sources without a GPU, and the object carries the entry point."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "build", "obj", "forward.o")
    r = subprocess.run(["make", "-C", os.path.join(root, "mixq_amd", "csrc"), "-B", "../../build/obj/forward.o"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "hipcc" in r.stdout and os.path.exists(obj) and b"mixq_linear_forward" in open(obj, "rb").read()


def test_missing_library_is_loud(monkeypatch, tmp_path):
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_capi.MixqBuildError):
        _capi.load()
