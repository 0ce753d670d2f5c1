"""Every store path of the fused GEMMs and of the quantise-side writers on strided, offset and guard-framed outputs (tests/frames.py).

The GEMMs pick their store path at run time from the output: staged = (N % 8 == 0) && (ldy % 8 == 0) && (y % 16 == 0) - LDS-staged 16-byte
row stores (buffer stores on a per-panel descriptor whose length and offsets come from ldy in gemm_wreg.hip), or 8-byte pieces under
m < M && n < N.  Every test here runs its kernels over frames.LAYOUTS(N) - exact fit, a padded row, a column slice of a wider buffer,
ld % 8 == 4, a base that is 8- but not 16-byte aligned, and both - and checks, for every launch:
  (a) every element of y against the existing high-precision reference within the existing bound (fp16: oracle.linear_fused with
      test_gpu_parity.ulp_tol; bf16: the float64 reference() / check() of test_gpu_bf16_gemm.py) - no tolerance of its own;
  (b) nothing outside the window changed (Frame.assert_untouched names the first offending (row, column));
  (c) after (a): the bytes equal those of the exact-fit layout for the same tiling - the store path is a compile-time switch around
      identical arithmetic, so this is an identity;
  (d) no input operand changed (q_x, q_w, x_scale, scale_col, x_out, w_out, addend, bias - the last three in frames of their own).
No layout, tiling or operand combination is skipped or sampled (tests/test_frames_host.py shows the layout list reaches every store class
for each N used here; COMBOS is the full cross product of the operand forms).  Nothing here launches with an output aligned to less than the documented 8 bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from frames import GUARD_ROWS, LAYOUTS, Frame, classes_possible, store_class  # noqa: E402
from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib  # noqa: E402
from mixq_amd._capi import ACT_NONE, ACT_SILU, ACT_SILU_MUL, ACT_SILU_PAIR, FMT_F16X64, FMT_F6X128, FMT_P16X64, FMT_PLAIN, FMT_R6X128  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402
from mixq_amd.fused import interleave_pair_rows  # noqa: E402
from mixq_amd.linear import kept_outlier_map  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_gpu_bf16_gemm import BF16_FP6, BF16_INT8, Problem, _quantise64, check, reference, unpack_i4  # noqa: E402
from test_gpu_fp6 import F6_TILINGS  # noqa: E402
from test_gpu_pair import _case as pair_case  # noqa: E402
from test_gpu_parity import _fused_case, _skinny_id, _tiled_configs, _w8a16_case, _wr_configs, make_x, n, t, ulp_tol  # noqa: E402

DEV = "cuda"
F16, BF = torch.float16, torch.bfloat16
NAN_BITS = 0x7FC1                                          # a NaN in bf16 and in fp16: the pad columns of x_out / w_out
SHAPES = [(200, 512, 1000),                                # partial last M and N tiles, staged
          (200, 512, 1004),                                # unstaged by N
          (24, 512, 256),                                  # small batch
          (1, 512, 256)]                                   # one row
PAIR_SHAPE = (200, 512, 1168)                              # the joint gate / up form: y has 584 = 8 * 73 columns (staged, a partial last N tile)
PAIR_TILINGS = ["wr128x192_s16_d4_l2", "wr128x256_s16_d3_l2", "wr64x192_s16_d4_l2", "wr64x256_s16_d4_l2", "wr32x64_s8_d6_l1"]
# The operand sweep: the full cross product the store paths are run over - outlier count {0, 17, 41, 17 as a count in device memory below a
# capacity of 48} x (act NONE / SILU with the addend absent or at lda N, N + 4, 2N + 64 with a column offset, 0 = one row broadcast; SILU_MUL
# with its multiplier at the same four strides) x bias on / off = 4 x 14 x 2 = 112 combinations.  Nothing is thinned.
def _combos():
    pairs = [(a, k) for a in (ACT_NONE, ACT_SILU) for k in (None, "N", "N+4", "wide", "bcast")] + [(ACT_SILU_MUL, k) for k in ("N", "N+4", "wide", "bcast")]
    return [dict(n=n_out, dev=dev, act=a, add=k, bias=bias) for n_out, dev in ((0, False), (17, False), (41, False), (17, True)) for a, k in pairs
            for bias in (False, True)]


COMBOS = _combos()
assert len(COMBOS) == 112
DEV_CAP = 48


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    lib = _capi.load()
    lib.mixq_gemm_set_config(-1); lib.mixq_quant_set_config(-1); lib.mixq_gemm_w8a16_set_config(-1)
    yield
    lib.mixq_gemm_set_config(-1); lib.mixq_quant_set_config(-1); lib.mixq_gemm_w8a16_set_config(-1)


def pad16(v):
    return (v + 15) // 16 * 16


def ibits(x):
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def same_bytes(a, b):
    return a.shape == b.shape and bool((ibits(a) == ibits(b)).all())


class Kept:
    """Copies of input tensors taken before the launches; unchanged() compares them byte for byte."""

    def __init__(self, **tensors):
        self.items = [(k, v, v.clone()) for k, v in tensors.items() if v is not None]

    def unchanged(self, what):
        for name, now, was in self.items:
            assert torch.equal(ibits(now), ibits(was)), f"{what}: the input operand {name} changed"


def framed(values, ld, col_off=0, elem_off=0, fill_nan_to=None):
    """An input operand inside a frame of its own: window = `values` ([R, C]), or [R, fill_nan_to] with NaN patterns behind column C."""
    R, Cc = values.shape
    cols = fill_nan_to or Cc
    f = Frame(R, cols, ld, col_off, elem_off, values.dtype, DEV, GUARD_ROWS)
    if fill_nan_to:
        f.view.view(torch.int16).fill_(NAN_BITS)
    f.view[:, :Cc] = values
    return f.freeze()


class Operands:
    """One (M, K, N, bit) problem on the device in every operand format its kernels read, the framed 16-bit inputs, and the reference of
    every operand combination (computed once: it does not depend on the tiling or on y's layout)."""

    def __init__(self, M, K, N, bit, dtype):
        self.M, self.K, self.N, self.bit, self.dtype = M, K, N, bit, dtype
        if dtype == F16:
            c = self.c = _fused_case(M, N, K, bit, seed=M + N + K + bit, n_out=41, bias=True, addend=True, act=0)
            self.mul_np = (np.random.default_rng(M + N + 99).standard_normal((M, N)) * 1.5).astype(np.float16)
            qx, qw = t(c["qx"]), t(c["qw"])
            self.q = {0: (qx, qw), 1: (mixlib.PackOperand(qx, FMT_P16X64), mixlib.PackOperand(qw, FMT_P16X64)),
                      2: (mixlib.PackOperand(qx, FMT_P16X64), mixlib.PackOperand(qw, FMT_F16X64))}
            if bit == 4:
                self.q[6] = (mixlib.PackOperand(qx, FMT_R6X128), mixlib.PackOperand(qw, FMT_F6X128))
            self.sx = torch.zeros((M, 1), dtype=F16, device=DEV)
            self.sx[:, 0] = t(c["sx"])
            self.sw, self.bias = t(c["sw"]), t(c["bias"])
            self.add_vals, self.mul_vals, self.xo_vals, self.wo_vals = t(c["addend"]), t(self.mul_np), t(c["xo"]), t(c["wo"])
        else:
            p = self.p = Problem(bit, M, K, N, seed=1000 * bit + M + N, dtype=BF)
            self.q = {2 if bit == 8 else 6: (p.qx_img, p.qw_img)}
            self.sx, self.sw, self.bias = p.sx, p.sw, p.bias
            self.add_vals, self.mul_vals, self.xo_vals, self.wo_vals = p.addend, p.mul, p.xo_vals, p.wo_vals
        self.kept = Kept(sx=self.sx, sw=self.sw, bias=self.bias, **{f"q_x{k}": v[0] for k, v in self.q.items()}, **{f"q_w{k}": v[1] for k, v in self.q.items()})
        self._frames, self._checks = {}, {}

    # ---- framed inputs -----------------------------------------------------------------------------------------------------------
    def outliers(self, n_out, dev):
        """(x_out frame, w_out frame, n_out argument, n_out_dev): capacity pad16(n) - or DEV_CAP with the count in device memory -, NaN
        patterns in every column >= n, and DIFFERENT row strides: capacity + 8 and capacity + 32."""
        if n_out == 0:
            return None, None, 0, None
        key = ("o", n_out, dev)
        if key not in self._frames:
            cap = DEV_CAP if dev else pad16(n_out)
            fx = framed(self.xo_vals[:, :n_out], cap + 8, fill_nan_to=cap)
            fw = framed(self.wo_vals[:, :n_out], cap + 32, fill_nan_to=cap)
            n_dev = torch.tensor([n_out], dtype=torch.int32, device=DEV) if dev else None
            self._frames[key] = (fx, fw, cap if dev else n_out, n_dev)
        return self._frames[key]

    def addend(self, kind, act):
        """(frame, the tensor FusedLinear gets, its [M, N] values) for lda = N, N + 4, 2N + 64 with a column offset, or 0."""
        if kind is None:
            return None, None, None
        key = ("a", kind, act == ACT_SILU_MUL)
        if key not in self._frames:
            vals = self.mul_vals if act == ACT_SILU_MUL else self.add_vals
            N = self.N
            if kind == "bcast":
                f = framed(vals[:1], N)
                self._frames[key] = (f, f.view.as_strided((self.M, N), (0, 1), f.view.storage_offset()), vals[:1].expand(self.M, N))
            else:
                ld, off = {"N": (N, 0), "N+4": (N + 4, 0), "wide": (2 * N + 64, N + 8)}[kind]
                f = framed(vals, ld, off)
                self._frames[key] = (f, f.view, vals)
            a = self._frames[key][1]
            assert a.stride(0) == {"N": N, "N+4": N + 4, "wide": 2 * N + 64, "bcast": 0}[kind] and a.data_ptr() % 8 == 0
        return self._frames[key]

    # ---- references --------------------------------------------------------------------------------------------------------------
    def checker(self, combo):
        """check(y, what) for one operand combination: (a) of the module docstring."""
        key = (combo["n"], combo["act"], combo["add"], combo["bias"])
        if key in self._checks:
            return self._checks[key]
        n_out, act = combo["n"], combo["act"]
        if self.dtype == F16:
            c = self.c
            a = None
            if combo["add"] is not None:
                a = self.mul_np if act == ACT_SILU_MUL else c["addend"]
                a = np.ascontiguousarray(np.broadcast_to(a[:1], a.shape)) if combo["add"] == "bcast" else a
            ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], xo=np.ascontiguousarray(c["xo"][:, :n_out]) if n_out else None,
                                 wo=np.ascontiguousarray(c["wo"][:, :n_out]) if n_out else None, addend=a, bias=c["bias"] if combo["bias"] else None,
                                 act=act, bit=self.bit).astype(np.float32)
            fn = fp16_checker(ref)
        else:
            _, _, a = self.addend(combo["add"], act)
            ref, bound = reference(self.p.acc, self.sx, self.sw, self.xo_vals, self.wo_vals, n_out, a, self.bias if combo["bias"] else None, act)
            fn = lambda y, what: check(y, ref, bound, what)  # noqa: E731
        self._checks[key] = fn
        return fn

    def launch(self, fmt, combo, y, **kw):
        fx, fw, n_arg, n_dev = self.outliers(combo["n"], combo["dev"])
        _, a, _ = self.addend(combo["add"], combo["act"])
        qx, qw = self.q[fmt]
        out = mixlib.FusedLinear(qx, qw, self.sx, self.sw, None if fx is None else fx.view, None if fw is None else fw.view, n_arg,
                                 self.bias if combo["bias"] else None, self.M, self.N, self.K, bit=self.bit, act=combo["act"], n_out_dev=n_dev, addend=a,
                                 out=y, dtype=self.dtype, **kw)
        assert out is y

    def inputs_unchanged(self, combo, what):
        self.kept.unchanged(what)
        fx, fw, _, _ = self.outliers(combo["n"], combo["dev"])
        fa, _, _ = self.addend(combo["add"], combo["act"])
        for name, f in (("x_out", fx), ("w_out", fw), ("addend", fa)):
            if f is not None:
                f.assert_unchanged(f"{what}: input operand {name}")


def fp16_checker(ref):
    """tests/test_gpu_parity.py's comparison - |y - ref| <= ulp_tol(ref) in float32, y finite - for every element, evaluated on the device."""
    tol = ulp_tol(ref)
    ref_t, tol_t = t(ref), t(tol)

    def fn(y, what):
        assert y.dtype == F16 and tuple(y.shape) == tuple(ref_t.shape), what
        yf = y.float()
        d = (yf - ref_t).abs()
        bad = ~(torch.isfinite(yf) & (d.to(tol_t.dtype) <= tol_t))
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            r, cc = divmod(i, y.shape[1])
            raise AssertionError(f"{what}: {int(bad.sum())} of {y.numel()} elements outside ulp_tol; first at [{r},{cc}]: y {float(y[r, cc])} ref {float(ref_t[r, cc])} "
                                 f"tol {float(tol_t[r, cc])}; max |d| {float(d.max())}")
    return fn


_ops = {}


def operands(M, K, N, bit, dtype):
    key = (M, K, N, bit, dtype)
    if key not in _ops:
        _ops[key] = Operands(M, K, N, bit, dtype)
    return _ops[key]


_yframes = {}


def y_frame(rows, cols, layout, dtype):
    """One frame per (window, layout, dtype), reset to the pattern before every launch (so an element the kernel leaves out fails (a))."""
    key = (rows, cols, layout, dtype)
    if key not in _yframes:
        ld, col_off, elem_off = layout
        _yframes[key] = Frame(rows, cols, ld, col_off, elem_off, dtype, DEV, GUARD_ROWS)
    f = _yframes[key]
    f.reset()
    return f


def sweep_layouts(op, fmt, what, combos=COMBOS, cols=None, launch=None, checker=None, after=None):
    """Every layout of LAYOUTS x every operand combination for the tiling that is forced right now: (a), (b), (c), (d).  Returns the store
    classes that ran."""
    cols = cols or op.N
    layouts = LAYOUTS(cols)
    ran = set()
    for combo in combos:
        first = None
        chk = (checker or op.checker)(combo)
        for layout in layouts:
            f = y_frame(op.M, cols, layout, op.dtype)
            y = f.view
            assert y.data_ptr() % 8 == 0
            cls = store_class(cols, y.stride(0), y.data_ptr())
            w = f"{what} ld={layout[0]} col_off={layout[1]} elem_off={layout[2]} [{cls}] n_out={combo['n']} dev_count={combo['dev']} act={combo['act']} " \
                f"addend={combo['add']} bias={combo['bias']}"
            (launch or op.launch)(fmt, combo, y)
            chk(y, w)                                                               # (a)
            f.assert_untouched(w)                                                   # (b)
            if first is None:
                first = y.clone()
            else:
                assert same_bytes(y, first), f"{w}: differs from the exact-fit layout in {int((ibits(y) != ibits(first)).sum())} elements"   # (c)
            op.inputs_unchanged(combo, w)                                           # (d)
            if after is not None:
                after(combo, y, w)
            ran.add(cls)
    assert ran == classes_possible(cols), (what, ran)
    return ran


def forced(names_or_ids):
    """Iterate (id, name) over tilings, each forced through mixq_gemm_set_config while the body runs; automatic again afterwards."""
    lib, names = _capi.load(), _capi.gemm_config_names()
    try:
        for c in names_or_ids:
            cid = names.index(c) if isinstance(c, str) else c
            assert lib.mixq_gemm_set_config(cid) == 0
            yield cid, (names[cid] if cid >= 0 else "auto")
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0


# ---- 2. every fused-GEMM family x every layout ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_every_lds_staged_tiling_of_gemm_hip_plain_and_p16x64(M, K, N, bit):
    op = operands(M, K, N, bit, F16)
    for _, name in forced(_tiled_configs()):
        for fmt in (0, 1):
            sweep_layouts(op, fmt, f"W{bit} {name} {'plain' if fmt == 0 else 'P16X64'} {M}x{K}->{N}")


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_every_weights_in_registers_tiling_int8_fp16(M, K, N):
    op = operands(M, K, N, 8, F16)
    for _, name in forced(_wr_configs()):
        sweep_layouts(op, 2, f"W8 {name} {M}x{K}->{N}")


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_every_weights_in_registers_tiling_int4_nibbles_and_fp6(M, K, N):
    op = operands(M, K, N, 4, F16)
    names = _capi.gemm_config_names()
    # (the nibble form: 128 x 256 has none - accumulators + ring + expanded nibbles exceed the registers - as in test_every_wreg_tiling_full_epilogue_and_int4)
    for _, name in forced([c for c in _wr_configs() if "128x256" not in names[c]]):
        sweep_layouts(op, 2, f"W4 nibbles {name} {M}x{K}->{N}")
    for _, name in forced(F6_TILINGS):
        sweep_layouts(op, 6, f"W4 FP6 {name} {M}x{K}->{N}")


@pytest.mark.parametrize("bit,names", [(8, BF16_INT8), (4, BF16_FP6)])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_every_bf16_tiling(M, K, N, bit, names):
    op = operands(M, K, N, bit, BF)
    for _, name in forced(names):
        sweep_layouts(op, 2 if bit == 8 else 6, f"bf16 W{bit} {name} {M}x{K}->{N}")


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("M,K,N", [(24, 512, 1000), (24, 512, 1004), (24, 512, 256), (1, 512, 256)])
def test_small_batch_kernel_of_gemm_skinny(M, K, N, bit):
    op = operands(M, K, N, bit, F16)
    for _ in forced([_skinny_id()]):
        for fmt in (1, 2):
            sweep_layouts(op, fmt, f"W{bit} decode32 fmt {fmt} {M}x{K}->{N}")


@pytest.mark.parametrize("bit,M,K,N", [(8, 200, 512, 1000), (8, 24, 512, 256), (4, 200, 512, 1004), (4, 1, 512, 256)])
def test_automatic_pick_every_layout(bit, M, K, N):
    assert _capi.load().mixq_gemm_set_config(-1) == 0
    for dtype in (F16, BF):
        op = operands(M, K, N, bit, dtype)
        for fmt in op.q:
            sweep_layouts(op, fmt, f"{dtype} W{bit} auto fmt {fmt} {M}x{K}->{N}")


# ---- the joint gate / up form: y has N / 2 columns --------------------------------------------------------------------------------
class PairOperands:
    def __init__(self, M, K, N2, bit):
        self.M, self.K, self.N, self.bit, self.dtype = M, K, N2, bit, F16           # N: the interleaved rows; y has N / 2 columns
        c = self.c = pair_case(M, N2 // 2, K, 41, True, seed=M + N2, bit=bit)
        u, g = c["up"], c["gate"]
        xf, wf = (FMT_P16X64, FMT_F16X64) if bit == 8 else (FMT_R6X128, FMT_F6X128)
        self.qx = mixlib.PackOperand(t(c["qx"]), xf)
        self.qw = mixlib.PackOperand(interleave_pair_rows(t(u["qw"]), t(g["qw"])), wf)
        self.sx = torch.zeros((M, 1), dtype=F16, device=DEV)
        self.sx[:, 0] = t(c["sx"])
        self.sw = interleave_pair_rows(t(u["sw"]).reshape(-1), t(g["sw"]).reshape(-1)).reshape(1, -1)
        self.bias = interleave_pair_rows(t(u["bias"]), t(g["bias"]))
        self.xo_vals, self.wo_vals = t(c["xo"]), interleave_pair_rows(t(u["wo"]), t(g["wo"]))
        self.kept = Kept(q_x=self.qx, q_w=self.qw, sx=self.sx, sw=self.sw, bias=self.bias)
        self._frames, self._checks = {}, {}

    outliers = Operands.outliers

    def addend(self, kind, act):
        return None, None, None

    inputs_unchanged = Operands.inputs_unchanged

    def checker(self, combo):
        key = (combo["n"], combo["bias"])
        if key not in self._checks:
            c, n_out = self.c, combo["n"]
            u, g = c["up"], c["gate"]
            xo = np.ascontiguousarray(c["xo"][:, :n_out]) if n_out else None
            wo = lambda d: np.ascontiguousarray(d["wo"][:, :n_out]) if n_out else None  # noqa: E731
            b = lambda d: d["bias"] if combo["bias"] else None  # noqa: E731
            up = O.linear_fused(c["qx"], u["qw"], c["sx"], u["sw"], xo=xo, wo=wo(u), addend=None, bias=b(u), act=0, bit=self.bit)
            ref = O.linear_fused(c["qx"], g["qw"], c["sx"], g["sw"], xo=xo, wo=wo(g), addend=up, bias=b(g), act=2, bit=self.bit).astype(np.float32)
            self._checks[key] = fp16_checker(ref)
        return self._checks[key]

    def launch(self, fmt, combo, y):
        fx, fw, n_arg, n_dev = self.outliers(combo["n"], combo["dev"])
        out = mixlib.FusedLinear(self.qx, self.qw, self.sx, self.sw, None if fx is None else fx.view, None if fw is None else fw.view, n_arg,
                                 self.bias if combo["bias"] else None, self.M, self.N, self.K, bit=self.bit, act=ACT_SILU_PAIR, n_out_dev=n_dev, out=y)
        assert out is y


PAIR_COMBOS = [dict(n=0, dev=False, act=ACT_SILU_PAIR, add=None, bias=False), dict(n=17, dev=True, act=ACT_SILU_PAIR, add=None, bias=True),
               dict(n=41, dev=False, act=ACT_SILU_PAIR, add=None, bias=False), dict(n=17, dev=False, act=ACT_SILU_PAIR, add=None, bias=True)]


@pytest.mark.parametrize("bit", [8, 4])
def test_joint_gate_up_form_every_paired_tiling(bit):
    """MIXQ_ACT_SILU_PAIR at 200 x 512 -> 2 x 584: M > 128, N / 2 = 584 a multiple of 8 but not of 64, so the staged path of the paired
    epilogue AND a partial last N tile are reached; the layouts are built on the N / 2 columns y has."""
    M, K, N2 = PAIR_SHAPE
    assert M > 128 and N2 % 64 and (N2 // 2) % 8 == 0 and (N2 // 2) % 64
    op = PairOperands(M, K, N2, bit)
    # the tilings with the paired epilogue (gemm_wreg.hip's table): all five in int8; in the FP6 form every one but 128 x 256, which has no FP6
    # form at all and answers MIXQ_EINVAL before any launch
    tilings = PAIR_TILINGS if bit == 8 else [nm for nm in PAIR_TILINGS if nm != "wr128x256_s16_d3_l2"]
    assert len(tilings) == (5 if bit == 8 else 4)
    ran = 0
    for _, name in forced([-1] + tilings):
        sweep_layouts(op, None, f"W{bit} pair {name} {M}x{K}->2x{N2 // 2}", combos=PAIR_COMBOS, cols=N2 // 2)
        ran += 1
    assert ran == (6 if bit == 8 else 5)
    if bit == 4:
        for _ in forced(["wr128x256_s16_d3_l2"]):
            f = y_frame(M, N2 // 2, LAYOUTS(N2 // 2)[0], F16)
            with pytest.raises(_capi.MixqError) as e:
                op.launch(None, PAIR_COMBOS[0], f.view)
            assert e.value.code == _capi.MIXQ_EINVAL, str(e.value)
            f.assert_untouched("W4 pair wr128x256_s16_d3_l2: refused before any launch")


# ---- the automatic pick where it runs TWO launches: the second writes y from column n1 on ----------------------------------------------
@pytest.mark.parametrize("bit,M,N,K", [(8, 2048, 8200, 128), (4, 1024, 9224, 256)])
def test_the_n_split_writes_a_strided_y(bit, M, N, K):
    """With ld > N this is the one place a column offset and a row stride combine inside the library."""
    fmt = 2 if bit == 8 else 3
    assert _capi.load().mixq_gemm_set_config(-1) == 0
    combos = [dict(n=17, dev=False, act=ACT_NONE, add="N+4", bias=True), dict(n=17, dev=True, act=ACT_SILU_MUL, add="wide", bias=True),
              dict(n=0, dev=False, act=ACT_SILU, add=None, bias=False), dict(n=41, dev=False, act=ACT_NONE, add="bcast", bias=True)]
    for dtype in (F16, BF):            # (the bf16 entry points pick among their own tilings: their own plan, mixq_gemm_pick_split_bf16)
        plan = _capi.gemm_split_plan(M, N, K, bit, fmt, bf16=dtype == BF)
        assert plan is not None and 0 < plan[0] < N and plan[0] % 64 == 0, (dtype, plan)
        if dtype == BF:
            assert plan[1] in (BF16_INT8 if bit == 8 else BF16_FP6), plan
        op = Operands(M, K, N, bit, dtype)
        sweep_layouts(op, 2 if bit == 8 else 6, f"{dtype} W{bit} split at {plan[0]} ({plan[1]}) {M}x{K}->{N}", combos=combos)
    _yframes.clear()
    torch.cuda.empty_cache()


# ---- the row-maximum side output ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF])
@pytest.mark.parametrize("M,K,N", [(200, 512, 1000), (200, 512, 1004), (130, 512, 256)])
def test_row_amax_on_a_strided_y(M, K, N, dtype):
    """mixq_gemm_i8_fused_amax(_bf16): row_amax holds M live entries inside a frame - entries >= M stay untouched - and equals the masked
    maximum of the bit patterns of the bytes actually in y, on every layout, for every int8 tiling."""
    op = operands(M, K, N, 8, dtype)
    assert mixlib.amax_supported(M, N, K, FMT_P16X64, FMT_F16X64, dtype=dtype)
    ind = torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(5))[:23])[0].to(torch.int32).to(DEV)
    cm = kept_outlier_map(ind, N)
    cm_kept = Kept(col_mask=cm)
    fa = Frame(1, M, M + 64, 0, 0, torch.int32, DEV, 2)

    def launch(fmt, combo, y):
        fa.reset()
        fa.view.zero_()
        op.launch(fmt, combo, y, row_amax=fa.view[0], col_mask=cm)

    def after(combo, y, w):
        fa.assert_untouched(f"{w}: row_amax")
        b = ibits(y).int() & 0x7FFF
        b[:, ind.long()] = 0
        assert torch.equal(fa.view[0], b.max(dim=1).values.to(torch.int32)), f"{w}: row_amax is not the masked maximum of y's bit patterns"
        cm_kept.unchanged(w)

    # (the side output is a run-time branch of every weights-in-registers tiling's epilogue: every one is forced, and the automatic pick)
    for _, name in forced([-1] + (BF16_INT8 if dtype == BF else _wr_configs())):
        sweep_layouts(op, 2, f"{dtype} amax {name} {M}x{K}->{N}", launch=launch, after=after)


# ---- the one-call forward = its two calls, with frames around everything it writes ------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF])
@pytest.mark.parametrize("bit", [8, 4])
def test_linear_forward_is_its_two_calls_on_strided_x_and_y(bit, dtype):
    M, K, N = 200, 512, 1000
    assert _capi.load().mixq_gemm_set_config(-1) == 0
    op = operands(M, K, N, bit, dtype)
    sfx = "" if dtype == F16 else "_bf16"
    cols = [5, 77, 130, 131, 300, 511, 64, 2, 400]
    nc, cap = len(cols), 16
    ind = torch.zeros(cap, dtype=torch.int32, device=DEV)
    ind[:nc] = torch.tensor(cols, dtype=torch.int32)
    n_dev = torch.tensor([nc], dtype=torch.int32, device=DEV)
    x0 = t(make_x(M, K, seed=3, outlier_cols=cols)).to(dtype)
    qfmt, wfmt = (FMT_P16X64, FMT_F16X64) if bit == 8 else (FMT_R6X128, FMT_F6X128)
    layout = (_capi.X_PACKED | _capi.W_F16X64) if bit == 8 else _capi.XW_F6X128
    qw = op.q[2 if bit == 8 else 6][1]
    fw = framed(op.wo_vals[:, :nc], cap + 32, fill_nan_to=cap)
    rows16, rb = mixlib.packed_rows(M), mixlib._q_row_bytes(K, bit, qfmt)
    live = ibits(mixlib.PackOperand(torch.full((M, K if bit == 8 else K // 2), 0xFF, dtype=torch.uint8, device=DEV).view(torch.int8 if bit == 8 else torch.uint8), qfmt)).reshape(-1) != 0
    ldx, ldo = K + 64, cap + 16
    kept = Kept(ind=ind, n_dev=n_dev, q_w=qw, sw=op.sw, bias=op.bias)
    for ylayout in LAYOUTS(N)[1:]:                                             # ldy > N in every one
        outs = []
        for one_call in (False, True):
            fx = framed(x0, ldx)
            fs = Frame(1, M, M + 64, 0, 0, F16, DEV, 2)
            fq = Frame(1, rows16 * rb, rows16 * rb, 0, 0, torch.uint8, DEV, 2)
            fo = Frame(M, ldo, ldo, 0, 0, dtype, DEV, GUARD_ROWS)          # (columns n .. ldo-1 are written with zeros: they belong to the window)
            fy = Frame(M, N, *ylayout, dtype, DEV, GUARD_ROWS)
            if one_call:
                a = _capi.LinearArgs()
                a.x, a.ldx, a.ind, a.n_cap, a.n_dev = fx.view.data_ptr(), ldx, ind.data_ptr(), cap, n_dev.data_ptr()
                a.x_scale, a.q_x, a.x_out, a.ldxo = fs.view.data_ptr(), fq.view.data_ptr(), fo.view.data_ptr(), ldo
                a.q_w, a.scale_col, a.w_out, a.ldwo, a.bias = qw.data_ptr(), op.sw.data_ptr(), fw.view.data_ptr(), fw.view.stride(0), op.bias.data_ptr()
                a.y, a.ldy, a.M, a.N, a.K, a.bit, a.sigma, a.act, a.qfmt, a.wfmt = fy.view.data_ptr(), ylayout[0], M, N, K, bit, 6.0, ACT_NONE, qfmt, wfmt
                _capi.call("mixq_linear_forward" + sfx, C.byref(a), mixlib._stream())
            else:
                _capi.call("mixq_quant_fused" + sfx, fx.view.data_ptr(), ind.data_ptr(), cap, n_dev.data_ptr(), fs.view.data_ptr(), fq.view.data_ptr(),
                           fo.view.data_ptr(), None, M, K, ldx, ldo, bit, 6.0, qfmt, mixlib._stream())
                _capi.call(("mixq_gemm_i8_fused" if bit == 8 else "mixq_gemm_i4_fused") + sfx, fq.view.data_ptr(), qw.data_ptr(), fs.view.data_ptr(), op.sw.data_ptr(),
                           fo.view.data_ptr(), ldo, fw.view.data_ptr(), fw.view.stride(0), cap, n_dev.data_ptr(), None, 0, op.bias.data_ptr(), fy.view.data_ptr(),
                           ylayout[0], M, N, K, ACT_NONE, layout, mixlib._stream())
            torch.cuda.synchronize()
            w = f"{dtype} W{bit} {'one call' if one_call else 'two calls'} ldy={ylayout}"
            for name, f in (("x", fx), ("x_scale", fs), ("q_x", fq), ("x_out", fo), ("y", fy)):
                f.assert_untouched(f"{w}: {name}")
            fw.assert_unchanged(f"{w}: w_out")
            kept.unchanged(w)
            # rows >= M of the packed image are left untouched; only the outlier columns of x changed, to zero
            q_now, q_was = fq.view[0], fq.saved_view()[0]
            assert torch.equal(q_now[~live], q_was[~live]), f"{w}: rows >= M of the packed activations were written"
            want_x = x0.clone()
            want_x[:, cols] = 0
            assert same_bytes(fx.view, want_x), f"{w}: x"
            assert same_bytes(fo.view[:, :nc], x0[:, cols]) and int(ibits(fo.view[:, nc:]).abs().max()) == 0, f"{w}: x_out (columns n .. ldo-1 are written with zeros)"
            outs.append([f.view.clone() for f in (fx, fs, fq, fo, fy)])
        for name, a2, a1 in zip(("x", "x_scale", "q_x", "x_out", "y"), *outs):
            assert same_bytes(a2, a1), f"{dtype} W{bit} ldy={ylayout}: {name} differs between the one call and its two calls"
        # ... and y is right: the quantised operands the pass wrote, through the reference
        y = outs[1][4]
        if dtype == F16:
            xz = n(x0).copy()
            xo_ref = O.extract_outliers_zero(xz, np.array(cols, np.int32))
            q_ref, s_ref = O.find_row_scale(xz, bit)
            ref = O.linear_fused(q_ref, op.c["qw"], s_ref, op.c["sw"], xo=xo_ref, wo=np.ascontiguousarray(op.c["wo"][:, :nc]), bias=op.c["bias"], act=0, bit=bit)
            fp16_checker(ref.astype(np.float32))(y, f"W{bit} one call ldy={ylayout}")
        else:
            q64, s = _quantise64(x0, ind[:nc], bit)
            w_int = mixlib.UnpackOperand(qw, N)                                     # the plain [N, KB] matrix back from the weight image
            w_int = w_int.view(torch.int8).to(torch.float64) if bit == 8 else unpack_i4(w_int.view(torch.uint8)).to(torch.float64)
            ref, bound = reference(q64 @ w_int.T, s.reshape(-1), op.sw, x0[:, cols], op.wo_vals, nc, None, op.bias, ACT_NONE)
            check(y, ref, bound, f"bf16 W{bit} one call ldy={ylayout}")


# ---- the unfused pair -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", [(200, 512, 1000), (200, 512, 1004), (1, 512, 256)])
def test_gemm_i8_and_dequant_with_every_stride_different_from_n(M, K, N):
    """mixq_gemm_i8 + mixq_dequant with ldy32, ldy and lda all different from N (and from each other), frames around both outputs."""
    assert _capi.load().mixq_gemm_set_config(-1) == 0
    c = _fused_case(M, N, K, 8, seed=M + N, n_out=0, bias=True, addend=True, act=0)
    qx, qw = t(c["qx"]), t(c["qw"])
    sx, sw, bias = t(c["sx"]), t(c["sw"]), t(c["bias"])
    kept = Kept(qx=qx, qw=qw, sx=sx, sw=sw, bias=bias)
    acc_ref = O.gemm_i8(c["qx"], c["qw"])
    for ld32, ldy, lda in ((N + 4, N + 8, N + 16), (N + 8, N + 4, 2 * N + 64), (N + 12, N, N + 4)):
        f32 = Frame(M, N, ld32, 0, 0, torch.int32, DEV, GUARD_ROWS)
        _capi.call("mixq_gemm_i8", qx.data_ptr(), qw.data_ptr(), f32.view.data_ptr(), ld32, M, N, K, mixlib._stream())
        f32.assert_untouched(f"mixq_gemm_i8 ldy={ld32}")
        assert np.array_equal(n(f32.view), acc_ref)
        f32.freeze()
        fa = framed(t(c["addend"]), lda, 8 if lda > N + 8 else 0)
        for act in (ACT_NONE, ACT_SILU):
            fy = Frame(M, N, ldy, 0, 0, F16, DEV, GUARD_ROWS)
            _capi.call("mixq_dequant", f32.view.data_ptr(), ld32, sx.data_ptr(), sw.data_ptr(), fa.view.data_ptr(), lda, bias.data_ptr(), fy.view.data_ptr(), ldy,
                       M, N, act, mixlib._stream())
            w = f"mixq_dequant ldy32={ld32} ldy={ldy} lda={lda} act={act}"
            ref = O.linear_fused(c["qx"], c["qw"], c["sx"], c["sw"], addend=c["addend"], bias=c["bias"], act=act, bit=8).astype(np.float32)
            fp16_checker(ref)(fy.view, w)
            fy.assert_untouched(w)
            f32.assert_unchanged(f"{w}: y32")
            fa.assert_unchanged(f"{w}: addend")
            kept.unchanged(w)


# ---- weight-only W8A16: its `wide` selector is the same expression ----------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_w8a16_every_configuration_every_layout(M, K, N):
    q, s, x, b = _w8a16_case(M, N, K, 7 * M + N + K, True)
    lib, names = _capi.load(), _capi.w8a16_config_names()
    wp, sw, bias = mixlib.PackW8A16(t(q)), t(s), t(b)
    fx = framed(t(x), K + 8)                                                       # ldx > K (ldx % 8 == 0, x 16-byte aligned)
    kept = Kept(wp=wp, sw=sw, bias=bias)
    chk = fp16_checker(O.w8a16_linear(x, q, s, b).astype(np.float32))
    try:
        for cfg in [-1] + [i for i, nm in enumerate(names) if "abl" not in nm and not ("decode" in nm and M > 32)]:   # (the K-split kernel takes M <= 32)
            assert lib.mixq_gemm_w8a16_set_config(cfg) == 0
            first, ran = None, set()
            for layout in LAYOUTS(N):
                f = y_frame(M, N, layout, F16)
                y = f.view
                cls = store_class(N, y.stride(0), y.data_ptr())
                w = f"w8a16 {names[cfg] if cfg >= 0 else 'auto'} {M}x{K}->{N} ld={layout[0]} col_off={layout[1]} elem_off={layout[2]} [{cls}]"
                assert mixlib.W8A16Linear(fx.view, wp, sw, bias, N, K, out=y) is y
                chk(y, w)
                f.assert_untouched(w)
                first = y.clone() if first is None else first
                assert same_bytes(y, first), f"{w}: differs from the exact-fit layout"
                fx.assert_unchanged(f"{w}: x")
                kept.unchanged(w)
                ran.add(cls)
            assert ran == classes_possible(N)
    finally:
        lib.mixq_gemm_w8a16_set_config(-1)


# ---- 3. the writers on the quantise side -------------------------------------------------------------------------------------------------
QFMTS = {8: [FMT_PLAIN, FMT_P16X64, FMT_F16X64], 4: [FMT_PLAIN, FMT_P16X64, FMT_F6X128, FMT_R6X128]}
QUANT_SHAPES = [(1, 512), (17, 512), (130, 512), (17, 30720)]           # K > 30000: the slow form of the kept-map route (the row's image does not fit LDS)
N_COLS = 41


def shared_x(M, K, cols, seed):
    """The same values as fp16 (numpy, for the oracle) and on the device as fp16 and bf16: every value is 0 or in fp16's normal range and has
    at most 8 significand bits, so both containers hold it exactly (tests/test_gpu_bf16.py::_pair)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 1.5
    x[:, cols] *= 25
    xb = x.bfloat16()
    xb[xb.abs() < 2.0 ** -14] = 0
    xh = xb.half()
    assert torch.equal(xh.bfloat16().view(torch.int16), xb.view(torch.int16))
    return xh.numpy().copy(), {F16: xh.to(DEV), BF: xb.to(DEV)}


def live_bytes(M, K, bit, qfmt):
    """Which bytes of a packed [roundup(M,16), row bytes] activation image belong to rows < M: the image of an all-ones-bits matrix (int8 -1 /
    nibble -1, whose FP6 code 0x2c leaves no zero byte in the bit stream) packed by mixq_pack_operand, which zero-fills rows >= M."""
    KB = K if bit == 8 else K // 2
    ones = torch.full((M, KB), 0xFF, dtype=torch.uint8, device=DEV)
    return mixlib.PackOperand(ones, qfmt).reshape(-1) != 0


class QuantFrames:
    """Frames around everything a quantise pass writes: x (in place, ldx > K), x_scale (M live entries), the q image, x_out [M, ldo]."""

    def __init__(self, x, M, K, bit, qfmt, ldo, dtype):
        self.M, self.K, self.bit, self.qfmt = M, K, bit, qfmt
        self.fx = framed(x, K + 64)
        self.fs = Frame(1, M, M + 64, 0, 0, F16, DEV, 2)
        self.rows = mixlib.packed_rows(M) if qfmt else M
        self.rb = mixlib._q_row_bytes(K, bit, qfmt)
        self.fq = Frame(1, self.rows * self.rb, self.rows * self.rb, 0, 0, torch.uint8, DEV, 2)
        self.fo = Frame(M, ldo, ldo, 0, 0, dtype, DEV, GUARD_ROWS) if ldo else None       # (columns n .. ldo-1 are written with zeros: part of the window)
        self.flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def check(self, what, q_ref, s_ref, x_ref, xo_ref, n_cols, x_written=True):
        """Byte equality with the oracle, and the header's promises about the frame."""
        M, K, bit, qfmt = self.M, self.K, self.bit, self.qfmt
        for name, f in (("x", self.fx), ("x_scale", self.fs), ("q", self.fq)) + ((("x_out", self.fo),) if self.fo is not None else ()):
            f.assert_untouched(f"{what}: {name}")
        KB = K if bit == 8 else K // 2
        img = self.fq.view[0]
        if qfmt == FMT_PLAIN:
            plain = img.reshape(M, KB)
        else:
            live = live_bytes(M, K, bit, qfmt)
            assert torch.equal(img[~live], self.fq.saved_view()[0][~live]), f"{what}: rows >= M of the packed image were written"
            plain = torch.empty((M, KB), dtype=torch.uint8, device=DEV)
            _capi.call("mixq_unpack_operand", img.contiguous().data_ptr(), plain.data_ptr(), M, KB, qfmt, mixlib._stream())
        assert np.array_equal(n(plain), q_ref.view(np.uint8).reshape(M, KB)), f"{what}: q"
        assert np.array_equal(n(self.fs.view[0]).view(np.uint16), s_ref.view(np.uint16).reshape(-1)), f"{what}: x_scale"
        # x: only the outlier columns of the live rows changed (to zero) - or nothing at all (x_written = False: the pass reads x only)
        got_x = n(self.fx.view.float())
        assert np.array_equal(got_x, x_ref.astype(np.float32)), f"{what}: x"
        if not x_written:
            self.fx.assert_unchanged(f"{what}: x is not modified")
        if self.fo is not None:
            assert np.array_equal(n(self.fo.view[:, :n_cols].float()), xo_ref.astype(np.float32)), f"{what}: x_out"
            assert int(ibits(self.fo.view[:, n_cols:]).abs().max()) == 0, f"{what}: x_out columns n .. ldo-1 are zeros"


def _cols(K, seed):
    return sorted(torch.randperm(K, generator=torch.Generator().manual_seed(seed))[:N_COLS].tolist())


@pytest.mark.parametrize("dtype", [F16, BF])
@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("M,K", QUANT_SHAPES)
def test_quantise_passes_write_inside_their_frames(M, K, bit, dtype):
    """mixq_find_row_scale, mixq_quant_fused, mixq_quant_fused_masked, mixq_quant_known_amax and mixq_extract_outliers_zero (and their bf16
    twins) into every q format, with ldx > K and ldo in {pad16(n), pad16(n) + 16}: the oracle's bytes, and nothing outside the windows."""
    sfx = "" if dtype == F16 else "_bf16"
    cols = _cols(K, M + K)
    x_np, x_dev = shared_x(M, K, cols, seed=M + K + bit)
    x = x_dev[dtype]
    ind_np = np.array(cols, np.int32)
    ind = t(ind_np)
    cm = kept_outlier_map(ind, K)
    kept = Kept(ind=ind, col_mask=cm)
    st = mixlib._stream()
    # references (the oracle runs on the fp16 values, which both containers hold exactly)
    q0, s0 = O.find_row_scale(x_np, bit)
    xz = x_np.copy()
    xo_ref = O.extract_outliers_zero(xz, ind_np)
    q1, s1 = O.find_row_scale(xz, bit)
    for ldo in (pad16(N_COLS), pad16(N_COLS) + 16):
        # mixq_extract_outliers_zero
        fx = framed(x, K + 64)
        fo = Frame(M, ldo, ldo, 0, 0, dtype, DEV, GUARD_ROWS)
        _capi.call("mixq_extract_outliers_zero" + sfx, fx.view.data_ptr(), ind.data_ptr(), N_COLS, fo.view.data_ptr(), M, K, K + 64, ldo, st)
        w = f"mixq_extract_outliers_zero{sfx} {M}x{K} ldo={ldo}"
        fx.assert_untouched(f"{w}: x")
        fo.assert_untouched(f"{w}: x_out")
        assert np.array_equal(n(fx.view.float()), xz.astype(np.float32)), f"{w}: x"
        assert np.array_equal(n(fo.view[:, :N_COLS].float()), xo_ref.astype(np.float32)), f"{w}: x_out"
        assert int(ibits(fo.view[:, N_COLS:]).abs().max()) == 0, f"{w}: x_out columns n .. ldo-1 are zeros"
        for qfmt in QFMTS[bit]:
            # mixq_find_row_scale: reads x only
            b = QuantFrames(x, M, K, bit, qfmt, 0, dtype)
            _capi.call("mixq_find_row_scale" + sfx, b.fx.view.data_ptr(), b.fs.view.data_ptr(), b.fq.view.data_ptr(), M, K, K + 64, bit, qfmt, st)
            b.check(f"mixq_find_row_scale{sfx} {M}x{K} W{bit} fmt {qfmt}", q0, s0, x_np, None, 0, x_written=False)
            for entry in ("mixq_quant_fused", "mixq_quant_fused_masked", "mixq_quant_known_amax"):
                b = QuantFrames(x, M, K, bit, qfmt, ldo, dtype)
                head = (b.fx.view.data_ptr(), ind.data_ptr(), N_COLS, None)
                tail = (b.fs.view.data_ptr(), b.fq.view.data_ptr(), b.fo.view.data_ptr(), b.flag.data_ptr(), M, K, K + 64, ldo, bit, 6.0, qfmt, st)
                w = f"{entry}{sfx} {M}x{K} W{bit} fmt {qfmt} ldo={ldo}"
                if entry == "mixq_quant_fused":
                    _capi.call(entry + sfx, *head, *tail)
                elif entry == "mixq_quant_fused_masked":
                    _capi.call(entry + sfx, *head, cm.data_ptr(), cm.numel(), *tail)
                else:
                    fa = Frame(1, M, M + 64, 0, 0, torch.int32, DEV, 2)
                    bits_ = ibits(x).int() & 0x7FFF
                    bits_[:, cols] = 0
                    fa.view[0] = bits_.max(dim=1).values.to(torch.int32)
                    _capi.call(entry + sfx, *head, fa.view.data_ptr(), cm.data_ptr(), cm.numel(), *tail)
                    fa.assert_untouched(f"{w}: row_amax")
                    assert int(fa.view.abs().max()) == 0, f"{w}: row_amax is cleared"
                b.check(w, q1, s1, xz, xo_ref, N_COLS)
                assert bool(b.flag.item()) == O.mispredicted(s1, 6.0, bit), f"{w}: flag"
                kept.unchanged(w)


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("M,K", QUANT_SHAPES)
def test_rmsnorm_family_writes_inside_its_frames_and_leaves_x_alone(M, K, bit):
    """mixq_rmsnorm, mixq_rmsnorm_quant_fused and its masked form with ldx > K, ldout > K and ldxo in {pad16(n), pad16(n) + 16}."""
    cols = _cols(K, M + K + 1)
    rng = np.random.default_rng(M + K)
    x_np = make_x(M, K, seed=M + K, outlier_cols=cols)
    w_np = (rng.random(K) + 0.5).astype(np.float16)
    ind_np = np.array(cols, np.int32)
    x, wt, ind = t(x_np), t(w_np), t(ind_np)
    cm = kept_outlier_map(ind, K)
    kept = Kept(weight=wt, ind=ind, col_mask=cm)
    st = mixlib._stream()
    fx = framed(x, K + 64)
    fout = Frame(M, K, K + 8, 0, 0, F16, DEV, GUARD_ROWS)
    _capi.call("mixq_rmsnorm", fx.view.data_ptr(), wt.data_ptr(), fout.view.data_ptr(), M, K, K + 64, K + 8, 1e-5, st)
    fout.assert_untouched(f"mixq_rmsnorm {M}x{K}: out")
    fx.assert_unchanged(f"mixq_rmsnorm {M}x{K}: x is not modified")
    assert np.array_equal(n(fout.view).view(np.uint16), O.rmsnorm(x_np, w_np, 1e-5).view(np.uint16))
    y_ref, xo_ref, q_ref, s_ref = O.rmsnorm_quant(x_np, w_np, 1e-5, ind_np, bit)
    for ldxo in (pad16(N_COLS), pad16(N_COLS) + 16):
        for qfmt in QFMTS[bit]:
            for masked in (False, True):
                b = QuantFrames(x, M, K, bit, qfmt, ldxo, F16)
                fout = Frame(M, K, K + 8, 0, 0, F16, DEV, GUARD_ROWS)
                w = f"mixq_rmsnorm_quant_fused{'_masked' if masked else ''} {M}x{K} W{bit} fmt {qfmt} ldxo={ldxo}"
                head = (b.fx.view.data_ptr(), wt.data_ptr(), fout.view.data_ptr(), ind.data_ptr(), N_COLS, None)
                tail = (b.fs.view.data_ptr(), b.fq.view.data_ptr(), b.fo.view.data_ptr(), b.flag.data_ptr(), M, K, K + 64, K + 8, ldxo, 1e-5, bit, 6.0, qfmt, st)
                if masked:
                    _capi.call("mixq_rmsnorm_quant_fused_masked", *head, cm.data_ptr(), cm.numel(), *tail)
                else:
                    _capi.call("mixq_rmsnorm_quant_fused", *head, *tail)
                fout.assert_untouched(f"{w}: out")
                assert np.array_equal(n(fout.view).view(np.uint16), y_ref.view(np.uint16)), f"{w}: out"
                b.check(w, q_ref, s_ref, x_np, xo_ref, N_COLS, x_written=False)
                kept.unchanged(w)


@pytest.mark.parametrize("bit", [8, 4])
def test_dequant_weight_cols_writes_columns_0_to_n_only(bit):
    N, K = 200, 512
    rng = np.random.default_rng(N + bit)
    wq = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
    ind_np = np.sort(rng.choice(K, N_COLS, replace=False)).astype(np.int32)
    if bit == 8:
        qw, sw = O.quant_weight_w8(wq)
    else:
        qw, sw, _ = O.quant_weight_w4(wq, np.zeros(0, np.int32))
    ref = O.dequant_weight_cols(qw, sw, ind_np, bit)
    q_dev, s_dev, ind = t(qw), t(sw), t(ind_np)
    kept = Kept(qw=q_dev, sw=s_dev, ind=ind)
    for ldo in (pad16(N_COLS), pad16(N_COLS) + 16, N_COLS + 3):
        f = Frame(N, N_COLS, ldo, 0, 0, F16, DEV, GUARD_ROWS)                   # columns n .. ldo-1 are guard: the header writes columns 0 .. n-1 only
        _capi.call("mixq_dequant_weight_cols", q_dev.data_ptr(), s_dev.data_ptr(), ind.data_ptr(), N_COLS, f.view.data_ptr(), N, K, ldo, bit, mixlib._stream())
        f.assert_untouched(f"mixq_dequant_weight_cols W{bit} ldo={ldo}")
        assert np.array_equal(n(f.view).view(np.uint16), np.ascontiguousarray(ref).view(np.uint16)), ldo
        kept.unchanged(f"mixq_dequant_weight_cols W{bit} ldo={ldo}")


# ---- 4. operator level: a column slice of a wider activation buffer -----------------------------------------------------------------------
@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("dtype", [F16, BF])
def test_layer_on_a_column_slice_of_a_wide_buffer(dtype, bit):
    """MixLinear_GEMM fed wide[:, off : off + K] (stride(0) % 8 == 0) through the search phase, the frozen one-call route and a graph replay:
    the outputs equal those for a contiguous clone of the same values byte for byte, and in `wide` nothing outside the outlier columns of
    the slice changes (the reference zeroes those in place)."""
    M, K, N, off, ldw = 192, 512, 256, 72, 1024
    cols1, col2 = [3, 200, 411], 77
    big = 6.0e4 if dtype == BF else 40.0
    from test_gpu_bf16_gemm import _make_x

    def make_layer():
        torch.manual_seed(11)
        lin = torch.nn.Linear(K, N, bias=True).to(dtype)
        cache = MixLibCache(M, bit=bit, device=DEV, config=MixqConfig(act_dtype=dtype))
        kw = {}
        if bit == 4:
            rest = [c for c in torch.randperm(K, generator=torch.Generator().manual_seed(2)).tolist() if c not in cols1 + [col2]]
            ls = torch.ones(K)
            ls[cols1 + rest[:128 - len(cols1)]] = 20.0
            kw["layer_scales"] = ls
        return MixLinear_GEMM.from_linear(lin, bit, cache=cache, dev=DEV, **kw)

    xs = [_make_x(M, K, cols1, 1, big), _make_x(M, K, cols1 + [col2], 2, big), _make_x(M, K, cols1 + [col2], 3, big), _make_x(M, K, cols1 + [col2], 4, big)]
    xs = [v.to(dtype).to(DEV) for v in xs]
    sliced, plain = make_layer(), make_layer()

    def in_wide(x):
        f = Frame(M, K, ldw, off, 0, dtype, DEV, 8)
        f.view.copy_(x)
        return f.freeze()

    def check_wide(f, x, layer, what):
        f.assert_untouched(f"{what}: wide")
        want = x.clone()
        want[:, layer.ind.long()] = 0
        assert same_bytes(f.view, want), f"{what}: the slice changed outside its outlier columns"

    for call in range(3):                                                      # the search phase (a new outlier column at call 1), then frozen
        f = in_wide(xs[call])
        assert f.view.stride(0) % 8 == 0 and not f.view.is_contiguous()
        y_s = sliced(f.view, None, True)
        y_p = plain(xs[call].clone(), None, True)
        torch.cuda.synchronize()
        assert same_bytes(y_s, y_p), f"call {call}"
        assert torch.equal(sliced.ind, plain.ind)
        check_wide(f, xs[call], sliced, f"call {call}")
    assert sliced.add_outliers is False and plain.add_outliers is False
    for one_call in (False, True):
        sliced.config.one_call_forward = plain.config.one_call_forward = one_call
        f = in_wide(xs[3])
        y_s = sliced(f.view, None, True)
        y_p = plain(xs[3].clone(), None, True)
        torch.cuda.synchronize()
        assert same_bytes(y_s, y_p), f"frozen one_call={one_call}"
        check_wide(f, xs[3], sliced, f"frozen one_call={one_call}")
    y_frozen = y_p.clone()
    # hipGraph: captured once on a side stream on the slice, replayed on restored inputs
    f = in_wide(xs[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sliced(f.view, None, True)
        f.view.copy_(xs[3])
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            yg = sliced(f.view, None, True)
        for _ in range(3):
            f.view.copy_(xs[3])
            yg.zero_()
            g.replay()
            side.synchronize()
            assert same_bytes(yg, y_frozen)
            check_wide(f, xs[3], sliced, "graph replay")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    del g
