"""The joint gate / up launch in bfloat16 on the MI355X (ABI 1.5: mixq_gemm_i8_pair_bf16 / mixq_gemm_i4_pair_bf16, the nine kernels of
gemm_wreg_bf16_pair.hip).

The contract (include/mixq_hip.h, "bf16 joint gate / up launch") is the two-launch route's operations from one launch:
    z     = float(acc) * sx[m] * sw[n] + sum_j xo[m,j] * wo[n,j]
    up16  = RNE_bf16(z_up + bias_up)
    y     = RNE_bf16((silu(z_gate) + bias_gate) * float(up16))
so every test's first expectation is BYTES: up_proj's launch followed by gate_proj's MIXQ_ACT_SILU_MUL launch through the `_bf16` entry
points on the de-interleaved operands.  Beside that: the float64 bound of tests/test_gpu_bf16_gemm.py (imported, not restated), guard
frames around y on the staged and both unstaged store paths, an exact problem whose float64 expectation holds bit for bit, the row-maximum
side output, and norm -> MixLlamaMLP(residual=) with `MixqConfig.joint_gate_up_bf16` on against the same block with it off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact as E  # noqa: E402
from frames import Frame  # noqa: E402
from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib  # noqa: E402
from mixq_amd._capi import ACT_NONE, ACT_SILU_MUL, ACT_SILU_PAIR, FMT_F16X64, FMT_F6X128, FMT_P16X64, FMT_R6X128  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402
from mixq_amd.fused import FasterTransformerRMSNorm, MixLlamaMLP, interleave_pair_rows  # noqa: E402
from mixq_amd.linear import kept_outlier_map  # noqa: E402
from test_gpu_bf16_gemm import check, pack_i4, reference  # noqa: E402  (the float64 restatement and bound of the bf16 GEMM tests)

DEV = "cuda"
BF, F16, F64 = torch.bfloat16, torch.float16, torch.float64
NAN_BITS = 0x7FC1                                          # a NaN in bf16: what the pad columns of x_out / w_out hold
# the tilings with the paired epilogue's bf16 form (gemm_wreg.hip's g_wr rows 0, 5, 7, 8, 14; 128 x 256 is int8 only)
PAIR_INT8 = ["wr128x192_s16_d4_l2", "wr128x256_s16_d3_l2", "wr64x192_s16_d4_l2", "wr64x256_s16_d4_l2", "wr32x64_s8_d6_l1"]
PAIR_FP6 = [n for n in PAIR_INT8 if n != "wr128x256_s16_d3_l2"]
SMALL = "wr32x64_s8_d6_l1"
# (outlier columns as passed, live count in device memory or None): none; 17 columns of capacity (32 with the pad) of which a device-resident
# count keeps 9 - columns 9 .. 16 hold finite values that must be ignored, 17 .. 31 NaN patterns; 41, a second tail k-step
CASES = {"n0": (0, None), "n17_dev9": (17, 9), "n41": (41, None)}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    _capi.load().mixq_gemm_set_config(-1)
    yield
    _capi.load().mixq_gemm_set_config(-1)


def forced(names):
    """Iterate over tilings, each forced through mixq_gemm_set_config while the body runs ("auto": the automatic pick); automatic afterwards."""
    lib, table = _capi.load(), _capi.gemm_config_names()
    try:
        for name in names:
            assert lib.mixq_gemm_set_config(-1 if name == "auto" else table.index(name)) == 0
            yield name
    finally:
        assert lib.mixq_gemm_set_config(-1) == 0


def bits(t):
    return t.contiguous().view(torch.int16)


def pad16(v):
    return (v + 15) // 16 * 16


class PairProblem:
    """up_proj and gate_proj of one block ([N, K] each) over one quantised activation: the two layers' own images and operands, the
    interleaved ones, the exact contractions, and - made once, with the automatic pick, and left unchanged - the two-launch route's bytes
    with their float64 reference and bound for every (case, bias)."""

    def __init__(self, bit, M, K, N, seed):
        g = torch.Generator().manual_seed(seed)
        self.bit, self.M, self.K, self.N = bit, M, K, N
        lim = 127 if bit == 8 else 7
        qx = torch.randint(-lim, lim + 1, (M, K), generator=g, dtype=torch.int16)
        qw = {w: torch.randint(-lim - (bit == 4), lim + 1, (N, K), generator=g, dtype=torch.int16) for w in ("up", "gate")}
        xf, wf = (FMT_P16X64, FMT_F16X64) if bit == 8 else (FMT_R6X128, FMT_F6X128)
        plain = (lambda q: q.to(torch.int8).to(DEV)) if bit == 8 else (lambda q: pack_i4(q).to(DEV))
        self.qx_img = mixlib.PackOperand(plain(qx), xf)
        self.w_img = {w: mixlib.PackOperand(plain(qw[w]), wf) for w in qw}
        self.w_img["joint"] = mixlib.PackOperand(interleave_pair_rows(plain(qw["up"]), plain(qw["gate"])), wf)
        self.acc = {w: qx.to(DEV).to(F64) @ qw[w].to(DEV).to(F64).T for w in qw}
        amp = 0.02 if bit == 8 else 0.3
        self.sx = ((torch.rand(M, 1, generator=g) + 0.5) * amp).half().to(DEV)
        self.sw = {w: ((torch.rand(1, N, generator=g) + 0.5) * amp * (0.2 if w == "gate" else 1.0)).half().to(DEV) for w in qw}
        self.bias = {w: (torch.randn(N, generator=g) * 3).half().to(DEV) for w in qw}
        self.sw["joint"] = interleave_pair_rows(self.sw["up"].reshape(-1), self.sw["gate"].reshape(-1)).reshape(1, -1)
        self.bias["joint"] = interleave_pair_rows(self.bias["up"], self.bias["gate"])
        # outlier operands: activation columns up to ~1e5 (fp16 cannot hold them), weights of ordinary size
        self.xo_vals = (torch.randn(M, 48, generator=g) * torch.logspace(1, 5, 48)[torch.randperm(48, generator=g)]).to(BF).to(DEV)
        self.wo_vals = {w: (torch.randn(N, 48, generator=g) * 0.05 * (0.02 if w == "gate" else 1.0)).to(BF).to(DEV) for w in qw}
        self.wo_vals["joint"] = interleave_pair_rows(self.wo_vals["up"], self.wo_vals["gate"])
        self._o = {}
        assert _capi.load().mixq_gemm_set_config(-1) == 0
        self.want = {(c, b): self._two_launches(c, b) for c in CASES for b in (False, True)}
        torch.cuda.synchronize()

    def outliers(self, which, case):
        """(x_out, w_out, n_out argument, device count tensor): [rows, pad16(n)] holding n columns and NaN patterns in the pad; with a device
        count the argument is the capacity."""
        key = (which, case)
        if key not in self._o:
            n, live = CASES[case]
            if n == 0:
                self._o[key] = (None, None, 0, None)
            else:
                out = []
                for vals in (self.xo_vals, self.wo_vals[which]):
                    t = torch.full((vals.shape[0], pad16(n)), NAN_BITS, dtype=torch.int16, device=DEV).view(BF)
                    t[:, :n] = vals[:, :n]
                    out.append(t)
                n_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
                self._o[key] = (out[0], out[1], pad16(n) if live is not None else n, n_dev)
        return self._o[key]

    def launch(self, which, case, bias, act, addend=None, **kw):
        xo, wo, n_arg, n_dev = self.outliers(which, case)
        rows = 2 * self.N if which == "joint" else self.N
        return mixlib.FusedLinear(self.qx_img, self.w_img[which], self.sx, self.sw[which], xo, wo, n_arg, self.bias[which] if bias else None, self.M, rows,
                                  self.K, bit=self.bit, act=act, n_out_dev=n_dev, addend=addend, dtype=BF, **kw)

    def _two_launches(self, case, bias):
        """(bits of y, float64 reference, bound): up_proj's launch, gate_proj's MIXQ_ACT_SILU_MUL launch on that tensor - each within the
        bf16 GEMM tests' float64 bound over the operands it read."""
        n, live = CASES[case]
        n_live = n if live is None else live
        up = self.launch("up", case, bias, ACT_NONE)
        xo, wo_u, _, _ = self.outliers("up", case)
        ref, bound = reference(self.acc["up"], self.sx, self.sw["up"], xo, wo_u, n_live, None, self.bias["up"] if bias else None, ACT_NONE)
        check(up, ref, bound, f"two launches, up_proj {case} bias={bias}")
        y = self.launch("gate", case, bias, ACT_SILU_MUL, addend=up)
        _, wo_g, _, _ = self.outliers("gate", case)
        ref, bound = reference(self.acc["gate"], self.sx, self.sw["gate"], xo, wo_g, n_live, up, self.bias["gate"] if bias else None, ACT_SILU_MUL)
        check(y, ref, bound, f"two launches, gate_proj {case} bias={bias}")
        return bits(y).clone(), ref, bound


_problems = {}


def problem(bit, M, K=512, N=584):
    key = (bit, M, K, N)
    if key not in _problems:
        _problems[key] = PairProblem(bit, M, K, N, seed=77 * bit + M + N)
    return _problems[key]


# ---- 1. every form forced, and the automatic pick: the two launches' bytes, the float64 bound, nothing outside the window ----------------
def layouts(N):
    """(ld, col_off, elem_off) of y: staged; unstaged by ldy % 8 != 0; unstaged by a base offset of 8 bytes."""
    return [(N, 0, 0), (N + 4, 0, 0), (N + 8, 0, 4)]


@pytest.mark.parametrize("bit,name", [(8, n) for n in ["auto"] + PAIR_INT8] + [(4, n) for n in ["auto"] + PAIR_FP6])
def test_each_paired_bf16_form_equals_the_two_launches(bit, name):
    """200 x 512 -> 2 x 584 (24 rows too for the 32 x 64 tiling and the pick): a partial last M tile and, 584 = 8 x 73 not being a multiple
    of any tile's output width, a partial last N tile for every tiling."""
    launches = 0
    for M in ((200, 24) if name in ("auto", SMALL) else (200,)):
        p = problem(bit, M)
        N = p.N
        frames = [Frame(M, N, ld, co, eo, BF, DEV) for ld, co, eo in layouts(N)]
        assert [(f.view.stride(0) % 8, f.view.data_ptr() % 16) for f in frames] == [(0, 0), (4, 0), (0, 8)]
        for _ in forced([name]):
            for case in CASES:
                for bias in (False, True):
                    want, ref, bound = p.want[(case, bias)]
                    for f in frames:
                        what = f"W{bit} pair bf16 {name} {M}x{p.K}->2x{N} {case} bias={bias} ld={f.ld} offset={f.elem_off}"
                        f.reset()
                        out = p.launch("joint", case, bias, ACT_SILU_PAIR, out=f.view)
                        assert out is f.view
                        f.assert_untouched(what)
                        y = f.view.contiguous()
                        assert torch.equal(bits(y), want), f"{what}: y differs from the two launches in {int((bits(y) != want).sum())} of {y.numel()} elements"
                        check(y, ref, bound, what)
                        launches += 1
    torch.cuda.synchronize()
    assert launches == 18 * (2 if name in ("auto", SMALL) else 1)


def test_the_library_answers_for_these_problems():
    q = _capi.load().mixq_gemm_pair_supported_bf16
    assert q(200, 2 * 584, 512, 8, _capi.X_PACKED | _capi.W_F16X64) == 1 and q(24, 2 * 584, 512, 4, _capi.XW_F6X128) == 1
    p = problem(8, 200)
    with pytest.raises(RuntimeError, match="no addend"):
        p.launch("joint", "n0", False, ACT_SILU_PAIR, addend=torch.zeros(200, 584, dtype=BF, device=DEV))
    for _ in forced(["wr128x128_s16_d4_l2"]):              # a tiling with a bf16 form but no paired one: refused, nothing written
        f = Frame(200, 584, 584, 0, 0, BF, DEV)
        with pytest.raises(_capi.MixqError) as e:
            p.launch("joint", "n0", False, ACT_SILU_PAIR, out=f.view)
        assert e.value.code == _capi.MIXQ_EINVAL
        torch.cuda.synchronize()
        f.assert_unchanged("a forced tiling without the paired bf16 form")


# ---- 2. exact operands: the float64 expectation bit for bit --------------------------------------------------------------------------
def poisoned(vals, n, dtype=E.BF16):
    t = torch.full((vals.shape[0], pad16(n)), NAN_BITS, dtype=torch.int16).view(E.torch_dtype(dtype))
    if n:
        t[:, :n] = E.as_tensor(vals[:, :n], dtype)
    return t.to(DEV)


def exact_bias_gate(N):
    """fp16 values +-(1 + k / 8) 2^-e, e in 0 .. 3: four significand bits, magnitudes in [1/8, 2) - a product with a bf16 value is exact in fp32
    (12 bits) and stays far inside its range at both ends of the wide problem (2^+-80)."""
    n = np.arange(N)
    return (1.0 + (n % 8) / 8.0) * np.exp2(-(n % 4).astype(np.float64)) * np.where(n % 3 == 0, -1.0, 1.0)


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("kind", ["main", "wide"])
def test_exact_operands_match_the_float64_expectation_bit_for_bit(kind, bit):
    """The scheme of test_gpu_exact.py's fp16 pair case, mirrored: there the up half is held constant and SiLU is swept under its derived
    bound; here the GATE half is neutralised - zero weights and zero outlier weights, so z_gate = +0, mixq_silu(0) = 0 * rcp(2) = 0 exactly
    and silu + bias_gate = bias_gate, a constant per column - and the UP half is an exact problem of tests/exact.py in bf16 (every partial
    sum exact in fp32: up16 = RNE_bf16(z_up + bias_up) with no other rounding).  (bias_gate) * float(up16) is a 12-bit product, exact in
    fp32, and the one rounding left is the last:
        y = RNE_bf16( bias_gate[n] * RNE_bf16(z_up[m, n] + bias_up[n]) )                in float64, no tolerance.
    So a kernel that skipped up's intermediate rounding, rounded either step toward zero or took the product in 16 bits cannot pass.
    `main`: outlier counts 0, 1, 17, 33 and 41 (the 16-column pad, a second tail k-step), bias_up on and off; `wide`: the bf16 range edges -
    tail operands at 2^+-40, outputs from 2^-80 to 2^80, bias_up = 0 (fp16 cannot follow the range).  Where the exact z_up is 0 either
    zero sign passes, as everywhere in tests/exact.py."""
    N, K = 136, E.K_MAIN                                    # 2 N = 272: a partial tile for every tiling; y is staged (N % 8 == 0)
    bg = exact_bias_gate(N)
    assert E.representable(bg, E.F16)
    names = ["auto"] + (PAIR_INT8 if bit == 8 else PAIR_FP6)
    for M in E.M_SHAPES:
        p = E.problem(kind, bit, E.BF16, M, N)
        qx, qw = p.q_plain()
        xf, wf = (FMT_P16X64, FMT_F16X64) if bit == 8 else (FMT_R6X128, FMT_F6X128)
        qx_img = mixlib.PackOperand(qx.to(DEV), xf)
        qw_img = mixlib.PackOperand(interleave_pair_rows(qw, torch.zeros_like(qw)).to(DEV), wf)
        sx = torch.from_numpy(p.sx.copy()).reshape(-1, 1).to(DEV)
        sw = interleave_pair_rows(torch.from_numpy(p.sw.copy()), torch.ones(N, dtype=F16)).reshape(1, -1).to(DEV)
        bias = interleave_pair_rows(torch.from_numpy(p.bias.copy()), E.as_tensor(bg, E.F16)).to(DEV)
        bias_off = interleave_pair_rows(torch.zeros(N, dtype=F16), E.as_tensor(bg, E.F16)).to(DEV)
        combos = [(n, b) for n in (0, 1, 17, 33, 41) for b in (False, True)] if kind == "main" else [(E.EDGE_N_OUT, False), (1, False)]
        for n_out, with_bias in combos:
            up_bits, z_up = p.expected(n_out, None, with_bias)
            up16 = E.from_bits(up_bits, E.BF16)
            assert np.isfinite(up16).all()
            z = up16 * bg[None, :]
            want = E.to_bits(z, E.BF16)
            assert not ((z_up != 0) & (up16 == 0)).any()    # (up16 = +-0 only where z_up cancels exactly: that sign is free, and z == 0 there)
            xo = poisoned(p.xo, n_out)
            wo = torch.full((2 * N, pad16(n_out)), NAN_BITS, dtype=torch.int16, device=DEV).view(BF)
            if n_out:
                wo[:, :n_out] = interleave_pair_rows(E.as_tensor(p.wo[:, :n_out], E.BF16), torch.zeros(N, n_out, dtype=BF)).to(DEV)
            for name in forced(names):
                y = mixlib.FusedLinear(qx_img, qw_img, sx, sw, xo if n_out else None, wo if n_out else None, n_out, bias if with_bias else bias_off, M, 2 * N, K,
                                       bit=bit, act=ACT_SILU_PAIR, dtype=BF)
                assert tuple(y.shape) == (M, N)
                E.assert_exact(y.view(torch.int16).cpu().numpy().view(np.uint16), want, z, E.BF16, f"{p.name} pair {name} n_out={n_out} bias_up={with_bias}")
    assert (np.abs(E.from_bits(want, E.BF16)) > 0).mean() > 0.5     # (the last expectation is not a field of zeros)


@pytest.mark.parametrize("bit", [8, 4])
def test_silu_in_the_paired_bf16_form_over_signs_significands_and_exponents(bit):
    """test_gpu_exact.py's fp16 pair case with the container swapped: the up rows have a zero main term and a zero tail, so up16 =
    RNE_bf16(0 + bias_up) = bias_up, a constant per column that bf16 holds exactly; z_gate arrives through one outlier column, exact in fp32,
    over 124 significands x both signs x 32 exponents; y = (silu(z_gate) + bias_gate) * bias_up within the bound derived from the
    instructions mixq_silu issues (exact.silu_reference, bf16)."""
    xo_np, wo_np, z, mul_np = E.silu_mul_operands(E.BF16)
    rows, N = 248, 256
    bias_u, bias_g = mul_np[0], E.silu_bias_vector(N)
    K = 64 if bit == 8 else 128
    lim = 127 if bit == 8 else 7
    rng = np.random.default_rng(bit)
    qx, qw2 = np.zeros((rows, K), np.int8), rng.integers(-lim, lim + 1, (2 * N, K)).astype(np.int8)
    qx, qw2 = (torch.from_numpy(qx), torch.from_numpy(qw2)) if bit == 8 else (torch.from_numpy(E.pack_i4(qx)), torch.from_numpy(E.pack_i4(qw2)))
    xf, wf = (FMT_P16X64, FMT_F16X64) if bit == 8 else (FMT_R6X128, FMT_F6X128)
    qx, qw2 = mixlib.PackOperand(qx.to(DEV), xf), mixlib.PackOperand(qw2.to(DEV), wf)
    sx = torch.full((rows, 1), 0.125, dtype=F16, device=DEV)
    sw2 = torch.full((1, 2 * N), 0.125, dtype=F16, device=DEV)
    xo = poisoned(xo_np[:, None], 1)
    wo2 = poisoned(np.zeros((2 * N, 1)), 1)
    wo2[:, :1] = interleave_pair_rows(torch.zeros((N, 1), dtype=BF, device=DEV), E.as_tensor(wo_np[:, None], E.BF16).to(DEV))
    bias2 = interleave_pair_rows(E.as_tensor(bias_u, E.F16).to(DEV), E.as_tensor(bias_g, E.F16).to(DEV))
    ref, bound = E.silu_reference(z, bias_g[None, :], bias_u[None, :], E.BF16)
    for name in forced(["auto"] + (PAIR_INT8 if bit == 8 else PAIR_FP6)):
        y = mixlib.FusedLinear(qx, qw2, sx, sw2, xo, wo2, 1, bias2, rows, 2 * N, K, bit=bit, act=ACT_SILU_PAIR, dtype=BF)
        worst = E.silu_check(y.view(torch.int16).cpu().numpy().view(np.uint16), ref, bound, E.BF16, f"W{bit} {name} ACT_SILU_PAIR bf16")
        print(f"pair bf16 W{bit} {name}: SiLU sweep worst err / bound = {worst:.4f}")


# ---- 3. the row-maximum side output ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,masked", [(200, True), (200, False), (24, True)])
def test_row_amax_equals_the_two_launch_route_and_ignores_columns_past_the_output(M, masked):
    """row_amax of mixq_gemm_i8_pair_bf16 = the words mixq_gemm_i8_fused_amax_bf16(MIXQ_ACT_SILU_MUL) leaves on the two-launch route = the
    maximum of the bf16 bit patterns & 0x7fff of the y it wrote over the unmasked OUTPUT columns c < N / 2.  584 output columns end inside
    every tiling's last tile: its remaining physical columns (past the interleaved N) are computed from zero scales and count for nothing;
    col_mask is indexed by output column, so the up rows (odd pairs of the interleaved order) never reach it."""
    p = problem(8, M)
    N = p.N
    assert mixlib.amax_supported(M, 2 * N, p.K, FMT_P16X64, FMT_F16X64, dtype=BF)
    ind = torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(5))[:23])[0].to(torch.int32).to(DEV) if masked else None
    cm = kept_outlier_map(ind, N) if masked else None
    cm_saved = None if cm is None else cm.clone()
    case, bias = "n41", True
    up = p.launch("up", case, bias, ACT_NONE)
    ra2 = torch.zeros(M, dtype=torch.int32, device=DEV)
    y2 = p.launch("gate", case, bias, ACT_SILU_MUL, addend=up, row_amax=ra2, col_mask=cm)
    assert torch.equal(bits(y2), p.want[(case, bias)][0])
    b = bits(y2).int() & 0x7FFF
    if masked:
        b[:, ind.long()] = 0
    assert torch.equal(ra2, b.max(dim=1).values.to(torch.int32))
    assert int(ra2.min()) > 0
    for name in forced(["auto"] + PAIR_INT8):
        fa = Frame(1, M, M + 64, 0, 0, torch.int32, DEV, 2)
        fa.view.zero_()
        y = p.launch("joint", case, bias, ACT_SILU_PAIR, row_amax=fa.view[0], col_mask=cm)
        assert torch.equal(bits(y), bits(y2)), name
        assert torch.equal(fa.view[0], ra2), f"{name}: row_amax differs from the two-launch route's in {int((fa.view[0] != ra2).sum())} of {M} rows"
        fa.assert_untouched(f"{name}: row_amax past row M")
    if masked:
        assert torch.equal(cm, cm_saved)
    with pytest.raises(RuntimeError, match="int8"):          # the FP6 form has no row-maximum output, as in fp16
        problem(4, M).launch("joint", case, bias, ACT_SILU_PAIR, row_amax=torch.zeros(M, dtype=torch.int32, device=DEV))


# ---- 4. the modules: norm -> MixLlamaMLP(residual=) with the flag on = with the flag off --------------------------------------------------
EPS = 1e-5


def _make_x(M, K, cols, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 0.8
    for i, c in enumerate(cols):
        x[:, c] *= 60.0 / (1 + (i % 3))
    return x.to(dtype)


def run_block(dtype, bit, joint_bf16):
    """norm -> MixLlamaMLP(x, residual=r) at M = 48, 256 -> 512 -> 256 from fixed seeds: the search phase, the frozen state, one hipGraph
    replay.  Returns (bits of the frozen output, facts about the route, the graph)."""
    M, H, I = 48, 256, 512
    cols1, col2 = [3, 100, 200], 177
    boost = [5, 100, 300]                                   # up / gate output channels 12 times larger: down_proj's own outlier columns
    torch.manual_seed(5)
    cfg = MixqConfig(act_dtype=dtype, fused_bf16=(dtype == BF), joint_gate_up_bf16=joint_bf16)
    cache = MixLibCache(M, bit=bit, device=DEV, config=cfg)

    def make(k, n_, static):
        lin = torch.nn.Linear(k, n_, bias=True)
        if n_ == I:
            lin.weight.data[boost] *= 12.0
        kw = {}
        if bit == 4:                                         # 4-bit layers carry 128 static 16-bit columns
            rest = [c for c in torch.randperm(k, generator=torch.Generator().manual_seed(2)).tolist() if c not in static + [col2]]
            ls = torch.ones(k)
            ls[static + rest[:128 - len(static)]] = 20.0
            kw["layer_scales"] = ls
        return MixLinear_GEMM.from_linear(lin.to(dtype), bit, cache=cache, dev=DEV, **kw)
    up, gate, down = make(H, I, cols1), make(H, I, cols1), make(I, H, boost)
    wn = (torch.rand(H) + 0.5).to(dtype).to(DEV)
    norm = FasterTransformerRMSNorm(wn, EPS, cache)
    norm.next_layer = up
    mlp = MixLlamaMLP(gate, down, up, cache)
    r = (torch.randn(M, H, generator=torch.Generator().manual_seed(9)) * 3).to(dtype).to(DEV)
    xs = [_make_x(M, H, cols1 if i == 0 else cols1 + [col2], 20 + i, dtype).to(DEV) for i in range(4)]
    seen = {"joint_calls": 0, "handed_over": None, "applies": None}
    joint = mlp._forward_joint

    def joint_recorded(x, c):
        out = joint(x, c)
        seen["joint_calls"] += 1
        seen["handed_over"] = hasattr(out, "_mixq_row_amax")
        return out
    object.__setattr__(mlp, "_forward_joint", joint_recorded)

    def forward(x):
        hidden = norm(x)
        seen["applies"] = mlp._joint_applies(cache)         # (asked where forward() asks: the norm's q_xcache is in place)
        y = mlp(hidden, residual=r)
        torch.cuda.synchronize()
        return y

    for call in range(8):
        forward(xs[min(call, 3)].clone())
        if call >= 2 and not (up.add_outliers or down.add_outliers):
            break
    # (gate_proj runs through forward_without_preconditionFusedSilu, which follows up_proj's columns and keeps no search state of its own)
    assert not (up.add_outliers or down.add_outliers)
    assert col2 in up.ind.tolist() and torch.equal(gate.ind, up.ind) and int(down.ind.numel()) > 0
    for _ in range(3):                                      # (settles kept plans, gate_proj's take-over of the last column, the joint image, the hand-over buffer)
        forward(xs[3].clone())
    calls_before = seen["joint_calls"]
    y_on = forward(xs[3].clone())
    assert y_on.dtype == dtype and tuple(y_on.shape) == (M, H) and bool(torch.isfinite(y_on.float()).all())
    facts = dict(applies=seen["applies"], image=mlp._joint is not None, ran_joint=seen["joint_calls"] > calls_before, handed_over=seen["handed_over"],
                 wo_dtype=None if mlp._joint is None or mlp._joint["wo"] is None else mlp._joint["wo"].dtype)
    object.__setattr__(mlp, "_forward_joint", joint)
    # one hipGraph: a single linear chain on a side stream, replayed on restored inputs
    xg, x3 = xs[3].clone(), xs[3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mlp(norm(xg), residual=r)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            yg = mlp(norm(xg), residual=r)
        xg.copy_(x3)
        yg.zero_()
        g.replay()
        side.synchronize()
        assert torch.equal(yg.view(torch.int16), y_on.view(torch.int16)), "hipGraph replay"
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return y_on.view(torch.int16).clone(), facts, g


@pytest.mark.parametrize("bit", [8, 4])
def test_mlp_block_with_the_joint_bf16_launch_equals_the_two_launch_block(bit):
    before, f16_facts, g0 = run_block(F16, bit, False)
    off, off_facts, g1 = run_block(BF, bit, False)
    on, on_facts, g2 = run_block(BF, bit, True)
    after, _, g3 = run_block(F16, bit, False)
    # the flag off: the two launches, no joint image (pinned); the flag on: the joint route after the freeze, on an image of its own
    assert off_facts["applies"] is False and not off_facts["image"] and not off_facts["ran_joint"], off_facts
    assert on_facts["applies"] is True and on_facts["image"] and on_facts["ran_joint"], on_facts
    assert on_facts["wo_dtype"] == BF                       # the tail's weight operand: the bf16 image of the interleaved weight_cache
    assert on_facts["handed_over"] == (bit == 8), on_facts  # down_proj's row maxima leave the joint launch (int8 layers only)
    assert torch.equal(on, off), f"W{bit}: the joint bf16 block differs from the two-launch block in {int((on != off).sum())} of {on.numel()} elements"
    assert f16_facts["applies"] is True and f16_facts["ran_joint"]      # (the fp16 block runs ITS joint route as ever ...)
    assert torch.equal(before, after)                       # ... and gives the bytes it gave before
    del g0, g1, g2, g3
