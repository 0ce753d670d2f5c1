"""tests/backend_oracle.py held to the kernels: the same operands through mixq_amd.mixlib on the MI355X and through the oracle backend on
the host, for float16 and bfloat16, W8 and W4 - so that what tests/test_operator_stateful.py runs on the CPU is what the GPU computes.

Bit for bit (the project proves these kernels exact elsewhere): FindRowScale(Packed), QuantFused with and without kept map and device
count, ExtractOutliersAndSetToZeros, DetectOutlierCols, layernorm_forward_cuda, RMSNormQuantFused (out, x_out, x_scale, q after unpacking,
the misprediction flag), ForwardPlan.run's q and x_out, and - on the exact operands of tests/exact.py, where the kernels' only rounding is
the last one - FusedLinear(ACT_NONE) and W8A16Linear with and without an addend.
Within bounds the project has already derived, no new tolerance: the SiLU forms and ACT_SILU_PAIR against exact.silu_reference (exact z:
the bound is mixq_silu's alone), W8A16Linear in bfloat16 on free operands against w8a16_bf16_ref.bound, ForwardPlan.run's y against
tests/test_gpu_bf16_gemm.py::reference (bfloat16) / the oracle within tests/test_gpu_parity.py::ulp_tol (float16), as
tests/test_gpu_residual.py does.  Kernel and oracle are each held to the same float64 reference; the worst ratio of each is printed.

Shapes, the smallest that reach every branch: M in {1, 16, 24}, K = 128 (8-bit) / 256 (4-bit: FP6 needs K % 128), N = 64, outlier counts
{0, 3, 17} - none, one padded k-step, a second k-step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import backend_oracle as B  # noqa: E402
import exact as E  # noqa: E402
import w8a16_bf16_ref as W  # noqa: E402
from mixq_amd import _capi, mixlib  # noqa: E402
from mixq_amd._capi import ACT_NONE, ACT_SILU, ACT_SILU_MUL, ACT_SILU_PAIR, FMT_F16X64, FMT_F6X128, FMT_P16X64, FMT_PLAIN, FMT_R6X128  # noqa: E402
from mixq_amd.linear import kept_outlier_map  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_gpu_bf16_gemm import check as check_bf16, reference as reference_bf16, unpack_i4  # noqa: E402
from test_gpu_parity import ulp_tol  # noqa: E402

DEV = "cuda"
BF, F16, F64 = torch.bfloat16, torch.float16, torch.float64
MS, N, N_OUTS = (1, 16, 24), 64, (0, 3, 17)
CASES = [(dt, bit) for dt in (F16, BF) for bit in (8, 4)]
IDS = [f"{str(dt).replace('torch.', '')}-W{bit}" for dt, bit in CASES]
HOT = [5, 77, 100]


def K_of(bit):
    return 128 if bit == 8 else 256


def name_of(dt):
    return E.F16 if dt == F16 else E.BF16


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    lib = _capi.load()
    lib.mixq_gemm_set_config(-1); lib.mixq_gemm_w8a16_set_config(-1)
    yield


def bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same(what, gpu, cpu):
    a, b = gpu.detach().cpu().contiguous(), cpu.detach().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype} {tuple(a.shape)} on the GPU, {b.dtype} {tuple(b.shape)} from the oracle"
    a, b = (a.view(torch.int16), b.view(torch.int16)) if a.dtype in (F16, BF) else (a, b)
    if not torch.equal(a, b):
        d = a != b
        raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} elements differ between the kernel and the oracle; first at {tuple(int(i) for i in torch.nonzero(d)[0])}")


def plain(mod, q, M):
    return mod.UnpackOperand(q, M) if mod.fmt_of(q) != FMT_PLAIN else q[:M]


def make_x(M, K, dt, seed):
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed))
    x[:, HOT] *= 30
    if M > 2:
        x[2] = 0                                                              # an all-zero row
    if dt == BF:
        x[1::3] *= 2.0 ** 10                                                  # rows float16 cannot hold (x_scale stays float16: max / qmax fits it)
    return x.to(dt)


def outlier_cols(n, K):
    rest = [c for c in np.random.default_rng(n).permutation(K).tolist() if c not in HOT]
    return ([HOT[1], HOT[0]] + rest)[:n]                                      # (unsorted; HOT[2] stays in: the misprediction flag is raised)


# ---- 1. the quantise family, detection and the norm: bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,bit", CASES, ids=IDS)
def test_quantise_family_detection_and_norm_bit_for_bit(dt, bit):
    K = K_of(bit)
    packed = (FMT_P16X64, FMT_F16X64) if bit == 8 else (FMT_P16X64, FMT_R6X128)
    for M in MS:
        x = make_x(M, K, dt, 10 * M + bit)
        xg = x.to(DEV)
        sg, sc = torch.zeros((M, 1), dtype=F16, device=DEV), torch.zeros((M, 1), dtype=F16)
        what = f"{dt} W{bit} M={M}"
        same(what + " FindRowScale q", mixlib.FindRowScale(xg, sg, M, K, bit), B.FindRowScale(x, sc, M, K, bit))
        same(what + " FindRowScale x_scale", sg, sc)
        for fmt in packed:
            qg, qc = mixlib.FindRowScalePacked(xg, sg, M, K, bit, fmt=fmt), B.FindRowScalePacked(x, sc, M, K, bit, fmt=fmt)
            assert mixlib.fmt_of(qg) == B.fmt_of(qc) == fmt
            same(f"{what} FindRowScalePacked fmt={fmt}", plain(mixlib, qg, M), plain(B, qc, M))
            same(what + " FindRowScalePacked x_scale", sg, sc)
        ig, cg = mixlib.DetectOutlierCols(xg, 6.0)
        ic, cc = B.DetectOutlierCols(x, 6.0)
        assert int(cg.item()) == int(cc.item()) >= (len(HOT) if M > 1 else 0), what
        same(what + " DetectOutlierCols", ig[: int(cg.item())], ic[: int(cc.item())])
        w = (0.5 + torch.rand(K, generator=torch.Generator().manual_seed(3))).to(dt)
        og, oc = torch.empty_like(xg), torch.empty_like(x)
        mixlib.layernorm_forward_cuda(xg, w.to(DEV), og, 1e-5)
        B.layernorm_forward_cuda(x, w, oc, 1e-5)
        same(what + " layernorm_forward_cuda", og, oc)
        for n in N_OUTS[1:] + N_OUTS[:1]:
            cols = outlier_cols(n, K)
            ind = torch.tensor(cols, dtype=torch.int32)
            if n:
                a, b = xg.clone(), x.clone()
                same(f"{what} n={n} ExtractOutliersAndSetToZeros x_out", mixlib.ExtractOutliersAndSetToZeros(ind.to(DEV), a), B.ExtractOutliersAndSetToZeros(ind, b))
                same(f"{what} n={n} ExtractOutliersAndSetToZeros x", a, b)
            # (count, capacity, device count, kept map): the plain call, the capacity-padded buffer with its device count, the kept map on top
            forms = [(n, None, False)] + ([(16 * ((n + 15) // 16), n, False), (16 * ((n + 15) // 16), n, True), (n, None, True)] if n else [])
            for cap, live, kept in forms:
                buf = torch.zeros(cap, dtype=torch.int32)
                buf[:n] = ind
                n_dev = None if live is None else torch.tensor([live], dtype=torch.int32)
                cm = kept_outlier_map(ind, K) if kept else None
                g = lambda t: None if t is None else t.to(DEV)
                for fmt in (FMT_PLAIN, packed[-1] if bit == 4 else packed[0]):
                    ctx = f"{what} n={n} cap={cap} live={live} kept={kept} fmt={fmt}"
                    a, b = xg.clone(), x.clone()
                    fg, fc = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32)
                    qg, xog = mixlib.QuantFused(a, g(buf) if n else None, sg, bit, 6.0, flag=fg, n_dev=g(n_dev), fmt=fmt, col_mask=g(cm))
                    qc, xoc = B.QuantFused(b, buf if n else None, sc, bit, 6.0, flag=fc, n_dev=n_dev, fmt=fmt, col_mask=cm)
                    same(ctx + " QuantFused q", plain(mixlib, qg, M), plain(B, qc, M))
                    same(ctx + " QuantFused x_scale", sg, sc)
                    same(ctx + " QuantFused x (zeroed in place)", a, b)
                    assert int(fg.item()) == int(fc.item()), ctx + " the misprediction flag"
                    if n:
                        same(ctx + " QuantFused x_out", xog[:, :n], xoc[:, :n])
                    fg.zero_(); fc.zero_()
                    qg, xog = mixlib.RMSNormQuantFused(xg, w.to(DEV), og, 1e-5, g(buf) if n else None, sg, bit, flag=fg, fmt=fmt, n_dev=g(n_dev), col_mask=g(cm))
                    qc, xoc = B.RMSNormQuantFused(x, w, oc, 1e-5, buf if n else None, sc, bit, flag=fc, fmt=fmt, n_dev=n_dev, col_mask=cm)
                    same(ctx + " RMSNormQuantFused out", og, oc)
                    same(ctx + " RMSNormQuantFused q", plain(mixlib, qg, M), plain(B, qc, M))
                    same(ctx + " RMSNormQuantFused x_scale", sg, sc)
                    assert int(fg.item()) == int(fc.item()), ctx
                    if n:
                        same(ctx + " RMSNormQuantFused x_out", xog[:, :n], xoc[:, :n])
    torch.cuda.synchronize()


# ---- 2. FusedLinear on exact operands ---------------------------------------------------------------------------------------------------
def exact_operands(bit, dt, M, rows, seed):
    kw = dict(q_max=31, xo_max=16, wo_max=8, add_max=255, bias_max=255) if (dt == BF and bit == 8) else {}      # (as exact.problem: bf16 keeps 8 bits)
    p = E.exact_problem(bit, M, K_of(bit), rows, max(N_OUTS), dtype=name_of(dt), seed=seed, **kw)
    p.check_conditions()
    return p


def both_backends(p, dt):
    """[(module, device, packed q_x, packed q_w, x_scale, scale_col)] for the HIP backend and the oracle"""
    qx, qw = p.q_plain()
    fx, fw = (FMT_P16X64, FMT_F16X64) if p.bit == 8 else (FMT_R6X128, FMT_F6X128)
    out = []
    for mod, dev in ((mixlib, DEV), (B, "cpu")):
        out.append((mod, dev, mod.PackOperand(qx.to(dev), fx), mod.PackOperand(qw.to(dev), fw), torch.from_numpy(p.sx.copy()).reshape(-1, 1).to(dev),
                    torch.from_numpy(p.sw.copy()).reshape(1, -1).to(dev)))
    return out


def padded(v, dt, dev):
    """[R, n] float64 -> [R, pad16(n)] in the container with NaN patterns in the pad"""
    n = v.shape[1]
    t = torch.full((v.shape[0], (n + 15) // 16 * 16), 0x7FC1, dtype=torch.int16).view(dt)
    t[:, :n] = E.as_tensor(v, name_of(dt))
    return t.to(dev)


def run_fused(be, p, dt, n_out, dev_count, act, addend, bias, rows=None):
    mod, dev, qx, qw, sx, sw = be
    xo = wo = n_dev = None
    cap = n_out
    if n_out:
        xo, wo = padded(p.xo[:, :n_out], dt, dev), padded(p.wo[:, :n_out], dt, dev)
        if dev_count:
            cap, n_dev = xo.shape[1], torch.tensor([n_out], dtype=torch.int32, device=dev)
        xo, wo = xo[:, :cap], wo[:, :cap]
    kw = {} if dt == F16 else {"dtype": dt}
    return mod.FusedLinear(qx, qw, sx, sw, xo, wo, cap, torch.from_numpy(p.bias.copy()).to(dev) if bias else None, p.M, p.N, p.K, bit=p.bit, act=act,
                           n_out_dev=n_dev, addend=None if addend is None else E.as_tensor(addend, name_of(dt)).to(dev), **kw)


@pytest.mark.parametrize("dt,bit", CASES, ids=IDS)
def test_fused_linear_on_exact_operands(dt, bit):
    """ACT_NONE: kernel == oracle == RNE_16 of the float64 sum, bit for bit.  SILU / SILU_MUL / SILU_PAIR: each within exact.silu_reference's bound."""
    nm = name_of(dt)
    worst = {"kernel": 0.0, "oracle": 0.0}
    for M in MS:
        p = exact_operands(bit, dt, M, N, 100 * bit + M)
        p2 = exact_operands(bit, dt, M, 2 * N, 200 * bit + M)              # the interleaved gate / up rows of ACT_SILU_PAIR
        bes, bes2 = both_backends(p, dt), both_backends(p2, dt)
        ru, rg = O.pair_rows_split(np.arange(2 * N))
        b64, b2 = p.bias.astype(np.float64), p2.bias.astype(np.float64)
        for n_out in N_OUTS:
            for dev_count in ((False, True) if n_out else (False,)):
                for addend, bias in ((None, False), (True, False), (None, True), (True, True)):
                    ctx = f"{dt} W{bit} M={M} n_out={n_out} dev_count={dev_count} addend={addend} bias={bias}"
                    want, z = p.expected(n_out, addend, bias)
                    ys = [run_fused(be, p, dt, n_out, dev_count, ACT_NONE, p.addend if addend else None, bias) for be in bes]
                    for who, y in zip(worst, ys):
                        assert y.dtype == dt and tuple(y.shape) == (M, N)
                        E.assert_exact(bits(y), want, z, nm, f"{ctx} ACT_NONE {who}")
                    # SiLU over the same z; the multiplier of SILU_MUL: the addend's values (container values of mixed sign)
                    for act in (ACT_SILU, ACT_SILU_MUL):
                        if act == ACT_SILU_MUL and not addend:
                            continue
                        zz = p.z(n_out, addend if act == ACT_SILU else None, False)
                        ref, bound = E.silu_reference(zz, b64 if bias else None, p.addend if act == ACT_SILU_MUL else None, nm)
                        for who, be in zip(worst, bes):
                            y = run_fused(be, p, dt, n_out, dev_count, act, p.addend if addend else None, bias)
                            worst[who] = max(worst[who], E.silu_check(bits(y), ref, bound, nm, f"{ctx} act={act} {who}"))
                if dev_count:
                    continue
                for bias in (False, True):
                    # the joint launch: up rounded to the container (exact), then gate's SiLU-and-multiply on it
                    z2 = p2.z(n_out)
                    up_bits = E.to_bits(z2[:, ru] + (b2[ru] if bias else 0.0), nm)
                    ref, bound = E.silu_reference(z2[:, rg], b2[rg] if bias else None, E.from_bits(up_bits, nm), nm)
                    for who, be in zip(worst, bes2):
                        y = run_fused(be, p2, dt, n_out, False, ACT_SILU_PAIR, None, bias)
                        assert y.dtype == dt and tuple(y.shape) == (M, N)
                        worst[who] = max(worst[who], E.silu_check(bits(y), ref, bound, nm, f"{dt} W{bit} M={M} n_out={n_out} bias={bias} SILU_PAIR {who}"))
    torch.cuda.synchronize()
    print(f"FusedLinear {dt} W{bit}: ACT_NONE bit for bit; SiLU forms worst |err| / bound  kernel {worst['kernel']:.4f}  oracle {worst['oracle']:.4f}")


# ---- 3. weight-only ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF], ids=["float16", "bfloat16"])
def test_w8a16_linear_with_and_without_addend(dt):
    nm, K = name_of(dt), 128
    worst = {"kernel": 0.0, "oracle": 0.0}
    for M in MS:
        x, qkn, scale, bias, z, q = E.w8a16_problem(M, K, N)
        add = E._fit(np.random.default_rng(2000 + M + N).integers(-2000, 2001, (M, N)), E.BF16) * 2.0 ** -12      # (fits both containers)
        free = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(dt)
        free_wide = (3 * torch.randn(M, N + 8, generator=torch.Generator().manual_seed(M + 1))).to(dt)                 # (a row-strided addend: its first N columns)
        for who, (mod, dev) in zip(worst, ((mixlib, DEV), (B, "cpu"))):
            qt, st, bt = torch.from_numpy(qkn.copy()).to(dev), torch.from_numpy(scale.copy()).to(dev), torch.from_numpy(bias.copy()).to(dev)
            img = mod.PackW8A16(qt) if dt == F16 else mod.PackW8A16(qt, dt)
            xt = E.as_tensor(x.astype(np.float64), nm).to(dev)
            for a in (None, add):
                za = z if a is None else z + a
                kw = {} if a is None else {"addend": E.as_tensor(a, nm).to(dev)}
                y = mod.W8A16Linear(xt, img, st, bt, N, K, **kw)
                assert y.dtype == dt
                E.assert_exact(bits(y), E.to_bits(za, nm), za, nm, f"W8A16 {dt} M={M} addend={a is not None} {who}")
            if dt == BF:                                                      # free operands: within w8a16_bf16_ref.bound of the float64 value
                for fa in (None, free_wide[:, :N]):
                    for b in (None, bias):
                        y = mod.W8A16Linear(free.to(dev), img, st, None if b is None else bt, N, K, **({} if fa is None else {"addend": free_wide.to(dev)[:, :N]}))
                        ab = None if fa is None else bits(fa)
                        z64, bound = W.z64(bits(free), qkn, scale, ab, b), W.bound(bits(free), qkn, scale, ab, b)
                        err = np.abs(E.from_bits(bits(y), nm) - z64)
                        assert (err <= bound).all(), f"W8A16 bf16 free operands M={M} {who}: worst err / bound {float((err / bound).max()):.3f}"
                        worst[who] = max(worst[who], float((err / bound).max()))
    torch.cuda.synchronize()
    print(f"W8A16Linear {dt}: exact operands bit for bit" + (f"; free operands worst |err| / bound  kernel {worst['kernel']:.4f}  oracle {worst['oracle']:.4f}" if dt == BF else ""))


# ---- 4. the kept argument block with a per-call addend ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,bit", CASES, ids=IDS)
def test_forward_plan_run_with_an_addend(dt, bit):
    K = K_of(bit)
    g = torch.Generator().manual_seed(50 + bit)
    lim = 127 if bit == 8 else 7
    qw_int = torch.randint(-lim, lim + 1, (N, K), generator=g, dtype=torch.int16)
    qw = qw_int.to(torch.int8) if bit == 8 else torch.from_numpy(E.pack_i4(qw_int.numpy()))
    sw = ((torch.rand(1, N, generator=g) + 0.5) * (0.02 if bit == 8 else 0.3)).half()
    bias = torch.randn(N, generator=g).half()
    qfmt, wfmt = (FMT_P16X64, FMT_F16X64) if bit == 8 else (FMT_R6X128, FMT_F6X128)
    worst = {"kernel": 0.0, "oracle": 0.0}
    for M in MS:
        x = make_x(M, K, dt, 70 * M + bit)
        wide = (3 * torch.randn(M, N + 8, generator=g)).to(dt)
        for n in N_OUTS:
            cols = outlier_cols(n, K)
            cap = (n + 15) // 16 * 16
            buf = torch.zeros(max(cap, 1), dtype=torch.int32)[:cap]
            buf[:n] = torch.tensor(cols, dtype=torch.int32)
            wo = torch.zeros((N, max(cap, 16)), dtype=dt)
            wo[:, :n] = (0.05 * torch.randn(N, n, generator=g)).to(dt)
            runs = {}
            for who, (mod, dev) in zip(worst, ((mixlib, DEV), (B, "cpu"))):
                xs = torch.zeros((M, 1), dtype=F16, device=dev)
                n_dev = torch.tensor([n], dtype=torch.int32, device=dev) if n else None
                cm = kept_outlier_map(buf[:n].to(dev), K) if n else None
                kw = {} if dt == F16 else {"dtype": dt}
                plan = mod.ForwardPlan(M, N, K, bit, 6.0, K, buf.to(dev) if n else None, n, n_dev, xs, mod.PackOperand(qw.to(dev), wfmt), sw.to(dev),
                                       wo[:, :cap].to(dev) if n else None, bias.to(dev), qfmt, kept_mask=cm, **kw)
                for kind in ("none", "contiguous", "row-strided"):
                    rd = None if kind == "none" else (wide.to(dev)[:, :N].contiguous() if kind == "contiguous" else wide.to(dev)[:, :N])
                    y, q, xo = plan.run(x.to(dev).clone(), **({} if rd is None else {"addend": rd}))
                    runs[(who, kind)] = (y, plain(mod, q, M), xo, xs.clone())
            for kind, r in (("none", None), ("contiguous", wide[:, :N]), ("row-strided", wide[:, :N])):
                ctx = f"ForwardPlan {dt} W{bit} M={M} n={n} addend={kind}"
                (yg, qg, xog, sg), (yc, qc, xoc, sc) = runs[("kernel", kind)], runs[("oracle", kind)]
                same(ctx + " q", qg, qc)
                same(ctx + " x_scale", sg, sc)
                if n:
                    same(ctx + " x_out", xog, xoc)
                assert yg.dtype == yc.dtype == dt
                if dt == BF:                                                  # tests/test_gpu_bf16_gemm.py: the float64 restatement over the operands the GEMM read
                    ints = (qc.to(F64) if bit == 8 else unpack_i4(qc).to(F64)) @ qw_int.to(F64).T
                    ref, bound = reference_bf16(ints, sc.reshape(-1), sw.reshape(-1), xoc, wo, n, r, bias, ACT_NONE)
                    worst["kernel"] = max(worst["kernel"], check_bf16(yg.cpu(), ref, bound, ctx + " kernel"))
                    worst["oracle"] = max(worst["oracle"], check_bf16(yc, ref, bound, ctx + " oracle"))
                else:                                                         # tests/test_gpu_residual.py: the oracle's fused linear and parity's tolerance
                    ref = yc.numpy()
                    err, tol = np.abs(yg.cpu().numpy().astype(np.float64) - ref.astype(np.float64)), ulp_tol(ref)
                    assert (err <= tol).all(), f"{ctx}: max err / tol {float((err / tol).max()):.3f}"
                    worst["kernel"] = max(worst["kernel"], float((err / tol).max()))
    torch.cuda.synchronize()
    print(f"ForwardPlan.run {dt} W{bit}: q, x_scale, x_out bit for bit; y worst |err| / bound  kernel {worst['kernel']:.4f}" + (f"  oracle {worst['oracle']:.4f}" if dt == BF else " (against the oracle)"))
