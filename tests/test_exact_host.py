"""tests/exact.py on the host: every configuration the GPU module launches satisfies the generator's conditions; the oracle equals the
float64 expectation BIT FOR BIT on each of them (the expectation is the contract, not a second opinion); the checkers reject numpy
emulations of four wrong kernels - a round-toward-zero conversion, the tail rounded to 16 bits before the addition, the main term rounded
to 16 bits before the addition, a half-precision exponential in SiLU - and accept a faithful fp32 emulation; and the expectations hold the
shares of roundings, ties, subnormals, underflows and overflows the GPU tests rely on."""
import numpy as np
import pytest

import exact as E
from exact import BF16, F16
from oracle import oracle as O

MAIN = [(bit, dt, M, N) for bit in (8, 4) for dt in (F16, BF16) for M in E.M_SHAPES for N in E.N_SHAPES]
EDGE = [(kind, bit, M) for kind in E.EDGES_F16 for bit in (8, 4) for M in E.M_SHAPES if not (kind == "long_k" and bit == 4)]
F32 = np.float32


def combos_main():
    return [(n, a, b) for n in E.N_OUTS for a in (None, True) for b in (False, True)] + [(17, "bcast", True)]


def oracle_bits(p, n_out, addend, bias):
    qx, qw = (p.qx, p.qw) if p.bit == 8 else (E.pack_i4(p.qx), E.pack_i4(p.qw))
    ad = None if not addend else np.ascontiguousarray(p.addend_values(addend)).astype(np.float16)
    y = O.linear_fused(qx, qw, p.sx, p.sw, xo=p.xo[:, :n_out].astype(np.float16) if n_out else None, wo=p.wo[:, :n_out].astype(np.float16) if n_out else None,
                       addend=ad, bias=p.bias if bias else None, act=0, bit=p.bit)
    return y.view(np.uint16)


# ---- numpy emulations of kernels, fp32 like the device ------------------------------------------------------------------------------------
def rtz_bits(v64, dtype):
    """Round toward zero: RNE, then one step back wherever RNE went away from zero (inf -> the largest finite value)."""
    b = E.to_bits(v64, dtype).copy()
    with np.errstate(invalid="ignore"):
        over = np.abs(E.from_bits(b, dtype)) > np.abs(v64)
    b[over] -= 1
    return b


def r16(v32, dtype):
    return E.from_bits(E.to_bits(v32.astype(np.float64), dtype), dtype).astype(F32)


def emulate(p, n_out, addend, bias, mode):
    """The epilogue in fp32, term by term, tail summed in DESCENDING column order (the oracle sums ascending).  mode: faithful | rtz |
    tail16 | main16."""
    with np.errstate(over="ignore"):
        a32 = p.acc.astype(F32)
        main = a32 * p.sx.astype(F32)[:, None] * p.sw.astype(F32)[None, :]
        tail = np.zeros((p.M, p.N), F32)
        for j in reversed(range(n_out)):
            tail = tail + np.outer(p.xo[:, j].astype(F32), p.wo[:, j].astype(F32))
        if mode == "tail16":
            tail = r16(tail, p.dtype)
        if mode == "main16":
            main = r16(main, p.dtype)
        v = main + tail
        if addend:
            v = v + p.addend_values(addend).astype(F32)
        if bias:
            v = v + p.bias.astype(F32)[None, :]
    v64 = v.astype(np.float64)
    if mode == "rtz":
        return rtz_bits(v64, p.dtype)
    return E.to_bits(v64, p.dtype) if p.dtype == F16 else E.to_bits(v, p.dtype)


# ---- 1. conditions and the oracle identity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit,dtype,M,N", MAIN)
def test_main_problems_satisfy_their_conditions_and_the_oracle_equals_the_expectation(bit, dtype, M, N):
    p = E.problem("main", bit, dtype, M, N)
    worst = p.check_conditions(bcast=True)
    assert worst < E.LIMIT and p.n_cap == max(E.N_OUTS)
    assert set(np.unique(p.q)) == {2.0 ** -e for e in range(9, 14)}, "every quantum 2^-9 .. 2^-13 occurs"
    agg = []
    for n_out, addend, bias in combos_main():
        want, z = p.expected(n_out, addend, bias)
        assert np.isfinite(E.from_bits(want, dtype)).all()
        if dtype == F16:                              # (the oracle restates the fp16 contract only)
            got = oracle_bits(p, n_out, addend, bias)
            assert not E.mismatches(got, want, z).any(), (n_out, addend, bias)
        assert not E.mismatches(emulate(p, n_out, addend, bias, "faithful"), want, z).any(), (n_out, addend, bias)
        agg.append((want, z))
    s = E.shares(np.concatenate([a for a, _ in agg]), np.concatenate([b for _, b in agg]), dtype)
    print(f"{p.name}: worst sum of absolute terms {worst:.4g} q; shares over {len(agg)} combinations {s}")
    assert s["away"] >= 0.30 and s["tie"] >= 0.02, s


@pytest.mark.parametrize("kind,bit,M", EDGE)
def test_edge_problems_satisfy_their_conditions_and_the_oracle_equals_the_expectation(kind, bit, M):
    p = E.problem(kind, bit, F16, M, E.N_SHAPES[0])
    for n_out, addend, bias in E.edge_combos(kind):
        want, z = p.expected(n_out, addend, bias)
        got = oracle_bits(p, n_out, addend, bias)
        assert not E.mismatches(got, want, z).any(), (kind, n_out, addend, bias)
        assert np.array_equal(got, want) or (z == 0).any()
        s = E.shares(want, z, F16)
        print(f"{p.name} n_out={n_out} addend={addend} bias={bias}: {s}")
        if kind == "tiny":
            assert (p.sw.astype(np.float64) < 2.0 ** -14).all() and (np.abs(p.wo[p.wo != 0]) < 2.0 ** -10).all() and (np.abs(p.wo[p.wo != 0]) < 2.0 ** -14).any()
            assert s["subnormal"] + s["flushed"] >= 0.85 and s["subnormal"] >= (0.5 if bit == 8 or n_out else 0.0), s
            rows = [3, M - 2]
            assert (p.sx[rows] == 0).all() and not p.qx[rows].any() and (z[rows] != 0).mean() > (0.5 if n_out or bias or addend else -1)
        if kind == "tinier":
            assert s["flushed"] >= 0.10 and s["neg_zero"] >= (100 if M == 72 else 30), s
        if kind == "overflow":
            assert 0.05 <= s["inf"] <= 0.50, s
            if n_out == 0 and not addend and not bias:
                r, c = (0, 0) if bit == 8 else (2, 2)
                assert z[r, c] == 65504.0 and want[r, c] == 0x7BFF and z[r, c + 1] == 65520.0 and want[r, c + 1] == 0x7C00
            assert s["has_max"] or n_out, s
        if kind == "long_k":
            assert (np.abs(p.acc) > 2 ** 24).mean() > 0.9 and np.isfinite(E.from_bits(want, F16)).all()


@pytest.mark.parametrize("bit", [8, 4])
@pytest.mark.parametrize("M", E.M_SHAPES)
def test_bf16_wide_problem(bit, M):
    p = E.problem("wide", bit, BF16, M, E.N_SHAPES[0])
    lo, hi = np.inf, 0.0
    for n_out, addend, bias in E.edge_combos("wide"):
        want, z = p.expected(n_out, addend, bias)
        v = E.from_bits(want, BF16)
        assert np.isfinite(v).all()
        assert not E.mismatches(emulate(p, n_out, addend, bias, "faithful"), want, z).any()
        nz = np.abs(v[v != 0])
        lo, hi = min(lo, nz.min()), max(hi, nz.max())
    assert lo <= 2.0 ** -70 and hi >= 2.0 ** 80, (lo, hi)


def test_w8a16_problem_and_the_oracle():
    for M in E.M_SHAPES:
        for N in E.N_SHAPES:
            x, qkn, scale, bias, z, q = E.w8a16_problem(M, E.K_MAIN, N)
            for b in (None, bias):
                zz = z if b is not None else z - bias.astype(np.float64)[None, :]
                want = E.to_bits(zz, F16)
                got = O.w8a16_linear(x, qkn, scale, b).view(np.uint16)
                assert not E.mismatches(got, want, zz).any()
                s = E.shares(want, zz, F16)
                assert s["away"] >= 0.30 and s["tie"] >= 0.02, s


def test_int32_extremes_expectation():
    y32, sx, sw, q = E.int32_extremes(72, 136)
    assert y32.max() == 2 ** 31 - 1 and y32.min() == -2 ** 31
    want = E.to_bits(y32.astype(F32).astype(np.float64) * q, F16)
    assert np.isfinite(E.from_bits(want, F16)).all()
    assert (y32.astype(F32).astype(np.int64) != y32).mean() > 0.1, "a good share of the values does not fit fp32"


def test_pair_oracle_equals_the_expectation():
    """oracle.linear_fused_pair on an exact problem whose up rows have a zero main term and tail: up = fp16(bias_up) exactly, so the
    pair's MIXQ_ACT_NONE part (the multiplier) is exact; its SiLU part is held to silu_reference."""
    xo, wo, z, mul = E.silu_mul_operands(F16)
    N = 256
    bias_g = E.silu_bias_vector(N)
    bias_u = mul[0]
    qx = np.zeros((248, 64), np.int8)
    qw2 = np.random.default_rng(1).integers(-128, 128, (2 * N, 64)).astype(np.int8)
    il = O.pair_rows_interleave
    wo2 = il(np.zeros((N, 1)), wo[:, None]).astype(np.float16)
    y = O.linear_fused_pair(qx, qw2, np.full(248, 0.125, np.float16), np.full(2 * N, 0.125, np.float16), xo=xo[:, None].astype(np.float16), wo2=wo2,
                            bias2=il(bias_u, bias_g).astype(np.float16))
    ref, bound = E.silu_reference(z, bias_g[None, :], bias_u[None, :], F16)
    E.silu_check(y.view(np.uint16), ref, bound, F16, "oracle pair")


# ---- 2. the checkers have teeth ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit,dtype", [(8, F16), (4, F16), (8, BF16), (4, BF16)])
def test_exact_comparison_rejects_three_wrong_kernels(bit, dtype):
    p = E.problem("main", bit, dtype, 72, 136)
    for n_out, addend, bias in ((17, True, True), (129, None, False), (41, True, False)):
        want, z = p.expected(n_out, addend, bias)
        assert not E.mismatches(emulate(p, n_out, addend, bias, "faithful"), want, z).any()
        bad = {mode: int(E.mismatches(emulate(p, n_out, addend, bias, mode), want, z).sum()) for mode in ("rtz", "tail16", "main16")}
        print(f"{p.name} n_out={n_out} addend={addend} bias={bias}: rejected elements {bad} of {z.size}")
        assert bad["rtz"] >= 0.30 * z.size, bad
        # (int4 at K = 128: |acc| <= 7168 and far below 2^11 in practice, so acc q fits 11 significand bits - a 16-bit main term is exact there
        # and cannot be told apart; the int8 problems tell it)
        assert bad["tail16"] > 0 and (bad["main16"] > 0 or (bit == 4 and dtype == F16)), bad
        with pytest.raises(AssertionError, match="differ from RNE_16"):
            E.assert_exact(emulate(p, n_out, addend, bias, "rtz"), want, z, dtype, "rtz")


@pytest.mark.parametrize("kind,bit", [(k, b) for k in ("tiny", "tinier", "overflow") for b in (8, 4)])
def test_exact_comparison_rejects_wrong_kernels_on_the_edges(kind, bit):
    p = E.problem(kind, bit, F16, 72, 136)
    n_out, addend, bias = E.EDGE_N_OUT, True, True
    want, z = p.expected(n_out, addend, bias)
    assert not E.mismatches(emulate(p, n_out, addend, bias, "faithful"), want, z).any()
    assert E.mismatches(emulate(p, n_out, addend, bias, "rtz"), want, z).sum() > 0.1 * z.size
    # a kernel that flushes fp16-subnormal scales or tail operands, or saturates instead of overflowing
    if kind == "overflow":
        sat = want.copy()
        sat[(sat & 0x7FFF) == 0x7C00] -= 1
        assert E.mismatches(sat, want, z).sum() >= 0.05 * z.size
    else:
        flushed = E.Exact(p.bit, p.dtype, p.qx, p.qw, p.sx, np.where(p.sw.astype(np.float64) < 2.0 ** -14, 0, p.sw), p.xo, np.where(np.abs(p.wo) < 2.0 ** -14, 0, p.wo),
                          p.addend, p.bias, p.q, "flushed")
        assert E.mismatches(emulate(flushed, n_out, addend, bias, "faithful"), want, z).sum() > (0.1 * z.size if kind == "tiny" else 0)
    # the sign of a zero: either sign where z == 0, the expected one where a nonzero z underflowed
    flip = want.copy()
    zeros = (want & 0x7FFF) == 0
    flip[zeros] ^= 0x8000
    assert E.mismatches(flip, want, z).sum() == int((zeros & (z != 0)).sum())


def _silu_emulation(v64, bias, mode, dtype):
    """mixq_silu in numpy fp32: v * (1 / (1 + exp2(-v * log2e))), + bias, one rounding.  mode: faithful | rtz | half_exp."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        v = v64.astype(F32)
        e = np.exp2((-v) * F32(1.4426950408889634))
        if mode == "half_exp":
            e = e.astype(np.float16).astype(F32)
        s = v * (F32(1) / (F32(1) + e))
        y = s + bias.astype(F32) if bias is not None else s
    y64 = y.astype(np.float64)
    return rtz_bits(y64, dtype) if mode == "rtz" else (E.to_bits(y64, dtype) if dtype == F16 else E.to_bits(y, dtype))


@pytest.mark.parametrize("with_bias", [False, True])
def test_silu_bound_over_every_fp16_argument_accepts_fp32_and_rejects_rtz_and_a_half_precision_exponential(with_bias):
    pat = E.all_finite_patterns(F16)
    assert pat.size == 248 * 256 == 63488
    z = E.from_bits(pat, F16).reshape(248, 256)
    bias = E.silu_bias_vector(256)[None, :] if with_bias else None
    ref, bound = E.silu_reference(z, bias, None, F16)
    worst = E.silu_check(_silu_emulation(z, bias, "faithful", F16), ref, bound, F16, "fp32 emulation")
    assert worst <= 1.0
    y = E.decode_for_bound(_silu_emulation(z, bias, "rtz", F16), F16)
    n_rtz = int((np.abs(y - ref) > bound).sum())
    y = E.decode_for_bound(_silu_emulation(z, bias, "half_exp", F16), F16)
    n_half = int((np.abs(y - ref) > bound).sum())
    print(f"fp16 SiLU sweep bias={with_bias}: fp32 emulation worst err / bound {worst:.3f}; rejected: round-toward-zero {n_rtz}, half-precision exponential {n_half}")
    assert n_rtz >= 15000 and n_half >= 1000, (n_rtz, n_half)
    with pytest.raises(AssertionError, match="outside the derived SiLU bound"):
        E.silu_check(_silu_emulation(z, bias, "half_exp", F16), ref, bound, F16, "half-precision exponential")


def test_silu_bound_over_every_bf16_argument_accepts_fp32():
    pat = E.all_finite_patterns(BF16)
    assert pat.size == 255 * 256
    z = E.from_bits(pat, BF16).reshape(255, 256)
    ref, bound = E.silu_reference(z, None, None, BF16)
    worst = E.silu_check(_silu_emulation(z, None, "faithful", BF16), ref, bound, BF16, "fp32 emulation")
    y = E.decode_for_bound(_silu_emulation(z, None, "rtz", BF16), BF16)
    assert worst <= 1.0 and int((np.abs(y - ref) > bound).sum()) >= 2000


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_silu_mul_operands_and_bound(dtype):
    xo, wo, z, mul = E.silu_mul_operands(dtype)
    assert z.shape == (248, 256) and np.array_equal(z.astype(F32).astype(np.float64), z)
    assert np.abs(z).min() == 2.0 ** -24 and np.abs(z).max() >= 2.0 ** 7 and (z < 0).mean() == 0.5
    bias = E.silu_bias_vector(256)[None, :]
    ref, bound = E.silu_reference(z, bias, mul, dtype)
    inner = E.from_bits(_silu_emulation(z, bias, "faithful", F16), F16)        # (placeholder container: re-done in fp32 below)
    with np.errstate(over="ignore", under="ignore"):
        v = z.astype(F32)
        s = v * (F32(1) / (F32(1) + np.exp2((-v) * F32(1.4426950408889634))))
        y = (s + bias.astype(F32)) * mul.astype(F32)
    bits = E.to_bits(y.astype(np.float64), dtype) if dtype == F16 else E.to_bits(y, dtype)
    assert E.silu_check(bits, ref, bound, dtype, "fp32 emulation of SILU_MUL") <= 1.0
    assert int((np.abs(E.decode_for_bound(rtz_bits(y.astype(np.float64), dtype), dtype) - ref) > bound).sum()) >= 10000
    del inner
