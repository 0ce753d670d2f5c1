"""What the Python layer (mixq_amd/mixlib.py, linear.py, fused.py) hands to the C ABI, recorded without a GPU.

The real modules run on CPU tensors once the C ABI is replaced by a recorder (`recording()`): the object `_capi.load()` returns then
records every launch as one string, "name(arg,arg,...)" - integers and floats by value, pointers as `-` (NULL) or `@<address % 16>` (CPU
allocations are 64-byte aligned, so this shows a view's offset and nothing of the allocator), a `mixq_linear_args` block as `{...}` of its
fields decoded the same way, in the struct's order - and answers 0.  The pure host queries (`mixq_gemm_amax_supported`, `mixq_gemm_decode_pick_bf16`, ...) go to the real library
and are recorded with their answer.  A symbol the library does not export raises AttributeError, as the real object does.

`SCENARIOS` is the list of calls tests/golden/host_calls.json was recorded from (tools/record_calls.py) and tests/test_host_calls.py
replays; `LAYER_SCENARIOS` names the ones tests/test_gpu_host_calls.py runs for real.  The recorder answers no device reads: the search
phase of a layer stays with the oracle-backed state-machine tests.
"""
from __future__ import annotations

import ctypes as C
import json
from contextlib import ExitStack, contextmanager
from unittest import mock

import torch

from mixq_amd import _capi, mixlib
from mixq_amd import fused as F
from mixq_amd import linear as L
from mixq_amd.cache import MixLibCache
from mixq_amd.config import MixqConfig
from mixq_amd._capi import (ACT_NONE, ACT_SILU, ACT_SILU_MUL, ACT_SILU_PAIR, FMT_PLAIN, FMT_P16X64, FMT_F16X64, FMT_F6X128, FMT_R6X128)

HOST_QUERIES = ("mixq_gemm_amax_supported", "mixq_gemm_amax_supported_bf16", "mixq_gemm_decode_pick_bf16", "mixq_gemm_pair_supported_bf16",
                "mixq_kept_map_words", "mixq_gemm_pick_config", "mixq_gemm_pick_config_fmt", "mixq_gemm_pick_split", "mixq_gemm_pick_split_bf16",
                "mixq_gemm_config_name", "mixq_gemm_num_configs", "mixq_gemm_w8a16_config_name", "mixq_gemm_w8a16_num_configs", "mixq_version",
                "mixq_gemm_workspace_bytes")
LIB_TOKEN = "<LIB>"                      # stands for _capi.LIB_PATH (an absolute path) in recorded messages


def _ptr(v):
    if v is None:
        return "-"
    if not isinstance(v, int) or isinstance(v, bool):
        raise TypeError(f"pointer argument: expected an address or None, got {type(v).__name__}")
    return f"@{v % 16}"


def _decode(argtype, v):
    if argtype is C.c_void_p:
        obj = getattr(v, "_obj", None)                       # ctypes.byref(struct)
        if isinstance(obj, _capi.LinearArgs):
            return "{" + ",".join(_decode(t, getattr(obj, name)) for name, t in obj._fields_) + "}"      # (in the struct's field order)
        return _ptr(v)
    if argtype is C.c_int:
        if not isinstance(v, int):
            raise TypeError(f"int argument: got {type(v).__name__} {v!r}")
        return str(int(v))
    if argtype is C.c_float:
        if not isinstance(v, (int, float)):
            raise TypeError(f"float argument: got {type(v).__name__} {v!r}")
        return repr(float(v))
    raise TypeError(f"unhandled argument type {argtype}")


class RecordingLib:
    """Stands where the ctypes library object stands."""

    def __init__(self, real, records, hide=()):
        self.__dict__.update(_real=real, _records=records, _hide=tuple(hide))

    def __getattr__(self, name):
        if name in self._hide:
            raise AttributeError(name)
        fn = getattr(self._real, name)                       # AttributeError for a symbol the real library lacks
        sig = _capi.SIGNATURES[name]
        if self._records is None and name not in HOST_QUERIES:
            return lambda *args: 0                           # (timing the Python layer alone: tools/host_cost.py)

        def entry(*args):
            if len(args) != len(sig):
                raise TypeError(f"{name}: {len(args)} arguments, the C ABI takes {len(sig)}")
            rec = f"{name}({','.join(_decode(t, a) for t, a in zip(sig, args))})"
            rc = fn(*args) if name in HOST_QUERIES else 0
            if name in HOST_QUERIES:
                rec += f" -> {int(rc)}"
            if self._records is not None:
                self._records.append(rec)
            return rc
        return entry


class _Stream:
    cuda_stream = 0


@contextmanager
def recording(hide=(), record=True):
    """Yields the list the records go to (record=False: None, launches only answer 0).  Only inside this context are the names patched."""
    records = [] if record else None
    real = _capi.load()
    lib = RecordingLib(real, records, hide)

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        if rc != 0:
            raise _capi.MixqError(name, rc)

    with ExitStack() as st:
        for target, attr, new in ((_capi, "load", lambda: lib), (_capi, "call", call), (mixlib, "_dev_check", lambda *ts: None),
                                  (mixlib, "dev_check", lambda *ts: None), (mixlib, "_stream", lambda: 0),
                                  (torch.cuda, "current_stream", lambda device=None: _Stream()),
                                  (torch.cuda, "is_current_stream_capturing", lambda: False)):
            st.enter_context(mock.patch.object(target, attr, new))
        try:
            yield records
        finally:
            mixlib._pending_extract = None
            mixlib._wpacked.clear()
            mixlib._wo_padded.clear()


def describe(v):
    """Shape, dtype, strides and tags of every tensor in a scenario's return value: "float16[16, 128]/[128, 1]", then " fmt=1",
    " w8a16=bfloat16" and the subclass's name where there is one."""
    if isinstance(v, torch.Tensor):
        fmt, w, cls = getattr(v, "_mixq_fmt", None), getattr(v, "_mixq_w8a16_dtype", None), type(v).__name__
        with torch._C.DisableTorchFunctionSubclass():
            return (f"{str(v.dtype)[6:]}{list(v.shape)}/{list(v.stride())}"
                    + ("" if fmt is None else f" fmt={fmt}") + ("" if w is None else f" w8a16={str(w)[6:]}") + ("" if cls == "Tensor" else f" {cls}"))
    if isinstance(v, (list, tuple)):
        return [describe(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


def run(scenario):
    """One scenario -> {"calls": [...], "out": ...} or {"calls": [...], "error": [type, message]}."""
    fn, hide = scenario[1], (scenario[2] if len(scenario) > 2 else ())
    prev = mixlib._cfg
    with recording(hide) as records:
        try:
            res = {"out": describe(fn())}
        except Exception as e:                               # a refusal scenario: the exception is the result
            res = {"error": [type(e).__name__, str(e).replace(_capi.LIB_PATH, LIB_TOKEN)]}
        finally:
            mixlib._pending_extract = None
            mixlib._cfg = prev
    return json.loads(json.dumps({"calls": records, **res}))


# ------------------------------------------------------------------------------------------------------------
# operands (values never matter: nothing is computed)
# ------------------------------------------------------------------------------------------------------------
K, N = 256, 128
F16, BF16 = torch.float16, torch.bfloat16
DT = {"fp16": F16, "bf16": BF16}


def z(*shape, dtype=F16):
    return torch.zeros(shape, dtype=dtype)


def qx(M, bit=8, fmt=FMT_P16X64):
    rows = M if fmt == FMT_PLAIN else mixlib.packed_rows(M)
    return mixlib.set_fmt(z(rows, mixlib._q_row_bytes(K, bit, fmt), dtype=torch.int8 if bit == 8 else torch.uint8), fmt)


def qw(bit=8, fmt=FMT_F16X64, n=N):
    return mixlib.set_fmt(z(n, mixlib._q_row_bytes(K, bit, fmt), dtype=torch.int8 if bit == 8 else torch.uint8), fmt)


def misaligned(M, cols, dtype):
    """An [M, cols] window whose base is 2 bytes past an 8-byte boundary."""
    return z(M * (cols + 4) + 8, dtype=dtype)[1:1 + M * (cols + 4)].view(M, cols + 4)[:, :cols]


def outl(M, n, dtype, rows=N):
    """(x_out, w_out, n, n_dev) - n live columns under a capacity of 16 with a device count; n = 0: none."""
    if not n:
        return None, None, 0, None
    return z(M, 16, dtype=dtype), z(rows, 32, dtype=dtype)[:, :16], 16, z(1, dtype=torch.int32)      # (ldxo = 16, ldwo = 32: a swap shows)


def zero_tag():
    return MixLibCache(inputdim=64, device="cpu").zeros


def fused_linear(M=16, bit=8, dt=F16, act=ACT_NONE, n=3, addend=None, out=None, x_fmt=None, w_fmt=None, **kw):
    x_fmt = x_fmt if x_fmt is not None else (FMT_P16X64 if bit == 8 else FMT_R6X128)
    w_fmt = w_fmt if w_fmt is not None else (FMT_F16X64 if bit == 8 else FMT_F6X128)
    rows = 2 * N if act == ACT_SILU_PAIR else N
    xo, wo, cap, n_dev = outl(M, n, dt, rows)
    extra = {} if dt == F16 else {"dtype": dt}
    return mixlib.FusedLinear(qx(M, bit, x_fmt), qw(bit, w_fmt, rows), z(64, 1), z(1, rows), xo, wo, cap, z(rows), M, rows, K, bit=bit, act=act,
                              n_out_dev=n_dev, addend=addend, out=out, **extra, **kw)


def amax_args(M=16):
    return {"row_amax": z(64, dtype=torch.int32), "col_mask": L.kept_outlier_map(IND3, N)}


IND3 = torch.tensor([1, 5, 9], dtype=torch.int32)


def ind_cap(n):
    if not n:
        return None, None
    buf = z(16, dtype=torch.int32)
    buf[:3] = IND3
    return buf, z(1, dtype=torch.int32)


def plan(M=16, bit=8, dt=F16, n=3, decode=False, act=ACT_NONE, kept=False, ldx=K, **kw):
    ind, n_dev = ind_cap(n)
    w_fmt = FMT_F16X64 if bit == 8 else (FMT_P16X64 if decode else FMT_F6X128)
    q_fmt = FMT_P16X64 if bit == 8 or decode else FMT_R6X128
    extra = {} if dt == F16 else {"dtype": dt}
    if decode:
        extra["decode"] = True
    return mixlib.ForwardPlan(M, N, K, bit, 6.0, ldx, ind, n, n_dev, z(64, 1), qw(bit, w_fmt), z(1, N), z(N, 32, dtype=dt)[:, :n] if n else None, z(N),
                              q_fmt, act=act, kept_mask=L.kept_outlier_map(IND3, K) if kept and n else None, **extra, **kw)


def quant_fused(M=16, bit=8, dt=F16, fmt=FMT_P16X64, n=3, masked=False, x_out=None, **kw):
    ind, n_dev = ind_cap(n)
    return mixlib.QuantFused(z(M, K, dtype=dt), ind, z(64, 1), bit, 6.0, x_out=x_out, flag=z(1, dtype=torch.int32), n_dev=n_dev, fmt=fmt,
                             col_mask=L.kept_outlier_map(IND3, K) if masked else None, **kw)


def norm_quant(M=16, bit=8, dt=F16, fmt=FMT_P16X64, n=3, masked=False, **kw):
    ind, n_dev = ind_cap(n)
    return mixlib.RMSNormQuantFused(z(M, K, dtype=dt), z(K, dtype=dt), z(M, K, dtype=dt), 1e-6, ind, z(64, 1), bit, fmt=fmt, n_dev=n_dev,
                                    col_mask=L.kept_outlier_map(IND3, K) if masked else None, **kw)


def reference_sequence(config, M=16, silu=False, bit=8):
    """The reference operator's own call order (extract, row scale, torch.mm, gemm + dequantise) against the shim."""
    with mixlib.configured(config):
        x = z(M, K)
        x_scale = z(64, 1)
        w = z(N, K, dtype=torch.int8)
        wc = z(N, 3)
        xo = mixlib.ExtractOutliersAndSetToZeros(IND3, x)
        q = mixlib.FindRowScale(x, x_scale, M, K, bit)
        prod = torch.mm(xo, wc.T)
        y32 = mixlib.gemm(q, w, M, N, K)
        y = (mixlib.dequantizeInt8Silu if silu else mixlib.dequantizeInt8)(y32, x_scale, z(1, N), prod, 8, M, N)
        return xo, q, prod, y32, y


# ------------------------------------------------------------------------------------------------------------
# layers and modules (frozen: the search phase needs device reads)
# ------------------------------------------------------------------------------------------------------------
def cache_of(**flags):
    dt = flags.pop("dt", F16)
    return MixLibCache(inputdim=64, sigma=6, bit=8, device=flags.pop("device", "cpu"), config=MixqConfig(act_dtype=dt, **flags))


def layer(cache, bit=8, n=3, k=K, n_out=N, bias=True, weight_only=False):
    dev = cache.device
    l = L.MixLinear_GEMM(k, n_out, bias, dev, bit, weight_only=weight_only, cache=cache, fp_features_num=3)
    l.q_weight.zero_()
    l.scale_col.fill_(1.0)
    if bias:
        l.bias.zero_()
    if weight_only:
        return l
    if bit == 4:
        l.ind.copy_(IND3)
        l.weight_cache.zero_()
    elif n:
        l.ind = IND3.to(dev)
        l.weight_cache = torch.zeros((n_out, 32), dtype=F16, device=dev)[:, :3]         # (row stride 32, x_out's is 16: a swap shows)
    l.add_outliers = False
    return l


def rand(shape, dtype, device):
    g = torch.Generator().manual_seed(7)
    return (torch.randn(shape, generator=g) * 0.5).to(dtype).to(device)


def frozen_layer(M=16, bit=8, residual=False, device="cpu", runs=1, **flags):
    cache = cache_of(device=device, **flags)
    l = layer(cache, bit)
    dt = cache.config.act_dtype
    res = {"residual": rand((M, N), dt, device)} if residual else {}
    return [l(rand((M, K), dt, device), None, True, **res) for _ in range(runs)]


def weight_only_layer(M=16, residual=False, device="cpu", **flags):
    cache = cache_of(device=device, **flags)
    l = layer(cache, 8, weight_only=True)
    dt = cache.config.act_dtype
    res = {"residual": rand((M, N), dt, device)} if residual else {}
    return [l(rand((M, K), dt, device), **res) for _ in range(2)]


def mlp_block(M=16, bit=8, residual=False, n=3, device="cpu", takeover=False, rounds=1, **flags):
    """FasterTransformerRMSNorm in front of MixLlamaMLP; a second round finds the images and kept blocks of the first."""
    cache = cache_of(device=device, **flags)
    dt = cache.config.act_dtype
    up, gate, down = layer(cache, bit, n), layer(cache, bit, n), layer(cache, bit, n, k=N, n_out=K)
    if n or bit == 4:
        gate.forward_without_precondition_len = 3
        cache.ind = up.ind
    if takeover:                         # gate_proj has not seen up_proj's outlier columns yet: it dequantises its own on the first forward
        gate.ind, gate.weight_cache, gate.forward_without_precondition_len = IND3[:0].to(device), None, -1
        cache.new_ind = up.ind
    norm = F.FasterTransformerRMSNorm(torch.ones(K, dtype=dt, device=device), cache=cache)
    norm.next_layer = up
    mlp = F.MixLlamaMLP(gate, down, up, cache)
    outs = []
    for _ in range(rounds):
        x = rand((M, K), dt, device)
        h = norm(x)
        res = {"residual": rand((M, K), dt, device)} if residual else {}
        outs += [h, mlp(h, **res)]
    return outs


def norm_alone(M=16, device="cpu", **flags):
    cache = cache_of(device=device, **flags)
    dt = cache.config.act_dtype
    norm = F.FasterTransformerRMSNorm(torch.ones(K, dtype=dt, device=device), cache=cache)
    return norm(rand((M, K), dt, device))


BF = dict(dt=BF16)
LAYER_SCENARIOS = []                     # (name, fn(device=...)) - what the GPU twin runs for real


def _layer_scenarios():
    S = LAYER_SCENARIOS
    for M in (16, 48):
        for bit in (8, 4):
            for name, flags in (("fp16", {}), ("bf16", BF), ("bf16-fused", dict(BF, fused_bf16=True)),
                                ("bf16-joint", dict(BF, fused_bf16=True, joint_gate_up_bf16=True)), ("bf16-w8a16", dict(BF, w8a16_bf16=True)),
                                ("bf16-decode", dict(BF, decode_bf16=True))):
                lone = name in ("fp16", "bf16", "bf16-decode")       # (the other three flags do not concern a lone layer: shown once each)
                for one in (True, False) if lone else (True,) if M == 16 else ():
                    S.append((f"layer/W{bit}/{name}/M{M}/one_call={int(one)}",
                              lambda device="cpu", M=M, bit=bit, flags=flags, one=one: frozen_layer(M, bit, device=device, runs=2, one_call_forward=one, **flags)))
            for name, flags in (("fp16", {}), ("bf16-decode", dict(BF, decode_bf16=True))):
                S.append((f"layer/W{bit}/{name}/M{M}/residual",
                          lambda device="cpu", M=M, bit=bit, flags=flags: frozen_layer(M, bit, residual=True, device=device, **flags)))
                S.append((f"layer/W{bit}/{name}/M{M}/residual/two_call",
                          lambda device="cpu", M=M, bit=bit, flags=flags: frozen_layer(M, bit, residual=True, device=device, one_call_forward=False, **flags)))
        for name, flags in (("fp16", {}), ("bf16-decode", dict(BF, decode_bf16=True))):
            S.append((f"layer/W4/{name}/M{M}/small_batch_m4",
                      lambda device="cpu", M=M, flags=flags: frozen_layer(M, 4, device=device, runs=2, small_batch_m4=32, **flags)))
        for name, flags in (("fp16", {}), ("bf16", dict(BF, w8a16_bf16=True))):
            for res in (False, True):
                S.append((f"weight_only/{name}/M{M}/residual={int(res)}",
                          lambda device="cpu", M=M, flags=flags, res=res: weight_only_layer(M, res, device=device, **flags)))
        joint_bf16 = dict(BF, fused_bf16=True, joint_gate_up_bf16=True)
        for bit in (8, 4):
            # fp16 and bf16 with the joint launch: every route at M = 16, the main one of each launch form at M = 48 too.  fused_bf16 alone has no
            # joint route; decode_bf16 moves no call that asks for a row maximum.
            for name, flags, joints, amaxes in (("fp16", {}, (True, False), (True, False)), ("bf16-joint", joint_bf16, (True, False), (True, False)),
                                                ("bf16", dict(BF, fused_bf16=True), (True,), (True, False)),
                                                ("bf16-joint-decode", dict(joint_bf16, decode_bf16=True), (True, False), (True,))):
                for joint in joints:
                    for amax in amaxes if M == 16 else (True,):
                        S.append((f"mlp/W{bit}/{name}/M{M}/joint={int(joint)}/amax={int(amax)}",
                                  lambda device="cpu", M=M, bit=bit, flags=flags, joint=joint, amax=amax:
                                  mlp_block(M, bit, device=device, rounds=2 if amax else 1, joint_gate_up=joint, fuse_down_amax=amax, **flags)))
                    if len(amaxes) == 2 and M == 16:
                        S.append((f"mlp/W{bit}/{name}/M{M}/joint={int(joint)}/residual",
                                  lambda device="cpu", M=M, bit=bit, flags=flags, joint=joint: mlp_block(M, bit, residual=True, device=device, joint_gate_up=joint, **flags)))
        S.append((f"mlp/W8/fp16/M{M}/takeover", lambda device="cpu", M=M: mlp_block(M, 8, takeover=True, device=device, joint_gate_up=False)))
        S.append((f"mlp/W8/fp16/M{M}/no_outliers", lambda device="cpu", M=M: mlp_block(M, 8, n=0, device=device)))
        for name, flags in (("fp16", {}), ("bf16", dict(BF, fused_bf16=True))):
            S.append((f"norm/{name}/M{M}/alone", lambda device="cpu", M=M, flags=flags: norm_alone(M, device=device, **flags)))


_layer_scenarios()


# ------------------------------------------------------------------------------------------------------------
# the scenario list
# ------------------------------------------------------------------------------------------------------------
SCENARIOS = []


def _add(name, fn, hide=()):
    SCENARIOS.append((name, fn, hide))


def _direct_scenarios():
    acts = {"none": ACT_NONE, "silu": ACT_SILU, "silu_mul": ACT_SILU_MUL, "pair": ACT_SILU_PAIR}
    for dn, dt in DT.items():
        for bit in (8, 4):
            for an, act in acts.items():
                for M in (16, 48) if act == ACT_NONE else (16,):     # (the batch size moves nothing in this layer: shown for one act)
                    for n in (0, 3):
                        mul = {"addend": z(M, N, dtype=dt)} if act == ACT_SILU_MUL else {}
                        _add(f"FusedLinear/W{bit}/{dn}/{an}/M{M}/n{n}", lambda M=M, bit=bit, dt=dt, act=act, n=n, mul=mul: fused_linear(M, bit, dt, act, n, **mul))
            _add(f"FusedLinear/W{bit}/{dn}/addend=zero_tag", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, addend=zero_tag()))
            _add(f"FusedLinear/W{bit}/{dn}/addend=real", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, addend=z(16, N + 8, dtype=dt)[:, :N]))
            _add(f"FusedLinear/W{bit}/{dn}/addend=misaligned", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, addend=misaligned(16, N, dt)))
            _add(f"FusedLinear/W{bit}/{dn}/silu_mul/addend=misaligned", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, ACT_SILU_MUL, addend=misaligned(16, N, dt)))
            _add(f"FusedLinear/W{bit}/{dn}/out=given", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, out=z(16, N + 8, dtype=dt)[:, :N]))
            _add(f"FusedLinear/W{bit}/{dn}/pair/out=given", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, ACT_SILU_PAIR, out=z(16, N, dtype=dt)))
            _add(f"FusedLinear/W{bit}/{dn}/decode/M16", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, decode=True, w_fmt=None if bit == 8 else FMT_P16X64,
                                                                                        x_fmt=None if bit == 8 else FMT_P16X64, addend=z(16, N, dtype=dt)))
            _add(f"FusedLinear/W{bit}/{dn}/decode/pair", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, ACT_SILU_PAIR, decode=True))
            _add(f"FusedLinear/W{bit}/{dn}/row_amax/decode", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, decode=True, **amax_args()))
            for an in ("none", "silu_mul", "pair"):
                mul = {"addend": z(16, N, dtype=dt)} if an == "silu_mul" else {}
                _add(f"FusedLinear/W{bit}/{dn}/row_amax/{an}", lambda bit=bit, dt=dt, an=an, mul=mul: fused_linear(16, bit, dt, acts[an], **mul, **amax_args()))
            _add(f"FusedLinear/W{bit}/{dn}/plain_operands", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, x_fmt=FMT_PLAIN, w_fmt=FMT_PLAIN))
            _add(f"FusedLinear/W{bit}/{dn}/x_packed=True", lambda bit=bit, dt=dt: fused_linear(16, bit, dt, x_fmt=FMT_PLAIN, w_fmt=FMT_PLAIN, x_packed=True, w_packed=True))
            # ForwardPlan: build and run
            for M in (16, 48):
                for n in (0, 3):
                    _add(f"ForwardPlan/W{bit}/{dn}/M{M}/n{n}", lambda M=M, bit=bit, dt=dt, n=n: plan(M, bit, dt, n, kept=True).run(z(M, K, dtype=dt)))
            _add(f"ForwardPlan/W{bit}/{dn}/addend", lambda bit=bit, dt=dt: plan(16, bit, dt).run(z(16, K, dtype=dt), addend=z(16, N + 4, dtype=dt)[:, :N]))
            _add(f"ForwardPlan/W{bit}/{dn}/addend=misaligned", lambda bit=bit, dt=dt: plan(16, bit, dt).run(z(16, K, dtype=dt), addend=misaligned(16, N, dt)))
            _add(f"ForwardPlan/W{bit}/{dn}/addend_then_none", lambda bit=bit, dt=dt: (lambda p: [p.run(z(16, K, dtype=dt), addend=z(16, N, dtype=dt)), p.run(z(16, K, dtype=dt))])(plan(16, bit, dt)))
            _add(f"ForwardPlan/W{bit}/{dn}/row_amax", lambda bit=bit, dt=dt: plan(16, bit, dt).run(z(16, K, dtype=dt), row_amax=z(64, dtype=torch.int32), col_mask=L.kept_outlier_map(IND3, K)))
            _add(f"ForwardPlan/W{bit}/{dn}/decode", lambda bit=bit, dt=dt: plan(16, bit, dt, decode=True).run(z(16, K, dtype=dt)))
            _add(f"ForwardPlan/W{bit}/{dn}/decode/pair", lambda bit=bit, dt=dt: plan(16, bit, dt, decode=True, act=ACT_SILU_PAIR))
            _add(f"ForwardPlan/W{bit}/{dn}/ldx", lambda bit=bit, dt=dt: plan(16, bit, dt, ldx=K + 8).run(z(16, K + 8, dtype=dt)[:, :K]))
            # the quantise family
            for fmt in (FMT_PLAIN, FMT_P16X64, FMT_F16X64) + ((FMT_F6X128, FMT_R6X128) if bit == 4 else ()):
                for n, masked in ((0, False), (3, False), (3, True)) + (((0, True),) if fmt == FMT_P16X64 else ()):      # (a map without columns: the unmasked call)
                    _add(f"QuantFused/W{bit}/{dn}/fmt{fmt}/n{n}/masked={int(masked)}", lambda bit=bit, dt=dt, fmt=fmt, n=n, masked=masked: quant_fused(16, bit, dt, fmt, n, masked))
                    _add(f"RMSNormQuantFused/W{bit}/{dn}/fmt{fmt}/n{n}/masked={int(masked)}", lambda bit=bit, dt=dt, fmt=fmt, n=n, masked=masked: norm_quant(48, bit, dt, fmt, n, masked))
                if fmt != FMT_PLAIN:
                    _add(f"FindRowScalePacked/W{bit}/{dn}/fmt{fmt}", lambda bit=bit, dt=dt, fmt=fmt: mixlib.FindRowScalePacked(z(48, K + 8, dtype=dt)[:, :K], z(64, 1), 48, K, bit, fmt))
            _add(f"QuantFused/W{bit}/{dn}/packed=True", lambda bit=bit, dt=dt: quant_fused(16, bit, dt, None, packed=True))
            _add(f"QuantFused/W{bit}/{dn}/x_out=given", lambda bit=bit, dt=dt: quant_fused(16, bit, dt, x_out=z(16, 32, dtype=dt)))
            _add(f"QuantFused/W{bit}/{dn}/no_n_dev", lambda bit=bit, dt=dt: mixlib.QuantFused(z(16, K, dtype=dt), IND3, z(64, 1), bit, 6))
            _add(f"RMSNormQuantFused/W{bit}/{dn}/3d", lambda bit=bit, dt=dt: mixlib.RMSNormQuantFused(z(2, 8, K, dtype=dt), z(K, dtype=dt), z(2, 8, K, dtype=dt), 1e-5, IND3, z(64, 1), bit, flag=z(1, dtype=torch.int32), packed=True))
            _add(f"FindRowScale/W{bit}/{dn}", lambda bit=bit, dt=dt: mixlib.FindRowScale(z(2, 8, K, dtype=dt), z(64, 1), 16, K, bit))
            _add(f"FindRowScale/W{bit}/{dn}/packed_operands", lambda bit=bit, dt=dt: _with(dict(packed_operands=True), lambda: mixlib.FindRowScale(z(16, K, dtype=dt), z(64, 1), 16, K, bit)))
        _add(f"ExtractOutliersAndSetToZeros/{dn}", lambda dt=dt: mixlib.ExtractOutliersAndSetToZeros(IND3, z(16, K, dtype=dt)))
        _add(f"ExtractOutliersAndSetToZeros/{dn}/n0", lambda dt=dt: mixlib.ExtractOutliersAndSetToZeros(IND3[:0], z(16, K, dtype=dt)))
        _add(f"ExtractOutliersAndSetToZeros/{dn}/fused_outliers", lambda dt=dt: _with(dict(fused_outliers=True), lambda: mixlib.ExtractOutliersAndSetToZeros(IND3, z(16, K, dtype=dt))))
        _add(f"DetectOutlierCols/{dn}", lambda dt=dt: mixlib.DetectOutlierCols(z(16, K, dtype=dt), 6.0))
        _add(f"layernorm_forward_cuda/{dn}", lambda dt=dt: mixlib.layernorm_forward_cuda(z(2, 8, K, dtype=dt), z(K, dtype=dt), z(2, 8, K, dtype=dt), 1e-6))
        _add(f"layernorm_extract/{dn}", lambda dt=dt: mixlib.layernorm_forward_cuda_extract_outliers(z(16, K, dtype=dt), z(K, dtype=dt), z(16, K, dtype=dt), 1e-6, IND3, z(64, 1)))
        _add(f"layernorm_extract/{dn}/n0", lambda dt=dt: mixlib.layernorm_forward_cuda_extract_outliers(z(16, K, dtype=dt), z(K, dtype=dt), z(16, K, dtype=dt), 1e-6, None, z(64, 1)))
        _add(f"layernorm_extract_int4/{dn}", lambda dt=dt: mixlib.layernorm_forward_cuda_extract_outliers_int4(z(16, K, dtype=dt), z(K, dtype=dt), z(16, K, dtype=dt), 1e-6, IND3, z(64, 1)))
        _add(f"amax_supported/{dn}", lambda dt=dt: [mixlib.amax_supported(M, N, K, FMT_P16X64, w, dtype=dt) for M in (16, 48) for w in (FMT_F16X64, FMT_P16X64)])
        # weight-only
        _add(f"PackW8A16/{dn}", lambda dt=dt: mixlib.PackW8A16(z(K, N, dtype=torch.int8), dt))
        for M in (16, 48):
            _add(f"W8A16Linear/{dn}/M{M}", lambda dt=dt, M=M: mixlib.W8A16Linear(z(M, K, dtype=dt), mixlib.PackW8A16(z(K, N, dtype=torch.int8), dt), z(N), z(N), N, K))
        _add(f"W8A16Linear/{dn}/addend", lambda dt=dt: mixlib.W8A16Linear(z(2, 8, K, dtype=dt), mixlib.PackW8A16(z(K, N, dtype=torch.int8), dt), z(N), None, N, K, addend=z(16, N + 4, dtype=dt)[:, :N]))
        _add(f"W8A16Linear/{dn}/addend=misaligned/out", lambda dt=dt: mixlib.W8A16Linear(z(16, K, dtype=dt), mixlib.PackW8A16(z(K, N, dtype=torch.int8), dt), z(N), z(N), N, K,
                                                                                         out=z(16, N + 8, dtype=dt)[:, :N], addend=misaligned(16, N, dt)))
        _add(f"W8A16Linear/{dn}/x_strided", lambda dt=dt: mixlib.W8A16Linear(z(16, K + 4, dtype=dt)[:, :K], mixlib.PackW8A16(z(K, N, dtype=torch.int8), dt), z(N), z(N), N, K))
        _add(f"W8A16Linear/{dn}/M0", lambda dt=dt: mixlib.W8A16Linear(z(0, K, dtype=dt), mixlib.PackW8A16(z(K, N, dtype=torch.int8), dt), z(N), z(N), N, K))
    _add("decode_pick", lambda: [mixlib.decode_pick(M, N, K, bit, x, w) for M in (16, 48) for bit in (8, 4) for x, w in ((FMT_P16X64, FMT_F16X64), (FMT_P16X64, FMT_P16X64), (FMT_PLAIN, FMT_PLAIN))])
    _add("DequantWeightCols/W8", lambda: mixlib.DequantWeightCols(z(N, K, dtype=torch.int8), z(1, N), IND3, 8))
    _add("DequantWeightCols/W4/out", lambda: mixlib.DequantWeightCols(z(N, K // 2, dtype=torch.uint8), z(1, N), IND3, 4, out=z(N, 16)[:, :3]))
    _add("DequantWeightCols/n0", lambda: mixlib.DequantWeightCols(z(N, K, dtype=torch.int8), z(1, N), IND3[:0], 8))
    _add("unpack_int4_to_fp16", lambda: mixlib.unpack_int4_to_fp16(z(N, K // 2, dtype=torch.uint8), IND3))
    for fmt in (FMT_P16X64, FMT_F16X64, FMT_F6X128, FMT_R6X128):
        _add(f"PackOperand/fmt{fmt}", lambda fmt=fmt: mixlib.PackOperand(z(N + 3, K // 2, dtype=torch.uint8), fmt))
        _add(f"UnpackOperand/fmt{fmt}", lambda fmt=fmt: mixlib.UnpackOperand(mixlib.PackOperand(z(N + 3, K // 2, dtype=torch.uint8), fmt), N + 3))
    _add("PackP16x64", lambda: mixlib.PackP16x64(z(N, K, dtype=torch.int8)))
    _add("UnpackOperand/fmt=arg", lambda: mixlib.UnpackOperand(z(N, K, dtype=torch.int8), N, FMT_F16X64))
    # the reference surface under each shim configuration
    for cn, cfg in (("default", mixlib.ShimConfig()), ("literal", mixlib.ShimConfig.literal()), ("fastest", mixlib.ShimConfig.fastest()),
                    ("fused_outliers", mixlib.ShimConfig(fused_outliers=True)), ("packed_operands", mixlib.ShimConfig(packed_operands=True))):
        for silu in (False, True):
            _add(f"shim/{cn}/silu={int(silu)}", lambda cfg=cfg, silu=silu: reference_sequence(cfg, silu=silu))
        _add(f"shim/{cn}/M48", lambda cfg=cfg: reference_sequence(cfg, M=48))
    _add("shim/fastest/product_read", lambda: _with(mixlib.ShimConfig.fastest(), lambda: (lambda r: [r[2] + 0, r[3] + 0])(reference_sequence(mixlib.ShimConfig.fastest()))))
    _add("shim/fastest/extract_read", lambda: _with(mixlib.ShimConfig.fastest(), lambda: mixlib.ExtractOutliersAndSetToZeros(IND3, z(16, K)) + 0))
    _add("shim/fastest/extract_twice", lambda: _with(mixlib.ShimConfig.fastest(), lambda: [mixlib.ExtractOutliersAndSetToZeros(IND3, z(16, K)) for _ in range(2)]))
    for bit, name in ((8, "int8FusedDequantize"), (8, "int8FusedDequantizeSilu"), (4, "int4FusedDequantize"), (4, "int4FusedDequantizeSilu")):
        for an, mk in (("zero_tag", zero_tag), ("real", lambda: z(16, N + 8)[:, :N]), ("none", lambda: None)):
            _add(f"{name}/addend={an}", lambda bit=bit, name=name, mk=mk: getattr(mixlib, name)(qx(16, bit, FMT_PLAIN), qw(bit, FMT_PLAIN), z(64, 1), z(1, N), mk(), 16, N,
                                                                                            K if bit == 8 else K // 2))
    _add("gemm/literal+dequantizeInt8/addend=real", lambda: _with(mixlib.ShimConfig.literal(), lambda: mixlib.dequantizeInt8(
        mixlib.gemm(qx(16, 8, FMT_PLAIN), qw(8, FMT_PLAIN), 16, N, K), z(64, 1), z(1, N), z(16, N), 8, 16, N)))


def _with(cfg, fn):
    with (mixlib.configured(cfg) if isinstance(cfg, mixlib.ShimConfig) else mixlib.configured(**cfg)):
        return fn()


def _refusal_scenarios():
    R = lambda name, fn, hide=(): _add("refuse/" + name, fn, hide)
    R("_rows/3d", lambda: mixlib.ExtractOutliersAndSetToZeros(IND3, z(2, 8, K)))
    for who, mk in (("dim", lambda: z(16)), ("shape", lambda: z(8, N)), ("stride1", lambda: z(N, 16).t()), ("stride0", lambda: z(16, N + 2)[:, :N]),
                    ("align", lambda: misaligned(16, N, F16))):
        R(f"_check_out/{who}", lambda mk=mk: fused_linear(out=mk()))
    R("_check_ind", lambda: mixlib.DequantWeightCols(z(N, K, dtype=torch.int8), z(1, N), IND3.long(), 8))
    R("_layout_bits/fp6", lambda: fused_linear(bit=4, x_fmt=FMT_P16X64, w_fmt=FMT_F6X128))
    R("_layout_bits/f16x64_x", lambda: fused_linear(x_fmt=FMT_F16X64))
    R("configure/fused_prepass", lambda: mixlib.configure(fused_prepass=True))
    R("_act_suffix", lambda: mixlib.FindRowScale(z(16, K, dtype=torch.float32), z(64, 1), 16, K))
    R("FindRowScale/x_scale", lambda: mixlib.FindRowScale(z(16, K), z(64, 1, dtype=BF16), 16, K))
    R("FindRowScale/shape", lambda: mixlib.FindRowScale(z(16, K), z(64, 1), 16, K + 64))
    R("FindRowScale/bit", lambda: mixlib.FindRowScale(z(16, K), z(64, 1), 16, K, 2))
    R("Extract/bf16_fused_outliers", lambda: _with(dict(fused_outliers=True), lambda: mixlib.ExtractOutliersAndSetToZeros(IND3, z(16, K, dtype=BF16))))
    R("_fused_dequant/packed_plain", lambda: mixlib.int8FusedDequantize(qx(16), z(N, 32, dtype=torch.int8), z(64, 1), z(1, N), None, 16, N, 32))
    R("gemm/packed", lambda: _with(mixlib.ShimConfig.literal(), lambda: mixlib.gemm(qx(16), qw(8, FMT_PLAIN), 16, N, K)))
    R("gemm/eshape", lambda: mixlib.gemm(qx(16, 8, FMT_PLAIN), qw(8, FMT_PLAIN), 16, N, K - 32))
    R("gemm/operands", lambda: mixlib.gemm(qx(16, 4, FMT_PLAIN), qw(4, FMT_PLAIN), 16, N, K))
    R("unpack_int4/contiguous", lambda: mixlib.unpack_int4_to_fp16(z(K // 2, N, dtype=torch.uint8).t(), IND3))
    R("PackOperand", lambda: mixlib.PackOperand(z(N, K)))
    R("UnpackOperand/untagged", lambda: mixlib.UnpackOperand(z(N, K, dtype=torch.int8), N))
    R("_q_row_bytes/fp6_bit8", lambda: quant_fused(bit=8, fmt=FMT_R6X128))
    R("_check_kept_map", lambda: mixlib.QuantFused(z(16, K), IND3, z(64, 1), 8, 6.0, col_mask=z(8, dtype=torch.int32)))
    R("QuantFused/x_scale", lambda: mixlib.QuantFused(z(16, K), IND3, z(8, 1), 8, 6.0))
    R("QuantFused/x_out_dtype", lambda: quant_fused(x_out=z(16, 16, dtype=BF16)))
    R("FindRowScalePacked/x_scale", lambda: mixlib.FindRowScalePacked(z(16, K), z(8, 1), 16, K))
    R("DequantWeightCols/q_w", lambda: mixlib.DequantWeightCols(qw(), z(1, N), IND3, 8))
    for name in ("mixq_gemm_i8_pair_bf16", "mixq_gemm_i4_pair_bf16"):
        R(f"missing/{name}", lambda name=name: fused_linear(16, 8 if "i8" in name else 4, BF16, ACT_SILU_PAIR), hide=(name,))
        R(f"_pair_bf16_entry/{name}", lambda name=name: mixlib._pair_bf16_entry(name), hide=(name,))
    for name in ("mixq_gemm_i8_decode_bf16", "mixq_gemm_i4_decode_bf16"):
        R(f"missing/{name}", lambda name=name: fused_linear(16, 8 if "i8" in name else 4, BF16, decode=True), hide=(name,))
        R(f"_decode_bf16_entry/{name}", lambda name=name: mixlib._decode_bf16_entry(name), hide=(name,))
    R("missing/mixq_gemm_decode_pick_bf16", lambda: mixlib.decode_pick(16, N, K, 8, FMT_P16X64, FMT_F16X64), hide=("mixq_gemm_decode_pick_bf16",))
    R("missing/mixq_linear_forward_decode_bf16", lambda: plan(16, 8, BF16, decode=True), hide=("mixq_linear_forward_decode_bf16",))
    R("missing/mixq_pack_w8a16_bf16", lambda: mixlib.PackW8A16(z(K, N, dtype=torch.int8), BF16), hide=("mixq_pack_w8a16_bf16",))
    R("missing/mixq_gemm_w8a16_bf16", lambda: mixlib.W8A16Linear(z(16, K, dtype=BF16), mixlib.PackW8A16(z(K, N, dtype=torch.int8), BF16), z(N), z(N), N, K),
      hide=("mixq_gemm_w8a16_bf16",))
    R("_check_same_dtype/x_out", lambda: mixlib.FusedLinear(qx(16), qw(), z(64, 1), z(1, N), z(16, 16, dtype=BF16), z(N, 16), 3, None, 16, N, K))
    R("_check_same_dtype/out", lambda: fused_linear(out=z(16, N, dtype=BF16)))
    R("_check_same_dtype/addend", lambda: fused_linear(addend=z(16, N, dtype=BF16)))
    R("_check_same_dtype/multiplier", lambda: fused_linear(act=ACT_SILU_MUL, addend=z(16, N, dtype=BF16)))
    R("FusedLinear/decode_fp16", lambda: fused_linear(decode=True))
    R("FusedLinear/decode_amax", lambda: fused_linear(dt=BF16, decode=True, **amax_args()))
    R("FusedLinear/decode_pair", lambda: fused_linear(dt=BF16, act=ACT_SILU_PAIR, decode=True))
    R("FusedLinear/scales_short", lambda: mixlib.FusedLinear(qx(16), qw(), z(8, 1), z(1, N), None, None, 0, None, 16, N, K))
    R("FusedLinear/pair_addend", lambda: fused_linear(act=ACT_SILU_PAIR, addend=z(16, N)))
    R("FusedLinear/mul_missing", lambda: fused_linear(act=ACT_SILU_MUL))
    R("FusedLinear/row_amax_bit4", lambda: fused_linear(bit=4, **amax_args()))
    R("FusedLinear/dtype", lambda: mixlib.FusedLinear(qx(16), qw(), z(64, 1), z(1, N), None, None, 0, None, 16, N, K, dtype=torch.float32))
    R("ForwardPlan/decode_fp16", lambda: plan(decode=True))
    R("ForwardPlan/decode_pair", lambda: plan(dt=BF16, decode=True, act=ACT_SILU_PAIR))
    R("ForwardPlan/scales_short", lambda: mixlib.ForwardPlan(96, N, K, 8, 6.0, K, None, 0, None, z(64, 1), qw(), z(1, N), None, None, FMT_P16X64))
    R("ForwardPlan/w_out_dtype", lambda: mixlib.ForwardPlan(16, N, K, 8, 6.0, K, *ind_cap(3)[:1], 3, ind_cap(3)[1], z(64, 1), qw(), z(1, N), z(N, 16, dtype=BF16), None, FMT_P16X64))
    R("ForwardPlan/w_out_stride", lambda: mixlib.ForwardPlan(16, N, K, 8, 6.0, K, *ind_cap(3)[:1], 3, ind_cap(3)[1], z(64, 1), qw(), z(1, N), z(N, 12), None, FMT_P16X64))
    R("ForwardPlan.run/addend_type", lambda: plan().run(z(16, K), addend=1.0))
    R("ForwardPlan.run/addend_shape", lambda: plan().run(z(16, K), addend=z(16, N + 1)))
    R("ForwardPlan.run/x_dtype", lambda: plan().run(z(16, K, dtype=BF16)))
    R("ForwardPlan.run/x_stride", lambda: plan().run(z(16, K + 8)[:, :K]))
    R("ForwardPlan.run/col_mask", lambda: plan().run(z(16, K), col_mask=z(4, dtype=torch.int32)))
    R("_check_norm_dtypes", lambda: mixlib.layernorm_forward_cuda(z(16, K), z(K, dtype=BF16), z(16, K), 1e-6))
    R("RMSNormQuantFused/x_scale_dtype", lambda: mixlib.RMSNormQuantFused(z(16, K, dtype=BF16), z(K, dtype=BF16), z(16, K, dtype=BF16), 1e-6, None, z(64, 1, dtype=BF16), 8))
    R("RMSNormQuantFused/x_scale", lambda: mixlib.RMSNormQuantFused(z(16, K), z(K), z(16, K), 1e-6, None, z(8, 1), 8))
    R("PackW8A16/tensor", lambda: mixlib.PackW8A16(z(K, N)))
    R("PackW8A16/dtype", lambda: mixlib.PackW8A16(z(K, N, dtype=torch.int8), torch.float32))
    pk = lambda dt=F16: mixlib.PackW8A16(z(K, N, dtype=torch.int8), dt)
    R("W8A16Linear/x_dtype", lambda: mixlib.W8A16Linear(z(16, K, dtype=torch.float32), pk(), z(N), None, N, K))
    R("W8A16Linear/bf16_scale", lambda: mixlib.W8A16Linear(z(16, K, dtype=BF16), pk(BF16), z(N, dtype=BF16), None, N, K))
    R("W8A16Linear/bf16_image", lambda: mixlib.W8A16Linear(z(16, K, dtype=BF16), pk(), z(N), None, N, K))
    R("W8A16Linear/fp16_image", lambda: mixlib.W8A16Linear(z(16, K), pk(BF16), z(N), None, N, K))
    R("W8A16Linear/shape", lambda: mixlib.W8A16Linear(z(16, K), pk(), z(N + 1), None, N, K))
    R("W8A16Linear/out_dtype", lambda: mixlib.W8A16Linear(z(16, K), pk(), z(N), None, N, K, out=z(16, N, dtype=BF16)))
    R("W8A16Linear/addend_dtype", lambda: mixlib.W8A16Linear(z(16, K), pk(), z(N), None, N, K, addend=z(16, N, dtype=BF16)))
    R("W8A16Linear/addend_shape", lambda: mixlib.W8A16Linear(z(16, K), pk(), z(N), None, N, K, addend=z(16, N + 2)[:, :N]))
    R("W8A16Linear/addend_alias", lambda: (lambda o: mixlib.W8A16Linear(z(16, K), pk(), z(N), None, N, K, out=o, addend=o))(z(16, N)))


# raise sites of mixlib.py the trace leaves out, with the reason (tests/test_host_calls.py checks the count against the file)
RAISES_LEFT_OUT = {
    "dev_check": "the recorder replaces it: a CPU tensor is what every scenario passes",
    "_check_out/device": "needs a second device",
    "ForwardPlan.run/addend device": "needs a second device (a non-tensor addend reaches the same raise: refuse/ForwardPlan.run/addend_type)",
    "ForwardPlan.run/x device": "needs a second device",
    "ForwardPlan.run/rc": "the recorder answers 0 to every launch",
    "decode_pick/rc": "the real query answers 0 or 1 for every problem it can be handed",
    "FusedLinear/pair rc, decode rc": "the recorder answers 0 to every launch",
    "W8A16Linear/addend device": "needs a second device (the dtype arm of the same raise: refuse/W8A16Linear/addend_dtype)",
}

_direct_scenarios()
_refusal_scenarios()
SCENARIOS += [(name, fn, ()) for name, fn in LAYER_SCENARIOS]
assert len({s[0] for s in SCENARIOS}) == len(SCENARIOS)


def record_all():
    return {s[0]: run(s) for s in SCENARIOS}


def dumps(table):
    return "{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in table.items()) + "\n}\n"
