#!/usr/bin/env python3
"""The frozen MixLinear_GEMM forward in bfloat16 next to the float16 forward, same process, bench.py's protocol (a hipGraph of --steps
forwards on pristine inputs, conditioned_replay: settle, then the median of back-to-back replays), the two dtypes ALTERNATING for
--rounds rounds so that both see the same box and the same clock history.  Default: the metric shape, 512 x 4096 -> 11008 with 41 outlier
columns.  Prints one JSON line: per dtype the us per forward of every round, their median and spread.

    python3 tools/bench_bf16.py [--bit 8|4] [--rounds 5] [--steps 20] [--once bf16] [--block]

--once DTYPE: build that layer, replay its graph for a profiler (rocprofv3 --kernel-trace --stats -- python3 tools/bench_bf16.py --once bf16);
  --once block_bf16_joint (or any other block form's name): the same for one form of --block.
--block: what a bfloat16 model gets with MixqConfig(fused_bf16=True), against float16, same protocol and the same alternating rounds:
  norm_quant   the fused norm + extract + quantise pass alone (mixlib.RMSNormQuantFused with the next layer's kept outlier map) on the
               metric's batch, 512 x 4096 with 41 kept outlier columns: mixq_rmsnorm_quant_fused_masked against its _bf16 twin
  block        FasterTransformerRMSNorm -> MixLlamaMLP at 4096 -> 11008 -> 4096, frozen, each dtype with the joint gate / up launch on and
               off: float16 as the model runs it (joint), float16 with joint_gate_up=False, bfloat16 as a fused_bf16 model runs it (the two
               launches), and bfloat16 with joint_gate_up_bf16=True (mixq_gemm_i8_pair_bf16 / mixq_gemm_i4_pair_bf16)
One JSON line: per form the us per call of every round, median, min, max; and what the joint launch saves in either dtype beside the
spread of the bfloat16 two-launch rounds.
--decode: MixqConfig.decode_bf16 off against on, the frozen bfloat16 forward (one call: quantise pass + GEMM) at M in {1, 16, 32} with
  HBM-COLD weights as tools/time_decode.py arranges them for float16: the launches of one hipGraph rotate through enough copies of the layer
  to exceed the 256 MB MALL, twice.  4096 -> 4096 and 11008 -> 4096 (the narrow layers of a Llama-7B block), W8 and W4 (flag on: the nibble
  image, small_batch_m4 = 32; flag off: the FP6 image), and 4096 -> 11008 as the control, where both configurations run the same kernel
  ("entry" in the output names the one-call entry point that ran).  Flag-off and flag-on rounds ALTERNATE on one box; flag off is the route (and the code object) of a library without the flag.  One
  JSON line per shape: per M the us per forward of every round, median, min, max, the off rounds' spread and on / off."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the protocol and the metric's shape, batches and outlier columns live there)
from mixq_amd import MixLibCache, MixLinear_GEMM, _capi, mixlib  # noqa: E402
from mixq_amd.config import MixqConfig  # noqa: E402


def build(dtype, device, rows, bit, steps, side):
    """A frozen layer of `dtype` and the captured graph of `steps` forwards; returns (graph, restore, layer, tiling name)."""
    torch.manual_seed(0)
    lin = torch.nn.Linear(bench.K, bench.N, bias=False).to(dtype)
    cache = MixLibCache(rows, sigma=bench.SIGMA, bit=bit, device=device, config=MixqConfig(act_dtype=dtype))
    kw = {}
    if bit == 4:                                                     # (bench.build_layer: the batch's outlier columns among the 128 static ones)
        scales = torch.ones(bench.K) + torch.arange(bench.K) * 1e-6
        cols = bench.outlier_columns(bench.K)
        scales[cols] = 20.0 + torch.arange(cols.numel()) * 1e-3
        kw["layer_scales"] = scales
    layer = MixLinear_GEMM.from_linear(lin, bit, cache=cache, dev=device, name="up_proj", **kw)
    _, base, pristine = bench.make_batches(steps, rows, device, 0)
    base, pristine = base.to(dtype), pristine.to(dtype)               # the fp16 batch rounded to the container (|x| <= ~100)
    nbuf = pristine.shape[0]
    for _ in range(3):
        layer(base.clone(), None, True)
    torch.cuda.synchronize()
    assert layer.add_outliers is False
    restore = lambda: pristine.copy_(base.unsqueeze(0).expand_as(pristine))
    with torch.cuda.stream(side):
        for i in range(3):
            y = layer(pristine[i % nbuf], None, True)
        torch.cuda.synchronize()
        assert y.dtype == dtype
        restore()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(steps):
                layer(pristine[i % nbuf], None, True)
        torch.cuda.synchronize()
    lib = _capi.load()
    names = _capi.gemm_config_names()
    # (the fp16 choice; the bf16 forms pick by the same cost model over the tilings that have a bf16 form)
    cfg = names[lib.mixq_gemm_pick_config_fmt(rows, bench.N, bench.K, bit, mixlib.fmt_of(layer._wpk))]
    return g, restore, layer, cfg


def _capture(fn, steps, side, warm=4):
    """`steps` calls of fn(i) as one hipGraph on the side stream, after `warm` eager calls there."""
    with torch.cuda.stream(side):
        for i in range(warm):
            fn(i % steps)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(steps):
                fn(i)
        torch.cuda.synchronize()
    return g


def build_norm_quant(dtype, device, rows, bit, steps, side):
    """The fused norm + extract + quantise pass of a frozen next layer: (graph, restore)."""
    from mixq_amd.linear import kept_outlier_map
    cols, base, _ = bench.make_batches(1, rows, device, 0)
    base = base.to(dtype)
    ind = cols.to(torch.int32).to(device)
    cmap = kept_outlier_map(ind, bench.K)
    torch.manual_seed(3)
    w = (torch.rand(bench.K) + 0.5).to(dtype).to(device)
    xs = torch.zeros((rows, 1), dtype=torch.float16, device=device)
    out = torch.empty_like(base)
    fmt = _capi.FMT_P16X64 if bit == 8 else _capi.FMT_R6X128
    g = _capture(lambda i: mixlib.RMSNormQuantFused(base, w, out, 1e-5, ind, xs, bit, fmt=fmt, col_mask=cmap), steps, side)
    return g, None, int(ind.numel())


def build_block(dtype, device, rows, bit, steps, side, joint):
    """norm -> MixLlamaMLP of bench.py's secondary block figure (up / gate of `bit` bits, an 8-bit down_proj), frozen: (graph, restore).
    joint: the joint gate / up launch - joint_gate_up for float16; bfloat16 keeps that switch on and takes joint_gate_up_bf16."""
    from mixq_amd import FasterTransformerRMSNorm, MixLlamaMLP
    bf = dtype == torch.bfloat16
    cfg = MixqConfig(act_dtype=dtype, fused_bf16=bf, joint_gate_up=True if bf else joint, joint_gate_up_bf16=bf and joint)
    cache = MixLibCache(rows, sigma=bench.SIGMA, bit=bit, device=device, config=cfg)

    def make(seed, k, n, b, name):
        torch.manual_seed(seed)
        kw = {}
        if b == 4:
            scales = torch.ones(k) + torch.arange(k) * 1e-6
            cols = bench.outlier_columns(k)
            scales[cols] = 20.0 + torch.arange(cols.numel()) * 1e-3
            kw["layer_scales"] = scales
        return MixLinear_GEMM.from_linear(torch.nn.Linear(k, n, bias=False).to(dtype), b, cache=cache, dev=device, name=name, **kw)
    up, gate, down = make(21, bench.K, bench.N, bit, "up_proj"), make(22, bench.K, bench.N, bit, "gate_proj"), make(23, bench.N, bench.K, 8, "down_proj")
    torch.manual_seed(3)
    norm = FasterTransformerRMSNorm((torch.rand(bench.K) + 0.5).to(dtype).to(device), 1e-5, cache)
    norm.next_layer = up
    block = MixLlamaMLP(gate, down, up, cache)
    _, base, _ = bench.make_batches(1, rows, device, 0)
    base = base.to(dtype)
    bx = base.unsqueeze(0).repeat(steps, 1, 1).contiguous()
    for _ in range(4):
        block(norm(base.clone()))                            # freezes the predictions (and builds the joint image where it applies)
    torch.cuda.synchronize()
    assert not up.add_outliers and not down.add_outliers
    g = _capture(lambda i: block(norm(bx[i])), steps, side)
    return g, (lambda: bx.copy_(base.unsqueeze(0).expand_as(bx))), int(up.ind.numel()), block._joint is not None, (block, norm)


def block_mode(args, device, side):
    f16, bf = torch.float16, torch.bfloat16
    forms = {}
    forms["norm_quant_fp16"] = build_norm_quant(f16, device, args.batch, args.bit, args.steps, side)
    forms["norm_quant_bf16"] = build_norm_quant(bf, device, args.batch, args.bit, args.steps, side)
    forms["block_fp16"] = build_block(f16, device, args.batch, args.bit, args.steps, side, True)
    forms["block_fp16_two_launch"] = build_block(f16, device, args.batch, args.bit, args.steps, side, False)
    forms["block_bf16"] = build_block(bf, device, args.batch, args.bit, args.steps, side, False)
    forms["block_bf16_joint"] = build_block(bf, device, args.batch, args.bit, args.steps, side, True)
    assert [forms[n][3] for n in ("block_fp16", "block_fp16_two_launch", "block_bf16", "block_bf16_joint")] == [True, False, False, True]
    us = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, f in forms.items():
            ms, _, _ = bench.conditioned_replay(f[0], side, restore=f[1], replays=args.replays)
            us[name].append(round(ms * 1e3 / args.steps, 3))
    out = {"what": f"--block: fused norm + quantise ({args.batch} x {bench.K}, {forms['norm_quant_fp16'][2]} kept outlier columns, W{args.bit}) and norm -> MixLlamaMLP "
                   f"({bench.K} -> {bench.N} -> {bench.K}, up / gate W{args.bit}A{args.bit}, down W8A8, {forms['block_fp16'][2]} outlier columns of up_proj), "
                   f"hipGraph of {args.steps} calls, median of {args.replays} replays per round, {args.rounds} alternating rounds",
           "device": _capi.device_info()}
    for name in forms:
        v = sorted(us[name])
        out[name] = {"us_per_call_rounds": us[name], "median_us": bench.median(v), "min_us": v[0], "max_us": v[-1]}
        if name.startswith("block"):
            out[name]["joint_gate_up_launch"] = forms[name][3]
    out["norm_quant_bf16_over_fp16"] = round(out["norm_quant_bf16"]["median_us"] / out["norm_quant_fp16"]["median_us"], 4)
    out["block_bf16_over_fp16"] = round(out["block_bf16"]["median_us"] / out["block_fp16"]["median_us"], 4)
    out["block_bf16_over_fp16_two_launch"] = round(out["block_bf16"]["median_us"] / out["block_fp16_two_launch"]["median_us"], 4)
    out["block_bf16_joint_over_fp16"] = round(out["block_bf16_joint"]["median_us"] / out["block_fp16"]["median_us"], 4)
    # what the joint launch saves per block call, each dtype against its own two-launch form of the same rounds
    out["fp16_joint_saving_us"] = round(out["block_fp16_two_launch"]["median_us"] - out["block_fp16"]["median_us"], 3)
    out["bf16_joint_saving_us"] = round(out["block_bf16"]["median_us"] - out["block_bf16_joint"]["median_us"], 3)
    out["bf16_two_launch_spread_us"] = round(out["block_bf16"]["max_us"] - out["block_bf16"]["min_us"], 3)
    print(json.dumps(out))


def build_decode(device, K, N, bit, copies):
    """`copies` frozen bfloat16 layers K -> N over ONE shared config (the flag is flipped on it), and the outlier columns of the batch."""
    import copy
    cfg = MixqConfig(act_dtype=torch.bfloat16)
    cache = MixLibCache(32, sigma=bench.SIGMA, bit=bit, device=device, config=cfg)
    torch.manual_seed(0)
    kw = {}
    if bit == 4:
        scales = torch.ones(K) + torch.arange(K) * 1e-6
        cols = bench.outlier_columns(K)
        scales[cols] = 20.0 + torch.arange(cols.numel()) * 1e-3
        kw["layer_scales"] = scales
    first = MixLinear_GEMM.from_linear(torch.nn.Linear(K, N, bias=False).to(torch.bfloat16), bit, cache=cache, dev=device, **kw)
    _, base, _ = bench.make_batches(1, 32, device, 0, Kc=K)
    base = base.to(torch.bfloat16)
    for _ in range(3):
        first(base.clone(), None, True)
    torch.cuda.synchronize()
    assert first.add_outliers is False
    layers = [first] + [copy.deepcopy(first) for _ in range(copies - 1)]
    for l in layers:
        l.cache = cache
        l.config = cfg
    return layers, cfg, base


def decode_mode(args, device, side):
    shapes = [(4096, 4096), (11008, 4096), (4096, 11008)]
    for K, N in shapes:
        for bit in (8, 4):
            image = K * N * (1.0 if bit == 8 else 0.5)
            copies = max(2, int(300e6 // image) + 1)                         # > 256 MB of weights per pass through the graph
            layers, cfg, base = build_decode(device, K, N, bit, copies)
            steps = 2 * copies
            out = {"what": f"--decode: frozen bfloat16 MixLinear_GEMM W{bit}A{bit}O16 forward {K} -> {N}, {int(layers[0].ind.numel())} outlier columns, hipGraph of "
                           f"{steps} forwards over {copies} copies of the layer (HBM-cold weights), median of {args.replays} replays per round, {args.rounds} "
                           f"alternating rounds", "K": K, "N": N, "bit": bit, "device": _capi.device_info()}
            for M in (1, 16, 32):
                x0 = base[:M].contiguous()
                bx = x0.unsqueeze(0).repeat(steps, 1, 1).contiguous()
                restore = lambda bx=bx, x0=x0: bx.copy_(x0.unsqueeze(0).expand_as(bx))
                graphs, route = {}, {}
                for name, flag in (("off", False), ("on", True)):
                    cfg.decode_bf16 = flag
                    cfg.small_batch_m4 = 32 if (flag and bit == 4) else 0     # (flag off: a bf16 layer has no nibble route)
                    graphs[name] = _capture(lambda i: layers[i % copies](bx[i], None, True), steps, side, warm=copies)
                    route[name] = layers[0]._plan.fn_name
                    restore()
                us = {"off": [], "on": []}
                for _ in range(args.rounds):
                    for name in ("off", "on"):
                        ms, _, _ = bench.conditioned_replay(graphs[name], side, restore=restore, replays=args.replays)
                        us[name].append(round(ms * 1e3 / steps, 3))
                r = {}
                for name in ("off", "on"):
                    v = sorted(us[name])
                    r[name] = {"entry": route[name], "us_per_forward_rounds": us[name], "median_us": bench.median(v), "min_us": v[0], "max_us": v[-1]}
                r["off_spread_us"] = round(r["off"]["max_us"] - r["off"]["min_us"], 3)
                r["on_over_off"] = round(r["on"]["median_us"] / r["off"]["median_us"], 4)
                out[f"M{M}"] = r
                del graphs
            cfg.decode_bf16, cfg.small_batch_m4 = False, 0
            print(json.dumps(out), flush=True)
            del layers
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bit", type=int, choices=[8, 4], default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=31)
    ap.add_argument("--batch", type=int, default=bench.M)
    ap.add_argument("--once", choices=["fp16", "bf16", "block_fp16", "block_fp16_two_launch", "block_bf16", "block_bf16_joint"], default=None)
    ap.add_argument("--block", action="store_true", help="time the fused norm + quantise pass and the norm -> MLP block, bf16 against fp16")
    ap.add_argument("--decode", action="store_true", help="time MixqConfig.decode_bf16 off against on at M in {1, 16, 32}, HBM-cold weights")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_bf16.py needs an MI355X")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    side = torch.cuda.Stream()
    if args.once and args.once.startswith("block_"):
        dt = torch.float16 if "fp16" in args.once else torch.bfloat16
        f = build_block(dt, device, args.batch, args.bit, args.steps, side, args.once in ("block_fp16", "block_bf16_joint"))
        with torch.cuda.stream(side):
            for _ in range(50):
                f[1]()
                f[0].replay()
        torch.cuda.synchronize()
        print(f"{args.once}: 50 replays of {args.steps} block calls, joint gate / up launch: {f[3]}")
        return
    if args.decode:
        return decode_mode(args, device, side)
    if args.block:
        return block_mode(args, device, side)
    dtypes = {"fp16": torch.float16, "bf16": torch.bfloat16}
    if args.once:
        g, restore, layer, _ = build(dtypes[args.once], device, args.batch, args.bit, args.steps, side)
        with torch.cuda.stream(side):
            for _ in range(50):
                restore()
                g.replay()
        torch.cuda.synchronize()
        print(f"{args.once}: 50 replays of {args.steps} forwards, {int(layer.ind.numel())} outlier columns")
        return
    built = {name: build(dt, device, args.batch, args.bit, args.steps, side) for name, dt in dtypes.items()}
    us = {name: [] for name in dtypes}
    for _ in range(args.rounds):
        for name in dtypes:
            g, restore, _, _ = built[name]
            ms, _, _ = bench.conditioned_replay(g, side, restore=restore, replays=args.replays)
            us[name].append(round(ms * 1e3 / args.steps, 3))
    flops = 2.0 * args.batch * bench.N * bench.K
    out = {"what": f"frozen MixLinear_GEMM W{args.bit}A{args.bit}O16 forward, {args.batch} x {bench.K} -> {bench.N}, "
                   f"{int(built['fp16'][2].ind.numel())} outlier columns, hipGraph of {args.steps} forwards, median of {args.replays} replays per round",
           "fp16_tiling": built["fp16"][3], "device": _capi.device_info()}
    for name in dtypes:
        v = sorted(us[name])
        med = bench.median(v)
        out[name] = {"us_per_forward_rounds": us[name], "median_us": med, "min_us": v[0], "max_us": v[-1], "tflops_at_median": round(flops / med / 1e6, 1)}
    out["bf16_over_fp16"] = round(out["bf16"]["median_us"] / out["fp16"]["median_us"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
