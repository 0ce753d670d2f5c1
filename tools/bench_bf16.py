#!/usr/bin/env python3
"""The frozen MixLinear_GEMM forward in bfloat16 next to the float16 forward, same process, bench.py's protocol (a hipGraph of --steps
forwards on pristine inputs, conditioned_replay: settle, then the median of back-to-back replays), the two dtypes ALTERNATING for
--rounds rounds so that both see the same box and the same clock history.  Default: the metric shape, 512 x 4096 -> 11008 with 41 outlier
columns.  Prints one JSON line: per dtype the us per forward of every round, their median and spread.

    python3 tools/bench_bf16.py [--bit 8|4] [--rounds 5] [--steps 20] [--once bf16]

--once DTYPE: build that layer, replay its graph for a profiler (rocprofv3 --kernel-trace --stats -- python3 tools/bench_bf16.py --once bf16)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bit", type=int, choices=[8, 4], default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=31)
    ap.add_argument("--batch", type=int, default=bench.M)
    ap.add_argument("--once", choices=["fp16", "bf16"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_bf16.py needs an MI355X")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    side = torch.cuda.Stream()
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
