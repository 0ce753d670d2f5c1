#!/usr/bin/env python3
"""Time the weight-only W8A16 GEMM per config and shape: one hipGraph of `--launches` launches per configuration, replayed
round-robin for `--rounds` rounds (interleaved A/B), median / min per configuration.  Development tool.
`--dtype bf16` times the bfloat16 kernels (mixq_gemm_w8a16_bf16), `--dtype both` puts the fp16 and the bf16 form of every configuration
into the SAME alternating rounds - one box, one clock history - and prints bf16 / fp16 beside the fp16 rounds' own spread; the shader clock
is sampled through the timed rounds (tools/yardstick.py's sampler)."""
import argparse
import os
import sys

import numpy as np
import torch
os.environ.setdefault("MIXQ_TUNING_LIB", "1")      # ablation kernels / trace stamps / probe knobs live in the tools build (make tuning)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mixq_amd import _capi, mixlib  # noqa: E402
from yardstick import Sampler  # noqa: E402

PEAK_F16 = 2516.0   # dense fp16 MFMA TFLOP/s: 256 CU x 4096 flop/clk x 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x11008x4096,512x4096x4096,512x4096x11008,16x11008x4096")
    ap.add_argument("--cfgs", default="auto", help="comma list of config names, 'auto', or 'all'")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--dtype", default="f16", choices=("f16", "bf16", "both"), help="activation container; 'both': fp16 and bf16 arms in the same rounds")
    args = ap.parse_args()
    dts = {"f16": [torch.float16], "bf16": [torch.bfloat16], "both": [torch.float16, torch.bfloat16]}[args.dtype]
    tag = {torch.float16: "f16", torch.bfloat16: "bf16"}
    smp = Sampler()
    print(f"sampler: {smp.source()}", flush=True)
    lib = _capi.load()
    names = _capi.w8a16_config_names()
    side = torch.cuda.Stream()
    for shp in args.shapes.split(","):
        M, N, K = (int(v) for v in shp.split("x"))
        g = torch.Generator().manual_seed(0)
        q = torch.randint(-128, 128, (K, N), generator=g, dtype=torch.int8).cuda()
        s = (torch.rand(N, generator=g) * 0.01 + 0.001).half().cuda()
        x32 = torch.randn(M, K, generator=g)
        xs = {dt: x32.to(dt).cuda() for dt in dts}
        wps = {dt: mixlib.PackW8A16(q) if dt == torch.float16 else mixlib.PackW8A16(q, dt) for dt in dts}
        outs = {dt: torch.empty(M, N, dtype=dt, device="cuda") for dt in dts}
        refs = {dt: xs[dt].float() @ (q.float() * s.float()) for dt in dts}
        if args.cfgs == "all":
            todo = ["auto"] + [nm for nm in names if (M <= 32) == nm.endswith("decode32") or "abl" not in nm and M <= 32]
        else:
            todo = args.cfgs.split(",")
        graphs, errs = [], {}
        with torch.cuda.stream(side):
            for nm in todo:
                c = -1 if nm == "auto" else names.index(nm)
                if nm.endswith("decode32") and M > 32:
                    continue
                for dt in dts:
                    if nm.endswith("decode32") and dt == torch.bfloat16:
                        continue                             # (the K-split kernel has no bf16 form)
                    assert lib.mixq_gemm_w8a16_set_config(c) == 0
                    run = lambda dt=dt: mixlib.W8A16Linear(xs[dt], wps[dt], s, None, N, K, out=outs[dt])
                    for _ in range(3):
                        y = run()
                    torch.cuda.synchronize()
                    arm = nm if len(dts) == 1 else f"{nm} {tag[dt]}"
                    errs[arm] = (y.float() - refs[dt]).abs().max().item() / refs[dt].abs().max().item()
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=side):
                        for _ in range(args.launches):
                            run()
                    torch.cuda.synchronize()
                    graphs.append((arm, gr))
            lib.mixq_gemm_w8a16_set_config(-1)
            times = {nm: [] for nm, _ in graphs}
            smp.start()
            for r in range(args.rounds + 2):
                for nm, gr in graphs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    gr.replay()
                    e1.record()
                    e1.synchronize()
                    if r >= 2:
                        times[nm].append(e0.elapsed_time(e1) * 1e3 / args.launches)
        clk = smp.stop(skip=0.0)
        print(f"{shp}: {args.rounds} interleaved rounds x {args.launches} launches; us per launch median / min / max; {clk}", flush=True)
        for nm, _ in graphs:
            t = np.array(times[nm])
            med = float(np.median(t))
            tf = 2.0 * M * N * K / med / 1e6
            print(f"  {nm:36s} {med:8.2f} {t.min():8.2f} {t.max():8.2f}   {tf:7.1f} TFLOP/s ({100 * tf / PEAK_F16:4.1f} % of fp16 peak)  rel_err {errs[nm]:.1e}", flush=True)
        if len(dts) == 2:                                    # bf16 against its fp16 twin, the fp16 rounds' own spread beside it
            for nm, _ in graphs:
                if nm.endswith(" bf16") and nm[:-5] + " f16" in times:
                    a, b = np.array(times[nm[:-5] + " f16"]), np.array(times[nm])
                    print(f"  {nm[:-5]:31s} bf16 / f16 median {np.median(b) / np.median(a):6.3f}  (per round: median {np.median(b / a):6.3f}, "
                          f"min {np.min(b / a):6.3f}, max {np.max(b / a):6.3f});  f16 rounds' spread (max - min) / median {(a.max() - a.min()) / np.median(a) * 100:5.1f} %, "
                          f"(p90 - p10) / median {(np.percentile(a, 90) - np.percentile(a, 10)) / np.median(a) * 100:5.1f} %", flush=True)


if __name__ == "__main__":
    main()
