#!/usr/bin/env python3
"""Host cost of a frozen layer's forward - the Python between `layer(x)` and the C ABI - without a GPU.

    python tools/host_cost.py [--root OTHER_CHECKOUT] [--calls 20000]

Runs a frozen W8A8 MixLinear_GEMM (16 x 256 -> 128, 3 outlier columns) on CPU tensors with the C ABI answering 0 (tests/call_trace.py:
recording(record=False)) and prints microseconds per `layer(x, None, True)` for the float16 and the bfloat16 layer (`--calls` forwards in ten blocks).  `--root` times the
mixq_amd package of another checkout (one that has its library built) with this checkout's harness: alternate the two for a comparison.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--calls", type=int, default=20000)
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.root), os.path.join(ROOT, "tests")]
    import torch
    import call_trace as ct
    torch.set_num_threads(1)
    out = []
    with ct.recording(record=False):
        for name, flags in (("fp16", {}), ("bf16", dict(dt=ct.BF16))):
            cache = ct.cache_of(**flags)
            layer = ct.layer(cache, 8)
            x = ct.rand((16, ct.K), cache.config.act_dtype, "cpu")
            for _ in range(2000):
                layer(x, None, True)
            blocks = []                                      # ten blocks: the median block is the figure, the fastest its floor
            for _ in range(10):
                t0 = time.perf_counter()
                for _ in range(args.calls // 10):
                    layer(x, None, True)
                blocks.append((time.perf_counter() - t0) / (args.calls // 10) * 1e6)
            blocks.sort()
            out.append(f"{name} median {(blocks[4] + blocks[5]) / 2:.2f} min {blocks[0]:.2f} us")
    print(os.path.abspath(args.root), " ".join(out))
