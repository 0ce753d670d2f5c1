#!/usr/bin/env python3
"""Record which kernel the fused GEMM entry points choose, per problem, as tests/golden/routes.json.

    python tools/record_routes.py [path/to/libmixq_hip.so] [-o tests/golden/routes.json]

Loads the library by path with ctypes (no torch, no GPU: only the queries of the C ABI are called, never a launch; without a device
mixq_num_cus() answers 256, the MI355X's own count) and asks, for every problem of GRID x both bit widths x the four weight formats:

    mixq_gemm_pick_config_fmt                      the config id (names in "config_names")
    mixq_gemm_pick_split, mixq_gemm_pick_split_bf16  1 / 0, and n1 / cfg2 where the launch is an N split (else 0 / -1)
    mixq_gemm_amax_supported, _bf16                with the layout flags a launch of that format passes

tests/test_routes_host.py compares the in-tree library with the recorded table row for row, so a change to the dispatcher that moves a
route fails there.  A change that MEANS to move routes - a retuned cost model, a new tiling - regenerates the fixture with this tool from
the new library and commits it with the change.
"""
import argparse
import ctypes as C
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = {"M": [1, 16, 32, 33, 64, 128, 512, 2048, 4096, 8192],
        "N": [64, 4096, 6144, 8192, 11008, 14336, 28672],
        "K": [128, 4096, 8192, 14336],
        "bit": [8, 4],
        "fmt": [0, 1, 2, 3]}                       # MIXQ_FMT_PLAIN, P16X64, F16X64, F6X128 (include/mixq_hip.h)
LAYOUT_OF_FMT = {0: 0, 1: 1 | 2, 2: 1 | 8, 3: 16}   # MIXQ_X_PACKED = 1, MIXQ_W_PACKED = 2, MIXQ_W_F16X64 = 8, MIXQ_XW_F6X128 = 16
COLUMNS = ["M", "N", "K", "bit", "fmt", "cfg", "split", "n1", "cfg2", "split_bf16", "n1_bf16", "cfg2_bf16", "amax", "amax_bf16"]


def record(lib_path):
    lib = C.CDLL(lib_path)
    names = []
    buf = C.create_string_buffer(128)
    for c in range(lib.mixq_gemm_num_configs()):
        assert lib.mixq_gemm_config_name(c, buf, 128) == 0
        names.append(buf.value.decode())

    def split(fn, M, N, K, bit, fmt):
        n1, c2 = C.c_int(0), C.c_int(-1)
        r = fn(M, N, K, bit, fmt, C.byref(n1), C.byref(c2))
        return [r, n1.value, c2.value] if r == 1 else [r, 0, -1]

    rows = []
    for M in GRID["M"]:
        for N in GRID["N"]:
            for K in GRID["K"]:
                for bit in GRID["bit"]:
                    for fmt in GRID["fmt"]:
                        lay = LAYOUT_OF_FMT[fmt]
                        rows.append([M, N, K, bit, fmt, lib.mixq_gemm_pick_config_fmt(M, N, K, bit, fmt)]
                                    + split(lib.mixq_gemm_pick_split, M, N, K, bit, fmt)
                                    + split(lib.mixq_gemm_pick_split_bf16, M, N, K, bit, fmt)
                                    + [lib.mixq_gemm_amax_supported(M, N, K, lay), lib.mixq_gemm_amax_supported_bf16(M, N, K, lay)])
    return {"columns": COLUMNS, "config_names": names, "rows": rows}


def dumps(table):
    head = json.dumps({k: v for k, v in table.items() if k != "rows"}, separators=(",", ":"))
    body = ",\n".join(json.dumps(r, separators=(",", ":")) for r in table["rows"])
    return head[:-1] + ',"rows":[\n' + body + "\n]}\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("lib", nargs="?", default=os.path.join(ROOT, "mixq_amd", "libmixq_hip.so"))
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "routes.json"))
    args = ap.parse_args()
    table = record(os.path.abspath(args.lib))
    with open(args.out, "w") as f:
        f.write(dumps(table))
    print(f"{len(table['rows'])} problems, {len(set(r[5] for r in table['rows']))} distinct configs, "
          f"{sum(r[6] == 1 for r in table['rows'])} fp16 / {sum(r[9] == 1 for r in table['rows'])} bf16 N splits -> {args.out}")
