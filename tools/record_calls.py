#!/usr/bin/env python3
"""Record what the Python layer hands to the C ABI, per scenario, as tests/golden/host_calls.json.

    python tools/record_calls.py [-o tests/golden/host_calls.json]

Runs every scenario of tests/call_trace.py on CPU tensors with the C ABI replaced by a recorder (no GPU, no launch; the pure host queries
go to the built library) and writes one line per scenario.  tests/test_host_calls.py replays the scenarios on the in-tree code and compares
them with the file, so a change to mixlib.py / linear.py / fused.py that moves an argument, an entry point, a returned tensor's layout or
a refusal's words fails there.  A change that MEANS to move one regenerates the file with this tool and commits it with the change.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "host_calls.json"))
    args = ap.parse_args()
    import call_trace
    table = call_trace.record_all()
    with open(args.out, "w") as f:
        f.write(call_trace.dumps(table))
    errors = sum("error" in v for v in table.values())
    print(f"{len(table)} scenarios ({errors} end in an exception), {sum(len(v['calls']) for v in table.values())} records -> {args.out}")
