"""The route of every fused GEMM call - which kernel family and tiling, and whether the launch is an N split - as the queries of the C ABI
report it, against the table recorded in tests/golden/routes.json (tools/record_routes.py; no GPU needed: without a device the library
prices the MI355X's 256 compute units).  The launches follow the same planner the queries read (gemm.hip, plan_route), so a change that
moves a route shows here; one that means to regenerates the table with the tool."""
import json
import os
import sys

from mixq_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_routes  # noqa: E402


def test_every_recorded_route_is_the_route_the_library_takes():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "routes.json")))
    assert _capi.load().mixq_gemm_set_config(-1) == 0
    got = record_routes.record(_capi.LIB_PATH)
    assert got["columns"] == want["columns"] and got["config_names"] == want["config_names"]
    grid = record_routes.GRID
    assert len(want["rows"]) == len(grid["M"]) * len(grid["N"]) * len(grid["K"]) * len(grid["bit"]) * len(grid["fmt"])
    assert len(got["rows"]) == len(want["rows"])
    for g, w in zip(got["rows"], want["rows"]):
        assert g == w, dict(zip(want["columns"], zip(w, g)))
    # the table is worth its bytes: every kernel family, N splits in both containers, and both answers of the side-output question appear
    names = [want["config_names"][r[5]] for r in want["rows"] if r[5] >= 0]
    assert "decode32" in names and any(n.startswith("wr128x256") for n in names) and any(not n.startswith(("wr", "decode")) for n in names)
    assert any(r[6] == 1 for r in want["rows"]) and any(r[9] == 1 for r in want["rows"])
    assert {r[12] for r in want["rows"]} == {0, 1} and {r[13] for r in want["rows"]} == {0, 1}
