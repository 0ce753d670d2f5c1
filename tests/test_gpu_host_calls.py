"""The layer and module scenarios of tests/call_trace.py run for real, at the recorded shapes (16 and 48 x 256 -> 128) with random inputs:
the recorder behind tests/golden/host_calls.json answers 0 to everything, so this is where the library itself accepts those calls.  No call
is refused, every returned tensor has the shape, dtype, strides and format tag of the CPU recording, and the outputs are finite."""
import json
import os

import pytest
import torch

import call_trace

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_calls.json")) as f:
    RECORDED = json.load(f)
FAMILIES = ("layer/W8", "layer/W4", "weight_only", "mlp/W8", "mlp/W4", "norm")


def test_families_cover_the_layer_scenarios():
    assert all(name.startswith(FAMILIES) for name, _ in call_trace.LAYER_SCENARIOS) and len(call_trace.LAYER_SCENARIOS) > 100


@pytest.mark.parametrize("family", FAMILIES)
def test_recorded_layer_scenarios_run_on_the_library(family):
    bad = []
    for name, fn in call_trace.LAYER_SCENARIOS:
        if not name.startswith(family):
            continue
        assert "error" not in RECORDED[name], name               # (the recording itself holds no refusal for a layer scenario)
        try:
            outs = fn(device="cuda")
        except Exception as e:                                   # a refused call: the library's status, or a Python-side check
            bad.append(f"{name}: {type(e).__name__}: {e}")
            continue
        got = json.loads(json.dumps(call_trace.describe(outs)))
        if got != RECORDED[name]["out"]:
            bad.append(f"{name}: returned {got}, recorded {RECORDED[name]['out']}")
        elif not all(bool(torch.isfinite(t.float()).all()) for t in outs):
            bad.append(f"{name}: an output is not finite")
    torch.cuda.synchronize()
    assert not bad, f"{len(bad)} scenarios:\n" + "\n".join(bad[:8])
