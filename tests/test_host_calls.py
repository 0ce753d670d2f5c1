"""The Python layer's calls into the C ABI against the recording of tests/golden/host_calls.json (tests/call_trace.py; regenerate with
tools/record_calls.py when a change means to move one).  No GPU: the C ABI is a recorder, the tensors live in host memory."""
import json
import os

import pytest

import call_trace
from mixq_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_calls.json")
MIXLIB = os.path.join(os.path.dirname(_capi.__file__), "mixlib.py")

with open(GOLDEN) as f:
    RECORDED = json.load(f)


def test_scenario_list_is_the_recorded_one():
    assert [s[0] for s in call_trace.SCENARIOS] == list(RECORDED)


@pytest.mark.parametrize("chunk", range(8))
def test_host_calls_match_the_recording(chunk):
    """Scenario for scenario: the records in order, every returned tensor's shape / dtype / strides / tags, a refusal's type and words."""
    bad = []
    for s in call_trace.SCENARIOS[chunk::8]:
        got, want = call_trace.run(s), RECORDED[s[0]]
        if got != want:
            first = next((i for i, (a, b) in enumerate(zip(got["calls"], want["calls"])) if a != b), min(len(got["calls"]), len(want["calls"])))
            bad.append(f"{s[0]}: record {first}: got {got['calls'][first:first + 1]} want {want['calls'][first:first + 1]}; "
                       f"result got {got.get('out', got.get('error'))} want {want.get('out', want.get('error'))}")
    assert not bad, f"{len(bad)} scenarios differ from the recording:\n" + "\n".join(bad[:5])


# The trace's reach: every entry point of the C ABI is recorded at least once, except the ones mixlib.py never calls -
NOT_TRACED = set(_capi.TUNING_ONLY) | {
    "mixq_selftest_quant_exact", "mixq_selftest_quant_exact_bf16",                          # the library's self-test, driven by the GPU suite
    # tuning knobs and name / plan queries, called by tools/ and the helpers of _capi.py only
    "mixq_gemm_set_config", "mixq_quant_set_config", "mixq_gemm_w8a16_set_config", "mixq_gemm_num_configs", "mixq_gemm_config_name",
    "mixq_gemm_w8a16_num_configs", "mixq_gemm_w8a16_config_name", "mixq_gemm_pick_config", "mixq_gemm_pick_config_fmt", "mixq_gemm_pick_split",
    "mixq_gemm_pick_split_bf16", "mixq_gemm_pair_supported_bf16", "mixq_kept_map_words", "mixq_version", "mixq_device_info",
    "mixq_gemm_workspace_bytes", "mixq_gemm_set_workspace",                                 # _capi.ensure_workspace: needs a device
    "mixq_quant_known_amax", "mixq_quant_known_amax_bf16",                                  # launched inside mixq_linear_forward*, never from Python
    "mixq_pack_p16x64",                                                                     # superseded by mixq_pack_operand
}


def test_every_entry_point_mixlib_can_call_is_recorded():
    seen = {c.split("(")[0] for v in RECORDED.values() for c in v["calls"]}
    assert not (set(_capi.SIGNATURES) - seen - NOT_TRACED), sorted(set(_capi.SIGNATURES) - seen - NOT_TRACED)
    src = open(MIXLIB).read()
    assert not [n for n in NOT_TRACED - set(_capi.TUNING_ONLY) if f'"{n}"' in src]           # (an exception mixlib.py spells is no exception)
