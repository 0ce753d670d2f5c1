"""bench.py's plain run and its options: the timed region is exactly --steps steps (split_steps), --dump-outputs writes y of the last
timed step within 64 MB (output_sample), --full carries everything beyond the headline.  The CPU tests check the arithmetic; the GPU test
runs the plain line twice and holds the dumped outputs to each other and to the operator called directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


@pytest.mark.parametrize("replays", [1, 7, 31])
def test_split_steps_covers_exactly_the_timed_steps(replays):
    for steps in range(1, 3000):
        g, r, tail = bench.split_steps(steps, replays)
        assert g * r + tail == steps and 0 <= tail < g and r >= 1
        assert g >= min(steps, bench.GRAPH_STEPS)
        if steps >= bench.GRAPH_STEPS * replays:                  # long runs: about `replays` samples, never more and shorter ones
            assert replays <= r < 2 * replays + 1
    assert bench.split_steps(20, 31) == (20, 1, 0)                # the driver's --steps 20: one 20-step replay, as rounds 1-6 timed them
    assert bench.split_steps(23, 31) == (20, 1, 3)
    assert bench.split_steps(5, 31) == (5, 1, 0)


def test_output_sample_whole_and_sampled():
    y = (torch.randn(64, 48, generator=torch.Generator().manual_seed(3)) * 8).half()
    whole = bench.output_sample(y)
    assert list(whole) == ["y"] and whole["y"].dtype == np.float32 and np.array_equal(whole["y"], y.float().numpy())
    budget = 20 * (48 * 4 + 8)                                      # room for 20 of the 64 rows
    a, b = bench.output_sample(y, budget=budget), bench.output_sample(y, budget=budget)
    assert sorted(a) == ["y", "y_rows"] and a["y"].dtype == np.float32 and a["y_rows"].dtype == np.float64
    assert a["y"].nbytes + a["y_rows"].nbytes <= budget and a["y"].shape == (20, 48)
    rows = a["y_rows"].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 64
    assert np.array_equal(a["y"], y.float().numpy()[rows])
    assert np.array_equal(a["y"], b["y"]) and np.array_equal(a["y_rows"], b["y_rows"])      # fixed, seeded sample


def test_full_is_off_by_default():
    args = bench.parse(["--steps", "7"])
    assert args.full is False and args.dump_outputs is None and args.steps == 7
    args = bench.parse(["--full", "--dump-outputs", "out", "--no-secondary"])
    assert args.full is True and args.dump_outputs == "out" and args.no_secondary is True


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    """The plain run (no --full): the headline fields and nothing that needs runs of its own; 23 steps = one 20-step replay + a 3-step
    graph; two runs with the same arguments dump the same y, and that y is what the operator returns for the same seeded batch."""
    flops = 2.0 * 512 * 4096 * 11008
    ys = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "23", "--warmup", "2", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        out = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config", "timing"):
            assert key in out, key
        for key in ("roofline", "cpu_baseline", "secondary_configs", "max_abs_err_vs_dequant_linear", "ms_per_step_single_replay"):
            assert key not in out, key
        assert out["steps"] == 23 and out["warmup"] == 2 and out["unit"] == "TFLOPS" and out["dtype"] == "int8" and out["full"] is False
        tm = out["timing"]
        assert tm["steps_per_graph"] == 20 and tm["replays"] == 1 and tm["tail_replay_ms"] > 0
        assert tm["timed_region_ms"] >= tm["replay_ms_median"] + tm["tail_replay_ms"]
        assert out["ms_per_step"] == pytest.approx(tm["replay_ms_median"] / 20, rel=1e-3)
        assert out["value"] == pytest.approx(flops / (out["ms_per_step"] * 1e-3) / 1e12, rel=1e-3)
        assert sorted(os.listdir(d)) == ["y.npy"]
        y = np.load(d / "y.npy")
        assert y.dtype == np.float32 and y.shape == (512, 11008) and np.isfinite(y).all() and np.abs(y).max() > 0
        ys.append(y)
    assert np.array_equal(ys[0], ys[1])
    dev = torch.device("cuda", 0)
    _, _, layer = bench.build_layer(dev, 512)
    _, base, _ = bench.make_batches(1, 512, dev, 0)
    for _ in range(3):
        y_op = layer(base.clone(), None, True)
    torch.cuda.synchronize()
    assert float(np.abs(y_op.float().cpu().numpy() - ys[0]).max()) <= 1e-2
