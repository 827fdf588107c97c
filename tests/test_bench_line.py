"""bench.py's JSON line on the GPU (a reduced block count): the driver's contract keys, the
dominant kernel's roofline beside both halves, and with --full the self-check of the round
trip; a plain run's lean line and its --dump-outputs arrays."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_is_verified_and_complete():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--blocks", "2048", "--steps", "2",
                        "--warmup", "1", "--no-cpu-baseline", "--host-steps", "0"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["verified"] is True
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["value"] > 0
    rf = line["roofline"]
    assert rf["dominant_of_step"] in ("encode", "decode")
    half = line["roofline_" + rf["dominant_of_step"]]
    assert rf["achieved"] == half["achieved"] and rf["kernel"] == half["kernel"]
    ms = line["kernels_ms"]
    assert rf["dominant_of_step"] == ("decode" if ms["decode"] > ms["encode"] else "encode")
    assert 0 < rf["frac"] < 1.2


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline figure and what the timed steps' own events
    give, none of the legs that take runs of their own; --dump-outputs writes float arrays of
    the batch as the last timed step left it: every block repaired (status = 16 erasures), the
    sampled blocks consistent with the per-block byte sums, at most 64 MB in all."""
    import numpy as np

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--blocks", "2048",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "GiB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8"
    # value and ms_per_step are the same measurement: k * vec * blocks source bytes per step
    # (ms_per_step is rounded to 1e-4 ms, up to 1e-3 of a step of this small batch)
    assert line["value"] == pytest.approx(64 * 1400 * 2048 / (line["ms_per_step"] * 1e-3) / 2**30, rel=1e-2)
    for key in ("verified", "host_resident"):
        assert key not in line, key
    assert line["cpu_baseline"] is None and line["roofline_encode"]["achievable_copy"] is None
    files = sorted(p.name for p in out.iterdir())
    assert files == ["block_sums.npy", "blocks_sample.npy", "blocks_sample_index.npy", "status.npy"]
    arrs = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 * 10**6
    idx = arrs["blocks_sample_index"].astype(np.int64)
    sample = arrs["blocks_sample"]
    assert sample.shape == (len(idx), 96, 1400) and arrs["status"].shape == arrs["block_sums"].shape == (2048,)
    assert (arrs["status"] == 16).all()
    assert np.array_equal(sample.sum(axis=(1, 2), dtype=np.float64), arrs["block_sums"][idx])
    assert sample.min() >= 0 and sample.max() <= 255 and len(np.unique(sample)) == 256


def test_two_ranks_sharing_one_gpu():
    """The N-rank path of bench.py on a one-GPU box (--share-gpu: both ranks on cuda:0, gloo for
    the barrier and the reductions): weak-scaled block ranges, max-over-ranks timing, every
    rank's round trip verified, the CPU baseline on rank 0 only, one line marked as a rehearsal."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--full",
                        "--blocks", "2048", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                        "--host-steps", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["verified"] is True and "rehearsal" in line
    assert line["config"]["blocks_total"] == 4096 and line["config"]["blocks_per_gpu"] == 2048
    assert line["host_resident"]["value"] > 0 and line["value"] > 0
