"""bench.py's command line: --dump-outputs writes what the last timed step
returned, a plain run prints the result line without the figures that take
runs of their own, and --full brings those back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_is_float64_seeded_and_capped(tmp_path):
    import bench
    n = 3_000_000  # three columns of 24 MB each: over the cap together
    cols = {"a": np.arange(n, dtype=np.int64), "b:V": np.arange(n, dtype=np.int64) * 3, "count": [n]}
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), cols)
    files = sorted(os.listdir(tmp_path / "x"))
    assert files == ["a.npy", "b_V.npy", "count.npy"]
    got = {f: np.load(tmp_path / "x" / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in files) <= 64_000_000
    assert got["count.npy"].tolist() == [float(n)]
    # a sample, the same rows of every column, and the same from run to run
    assert 0 < got["a.npy"].size < n and np.array_equal(got["a.npy"] * 3, got["b_V.npy"])
    for f in files:
        assert np.array_equal(got[f], np.load(tmp_path / "y" / f))


def _bench(*argv):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--scale", "12", "--steps", "3", "--warmup", "1", *argv],
                       cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_count(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path / "out"))
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "joined rows/s"
    assert line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["value"] == pytest.approx(line["config"]["count"] / (line["ms_per_step"] * 1e-3))
    assert "cpu_baseline" not in line and "ms_per_step_pipelined" not in line["config"]
    assert "kernel_ms_per_query" not in line["roofline"]
    assert os.listdir(tmp_path / "out") == ["count.npy"]
    count = np.load(tmp_path / "out" / "count.npy")
    assert count.dtype == np.float64 and count.tolist() == [float(line["config"]["count"])]


@pytest.mark.gpu
def test_full_run_keeps_the_side_figures():
    line = _bench("--full", "--cpu-seconds", "0.2")
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["config"]["ms_per_step_pipelined"] > 0
    assert line["roofline"]["kernel_ms_per_query"] and line["roofline"]["kernel_event_frac"] > 0
    assert line["cpu_baseline"]["value"] > 0
