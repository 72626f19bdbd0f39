"""GPU tier: bench.py's plain run and --dump-outputs.  Without --full the run prints the headline line only - the contract fields and
the configuration, no roofline, legs, parity or CPU baseline, no bench_full.json - and DIR/slogl.npy holds the slogl of the last timed
step (the same sum as the first: same tables, same model)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    dump = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "KDE slogl M-samples/s" and out["unit"] == "M-samples/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f64" and out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1
    # value and ms_per_step describe the same timed steps: 1e5 test rows per step
    assert out["ms_per_step"] > 0 and abs(out["value"] - 100_000 / out["ms_per_step"] / 1e3) <= 1e-4 * out["value"]
    assert not set(out) & {"roofline", "cpu_baseline", "parity", "legs", "full"}
    assert not (tmp_path / "bench_full.json").exists()
    got = np.load(dump / "slogl.npy")
    assert got.dtype == np.float64 and got.shape == (1,)
    step0 = out["config"]["slogl_step0_rank_sum"]
    assert np.isfinite(got[0]) and abs(got[0] - step0) <= 1e-9 * abs(step0)
