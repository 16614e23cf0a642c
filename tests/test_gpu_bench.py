"""bench.py at N = 1 as the project runs it: a plain run makes the headline only (W warm-up + exactly K timed steps on a fresh
operator, --dump-outputs, one JSON line); --full adds everything that takes runs of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("processes", "cpu_baseline", "bare_spmv", "locate_E0", "fast_path", "matrix_free_hubbard")


def _bench(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "hubbard_4x3_half"] + args,
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_makes_the_headline_and_its_outputs_only(tmp_path):
    got = _bench(["--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    assert got["metric"] == "lanczos_iters_per_sec" and got["unit"] == "lanczos_iters/s" and got["higher_is_better"] is True
    assert got["dtype"] == "complex128" and got["steps"] == 3 and got["value"] > 0 and got["ms_per_step"] > 0
    assert not set(FULL_ONLY) & set(got) and got["e0"] is None, sorted(got)
    assert np.load(tmp_path / "lanczos_m.npy").tolist() == [5.0]                  # 2 warm-up + 3 timed steps
    assert np.load(tmp_path / "v.npy").shape == (2, 853776, 2)


def test_full_run_adds_the_measurements_of_their_own():
    got = _bench(["--full", "--steps", "3", "--warmup", "2", "--no-cpu-baseline"])
    assert got["steps"] == 3 and got["processes"]["n"] == 3 and not got["processes"]["incomplete"]
    assert abs(got["e0"] + 16.879382788684) < 1e-9
    for k in ("bare_spmv", "locate_E0", "fast_path", "matrix_free_hubbard"):
        assert k in got and not {"error", "failed"} & set(got[k]), (k, got.get(k))
    assert "cpu_baseline" not in got
