"""bench.py's plain run (what every benchmark of the project runs): the headline calls only, one JSON line, and --dump-outputs
writing what the last timed call returned -- the same bits from two processes with the same arguments, so that two builds can be
compared output for output.  What a plain run leaves out (inference-only calls, roofline, self_check, cpu_baseline) is checked
with --full by tests/test_gpu_dist.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, K, W = 300, 2, 1


def _plain_run(dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--T", str(T),
           "--dump-outputs", str(dump_dir)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, run.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_headline_calls_and_dumps_reproducible_outputs(tmp_path):
    out = _plain_run(tmp_path / "a")
    assert out["unit"] == "steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == K and out["warmup"] == W and out["value_mode"] == "learning_call" and out["config"]["T"] == T
    assert out["value"] == pytest.approx(K * T / (out["ms_per_step"] * 1e-3 * K), rel=1e-6)
    assert out["config"]["finite"] and out["build_info"]["built_from_this_tree"]
    assert out["roofline"] is None and out["config"]["inference_only"] is None
    assert "self_check" not in out and "cpu_baseline" not in out

    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(["energies.npy", "param_grads.npy"] + ["%s_layer%d.npy" % (k, l) for k in ("state", "records") for l in range(3)])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 1000 * 1000
    a = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert a["energies.npy"].shape[0] == T and a["param_grads.npy"].shape == (276146,) and float(np.abs(a["param_grads.npy"]).max()) > 0
    assert [a["state_layer%d.npy" % l].shape for l in range(3)] == [(6000, 30), (6000, 256), (6000, 256)]
    assert a["records_layer1.npy"].shape[0] == (T + 99) // 100 and a["records_layer1.npy"].shape[2] == 256

    _plain_run(tmp_path / "b")
    for f in files:
        assert np.array_equal(a[f], np.load(tmp_path / "b" / f)), f
