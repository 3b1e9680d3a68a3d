"""bench.py command line: --steps, ms_per_step, --full, --dump-outputs."""

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLAIMS = 500


def _run_bench(*extra):
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1",
         "--claims-per-step", str(CLAIMS)] + list(extra),
        capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load_dir(d):
    return {name: np.load(os.path.join(d, name)) for name in os.listdir(d)}


def test_dump_outputs_same_from_run_to_run_and_under_full(tmp_path):
    plain_dir = str(tmp_path / "plain")
    full_dir = str(tmp_path / "full")
    plain = _run_bench("--dump-outputs", plain_dir)
    full = _run_bench("--full", "--dump-outputs", full_dir)

    for data in (plain, full):
        assert data["metric"].startswith("pool claims/sec")
        assert data["unit"] == "claims/s"
        assert data["higher_is_better"] is True
        assert data["dtype"] == "n/a"
        assert data["steps"] == 2
        # ms_per_step is the time of one timed step: value claims/s
        # over CLAIMS claims (both rounded in the result line)
        assert data["ms_per_step"] > 0
        expect_ms = CLAIMS / data["value"] * 1000.0
        assert abs(data["ms_per_step"] - expect_ms) <= \
            0.01 * expect_ms + 0.001

    a, b = _load_dir(plain_dir), _load_dir(full_dir)
    assert sorted(a) == sorted(b) == ["claim_ok.npy", "ops_completed.npy"]
    for name in a:
        assert a[name].dtype == np.float32
        assert np.array_equal(a[name], b[name]), name
    # every claimer of the last step got a connection
    assert a["claim_ok.npy"].shape == (CLAIMS,)
    assert (a["claim_ok.npy"] == 1.0).all()
    assert a["ops_completed.npy"].tolist() == [float(CLAIMS)]


def test_dump_outputs_caps_size_with_fixed_sample(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "_DUMP_LIMIT_BYTES", 2 * 4 * 100)
    outputs = {"big": [float(i) for i in range(1000)], "small": [7.0]}
    bench.dump_outputs(outputs, str(tmp_path / "a"))
    bench.dump_outputs(outputs, str(tmp_path / "b"))
    a, b = _load_dir(str(tmp_path / "a")), _load_dir(str(tmp_path / "b"))
    assert a["big.npy"].shape == (100,)
    assert np.array_equal(a["big.npy"], b["big.npy"])
    # a sample of the original, in the original order
    assert (np.diff(a["big.npy"]) > 0).all()
    assert a["small.npy"].tolist() == [7.0]
