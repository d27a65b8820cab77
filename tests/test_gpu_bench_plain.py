"""The plain bench command (`python bench.py --gpus 1 --steps K --warmup W`, no --full) on the GPU
box: it times the K steps and prints the headline fields only, `--dump-outputs` writes what the
last timed step left, two runs with the same arguments write the same bytes, and a --full run
writes them too (the read-out comes before anything --full adds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = (1 << 18) + 3  # above bench.DUMP_SAMPLE: the sampled read-out; odd: a partial last block
ARGS = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--n-per-gpu", str(N)]
FULL_ONLY = ("roofline", "cpu_baseline", "fused_replay", "ensemble_every_1", "parity_sampled", "secondary",
             "path_rows", "cfg4_16M", "ensemble_check", "scaling_diag")


def run_bench(extra, out_dir):
    r = subprocess.run([sys.executable, "bench.py", *ARGS, "--dump-outputs", str(out_dir), *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return run_bench([], tmp_path_factory.mktemp("plain"))


def test_plain_line_is_the_headline_only(plain):
    out, _ = plain
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert out["metric"] == base["metric"] and out["unit"] == "steps/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["full"] is False
    assert (out["n_gpus"], out["steps"], out["warmup"]) == (1, 20, 5)
    assert out["config"]["instances_per_gpu"] == N
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(N / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert out["nonfinite_instances"] == 0 and out["ensemble"]["count"] == N
    for key in FULL_ONLY:
        assert key not in out, key


def test_dump_outputs_arrays(plain):
    out, arr = plain
    assert set(arr) == {"robot_index", "x", "P", "ensemble_mean", "ensemble_cov", "ensemble_count"}
    assert out["outputs_dumped"] == {k: list(a.shape) for k, a in arr.items()}
    k = arr["robot_index"].size
    assert arr["robot_index"][0] == 0 and arr["robot_index"][-1] == N - 1 and k <= 1 << 18
    assert arr["x"].shape == (6, k) and arr["P"].shape == (21, k)
    assert arr["x"].dtype == arr["P"].dtype == np.float32
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64e6
    assert np.isfinite(arr["x"]).all() and np.isfinite(arr["P"]).all()
    # the filter ran: the variances (packed lower triangle, k = i (i + 1) / 2 + i) stayed
    # positive and the states differ from robot to robot
    diag = arr["P"][[0, 2, 5, 9, 14, 20]]
    assert (diag > 0).all() and np.ptp(arr["x"], axis=1).min() > 0
    assert arr["ensemble_count"].tolist() == [N]


@pytest.mark.parametrize("extra", [[], ["--full", "--no-cpu-baseline", "--no-secondary"]], ids=["plain", "full"])
def test_same_arguments_same_outputs(plain, extra, tmp_path):
    """seeded inputs, no atomics in the tick or the record: a second run, plain or --full, writes
    the same bytes"""
    out, arr = run_bench(extra, tmp_path)
    assert out["full"] is bool(extra)
    assert set(arr) == set(plain[1])
    for name, a in arr.items():
        assert a.dtype == plain[1][name].dtype and np.array_equal(a.view(np.uint8), plain[1][name].view(np.uint8)), name
