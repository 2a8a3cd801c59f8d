"""bench.py without --full: the headline line alone, and --dump-outputs (what the last timed step computed, float64 .npy files)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, tmp_path):
    env = dict(os.environ, TMPDIR=str(tmp_path))
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    small = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--coarse", "2", "--levels", "3"]
    d = _bench(small + ["--dump-outputs", str(tmp_path / "a")], tmp_path)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - d["config"]["dofs_total"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    # what only --full measures is not in a plain line
    for key in ("roofline", "roofline_assembly", "solve", "known_answer", "cpu_baseline", "assembly_ms"):
        assert key not in d
    n = d["config"]["dofs_total"]
    assert n == 17 ** 3
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert set(got) == {"correction", "residual", "operator_sample_values", "operator_sample_rows", "operator_sample_cols"}
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert got["correction"].shape == (n,) and got["residual"].shape == (n,)
    assert np.linalg.norm(got["correction"]) > 0 and np.linalg.norm(got["residual"]) > 0
    k = got["operator_sample_values"].size
    assert 0 < k <= d["config"]["nnz_fine_this_gpu"] and got["operator_sample_rows"].size == k and got["operator_sample_cols"].size == k
    rows, cols = got["operator_sample_rows"], got["operator_sample_cols"]
    assert rows.min() >= 0 and rows.max() < n and cols.min() >= 0 and cols.max() < n and np.all(np.diff(rows) >= 0)
    # the same arguments give the same inputs: a second run dumps the same operator sample and (up to rounding) the same vectors
    _bench(small + ["--dump-outputs", str(tmp_path / "b")], tmp_path)
    for name, v in got.items():
        w = np.load(tmp_path / "b" / (name + ".npy"))
        assert w.shape == v.shape
        if name.startswith("operator_sample_r") or name.startswith("operator_sample_c"):
            assert np.array_equal(w, v)
        else:
            assert np.linalg.norm(w - v) <= 1e-12 * np.linalg.norm(v)
