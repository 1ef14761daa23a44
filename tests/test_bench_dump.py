"""``bench.py --dump-outputs DIR`` / ``--full``: the benchmark writes what its last
timed tick returned, the same arrays from the same arguments in every run, and a
plain run still prints the one result line."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--series", "200", "--ring", "480", "--season", "48", "--anomaly-frac", "0.05"]


def _bench(args, timeout=300):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args,
                         capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _check_dump(a, b, n_series, n_apps):
    assert set(a) == set(b) and {"health.npy", "verdict.npy", "sigma.npy"} <= set(a)
    assert all(f.endswith(".npy") for f in a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert a[f].shape == b[f].shape and np.array_equal(a[f], b[f], equal_nan=True), f
    assert a["health.npy"].shape == (n_apps, 2) and a["verdict.npy"].shape == (n_series,)
    assert int(a["health.npy"][:, 1].sum()) == n_series       # every series scored in the last tick
    assert set(np.unique(a["verdict.npy"]).tolist()) <= {0.0, 1.0}
    # the table the result line summarises is the one on disk
    return int((a["health.npy"][:, 0] > 0).sum())


def test_dump_outputs_cpu_repeatable(tmp_path):
    recs = [_bench(["--cpu", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / n)] + SMALL + extra)
            for n, extra in (("a", []), ("b", ["--full"]))]
    for r in recs:
        assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
        for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert k in r
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert _check_dump(a, b, 200, 40) == recs[0]["health"]["anomalous_apps"]
    assert recs[0]["health"] == recs[1]["health"] and recs[0]["detection"] == recs[1]["detection"]


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * 4096)
    out = {"verdict": torch.zeros(100, dtype=torch.int8), "forecast": torch.arange(4000.0).view(1000, 4),
           "count": torch.arange(5000, dtype=torch.int64), "_workspace": torch.zeros(3), "post_in_graph": True}
    health = torch.ones((10, 2), dtype=torch.int32)
    for d in ("x", "y"):
        names = bench.dump_outputs(str(tmp_path / d), out, health, 1, 0)
        assert sorted(names) == ["count.npy", "forecast.npy", "health.npy", "verdict.npy"]
    x, y = _load(tmp_path / "x"), _load(tmp_path / "y")
    assert x["verdict.npy"].shape == (100,) and x["verdict.npy"].dtype == np.float32
    assert x["health.npy"].shape == (10, 2)
    # each array's share is 3 KiB: 192 rows of 16 bytes, 384 8-byte values
    assert x["forecast.npy"].shape == (192, 4) and x["count.npy"].shape == (384,)
    assert x["count.npy"].dtype == np.float64
    rows = x["forecast.npy"][:, 0] / 4
    assert np.all(np.diff(rows) > 0) and np.array_equal(x["forecast.npy"][:, 1], x["forecast.npy"][:, 0] + 1)
    for f in x:
        assert np.array_equal(x[f], y[f])
    assert sum(v.nbytes for v in x.values()) <= 3 * 4096


@pytest.mark.gpu
def test_dump_outputs_gpu_repeatable(tmp_path):
    """The headline path (bf16 ring, HIP-graph ticks) at 5000 series: two runs write
    identical arrays, every series is scored, the injected regressions are on disk."""
    args = ["--steps", "3", "--warmup", "2", "--series", "5000", "--ring", "2880", "--anomaly-frac", "0.02"]
    recs = [_bench(args + ["--dump-outputs", str(tmp_path / n)]) for n in ("a", "b")]
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert _check_dump(a, b, 5000, 1000) == recs[0]["health"]["anomalous_apps"]
    assert recs[0]["config"]["hip_graph"] is True and recs[0]["dtype"] == "bf16"
    assert np.isfinite(a["sigma.npy"]).all()
    assert int(a["verdict.npy"].sum()) >= recs[0]["detection"]["tp"] > 0
