"""bench.py as a plain run: the headline alone, with --dump-outputs checked against the oracle.

(The --full run, every leg under torch.distributed.run, is tests/test_gpu_rccl.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_and_dump(gpu, oracle, tmp_path):
    """A plain run times the Z3 encode and nothing else, --steps sets the timed steps, and the dump
    holds the keys of the run's own points (regenerated here from the bench's seed), bit for bit."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = 100_003
    d = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--points", str(n), "--dump-outputs", d]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "points/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64+int64" and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3))
    assert "pip_join" not in line and "cpu_baseline" not in line
    assert line["roofline"].get("box_copy_gbs") is None
    detail = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith("BENCH_DETAIL ")][-1][13:])
    assert "extra" not in detail and "pip_join" not in detail

    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["bin", "z_hi32", "z_lo32"]
    assert got["bin"].dtype == np.float32 and got["z_hi32"].dtype == got["z_lo32"].dtype == np.float64
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    rows = bench.dump_rows(n).numpy()
    assert all(len(v) == len(rows) for v in got.values())
    dev = torch.device("cuda", 0)
    x = torch.empty(n, dtype=torch.float64, device=dev)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    t = torch.empty(n, dtype=torch.int64, device=dev)
    bench.gen_points(gpu, n, 0, (-180.0, -90.0, 180.0, 90.0), x, y, t)
    ob, oz, ost = oracle.z3_index_key_batch(x.cpu().numpy()[rows], y.cpu().numpy()[rows], t.cpu().numpy()[rows])
    assert not ost.any()
    assert np.array_equal(got["bin"].astype(np.int16), ob)
    z = (got["z_hi32"].astype(np.int64) << 32) | got["z_lo32"].astype(np.int64)
    assert np.array_equal(z, oz)


def test_dump_rows_sample_is_fixed():
    """Above DUMP_ROWS the dump is a sorted, seeded sample: the same rows on every call, inside [0, n)."""
    sys.path.insert(0, ROOT)
    import bench
    n = 10 * bench.DUMP_ROWS + 7
    a, b = bench.dump_rows(n).numpy(), bench.dump_rows(n).numpy()
    assert len(a) == bench.DUMP_ROWS and np.array_equal(a, b)
    assert a[0] >= 0 and a[-1] < n and np.all(np.diff(a) >= 0)
    assert 20 * len(a) <= 64 << 20
