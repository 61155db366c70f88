"""CPU: bench.py's --dump-outputs writer (float32 / float64 files, a fixed sample above the size limit) and its argument checks."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_records(dm, n, seed):
    rng = np.random.default_rng(seed)
    return {k: np.frombuffer(rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).tobytes(), dt).copy()
            for k, dt in (("plan", dm.PlanOut), ("state", dm.SceneState), ("grid_out", dm.GridOut))}


def _read(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_fixed_sample_under_the_limit(tmp_path, monkeypatch):
    import bench
    import dmpp_amd as dm
    n = 300
    recs = _random_records(dm, n, 5)
    limit = 2 << 20
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    bench.dump_outputs(str(tmp_path / "a"), np, recs)
    bench.dump_outputs(str(tmp_path / "b"), np, recs)
    a, b = _read(tmp_path / "a"), _read(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= limit
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    idx = a["scene_index.npy"].astype(np.int64)
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0)
    digest = (a["grid_out.order_digest.hi32.npy"].astype(np.uint64) << np.uint64(32)) | a["grid_out.order_digest.lo32.npy"].astype(np.uint64)
    assert np.array_equal(digest, recs["grid_out"]["order_digest"][idx])
    assert np.array_equal(a["grid_out.status.npy"], recs["grid_out"]["status"][idx].astype(np.float64))
    assert np.array_equal(a["state.faraim_dis.npy"], recs["state"]["faraim_dis"][idx], equal_nan=True)
    assert not [f for f in a if "_pad" in f]


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
