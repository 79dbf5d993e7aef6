"""bench.py's host-side helpers (no GPU): what --dump-outputs writes."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_float_arrays(tmp_path):
    bench = _bench()
    scores = np.random.default_rng(1).random((4, 10), dtype=np.float32)
    idx = np.arange(40, dtype=np.int64).reshape(4, 10) * 1_000_003
    bench.dump_outputs(str(tmp_path / "d"), {"scores": scores, "indices": idx})
    assert sorted(os.listdir(tmp_path / "d")) == ["indices.npy", "scores.npy"]
    s, i = np.load(tmp_path / "d" / "scores.npy"), np.load(tmp_path / "d" / "indices.npy")
    assert s.dtype == np.float32 and np.array_equal(s, scores)
    assert i.dtype == np.float64 and np.array_equal(i.astype(np.int64), idx)


def test_dump_outputs_keeps_a_fixed_sample_under_the_limit(tmp_path):
    bench = _bench()
    bench.DUMP_LIMIT_BYTES = 1 << 16
    n = 5000
    scores = np.arange(n * 10, dtype=np.float32).reshape(n, 10)
    idx = np.arange(n * 10, dtype=np.int64).reshape(n, 10)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"scores": scores, "indices": idx})
    files = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(files) == ["indices.npy", "sample_rows.npy", "scores.npy"]
    assert sum(a.nbytes for a in files.values()) <= bench.DUMP_LIMIT_BYTES
    rows = files["sample_rows.npy"].astype(np.int64)
    assert len(rows) > 1 and np.all(np.diff(rows) > 0)
    assert np.array_equal(files["scores.npy"], scores[rows]) and np.array_equal(files["indices.npy"], idx[rows])
    for f, a in files.items():                       # the same sample from run to run
        assert np.array_equal(a, np.load(tmp_path / "b" / f))
