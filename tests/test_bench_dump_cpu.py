"""bench.py --dump-outputs: float32 where every value is exact in it, float64 otherwise; beyond the size cap the same fixed, seeded
sample of rows from run to run.  CPU only (the GPU half: tests/test_gpu_bench_modes.py)."""
import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole_and_exact(tmp_path):
    arrays = {"hry": np.arange(256, dtype=np.uint8), "org": np.array([0, 5, 2**24 - 1], np.uint32),
              "twin": np.array([1, 0, 0xFFFFFFFF], np.uint32), "rec": np.array([[1.5, -2.25], [3.0, 1e-3]], np.float32),
              "wide": np.array([0.1, 2.0]), "small": np.array([-7, 300], np.int16)}
    bench.dump_outputs(str(tmp_path), arrays)
    got = _load(tmp_path)
    assert set(got) == set(arrays)
    for k, a in arrays.items():
        assert got[k].shape == a.shape and np.array_equal(got[k], a.astype(np.float64)), k
    assert {k: got[k].dtype for k in got} == {"hry": np.float32, "org": np.float32, "twin": np.float64, "rec": np.float32,
                                              "wide": np.float64, "small": np.float32}


def test_large_outputs_keep_a_fixed_sample_under_the_cap(tmp_path):
    n = 12_000_000
    arrays = {"a": np.arange(n, dtype=np.uint32), "b": np.arange(3 * n, dtype=np.uint32).reshape(n, 3)}
    bench.dump_outputs(str(tmp_path / "1"), arrays)
    bench.dump_outputs(str(tmp_path / "2"), arrays)
    one, two = _load(tmp_path / "1"), _load(tmp_path / "2")
    assert sum(os.path.getsize(tmp_path / "1" / (k + ".npy")) for k in one) < 64e6
    for k in arrays:
        assert np.array_equal(one[k], two[k]) and 0 < len(one[k]) < n
    assert (one["a"].dtype, one["b"].dtype) == (np.float32, np.float64)   # (b holds values beyond 2^24)
    rows = one["a"].astype(np.int64)
    assert np.all(np.diff(rows) > 0)                                      # rows in their order
    assert np.array_equal(one["b"], arrays["b"][rows])                    # the same rows of every array
