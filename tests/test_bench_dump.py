"""CPU: bench.py --dump-outputs' writer — float64 files, at most 64 MB in all, and a larger output replaced by the same seeded sample on
every run (two builds are compared file by file)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_is_bounded_and_repeatable(tmp_path):
    big = np.arange(24 << 20, dtype=np.float64)             # 192 MB alone
    arrays = {"aln_log_probs": -big, "seeds": np.arange(1000, dtype=np.int32), "map_gt": np.arange(6, dtype=np.int32).reshape(3, 2)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["aln_log_probs_sample.npy", "map_gt.npy", "seeds.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in names) <= 64e6
    for n in names:
        a, b = np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n))
        assert a.dtype == np.float64 and np.array_equal(a, b)
    s = np.load(str(tmp_path / "a" / "aln_log_probs_sample.npy"))
    assert len(s) == bench.DUMP_BYTES // 8 // 3 and np.all(np.diff(s) < 0)         # distinct elements, in index order
    assert np.array_equal(np.load(str(tmp_path / "a" / "seeds.npy")), np.arange(1000))
    assert np.array_equal(np.load(str(tmp_path / "a" / "map_gt.npy")), np.arange(6))
