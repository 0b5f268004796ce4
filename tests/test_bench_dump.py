"""bench.py --dump-outputs: the last timed step's poses as .npy files, whole or as a fixed seeded sample above the size limit."""
import os

import numpy as np

import bench


def test_dump_writes_the_poses_whole(tmp_path):
    poses = np.random.default_rng(1).standard_normal((32, 15, 4, 4)).astype(np.float32)
    bench.dump_outputs(str(tmp_path), poses)
    assert sorted(os.listdir(tmp_path)) == ["poses.npy"]
    got = np.load(tmp_path / "poses.npy")
    assert got.dtype == np.float32 and np.array_equal(got, poses)
    bench.dump_outputs(str(tmp_path), poses, rank=3)
    assert np.array_equal(np.load(tmp_path / "poses_rank3.npy"), poses)


def test_dump_samples_large_outputs_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 * 1024)
    poses = np.arange(16384 * 16, dtype=np.float32).reshape(16384, 1, 4, 4)     # 1 MB > the limit
    bench.dump_outputs(str(tmp_path / "a"), poses)
    bench.dump_outputs(str(tmp_path / "b"), poses)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT_BYTES
    keep = np.load(tmp_path / "a" / "poses_instances.npy")
    got = np.load(tmp_path / "a" / "poses.npy")
    assert keep.dtype == np.float64 and np.array_equal(keep, np.load(tmp_path / "b" / "poses_instances.npy"))
    assert np.array_equal(got, poses[keep.astype(np.int64)]) and np.array_equal(got, np.load(tmp_path / "b" / "poses.npy"))
