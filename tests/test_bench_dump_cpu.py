"""bench.py --dump-outputs (no GPU): the sampled frames are fixed for fixed arguments, every array is float32 / float64,
the ragged per-image lists come back whole through their counts, and the files stay under the size cap."""
import os

import numpy as np

import bench
from importlib import import_module

KP_DTYPE = import_module("mc-slam_amd._lib").KP_DTYPE


def _fake_path(ncams):
    def features(f, c):
        rng = np.random.default_rng(f * 16 + c)
        n = 1900 + (f * 7 + c) % 101
        k = np.zeros(n, KP_DTYPE)
        k["x"], k["y"], k["octave"] = rng.random(n) * 1280, rng.random(n) * 720, rng.integers(0, 8, n)
        return c - 1, k, rng.integers(0, 256, (n, 32), dtype=np.uint8)

    def tracks(f):
        return np.arange((30 + f) * ncams, dtype=np.int32).reshape(-1, ncams) - 1, f % 5
    return features, tracks


def test_dump_is_fixed_typed_and_complete(tmp_path):
    C, frames = 4, list(range(512))
    features, tracks = _fake_path(C)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, C, 2048, frames, tracks, features)
    bench.dump_outputs(b, C, 2048, frames, tracks, features)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) == sorted(n + ".npy" for n in (
        "frames", "tracks", "track_counts", "tracks_merged", "mono_index", "keypoint_counts", "keypoints", "descriptors"))
    d = {n[:-4]: np.load(os.path.join(a, n)) for n in names}
    for n in names:
        assert np.array_equal(d[n[:-4]], np.load(os.path.join(b, n)))
    assert all(x.dtype in (np.float32, np.float64) for x in d.values())
    assert sum(x.nbytes for x in d.values()) <= bench.DUMP_BYTES_MAX
    pick = d["frames"].astype(int)
    assert len(pick) == bench.DUMP_FRAMES and list(pick) == sorted(set(pick))
    # the concatenated lists split back into exactly what the path returned, frame by frame and camera by camera
    kpos, tpos = 0, 0
    for i, f in enumerate(pick):
        t, mg = tracks(f)
        assert d["track_counts"][i] == len(t) and d["tracks_merged"][i] == mg
        assert np.array_equal(d["tracks"][tpos:tpos + len(t)], t)
        tpos += len(t)
        for c in range(C):
            mono, k, desc = features(f, c)
            n = int(d["keypoint_counts"][i, c])
            assert n == len(k) and d["mono_index"][i, c] == mono
            assert np.array_equal(d["descriptors"][kpos:kpos + n], desc)
            assert np.array_equal(d["keypoints"][kpos:kpos + n, 0], k["x"]) and np.array_equal(d["keypoints"][kpos:kpos + n, 5], k["octave"])
            kpos += n
    assert kpos == len(d["keypoints"]) == len(d["descriptors"]) and tpos == len(d["tracks"])


def test_dump_of_a_tracks_only_path_and_a_small_step(tmp_path):
    C = 8
    _, tracks = _fake_path(C)
    bench.dump_outputs(str(tmp_path), C, 2048, [9, 3, 5], tracks, suffix="_r1")
    assert sorted(os.listdir(tmp_path)) == ["frames_r1.npy", "track_counts_r1.npy", "tracks_merged_r1.npy", "tracks_r1.npy"]
    assert list(np.load(str(tmp_path / "frames_r1.npy"))) == [3, 5, 9]
