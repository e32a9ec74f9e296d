"""k_track_compact at its own edges, through LocalMap.track on host arrays (no rig): candidate counts around one, two and four
workgroups of 256, rigs of 1 and 16 cameras, and validity patterns that put the kept candidates at the ends of a workgroup, in one
workgroup only, in none and in every other one.  The device store against the host-only store (and, for one camera, against the
restatement), bit for bit; the projected lists are also held against the pattern itself.

On the commit before the slot entry every test of this file fails (`python -m pytest -m gpu tests/test_gpu_track_compact.py`): the
fixture asks for LocalMap.track_rig_frame, which came with the kernel."""
import numpy as np
import pytest

import kfdb_cases as K
import track_cases as T
import track_ref as R
from test_track_cpu import D0

pytestmark = pytest.mark.gpu
N = 1024   # max_candidates of the fixture


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


def point(i):
    return 5.0 + 10.0 * (i % 64), 5.0 + 10.0 * (i // 64)


@pytest.fixture(scope="module")
def scene(mc):
    """landmark i < N in view at point(i); landmark N + i at the same place behind the rig: a pattern picks one of the two"""
    assert hasattr(mc.LocalMap, "track_rig_frame")
    rng = np.random.default_rng(0)
    store = {}
    for i in range(N):
        x, y = point(i)
        d = T.desc_at(D0, int(rng.integers(0, 10)), rng)
        store[i] = ((x, y, 1.0), d)
        store[N + i] = ((x, y, -1.0), d)
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    lms = [mc.LocalMap(voc, device=dev, max_landmarks=2 * N, max_candidates=N) for voc, dev in zip(vocs, (0, -1))]
    for lm in lms:
        T.fill(lm, store)
    # a few keypoints on landmarks of every workgroup's range, so kept rows carry matches as well
    on = [0, 1, 254, 255, 256, 257, 511, 512, 700, 1023]
    xy = np.array([point(i) for i in on], np.float32) + np.float32(0.25)
    ds = np.array([T.desc_at(D0, 2 * (j % 4)) for j in range(len(on))], np.uint8)
    return store, lms, xy, ds


def patterns(n):
    out = {"all": [True] * n, "none": [False] * n, "first": [i == 0 for i in range(n)], "last": [i == n - 1 for i in range(n)],
           "alternating blocks": [(i // 256) % 2 == 0 for i in range(n)], "other blocks": [(i // 256) % 2 == 1 for i in range(n)]}
    if n > 256:
        out["only 256"] = [i == 256 for i in range(n)]
    return out


@pytest.mark.parametrize("ncams", [1, 16])
@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513, 1024])
def test_compaction_edges(mc, scene, n, ncams):
    store, lms, xy, ds = scene
    v = T.flat_view(ncams=ncams)
    view = T.to_view(mc, v)
    kps = [xy[:len(xy) - (c % 3)] for c in range(ncams)]
    descs = [ds[:len(xy) - (c % 3)] for c in range(ncams)]
    for name, keep in patterns(n).items():
        lids = [i if keep[i] else N + i for i in range(n)]
        got = [T.as_lists(lm.track(view, kps, descs, lids)) for lm in lms]
        T.same(got[0], got[1], "device store against host-only store, %s" % name)
        want = [(i, T.f32bits(point(i)[0]), T.f32bits(point(i)[1])) for i in range(n) if keep[i]]
        for c in range(ncams):
            assert got[0]["proj"][c] == want, (name, c)
        if ncams == 1:
            ref = R.track(v, store, [a.tolist() for a in kps], descs, lids)
            T.same(got[0], T.ref_lists(ref, store), "device store against the restatement, %s" % name)
            if name == "all":
                assert len(ref["matches"][0]) >= 5
