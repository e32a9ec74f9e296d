"""The de-duplication of fast tracking on the device (k_track_dedup_min, k_track_dedup_win, k_track_dedup_emit: per pixel of the
matched keypoint the candidate with the least (distance, place in candidate order), the winners in candidate order) against the
serial list of the host-only store and against the restatement (track_ref.py).  Bit for bit: floats as raw bytes, every integer
and list, no tolerance.  Host arrays and the flat view of track_cases, so every query falls on a chosen keypoint at a chosen
distance (track_dedup_cases.scene) and the surviving entry is also written out by hand.

One case -- keypoints at 3e9, -3e9, inf and NaN -- is held against the host-only store alone: track_ref converts a coordinate
with int(), which raises for a NaN and does not follow the pixel rule outside int's range.  track_dedup_cases.answers asserts
from the arrays that every other case has ordinary coordinates.

On the commit before the de-duplication ran on the device every test of this file fails (`python -m pytest -m gpu
tests/test_gpu_track_dedup.py`): LocalMap has no last_track_timing5, which the fixture that makes the stores asks for."""
import numpy as np
import pytest

import kfdb_cases as K
import track_cases as T
import track_dedup_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture(scope="module")
def make(mc, vocs):
    """make(store) -> (device store, host-only store) holding it; max_candidates = 1024, so 1024 candidates fill the arg-min
    table to its design load (2048 slots a camera)"""
    def stores(store, max_landmarks=2048, max_candidates=1024):
        out = [mc.LocalMap(voc, device=dev, max_landmarks=max_landmarks, max_candidates=max_candidates) for voc, dev in zip(vocs, (0, -1))]
        assert out[0].last_track_timing5() == (0.0,) * 5                      # the de-duplication's time is there to be read
        for lm in out:
            T.fill(lm, store)
        return out
    return stores


def flat(mc, make, kps, specs, cols=1280, rows=720, **kw):
    store, xy, ds, lids = D.scene(kps, specs)
    got, ref = D.answers(mc, make(store), T.flat_view(cols, rows), store, [xy], [ds], lids, **kw)
    assert got["n_candidates"] == len(specs)
    return got, ref


@pytest.mark.parametrize("dists,winner", [((5, 3), 1), ((5, 5), 0), ((3, 5), 0), ((7, 5, 3), 2), ((5, 5, 3), 2), ((3, 7, 5), 0),
                                          ((5, 3, 3), 1), ((5, 3, 4), 1)])
def test_distance_order_on_one_keypoint(mc, make, dists, winner):
    """two and three landmarks on one keypoint: a later one takes the entry only with a strictly smaller distance"""
    got, _ = flat(mc, make, [(200.0, 100.0), (300.0, 100.0)], [(0, d) for d in dists] + [(1, 2)])
    assert got["matches"][0] == sorted([(0, winner, dists[winner]), (1, len(dists), 2)], key=lambda e: e[1])


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("dists", [(6, 2), (2, 6), (4, 4)])
def test_two_keypoints_on_one_pixel(mc, make, swap, dists):
    """(10.2, 5.7) and (10.9, 5.1) are pixel (10, 5): one entry, and it names the winner's own keypoint"""
    kps = [(10.2, 5.7), (10.9, 5.1)][::-1 if swap else 1]
    got, _ = flat(mc, make, kps, [(0, dists[0]), (1, dists[1])])
    assert got["best"][0] == [(0, dists[0]), (1, dists[1])]
    w = 1 if dists[1] < dists[0] else 0
    assert got["matches"][0] == [(w, w, dists[w])]


@pytest.mark.parametrize("better_first", [True, False])
@pytest.mark.parametrize("a,b", [(63, 64), (255, 256), (0, 257), (0, 1023)])
def test_a_group_across_wave_and_block_boundaries(mc, make, a, b, better_first):
    """candidates a and b are on keypoint 0; of the others every fourth is on a keypoint of its own, the rest match nothing.  The
    entry sits where the winner is in candidate order: at the later index when the better one comes last"""
    n = b + 1 if b > 300 else b + 40
    own = [j for j in range(n) if j % 4 == 1 and j not in (a, b)]
    kps = [(100.0, 100.0)] + [(100.0 + (i % 32) + 1, 101.0 + i // 32) for i in range(len(own))]
    specs = [None] * n
    for i, j in enumerate(own):
        specs[j] = (i + 1, (j * 7) % 19)
    specs[a], specs[b] = (0, 3 if better_first else 9), (0, 9 if better_first else 3)
    got, _ = flat(mc, make, kps, specs)
    w = a if better_first else b
    want = sorted([(i + 1, j, (j * 7) % 19) for i, j in enumerate(own)] + [(0, w, 3)], key=lambda e: e[1])
    assert got["matches"][0] == want
    assert got["matches"][0].index((0, w, 3)) == sum(j < w for j in own)


@pytest.mark.parametrize("n", [257, 1024])
def test_all_candidates_on_one_keypoint(mc, make, n):
    """every atomic of the arg-min lands on one address.  Equal distances: the first candidate holds the entry.  Distances that
    never rise and fall strictly over the last 257 candidates -- a 256-bit descriptor has 257 distances, so 1024 strictly falling
    ones do not exist; with 257 candidates the whole list falls strictly: the last candidate holds it.  One row either way"""
    got, _ = flat(mc, make, [(400.0, 300.0)], [(0, 11)] * n)
    assert got["matches"][0] == [(0, 0, 11)] and len(got["best"][0]) == n
    dists = [256] * (n - 257) + list(range(256, -1, -1))
    assert len(dists) == n and all(x > y for x, y in zip(dists[-257:], dists[-256:]))
    got, _ = flat(mc, make, [(400.0, 300.0)], [(0, d) for d in dists], max_hamming=257)
    assert got["matches"][0] == [(0, n - 1, 0)] and got["best"][0] == [(0, d) for d in dists]


@pytest.mark.parametrize("layout", ["grid", "strided"])
def test_1024_candidates_on_1024_pixels(mc, make, layout):
    """the table at its design load: 1024 keys in 2048 slots collide in their probe sequences whatever the hash is.  Nothing is
    a duplicate: the output is the input, in order"""
    n = 1024
    if layout == "grid":
        kps, cols = [(50.0 + k % 32, 60.0 + k // 32) for k in range(n)], 1280
    else:
        kps, cols = [(37.0 * k, 11.0) for k in range(n)], 37 * n
    got, _ = flat(mc, make, kps, [(k, (k * 5) % 19) for k in range(n)], cols=cols)
    assert got["matches"][0] == [(k, k, (k * 5) % 19) for k in range(n)]


def test_awkward_pixel_keys(mc, make):
    """(-0.5, -0.5) and (0.3, 0.2) are pixel (0, 0), whose key is zero; (-1.0, -1.0) has the all-ones key, and a second landmark
    on it is rejected: neither value is taken for an empty slot"""
    at = (0.0, 0.0)
    got, ref = flat(mc, make, [(-0.5, -0.5), (0.3, 0.2), (-1.0, -1.0)], [(0, 5, at), (1, 3, at), (2, 4, at), (2, 4, at), (2, 6, at)])
    assert got["best"][0] == [(0, 5), (1, 3), (2, 4), (2, 4), (2, 6)] and got["matches"][0] == [(1, 1, 3), (2, 2, 4)]
    assert (ref["stats"]["replaced"], ref["stats"]["rejected"]) == (1, 2)
    got, _ = flat(mc, make, [(-1.0, -1.0), (0.3, 0.2)], [(0, 4, at), (0, 2, at), (1, 7, at), (1, 7, at)])
    assert got["matches"][0] == [(0, 1, 2), (1, 2, 7)]


def test_keypoints_outside_int(mc, make):
    """keypoints at 3e9, -3e9 and inf share the pixel (INT32_MIN, 7): with max_d2 = inf -- which is meant here -- they are
    neighbours of a query and their entries meet in the de-duplication, which the host-only store's result shows (three queries
    matched to three keypoints, one entry).  A keypoint with a NaN coordinate has a NaN distance to every query: it is matched
    with no radius at all and never reaches the de-duplication.  The host-only store is the only oracle of this case"""
    nan = float("nan")
    kps = [(3e9, 7.2), (-3e9, 7.9), (float("inf"), 7.5), (nan, 7.0), (12.0, nan), (50.0, 7.0)]
    at = (10.0, 7.0)
    store, xy, ds, lids = D.scene(kps, [(0, 5, at), (1, 3, at), (2, 3, at), (3, 0, at), (4, 0, at), (5, 2, at), (2, 1, at)])
    lms = make(store)
    host = T.as_lists(lms[1].track(T.to_view(mc, T.flat_view()), [xy], [ds], lids, max_d2=float("inf")))
    assert host["best"][0] == [(0, 5), (1, 3), (2, 3), (-1, 10000), (-1, 10000), (5, 2), (2, 1)]
    assert host["matches"][0] == [(5, 5, 2), (2, 6, 1)]
    got, _ = D.answers(mc, lms, T.flat_view(), store, [xy], [ds], lids, restate=False, max_d2=float("inf"))
    assert got == host
    got, _ = D.answers(mc, lms, T.flat_view(), store, [xy], [ds], lids, restate=False)
    assert got["matches"][0] == [(5, 5, 2)]


@pytest.mark.parametrize("ncams", [1, 4, 16])
def test_rigs(mc, make, ncams):
    """cameras that keep unequal numbers of the landmarks and have unequal numbers of keypoints; camera 1 has queries and no match,
    camera 2 no keypoints; then the same stores with no candidate at all"""
    v, store, kps, descs, lids = D.rig_scene(ncams, seed=ncams)
    lms = make(store)
    got, ref = D.answers(mc, lms, v, store, kps, descs, lids)
    n_proj, n_match = [len(p) for p in got["proj"]], [len(m) for m in got["matches"]]
    counts = D.dedup_counts(ref, kps)
    assert n_match[0] > 0 and counts[0][0] > 0 and counts[0][1] > 0
    if ncams > 1:
        assert len(set(n_proj)) > 2 and len(set(len(k) for k in kps)) > 2
        assert n_proj[1] > 0 and len(kps[1]) > 0 and n_match[1] == 0 and len(kps[2]) == 0 and n_match[2] == 0
        assert all(n_match[c] > 0 and counts[c][0] > 0 and counts[c][1] > 0 for c in range(3, ncams))
    got, _ = D.answers(mc, lms, v, store, kps, descs, [-1, -1])
    assert got["n_candidates"] == 0 and not any(got["proj"]) and not any(got["matches"])


def test_seeded_scene(mc, make):
    """the seeded 4-camera scene of track_cases through all stages; from the restatement alone: the serial list replaces and
    rejects in every camera"""
    v, store, kps, descs, lids = T.scene(4)
    assert all(len(k) for k in kps)
    got, ref = D.answers(mc, make(store), v, store, kps, descs, lids)
    for c, (rep, rej) in enumerate(D.dedup_counts(ref, kps)):
        assert rep > 0 and rej > 0, (c, rep, rej)
    assert all(len(m) > 0 for m in got["matches"])


def test_timing5(mc, make):
    v, store, kps, descs, lids = D.rig_scene(2, seed=5)
    lm = make(store)[0]
    view = T.to_view(mc, v)
    lm.track(view, kps, descs, lids)
    us = lm.last_track_timing5()
    assert us[4] > 0 and us[:4] == lm.last_track_timing4() and all(t > 0 for t in us[1:])
    lm.track(view, kps, descs, [-1, -1])                                      # no candidate: nothing is launched
    assert lm.last_track_timing5() == us


def test_short_caps(mc, make):
    """MCORB_E_CAP with every count set -- n_match comes from the device now -- and the store is as it was"""
    L = mc._lib
    v, store, kps, descs, lids = D.rig_scene(4, seed=9)
    lm = make(store)[0]
    view = T.to_view(mc, v)
    watched = sorted(store)[::5]
    before = T.snapshot(lm, watched)
    full = lm.track(view, kps, descs, lids)
    n_proj, n_match = [len(a) for a in full.proj_lid], [len(a) for a in full.match_kp]
    assert max(n_match) > 1 and max(n_match) < max(n_proj)
    for caps in ((max(n_proj) - 1, max(n_match)), (max(n_proj), max(n_match) - 1), (0, 0)):
        err = T.expect(mc, L.E_CAP, lambda: lm.track(view, kps, descs, lids, caps=caps))
        assert (err.n_candidates, err.n_proj, err.n_match) == (full.n_candidates, n_proj, n_match)
    assert T.as_lists(lm.track(view, kps, descs, lids, caps=(max(n_proj), max(n_match)))) == T.as_lists(full)
    assert T.snapshot(lm, watched) == before
