"""Fast tracking on the device (device >= 0: k_track_project, k_track_match, points and descriptors read from the store's slots in
HBM) against the host-only store (device -1) and the restatement (track_ref.py) on the same inputs, bit for bit: floats as raw
bytes, every integer and list.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_track.py`)."""
import numpy as np
import pytest

import kfdb_cases as K
import oracle_lib as O
import track_cases as T
import track_ref as R
from test_track_cpu import D0, check_boundary_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def stores(mc, vocs, store, max_landmarks=4096):
    out = [mc.LocalMap(voc, device=dev, max_landmarks=max_landmarks, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]
    for lm in out:
        T.fill(lm, store)
    return out


def both(mc, lms, v, store, kps, descs, lids, restated=True, **kw):
    """the device store against the host-only one, and (unless the case is large) against the restatement"""
    xy, ds = T.kp_arrays(kps, descs)
    got = [T.as_lists(lm.track(T.to_view(mc, v), xy, ds, lids, **kw)) for lm in lms]
    T.same(got[0], got[1], "device store against host-only store")
    if restated:
        ref = R.track(v, store, [a.tolist() for a in xy], ds, [int(l) for l in lids], **kw)
        T.same(got[0], T.ref_lists(ref, store), "device store against the restatement")
    return got[0]


def crowd(rng, n, ncams=1, cols=1280, rows=720):
    """n landmarks in front of a flat rig, most of them inside the image, with descriptors a few bits from a common one"""
    pts = np.stack([rng.uniform(-60, cols + 60, n), rng.uniform(-40, rows + 40, n), np.ones(n)], axis=1)
    pts[::9, 2] = -1.0                                                        # some behind
    return {i: (tuple(pts[i].tolist()), T.desc_at(D0, int(rng.integers(0, 12)), rng)) for i in range(n)}


def keypoints(rng, n, cols=1280, rows=720, spread=1.0):
    xy = np.stack([rng.uniform(0, cols * spread, n), rng.uniform(0, rows * spread, n)], axis=1).astype(np.float32)
    return xy, np.array([T.desc_at(D0, int(rng.integers(0, 40)), rng) for _ in range(n)], np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_candidate_counts(mc, vocs, n):
    """the lane, wave and workgroup edges of both kernels (256 lanes per workgroup of k_track_project; 4 waves x 4 candidates per
    workgroup of k_track_match), two cameras with different keypoint counts"""
    rng = np.random.default_rng(n)
    store = crowd(rng, max(n, 1))
    v = T.flat_view(ncams=2)
    (k0, d0), (k1, d1) = keypoints(rng, 150), keypoints(rng, 37, spread=0.5)
    got = both(mc, stores(mc, vocs, store), v, store, [k0, k1], [d0, d1], list(rng.permutation(max(n, 1))[:n]))
    if n >= 63:
        assert 0.5 * n < len(got["proj"][0]) < n and sum(k >= 0 for k, _ in got["best"][0]) > n // 8


@pytest.mark.parametrize("n_kp", [0, 1, 9, 10, 11, 63, 64, 65, 1025])
def test_keypoint_counts(mc, vocs, n_kp):
    """keypoints per camera around the neighbour count, the wave width and the LDS tile (MCORB_TRACK_TILE + 1: two tiles, the
    second with one keypoint); the keypoints crowd a 300 x 300 window, so most queries there have more than 10 within reach"""
    assert n_kp != 1025 or n_kp == mc._lib.TRACK_TILE + 1
    rng = np.random.default_rng(n_kp)
    store = crowd(rng, 90, cols=400, rows=400)
    v = T.flat_view(400, 400)
    xy, ds = keypoints(rng, n_kp, 300, 300)
    if n_kp == 1025:   # the one keypoint of the second tile is the best match of landmark 0's query
        store[0] = ((200.0, 200.0, 1.0), store[0][1])
        xy[:1024][np.hypot(xy[:1024, 0] - 200, xy[:1024, 1] - 200) < 3] += 5
        xy[1024], ds[1024] = (200.5, 200.0), store[0][1]
    got = both(mc, stores(mc, vocs, store), v, store, [xy], [ds], list(range(90)))
    if n_kp == 1025:
        at = [l for l, _, _ in got["proj"][0]].index(0)
        assert got["best"][0][at] == (1024, 0)


@pytest.mark.parametrize("ncams", [1, 4, 16])
def test_rigs_with_unequal_cameras(mc, vocs, ncams):
    """different keypoint counts per camera, one camera empty, one with more than a tile"""
    rng = np.random.default_rng(ncams)
    store = crowd(rng, 70)
    v = T.flat_view(ncams=ncams)
    counts = [[1100], [130, 0, 1100, 7], [40 + 13 * c for c in range(16)]][(1, 4, 16).index(ncams)]
    if ncams == 16:
        counts[5], counts[11] = 0, 1030
    kd = [keypoints(rng, n) for n in counts]
    both(mc, stores(mc, vocs, store), v, store, [k for k, _ in kd], [d for _, d in kd], list(range(70)), restated=ncams < 16)


def test_boundary_rows_in_one_launch(mc, vocs):
    """every hand-derived projection row of track_cases (the image edges to one float ulp, z of +-0, +-1e-300 and NaN, the rigs
    whose cameras disagree about the front), against the answers written out by hand: three views, so three calls, each with all
    rows of its view in one launch of each kernel"""
    def lm_of(store):
        lm = mc.LocalMap(vocs[0], device=0, max_landmarks=256, max_candidates=256)
        T.fill(lm, store)
        return lm
    assert check_boundary_rows(mc, lm_of) >= 25


def test_neighbour_and_gate_rows_in_one_launch(mc, vocs):
    """the rows of test_track_cpu's neighbour and gate tests as one launch: a query per block of the image, each with its own
    keypoints -- 0, 1, 9, 10, 11 and 40 within reach, equal d2 at different indices (d2 = max_d2 exactly), d2 one ulp under and
    one ulp above 10000.0, distances 19, 20 and 21, two neighbours at one distance, landmarks that share a keypoint"""
    queries, kps, descs, want = [], [], [], {}
    far = T.desc_at(D0, 100)

    def block(i):
        return 250.0 * (i % 5) + 125.0, 250.0 * (i // 5) + 125.0              # centres 250 apart: no block reaches another's keypoints

    for i, n in enumerate([0, 1, 9, 10, 11, 40]):
        cx, cy = block(i)
        queries.append((cx, cy, D0))
        first = len(kps)
        kps += T.ring(cx, cy, n, step=0.5)
        descs += [far] * max(n - 1, 0) + [T.desc_at(D0, 3)] * min(n, 1)
        want[i] = (first + n - 1, 3) if 1 <= n <= 10 else (-1, 10000)
    cx, cy = block(6)                                                         # equal d2: index order
    queries.append((cx, cy, D0))
    first = len(kps)
    kps += T.ring(cx, cy, 9) + [(cx - 100.0, cy), (cx + 100.0, cy), (cx, cy - 100.0), (cx, cy + 100.0)]
    descs += [far] * 9 + [T.desc_at(D0, k) for k in (5, 4, 3, 2)]
    want[6] = (first + 9, 5)
    for j, (nbits, w) in enumerate([(19, 19), (20, None), (21, None)]):      # the gate
        cx, cy = block(7 + j)
        queries.append((cx, cy, D0))
        kps.append((cx + 5.0, cy))
        descs.append(T.desc_at(D0, nbits))
        want[7 + j] = (len(kps) - 1, w) if w is not None else (-1, 10000)
    cx, cy = block(10)                                                        # equal distances: the nearer holds
    queries.append((cx, cy, D0))
    kps += [(cx + 20.0, cy), (cx + 10.0, cy)]
    descs += [T.desc_at(D0, 7), np.bitwise_xor(T.desc_at(D0, 7), np.bitwise_xor(D0, T.desc_at(D0, 14)))]
    want[10] = (len(kps) - 1, 7)
    cx, cy = block(11)                                                        # three landmarks on one keypoint: 9, 7, 5
    for j, d in enumerate((9, 7, 5)):
        queries.append((cx + 2 * j, cy, T.desc_at(D0, d)))
        want[11 + j] = (len(kps), d)
    kps.append((cx + 1.0, cy))
    descs.append(D0)
    shared = len(kps) - 1
    # d2 one ulp under 10000.0 (derived in test_track_cpu.test_radius_gate_at_the_boundary): query x = 2^-46, keypoint (100, 1e-6);
    # and one ulp above: dx = 100, dy = 1e-6.  Both queries lie on the row y = 0, more than 100 px from every block's keypoints
    dy = float(np.float32(1e-6))
    queries.append((2.0 ** -46, 0.0, D0))
    kps.append((100.0, dy))
    descs.append(T.desc_at(D0, 1))
    want[len(queries) - 1] = (len(kps) - 1, 1)
    queries.append((1270.0, 0.0, D0))
    kps.append((1170.0, dy))
    descs.append(D0)
    want[len(queries) - 1] = (-1, 10000)
    store = T.flat_store(queries)
    got = both(mc, stores(mc, vocs, store), T.flat_view(1280, 1000), store, [kps], [descs], sorted(store))
    assert got["best"][0] == [want[i] for i in range(len(queries))]
    assert (shared, 13, 5) in got["matches"][0] and len(got["matches"][0]) == 8


def test_max_hamming_and_max_d2(mc, vocs):
    rng = np.random.default_rng(5)
    store = crowd(rng, 64)
    xy, ds = keypoints(rng, 200)
    lms = stores(mc, vocs, store)
    for kw in (dict(max_hamming=0), dict(max_hamming=257), dict(max_d2=0.0), dict(max_d2=float("inf")), dict(max_d2=float("nan")),
               dict(max_d2=400.0, max_hamming=30)):
        got = both(mc, lms, T.flat_view(), store, [xy], [ds], list(range(64)), **kw)
        if kw.get("max_hamming") == 0 or kw.get("max_d2") == 0.0:
            assert all(k == -1 for k, _ in got["best"][0])
        if kw.get("max_hamming") == 257:
            assert sum(k >= 0 for k, _ in got["best"][0]) > 20


def test_seeded_scene(mc, vocs):
    """the 4-camera scene of test_track_cpu through all three output stages"""
    v, store, kps, descs, lids = T.scene(4)
    lms = stores(mc, vocs, store)
    before = [T.snapshot(lm, sorted(store)[::17]) for lm in lms]
    got = both(mc, lms, v, store, kps, descs, lids)
    assert sum(len(p) for p in got["proj"]) > 1000 and sum(len(m) for m in got["matches"]) > 100
    assert [T.snapshot(lm, sorted(store)[::17]) for lm in lms] == before      # the call only reads the store


def test_sees_the_stores_hbm_state(mc, vocs):
    """points moved by mcorb_lmap_update_points and descriptors written by set_desc_from_entry just before the call: the kernels
    read the slots in HBM, not a host copy of what mcorb_lmap_set was given"""
    rng = np.random.default_rng(9)
    n = 80
    store = crowd(rng, n)
    xy, ds = keypoints(rng, 120)
    lms = stores(mc, vocs, store)
    first = both(mc, lms, T.flat_view(), store, [xy], [ds], list(range(n)))
    # a database entry whose LF descriptors become the landmarks' (device to device on the device store)
    new_desc = np.array([T.desc_at(ds[int(rng.integers(0, len(ds)))], int(rng.integers(0, 6)), rng) for _ in range(n)], np.uint8)
    moved = np.array([store[i][0] for i in range(n)]) + np.stack([rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), np.zeros(n)], axis=1)
    feats = rng.permutation(n).astype(np.int32)
    bow, fv = O.bow_transform(K.vocabulary(), new_desc, K.LEVELSUP)
    for lm, voc, dev in zip(lms, vocs, (0, -1)):
        db = mc.ORBDatabase(voc, device=dev, max_entries=2, max_words=600, max_feats=600)
        entry = db.add(bow, fv, new_desc)
        lm.set_desc_from_entry(db, entry, np.arange(n, dtype=np.int32), feats)
        upd, _ = lm.update_points(np.arange(n, dtype=np.int32), moved, max_diff=1e9)
        assert upd.all()
    store2 = {i: (tuple(moved[i].tolist()), new_desc[feats[i]]) for i in range(n)}
    second = both(mc, lms, T.flat_view(), store2, [xy], [ds], list(range(n)))
    assert second["proj"] != first["proj"] and second["best"] != first["best"]


def test_timing(mc, vocs):
    rng = np.random.default_rng(3)
    store = crowd(rng, 100)
    xy, ds = keypoints(rng, 300)
    lm = stores(mc, vocs, store)[0]
    assert lm.last_track_timing() == (0.0, 0.0)
    lm.track(T.to_view(mc, T.flat_view()), [xy], [ds], list(range(100)))
    us = lm.last_track_timing()
    assert us[0] > 0 and us[1] > 0
    lm.track(T.to_view(mc, T.flat_view()), [xy], [ds], [-1, -1])              # no candidate: nothing is launched
    assert lm.last_track_timing() == us


@pytest.mark.parametrize("refine", [False, True])
def test_host_arrays_with_an_empty_camera_in_the_middle(mc, vocs, refine):
    """host arrays through the frame's item: cameras of 5, 0 and 1025 keypoints, so that first[c], the running keypoint count,
    repeats (5, 5) and the last camera has one keypoint in a second LDS tile of k_track_match; 257 candidates, one past a workgroup
    of k_track_compact and of the de-duplication.  The device store against the host-only store in every field of the
    TrackResult, without and with set_track_refine (then last_track_pose too)"""
    import pose_cases as PC
    rng = np.random.default_rng(257)
    n = 257
    store = crowd(rng, n)
    for l in (1, 2, 3, 4, 5, 7):                                              # (none behind: crowd puts every ninth there)
        store[l] = ((100.0 + 150.0 * l, 90.0 * l, 1.0), store[l][1])
    v = T.flat_view(ncams=3)
    k0 = np.array([store[l][0][:2] for l in (1, 2, 3, 4, 5)], np.float32) + 0.25
    d0 = np.array([store[l][1] for l in (1, 2, 3, 4, 5)], np.uint8)
    k2, d2 = keypoints(rng, 1025)
    x7, y7 = store[7][0][:2]
    k2[:1024][np.hypot(k2[:1024, 0] - x7, k2[:1024, 1] - y7) < 3] += 5
    k2[1024], d2[1024] = (x7 + 0.5, y7), store[7][1]                           # the second tile's one keypoint: landmark 7's match
    xy, ds = T.kp_arrays([k0, np.zeros((0, 2), np.float32), k2], [d0, np.zeros((0, 32), np.uint8), d2])
    lids = list(rng.permutation(n))
    lms = stores(mc, vocs, store)
    got, poses = [], []
    for lm in lms:
        lm.set_track_refine(PC.INV_SIGMA2 if refine else None)
        got.append(T.as_lists(lm.track(T.to_view(mc, v), xy, ds, lids)))
        if refine:
            poses.append(PC.as_ref(lm.last_track_pose()))
        lm.set_track_refine(None)
    T.same(got[0], got[1], "device store against host-only store")
    assert got[0] == got[1]
    assert got[0]["n_candidates"] == n and len(got[0]["proj"][1]) > n // 2
    assert len(got[0]["matches"][0]) == 5 and got[0]["matches"][1] == [] and all(b == (-1, 10000) for b in got[0]["best"][1])
    assert (1024, 7, 0) in got[0]["matches"][2] and len(got[0]["matches"][2]) > 20
    if refine:
        PC.same(poses[0], poses[1], "last_track_pose, device store against host-only store")
        assert len(poses[0]["inliers"]) == sum(len(m) for m in got[0]["matches"]) and 0 < poses[0]["n_inliers"] < len(poses[0]["inliers"])
