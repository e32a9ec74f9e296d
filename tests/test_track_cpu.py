"""Fast tracking on the host-only store (device -1): mcorb_lmap_track against the plain-Python restatement of Tracking.cpp
(track_ref.py) and against answers written out by hand.  Every comparison is bit for bit, floats as raw bytes.  No GPU.

On the commit before this call existed every test of this file fails (`python -m pytest tests/test_track_cpu.py`): the package
has no track_view and LocalMap has no track."""
import ctypes as C
import math
import re
import os

import numpy as np
import pytest

import kfdb_cases as K
import track_cases as T
import track_ref as R
from track_cases import expect, f32bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def store_of(mc, voc, store, max_landmarks=4096, max_candidates=1024):
    lm = mc.LocalMap(voc, device=-1, max_landmarks=max_landmarks, max_candidates=max_candidates)
    T.fill(lm, store)
    return lm


D0 = np.arange(32, dtype=np.uint8) * 7 + 3          # some descriptor
FAR = T.desc_at(D0, 100)                            # one nobody matches


def flat(mc, voc, queries, kps, descs, cols=1280, rows=720, **kw):
    """one camera with x = X / 1: landmark i at queries[i] = (x, y, descriptor) -> (the result as lists, the restatement)"""
    store = T.flat_store(queries)
    return T.run(mc, store_of(mc, voc, store), T.flat_view(cols, rows), store, [kps], [descs], sorted(store), **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# projection: known answers written out by hand
# ---------------------------------------------------------------------------------------------------------------------------
def check_boundary_rows(mc, lm_of):
    """every row of track_cases.boundary_rows: one call (one launch of each kernel on a device store) per view -- there are three
    views -- with all its rows as candidates"""
    rows = T.boundary_rows()
    views = []
    for r in rows:
        if not any(r[1] is v for v in views):
            views.append(r[1])
    for v in views:
        mine = [r for r in rows if r[1] is v]
        store = {i: (r[2], D0) for i, r in enumerate(mine)}
        lm = lm_of(store)
        ncams = len(v["cams"])
        got, _ = T.run(mc, lm, v, store, [[]] * ncams, [[]] * ncams, list(range(len(mine))))
        for c in range(ncams):
            want = [(i, f32bits(r[3][c][0]), f32bits(r[3][c][1])) for i, r in enumerate(mine) if r[3] is not None and r[3][c] is not None]
            assert got["proj"][c] == want, (c, [r[0] for r in mine], got["proj"][c], want)
            assert got["best"][c] == [(-1, 10000)] * len(want) and got["matches"][c] == []
    return len(rows)


def test_projection_boundaries(mc, voc):
    assert check_boundary_rows(mc, lambda store: store_of(mc, voc, store)) >= 25
    # what the rows lean on
    assert T.up32(640) == 640.00006103515625 and T.down32(0.0) == -1.401298464324817e-45 and np.float32(640 + 1e-9) == np.float32(640)
    assert 3e-298 * (1.0 / 1e-300) != 300.0 and np.float32(3e-298 * (1.0 / 1e-300)) == np.float32(300.0)


def test_projection_general_pose_by_hand(mc, voc):
    """a quarter turn about z for the rig, a camera moved and turned about y, a skewed calibration: every number written out"""
    R0 = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    c, s = 0.8, 0.6                                                            # a 3-4-5 rotation about y, exact to a rounding
    Rc = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
    v = T.view([T.cam(Rc, (0.5, -0.25, 0.125), fx=400.0, fy=410.0, s=1.5, u0=320.0, v0=240.0)], 640, 480, R0, (1.0, 2.0, 3.0))
    X = (0.75, -1.5, 4.0)
    p0 = [(0.0 * X[0] + -1.0 * X[1] + 0.0 * X[2]) + 1.0, (1.0 * X[0] + 0.0 * X[1] + 0.0 * X[2]) + 2.0, (0.0 * X[0] + 0.0 * X[1] + 1.0 * X[2]) + 3.0]
    d = [p0[0] - 0.5, p0[1] - -0.25, p0[2] - 0.125]
    q = [c * d[0] + 0.0 * d[1] + -s * d[2], 0.0 * d[0] + 1.0 * d[1] + 0.0 * d[2], s * d[0] + 0.0 * d[1] + c * d[2]]   # R^T * d
    inv = 1.0 / q[2]
    pu, pv = q[0] * inv, q[1] * inv
    want = (np.float32(400.0 * pu + 1.5 * pv + 320.0), np.float32(410.0 * pv + 240.0))
    store = {11: (X, D0)}
    got, _ = T.run(mc, store_of(mc, voc, store), v, store, [[]], [[]], [11])
    assert got["proj"][0] == [(11, f32bits(want[0]), f32bits(want[1]))] and 0 < want[0] < 640 and 0 < want[1] < 480


# ---------------------------------------------------------------------------------------------------------------------------
# neighbours
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 9, 10, 11, 40])
def test_keypoints_in_radius(mc, voc, n):
    """n keypoints within reach at distances 10, 11, ..: the only one with a matching descriptor is the last, so it is matched
    iff it is among the 10 nearest; 5 more keypoints lie outside the radius and carry the descriptor itself"""
    kps = T.ring(500.0, 300.0, n) + [(500.0 + 100.5 + i, 300.0) for i in range(5)]
    descs = [FAR] * max(n - 1, 0) + [T.desc_at(D0, 3)] * min(n, 1) + [D0] * 5
    got, ref = flat(mc, voc, [(500.0, 300.0, D0)], kps, descs)
    want = (n - 1, 3) if 1 <= n <= 10 else (-1, 10000)
    assert got["best"][0] == [want] and got["matches"][0] == ([(n - 1, 0, 3)] if want[0] >= 0 else [])
    assert ref["stats"]["crowded"] == (n > 10) and ref["stats"]["empty"] == (n == 0)


def test_fewer_than_ten_keypoints_name_only_those(mc, voc):
    """3 keypoints in the camera, all out of reach; keypoint 0 carries the descriptor itself: the reference's zero-initialised
    result row would name it, the exact neighbours do not"""
    got, _ = flat(mc, voc, [(500.0, 300.0, D0)], [(100.0, 100.0), (900.0, 600.0), (20.0, 700.0)], [D0, D0, D0])
    assert got["best"][0] == [(-1, 10000)]


def test_radius_gate_at_the_boundary(mc, voc):
    """d2 = dx * dx + dy * dy around 10000.0 (the reference drops dists > 10000).  dx = 100, dy = 0: exactly 10000.0, inside.
    dx = 100, dy = 1e-6: the sum rounds to the next double above, outside.  One ulp under: the query at x = 2^-46 (a float) and the
    keypoint at (100, 1e-6): dx = -(100 - 2^-46) is exact in double, dx * dx = 10000 - 1.5625 ulp rounds to two ulps under 10000.0,
    and adding dy * dy = 0.55 ulp gives the double just under 10000.0: inside.  Then the keypoint one float ulp nearer and farther,
    and max_d2 one ulp either side of a d2 of exactly 10000.0"""
    dy, up0 = float(np.float32(1e-6)), T.up32(0.0)
    assert 100.0 * 100.0 + dy * dy == math.nextafter(10000.0, math.inf)
    x_under = 2.0 ** -46
    dx = float(np.float32(x_under)) - 100.0
    assert np.float32(x_under) == x_under and dx * dx == 10000.0 - 2 * math.ulp(9999.0) and dx * dx + dy * dy == math.nextafter(10000.0, -math.inf)
    for max_d2, inside in ((10000.0, True), (math.nextafter(10000.0, -math.inf), True), (10000.0 - 2 * math.ulp(9999.0), False)):
        got, _ = flat(mc, voc, [(x_under, 0.0, D0)], [(100.0, dy)], [D0], max_d2=max_d2)
        assert got["best"][0] == [(0, 0) if inside else (-1, 10000)], max_d2
    for kp, max_d2, inside in (((100.0, 0.0), 10000.0, True), ((100.0, dy), 10000.0, False),
                               ((T.down32(100.0), 0.0), 10000.0, True), ((T.up32(100.0), 0.0), 10000.0, False),   # one float ulp of kx
                               ((100.0, 0.0), math.nextafter(10000.0, math.inf), True),
                               ((100.0, 0.0), math.nextafter(10000.0, -math.inf), False),
                               ((100.0, dy), math.nextafter(10000.0, math.inf), True),
                               ((60.0, 80.0), 10000.0, True), ((100.0, 0.0), math.inf, True),
                               ((100.0, 0.0), math.nan, True),       # !(d2 > NaN): the reference's form drops nothing
                               ((0.0, 0.0), 0.0, True), ((up0, 0.0), 0.0, False)):          # the least float squared is a double > 0
        got, _ = flat(mc, voc, [(0.0, 0.0, D0)], [kp], [D0], max_d2=max_d2)
        assert got["best"][0] == [(0, 0) if inside else (-1, 10000)], (kp, max_d2)


def test_equal_d2_is_ordered_by_index(mc, voc):
    """9 keypoints nearer than 100, then four at d2 = 10000.0 exactly (left, right, above, below) at indices 9 .. 12 with
    descriptors at 5, 4, 3 and 2: only index 9 is among the 10"""
    kps = T.ring(500.0, 300.0, 9) + [(400.0, 300.0), (600.0, 300.0), (500.0, 200.0), (500.0, 400.0)]
    descs = [FAR] * 9 + [T.desc_at(D0, 5), T.desc_at(D0, 4), T.desc_at(D0, 3), T.desc_at(D0, 2)]
    got, _ = flat(mc, voc, [(500.0, 300.0, D0)], kps, descs)
    assert got["best"][0] == [(9, 5)]
    # the same keypoints in another order: the equal ones now come first in the array, the ring after them
    got, _ = flat(mc, voc, [(500.0, 300.0, D0)], kps[9:][::-1] + kps[:9], descs[9:][::-1] + descs[:9])
    assert got["best"][0] == [(0, 2)]


def test_the_eleventh_nearest_is_not_matched(mc, voc):
    kps = T.ring(500.0, 300.0, 11)
    got, _ = flat(mc, voc, [(500.0, 300.0, D0)], kps, [T.desc_at(D0, 15)] * 10 + [D0])
    assert got["best"][0] == [(0, 15)]                      # ten at 15: the nearest holds; the eleventh (distance 0) is not looked at
    got, _ = flat(mc, voc, [(500.0, 300.0, D0)], kps, [T.desc_at(D0, 25)] * 10 + [D0])
    assert got["best"][0] == [(-1, 10000)]


def test_a_camera_without_keypoints_and_a_nan_query(mc, voc):
    v = T.view([T.cam(), T.cam()], 640, 480)
    store = {0: ((50.0, 60.0, 1.0), D0), 1: ((1.0, 1.0, float("nan")), D0)}
    got, ref = T.run(mc, store_of(mc, voc, store), v, store, [[(50.0, 60.0), (51.0, 60.0)], []], [[D0, D0], []], [0, 1])
    nan = f32bits(np.float32(np.nan))
    assert nan == b"\x00\x00\xc0\x7f"                       # the default quiet NaN, whatever sign the machine's came with
    assert got["proj"][0] == got["proj"][1] == [(0, f32bits(50.0), f32bits(60.0)), (1, nan, nan)]
    assert got["best"][0] == [(0, 0), (-1, 10000)] and got["best"][1] == [(-1, 10000)] * 2
    assert got["matches"] == [[(0, 0, 0)], []] and ref["stats"]["empty"] == 3


# ---------------------------------------------------------------------------------------------------------------------------
# the descriptor gate
# ---------------------------------------------------------------------------------------------------------------------------
def test_hamming_gate(mc, voc):
    one = [(500.0, 300.0, D0)]
    for nbits, max_hamming, want in ((19, 20, (0, 19)), (20, 20, (-1, 10000)), (21, 20, (-1, 10000)), (0, 0, (-1, 10000)),
                                     (0, 1, (0, 0)), (256, 257, (0, 256)), (256, 256, (-1, 10000)), (21, 22, (0, 21))):
        got, _ = flat(mc, voc, one, [(505.0, 300.0)], [T.desc_at(D0, nbits)], max_hamming=max_hamming)
        assert got["best"][0] == [want], (nbits, max_hamming)
    # two neighbours at one distance: the nearer holds, whichever index it has; a farther one that is strictly better wins
    a = T.desc_at(D0, 7)                                                     # bits 0 .. 6
    c = np.bitwise_xor(a, np.bitwise_xor(D0, T.desc_at(D0, 14)))             # bits 7 .. 13
    assert R.hamming(D0, a) == R.hamming(D0, c) == 7 and R.hamming(a, c) == 14
    assert flat(mc, voc, one, [(520.0, 300.0), (510.0, 300.0)], [a, c])[0]["best"][0] == [(1, 7)]
    assert flat(mc, voc, one, [(510.0, 300.0), (520.0, 300.0)], [a, c])[0]["best"][0] == [(0, 7)]
    assert flat(mc, voc, one, [(510.0, 300.0), (520.0, 300.0)], [a, T.desc_at(D0, 6)])[0]["best"][0] == [(1, 6)]


# ---------------------------------------------------------------------------------------------------------------------------
# the de-duplication
# ---------------------------------------------------------------------------------------------------------------------------
def lm_desc(dist):
    """a landmark descriptor at `dist` from the keypoint descriptor D0"""
    return T.desc_at(D0, dist)


@pytest.mark.parametrize("dists,want", [((9, 5), [(0, 1, 5)]), ((5, 5), [(0, 0, 5)]), ((5, 9), [(0, 0, 5)]),
                                        ((9, 7, 5), [(0, 2, 5)]), ((9, 5, 7), [(0, 1, 5)]), ((5, 9, 5), [(0, 0, 5)]),
                                        ((7, 9, 5), [(0, 2, 5)]), ((5, 5, 5), [(0, 0, 5)])])
def test_landmarks_on_one_keypoint(mc, voc, dists, want):
    """two and three landmarks whose best keypoint is the same one: a later one replaces only when it is strictly better"""
    queries = [(300.0 + 2 * i, 200.0, lm_desc(d)) for i, d in enumerate(dists)]
    got, _ = flat(mc, voc, queries, [(301.0, 200.0)], [D0])
    assert got["best"][0] == [(0, d) for d in dists] and got["matches"][0] == want


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_two_keypoints_on_one_truncated_pixel(mc, voc, order):
    """(10.2, 5.7) and (10.9, 5.1) are both pixel (10, 5).  The entry found is compared by its own distance (the reference reads
    bestDists[k] of the new keypoint, which was never written: DESIGN.md section 8)"""
    kps = [[(10.2, 5.7), (10.9, 5.1)][i] for i in order]
    da, db = T.desc_at(D0, 40), T.desc_at(FAR, 40, np.random.default_rng(1))
    assert R.hamming(da, db) > 40
    descs = [[da, db][i] for i in order]
    # landmark 0 matches keypoint `a` at 6, landmark 1 matches keypoint `b` at 4 (replaces), landmark 2 matches `a` at 5 (rejected)
    queries = [(12.0, 6.0, T.desc_at(da, 6)), (12.0, 7.0, T.desc_at(db, 4)), (12.0, 8.0, T.desc_at(da, 5))]
    got, _ = flat(mc, voc, queries, kps, descs)
    ka, kb = order.index(0), order.index(1)
    assert got["best"][0] == [(ka, 6), (kb, 4), (ka, 5)] and got["matches"][0] == [(kb, 1, 4)]
    # the better one first: both later ones find its entry and leave it
    got, _ = flat(mc, voc, [queries[1], queries[0], queries[2]], kps, descs)
    assert got["best"][0] == [(kb, 4), (ka, 6), (ka, 5)] and got["matches"][0] == [(kb, 0, 4)]


def test_a_replacement_changes_the_order(mc, voc):
    """three keypoints matched in order, then a better landmark for the first: its entry moves to the end"""
    kps = [(100.0, 100.0), (400.0, 100.0), (700.0, 100.0)]
    ds = [T.desc_at(D0, 60), T.desc_at(D0, 60, np.random.default_rng(2)), T.desc_at(D0, 60, np.random.default_rng(3))]
    queries = [(101.0, 100.0, T.desc_at(ds[0], 8)), (401.0, 100.0, T.desc_at(ds[1], 3)), (701.0, 100.0, T.desc_at(ds[2], 2)),
               (99.0, 100.0, T.desc_at(ds[0], 1)), (399.0, 100.0, T.desc_at(ds[1], 3))]
    got, ref = flat(mc, voc, queries, kps, ds)
    assert got["matches"][0] == [(1, 1, 3), (2, 2, 2), (0, 3, 1)]
    assert (ref["stats"]["replaced"], ref["stats"]["rejected"]) == (1, 1)


def test_candidate_walk(mc, voc):
    """-1 and repeats are skipped, the order is the caller's"""
    queries = [(100.0 * (i + 1), 50.0, D0) for i in range(5)]
    store = T.flat_store(queries)
    lm = store_of(mc, voc, store)
    got, _ = T.run(mc, lm, T.flat_view(), store, [[]], [[]], [3, -1, 1, 3, 3, 0, -1, 1, 4])
    assert [p[0] for p in got["proj"][0]] == [3, 1, 0, 4] and got["n_candidates"] == 4
    got, _ = T.run(mc, lm, T.flat_view(), store, [[]], [[]], [-1, -1])
    assert got["proj"] == [[]] and got["n_candidates"] == 0
    got, _ = T.run(mc, lm, T.flat_view(), store, [[(1.0, 1.0)]], [[D0]], [])
    assert got["proj"] == [[]] and got["matches"] == [[]]


# ---------------------------------------------------------------------------------------------------------------------------
# errors and capacities: nothing in the store changes on any path
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors_and_caps(mc, voc):
    L = mc._lib
    queries = [(100.0 + 3 * i, 50.0, T.desc_at(D0, i % 5)) for i in range(70)]
    store = T.flat_store(queries)
    lm = mc.LocalMap(voc, device=-1, max_landmarks=128, max_candidates=64)
    T.fill(lm, store)
    lm.set([100], [[1.0, 2.0, 1.0]], [[0.0, 0.0, 1.0]])                      # a point, no descriptor
    lm.set_rays([3], [2])
    before = T.snapshot(lm, list(range(70)) + [100])
    v = T.to_view(mc, T.flat_view())
    kp, ds = [np.array([[100.0, 50.0], [130.0, 50.0]], np.float32)], [np.array([D0, D0])]
    ok = list(range(10))
    expect(mc, L.E_ARG, lambda: lm.track(v, kp, ds, [0, 128]))
    expect(mc, L.E_ARG, lambda: lm.track(v, kp, ds, [0, -2]))
    expect(mc, L.E_STATE, lambda: lm.track(v, kp, ds, [0, 100]))              # without a descriptor
    expect(mc, L.E_STATE, lambda: lm.track(v, kp, ds, [0, 101]))              # without a point
    err = expect(mc, L.E_CAP, lambda: lm.track(v, kp, ds, list(range(65))))   # more than max_candidates, before anything runs
    assert (err.n_candidates, err.n_proj, err.n_match) == (0, [0], [0])
    assert lm.track(v, kp, ds, list(range(64)) + [0, 1, -1]).n_candidates == 64
    expect(mc, L.E_ARG, lambda: lm.track(v, kp, ds, ok, max_hamming=-1))
    # an output that is short: MCORB_E_CAP with every count set
    full = lm.track(v, kp, ds, ok)
    np_, nm = len(full.proj_lid[0]), len(full.match_kp[0])
    assert np_ == 10 and nm == 2
    for caps in ((np_ - 1, nm), (np_, nm - 1), (0, 0)):
        err = expect(mc, L.E_CAP, lambda: lm.track(v, kp, ds, ok, caps=caps))
        assert (err.n_proj, err.n_match, err.n_candidates) == ([np_], [nm], 10)
    assert T.as_lists(lm.track(v, kp, ds, ok, caps=(np_, nm))) == T.as_lists(full)
    # the view and the frame, through the C ABI
    lids = np.array(ok, np.int32)
    xy, dd = np.ascontiguousarray(kp[0]), np.ascontiguousarray(ds[0])

    def call(view=v, ncams=1, n_kp=2, xy_ptr=xy.ctypes.data, d_ptr=dd.ctypes.data, out_null=None, lids_ptr=lids.ctypes.data, n=10):
        f = L.TrackFrame()
        f.ncams, f.n_kp[0], f.kp_xy[0], f.desc[0] = ncams, n_kp, xy_ptr, d_ptr
        o = L.TrackOut()
        o.cap_proj = o.cap_match = 16
        keep = []
        for name in ("proj_lid", "proj_xy", "best_kp", "best_dist", "match_kp", "match_lid", "match_dist", "match_pt"):
            keep.append(np.zeros(64, np.float64))                              # (room for any of them)
            setattr(o, name, None if name == out_null else keep[-1].ctypes.data)
        return lm.L.mcorb_lmap_track(lm.h, C.byref(view), C.byref(f), lids_ptr, n, 10000.0, 20, C.byref(o))

    assert call() == L.OK and call(out_null="match_pt") == L.OK
    for ncams in (0, -1, L.MAX_CAMS + 1):
        bad = T.to_view(mc, T.flat_view())
        bad.ncams = ncams
        assert call(view=bad, ncams=ncams) == L.E_ARG
    assert call(ncams=2) == L.E_ARG                                           # a frame of another camera count
    assert call(n_kp=-1) == L.E_ARG
    assert call(xy_ptr=None) == L.E_ARG and call(d_ptr=None) == L.E_ARG and call(n_kp=0, xy_ptr=None, d_ptr=None) == L.OK
    assert call(lids_ptr=None) == L.E_ARG and call(lids_ptr=None, n=0) == L.OK and call(n=-1) == L.E_ARG
    for name in ("proj_lid", "proj_xy", "best_kp", "best_dist", "match_kp", "match_lid", "match_dist"):
        assert call(out_null=name) == L.E_ARG, name
    assert T.snapshot(lm, list(range(70)) + [100]) == before


def test_abi_constants(mc):
    src = open(os.path.join(ROOT, "include", "mcorb.h")).read()
    assert int(re.search(r"#define MCORB_TRACK_TILE (\d+)", src).group(1)) == mc._lib.TRACK_TILE
    assert int(re.search(r"#define MCORB_TRACK_KNN (\d+)", src).group(1)) == mc._lib.TRACK_KNN == R.KNN
    assert C.sizeof(mc._lib.TrackCam) == 17 * 8 and C.sizeof(mc._lib.TrackView) == 12 * 8 + 16 + mc._lib.MAX_CAMS * 17 * 8


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded scene
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncams", [1, 4, 16])
def test_seeded_scene(mc, voc, ncams):
    v, store, kps, descs, lids = T.scene(ncams)
    # first, on the restatement alone: the scene reaches every branch often enough
    ref = R.track(v, store, [k.tolist() for k in kps], descs, lids)
    s = T.shares(ref["stats"])
    print("\nscene of %d cameras, %d landmarks, keypoints %s:" % (ncams, len(store), [len(k) for k in kps]))
    print("  pairs %(pairs)d: z <= 0 %(z_share).3f, bounds %(bounds_share).3f, projected %(projected_share).3f" % s)
    print("  queries %(queries)d: matched %(matched_share).3f, in radius but gated %(gated_share).3f, none in radius %(empty_share).3f, "
          "more than 10 in radius %(crowded_share).3f; replacements %(replaced)d, rejections %(rejected)d" % s)
    assert s["z_share"] >= 0.10 and s["bounds_share"] >= 0.10 and s["projected_share"] >= 0.30
    assert s["matched_share"] >= 0.20 and s["gated_share"] >= 0.10 and s["empty_share"] >= 0.05 and s["crowded_share"] >= 0.05
    assert s["replaced"] >= 20 and s["rejected"] >= 20
    lm = store_of(mc, voc, store)
    before = T.snapshot(lm, sorted(store)[::17])
    got, _ = T.run(mc, lm, v, store, kps, descs, lids)
    assert sum(len(m) for m in got["matches"]) == s["matched"] - s["replaced"] - s["rejected"]
    # bestMatchLandmarks are the store's points
    for c in range(ncams):
        pts = np.frombuffer(got["pts"][c], np.float64).reshape(-1, 3)
        for (_, lid, _), p in list(zip(got["matches"][c], pts))[::7]:
            assert p.tobytes() == lm.get(lid)[0].tobytes()
    assert T.snapshot(lm, sorted(store)[::17]) == before
