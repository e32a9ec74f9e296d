"""The landmarks' life on the host-only store (device -1): mcorb_lmap_observe, mcorb_lmap_update_points, mcorb_lmap_delete,
mcorb_lmap_observers, mcorb_lmap_set_rays and mcorb_lmap_get_observations against the plain-Python restatement of GlobalMap.cpp
(landmark_ref.py) and against answers written out by hand.  Every comparison is bit for bit.  No GPU.

On the commit before these calls existed every test of this file fails (`python -m pytest tests/test_landmark_cpu.py`): the
package has no obs_frame and LocalMap has none of the methods."""
import math

import numpy as np
import pytest

import kfdb_cases as K
import landmark_cases as Lc
import landmark_ref as R
import lmap_cases as Lm
import mapping_cases as Mc
from landmark_cases import bits, expect, frame, to_obs
from test_lmap_cpu import free, make


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def store(mc, voc, max_landmarks=4096):
    return mc.LocalMap(voc, device=-1, max_landmarks=max_landmarks, max_candidates=64)


ZERO = [[0.0, 0.0, 0.0]]


# ---------------------------------------------------------------------------------------------------------------------------
# known answers, written out by hand
# ---------------------------------------------------------------------------------------------------------------------------
def test_known_answers(mc, voc):
    lm = store(mc, voc)
    lm.set([0, 1], [[0.0, 0.0, 2.0]] * 2, ZERO * 2)
    # one camera at the origin: pt - c = (0, 0, 2) of length 2, the ray (0, 0, 2 * (1 / 2)), / 1
    assert lm.observe(mc.obs_frame(0, [[7]], [(0, 0, 0)]), [0], [0]).tolist() == [1]
    assert lm.get(0)[1].tolist() == [0.0, 0.0, 1.0] and lm.observations(0) == (1, [(0, 0)])
    # a camera at (3, 0, -2): pt - c = (-3, 0, 4) of length 5; -3 * (1.0 / 5.0) is not -3 / 5
    assert lm.observe(mc.obs_frame(0, [[7]], [(3, 0, -2)]), [1], [0]).tolist() == [1]
    assert lm.get(1)[1].tolist() == [-0.6000000000000001, 0.0, 0.8] and -0.6000000000000001 != -0.6 == -3 / 5
    # both cameras in one frame, on landmark 0: the second observation of the slot, n_rays 1 + 2
    fr2 = mc.obs_frame(4, [[-1, -1], [5, 9]], [(0, 0, 0), (3, 0, -2)])
    assert lm.observe(fr2, [0], [1]).tolist() == [3]
    acc = [0.0 + 0.0 + -3 * (1.0 / 5.0), 0.0, 0.0 + 2 * (1.0 / 2.0) + 4 * (1.0 / 5.0)]
    want = [(0.0 * 1.0 + acc[0]) * (1.0 / 3), 0.0, (1.0 * 1.0 + acc[2]) * (1.0 / 3)]
    assert lm.get(0)[1].tolist() == want and lm.observations(0) == (3, [(0, 0), (4, 1)])
    # a third observation from another keyframe, one camera at (0, 4, -1): pt - c = (0, -4, 3) of length 5; the running mean 3 + 1
    assert lm.observe(mc.obs_frame(9, [[2]], [(0, 4, -1)]), [0], [0]).tolist() == [4]
    want = [(want[0] * 3.0 + 0.0) * (1.0 / 4), (0.0 * 3.0 + -4 * (1.0 / 5.0)) * (1.0 / 4), (want[2] * 3.0 + 3 * (1.0 / 5.0)) * (1.0 / 4)]
    assert lm.get(0)[1].tolist() == want and lm.observations(0) == (4, [(0, 0), (4, 1), (9, 0)])
    assert lm.get(0)[0].tolist() == [0.0, 0.0, 2.0]                       # the point is never touched
    assert lm.observers([0, 1]).tolist() == [0, 4, 9]


def views_frame(kf_id, centres):
    """one feature that every camera sees"""
    return frame(kf_id, [[1] * len(centres)], centres)


@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 1), (4, 4), (8, 8)])
def test_first_and_later_observation(mc, voc, n1, n2):
    rng = np.random.default_rng(n1 * 10 + n2)
    pt = [0.3, -0.2, 6.0]
    f1, f2 = views_frame(1, rng.uniform(-1, 1, (n1, 3))), views_frame(2, rng.uniform(-1, 1, (n2, 3)))
    lm = store(mc, voc)
    lm.set([5], [pt], [[9.0, 9.0, 9.0]])                                  # the first observation replaces whatever normal was set
    ref = R.GlobalMap()
    ref.insert(5, pt, (9.0, 9.0, 9.0))
    for f, total in ((f1, n1), (f2, n1 + n2)):
        assert lm.observe(to_obs(mc, f), [5], [0]).tolist() == ref.observe(f, [5], [0]) == [total]
        Lc.same_landmark(mc, lm, 5, ref.mapPoints[5])
    # the written-out form, once more without the restatement's classes
    ray = lambda c: [(pt[k] - c[k]) * (1.0 / math.sqrt((pt[0] - c[0]) * (pt[0] - c[0]) + (pt[1] - c[1]) * (pt[1] - c[1]) + (pt[2] - c[2]) * (pt[2] - c[2])))
                     for k in range(3)]
    acc = [0.0] * 3
    for c in f1["centres"]:
        acc = [acc[k] + ray(c)[k] for k in range(3)]
    normal = [a * (1.0 / n1) for a in acc]
    acc = [0.0] * 3
    for c in f2["centres"]:
        acc = [acc[k] + ray(c)[k] for k in range(3)]
    normal = [(normal[k] * float(n1) + acc[k]) * (1.0 / (n1 + n2)) for k in range(3)]
    assert lm.get(5)[1].tolist() == normal


def test_record_leaves_normal_and_rays(mc, voc):
    lm = store(mc, voc)
    nrm = [[0.1, 0.2, 0.3]]
    lm.set([2], [[1.0, 2.0, 3.0]], nrm)
    lm.set_rays([2], [7])
    f = views_frame(3, [(0, 0, 0), (1, 0, 0)])
    assert lm.observe(to_obs(mc, f), [2, 2], [0, 0], mode=mc.OBS_RECORD).tolist() == [7, 7]
    assert bits(lm.get(2)[1]) == bits(nrm) and lm.observations(2) == (7, [(3, 0), (3, 0)])
    assert lm.observe(to_obs(mc, f), [2], [0]).tolist() == [9]            # not the first observation any more: 7 + 2
    ref = R.Landmark([1.0, 2.0, 3.0], nrm[0], 7)
    ref.KFs, ref.featInds = [3, 3], [0, 0]
    ref.add_lf_frame(f, 0)
    Lc.same_landmark(mc, lm, 2, ref)
    lm.set([2], [[1.0, 2.0, 3.5]], [[0.0, 1.0, 0.0]])                     # set leaves n_rays and the observations alone
    assert lm.observations(2) == (9, [(3, 0), (3, 0), (3, 0)])


def test_update_after_triangulation_needs_the_stored_rays(mc, voc):
    """a slot fresh from triangulate_neighbours, its two frames recorded, then a third keyframe: the restatement's third addLfFrame"""
    sc = Mc.scene(4, sizes=(40,), seed=5, zero_f=None)
    lm = store(mc, voc)
    Mc.fill_store(lm, sc["store"])
    got = Mc.run_scene(mc, lm, sc)
    idx = np.flatnonzero(got.new_lid >= 0)
    assert len(idx) >= 10
    rng = np.random.default_rng(1)
    f3 = Lc.random_frame(rng, 30, 4, 50, blind=0.0)
    nb, cur = frame(10, sc["neigh"][0]["match_index"], sc["neigh"][0]["centre_w"]), frame(20, sc["cur"]["match_index"], sc["cur"]["centre_w"])
    lids = got.new_lid[idx]
    q, t = sc["matches"][0][idx, 0], sc["matches"][0][idx, 1]
    views = [(sc["neigh"][0]["match_index"][a] != -1).sum() + (sc["cur"]["match_index"][b] != -1).sum() for a, b in zip(q, t)]
    assert lm.observe(to_obs(mc, nb), lids, q, mode=mc.OBS_RECORD).tolist() == views
    assert lm.observe(to_obs(mc, cur), lids, t, mode=mc.OBS_RECORD).tolist() == views
    assert len(set(views)) >= 3
    feats = rng.integers(0, 50, len(lids))
    lm.observe(to_obs(mc, f3), lids, feats)
    for i, lid, a, b, v, f in zip(idx, lids, q, t, views, feats):
        ref = R.Landmark(got.pt3d[i], got.normal[i], v)
        ref.record(nb, int(a)), ref.record(cur, int(b))
        ref.add_lf_frame(f3, int(f))
        Lc.same_landmark(mc, lm, int(lid), ref)


# ---------------------------------------------------------------------------------------------------------------------------
# an id more than once in a batch
# ---------------------------------------------------------------------------------------------------------------------------
def test_repeated_ids_equal_one_call_each(mc, voc):
    rng = np.random.default_rng(3)
    fr = Lc.random_frame(rng, 8, 4, 60, blind=0.0)
    pts = Lc.random_points(rng, 6)
    lids = np.array([0, 1, 0, 2, 3, 1, 0, 4, 5, 4], np.int32)            # 0 three times, 1 and 4 twice
    feats = rng.integers(0, 60, len(lids)).astype(np.int32)
    a, b = store(mc, voc), store(mc, voc)
    for lm in (a, b):
        lm.set(np.arange(6), pts, np.zeros((6, 3)))
        lm.observe(to_obs(mc, Lc.random_frame(np.random.default_rng(4), 2, 4, 9, blind=0.0)), [3, 4], [1, 2])   # 3 and 4 are not new
    na = a.observe(to_obs(mc, fr), lids, feats).tolist()
    nb = [int(b.observe(to_obs(mc, fr), [l], [f])[0]) for l, f in zip(lids, feats)]
    assert na == nb
    assert Lc.snapshot(a, range(6)) == Lc.snapshot(b, range(6))
    # update_points: the second item compares against the point the first one stored
    p1, p2, p3 = pts[0] + [1.0, 0, 0], pts[0] + [5.5, 0, 0], pts[0] + [9.0, 0, 0]
    upd, diff = a.update_points([0, 0, 0], [p1, p2, p3])
    assert upd.tolist() == [True, True, True] and bits(a.get(0)[0]) == bits(p3)       # 1.0, 4.5 and 3.5 apart
    one = [b.update_points([0], [p]) for p in (p1, p2, p3)]
    assert bits(diff) == bits([o[1][0] for o in one]) and bits(b.get(0)[0]) == bits(p3)
    upd, diff = a.update_points([1, 1], [pts[1] + [0, 6.0, 0], pts[1] + [0, 1.0, 0]])  # the first is refused, so the second is 1.0 apart
    assert upd.tolist() == [False, True] and 5.9 < diff[0] < 6.1 and 0.9 < diff[1] < 1.1


# ---------------------------------------------------------------------------------------------------------------------------
# update_points at the gate
# ---------------------------------------------------------------------------------------------------------------------------
def run_gate(mc, lm, lid0=0):
    """every row of gate_items on a slot of its own, the rows of one max_diff in one call -> [(replaced, diff_norm, stored point)]"""
    rows = Lc.gate_items()
    lids = np.arange(lid0, lid0 + len(rows), dtype=np.int32)
    lm.set(lids, [Lc.GATE_PT] * len(rows), [[0.0, 0.0, 1.0]] * len(rows))
    out = [None] * len(rows)
    order = sorted(range(len(rows)), key=lambda i: repr(rows[i][2]))
    by = {}
    for i in order:
        by.setdefault(repr(rows[i][2]), []).append(i)
    for sel in by.values():
        upd, diff = lm.update_points(lids[sel], [rows[i][1] for i in sel], max_diff=rows[sel[0]][2])
        for k, i in enumerate(sel):
            out[i] = (bool(upd[k]), float(diff[k]), lm.get(int(lids[i]))[0])
    return rows, out


def check_gate(rows, out):
    for (name, p, md, replaced), (upd, diff, stored) in zip(rows, out):
        ref = R.GlobalMap()
        ref.insert(0, Lc.GATE_PT)
        want = ref.update_landmark(0, p, md)
        assert upd == replaced == want[0], name
        assert bits(diff) == bits(want[1]) and bits(stored) == bits(ref.mapPoints[0].pt3D), name
        assert bits(stored) == bits(p if replaced else Lc.GATE_PT), name
    d = [o[1] for o in out]
    assert d[0] == 5.0 and d[1] == float(np.nextafter(5.0, 0.0)) and d[2] == float(np.nextafter(5.0, np.inf))
    assert math.isnan(d[3]) and d[4] == d[5] == float("inf") and d[6] == 0.0 and d[7] == 2.5 and d[8] == 2.0


def test_update_points_at_the_gate(mc, voc):
    lm = store(mc, voc)
    rows, out = run_gate(mc, lm)
    check_gate(rows, out)
    lm.set_rays([6], [3])                                                 # (slot 6 holds GATE_PT, 2.3 from the origin)
    before = Lc.snapshot(lm, [6])
    lm.update_points([6], [[0.0, 0.0, 0.0]])                              # normal, n_rays and observations are untouched
    after = Lc.snapshot(lm, [6])
    assert after[0][1:] == before[0][1:] and after[0][0] == bits([0.0, 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------------------
# the descriptor and the mono flag follow the latest observation
# ---------------------------------------------------------------------------------------------------------------------------
def test_descriptor_and_mono_follow_the_observation(mc, voc):
    kf = K.keyframe(64, 3)
    n = len(kf[2])
    a, db = make(mc, voc, -1, Lm.probe_of(Lm.pool()[0][:3]), max_landmarks=200)
    b = mc.LocalMap(voc, device=-1, max_landmarks=200, max_candidates=8)
    e = db.add(*kf)
    rng = np.random.default_rng(2)
    lids = rng.permutation(200)[:30].astype(np.int32)
    lids[7] = lids[3]                                                     # one landmark twice: the later row holds
    feats = rng.permutation(n)[:30].astype(np.int32)
    mono = rng.integers(0, 2, 30).astype(np.uint8)
    mono[3], mono[7] = 1, 0
    pts = Lc.random_points(rng, 30)
    fr = frame(6, np.ones((n, 2), np.int32), [(0, 0, 0), (0.5, 0, 0)])
    for lm in (a, b):
        lm.set(lids, pts, np.zeros((30, 3)))
    a.observe(to_obs(mc, fr), lids, feats, db=db, entry=e, mono=mono)
    b.observe(to_obs(mc, fr), lids, feats)
    b.set_desc_from_entry(db, e, lids, feats, mono)
    assert Lc.snapshot(a, lids) == Lc.snapshot(b, lids)
    assert np.array_equal(a.get(int(lids[3]))[2], db.entry(e)[2][feats[7]]) and a.get(int(lids[3]))[3] is False
    before = Lc.snapshot(a, lids)
    a.observe(to_obs(mc, fr), lids[:5], feats[5:10], mode=mc.OBS_RECORD)  # entry -1 keeps the descriptors, mono None the flags
    after = Lc.snapshot(a, lids)
    assert [x[:4] for x in after] == [x[:4] for x in before] and after[0][4][1][-1] == (6, int(feats[5]))
    a.observe(to_obs(mc, fr), lids[:1], feats[9:10], mode=mc.OBS_RECORD, db=db, entry=e)   # RECORD copies the row too
    assert np.array_equal(a.get(int(lids[0]))[2], db.entry(e)[2][feats[9]])


# ---------------------------------------------------------------------------------------------------------------------------
# delete and observers
# ---------------------------------------------------------------------------------------------------------------------------
def test_delete(mc, voc):
    d = Lm.pool()[0]
    view, land = Lm.front_store(d[:6])
    lm, db = make(mc, voc, -1, Lm.probe_of(d[:3]), land, max_landmarks=32)
    f = [frame(k, np.ones((9, 1), np.int32), [(0, 0, 0)]) for k in range(4)]
    lm.observe(to_obs(mc, f[2]), [0, 1, 2], [5, 6, 7])
    lm.observe(to_obs(mc, f[0]), [1, 2, 3], [1, 2, 3])
    lm.observe(to_obs(mc, f[3]), [1, 1], [8, 0])
    keep = Lc.snapshot(lm, [0, 3, 4, 5])
    expect(mc, mc.E_CAP, lambda: lm.delete([2, 1], cap=5))               # six pairs
    assert lm.delete_count.value == 6 and lm.observations(1)[1] == [(2, 6), (0, 1), (3, 8), (3, 0)]
    assert lm.delete([2, 1]) == [(2, 7), (0, 2), (2, 6), (0, 1), (3, 8), (3, 0)]   # lids order, then observation order
    for l in (1, 2):
        expect(mc, mc.E_STATE, lambda: lm.get(l))
        expect(mc, mc.E_STATE, lambda: lm.observations(l))
        expect(mc, mc.E_STATE, lambda: lm.search(Lm.to_view(mc, view), [0, l], [], db, 0, *free(3), levelsup=K.LEVELSUP))
        expect(mc, mc.E_STATE, lambda: lm.delete([l]))
        expect(mc, mc.E_STATE, lambda: lm.observe(to_obs(mc, f[0]), [l], [0]))
        expect(mc, mc.E_STATE, lambda: lm.update_points([l], ZERO))
    assert Lc.snapshot(lm, [0, 3, 4, 5]) == keep
    assert lm.search(Lm.to_view(mc, view), [0, 3, 4, 5], [], db, 0, *free(3), levelsup=K.LEVELSUP).new_lids.tolist() == [0, 3, 4, 5]
    assert lm.delete([4]) == [] and lm.delete([]) == []                   # a landmark nobody observes; an empty batch
    lm.set([1], [[1.0, 1.0, 1.0]], ZERO)                                  # set again after delete: a new landmark
    assert lm.observations(1) == (0, []) and lm.get(1)[2] is None and lm.get(1)[3] is False
    assert lm.observe(to_obs(mc, f[1]), [1], [4]).tolist() == [1] and lm.observations(1) == (1, [(1, 4)])


def test_observers(mc, voc):
    lm = store(mc, voc)
    lm.set(np.arange(5), Lc.random_points(np.random.default_rng(0), 5), np.zeros((5, 3)))
    f = {k: frame(k, np.ones((3, 1), np.int32), [(0, 0, 0)]) for k in (40, 7, 19, 3)}
    for k, lids in ((40, [0, 1]), (7, [1, 2]), (19, [0, 2, 3]), (3, [3]), (7, [0])):
        lm.observe(to_obs(mc, f[k]), lids, [0] * len(lids))
    assert lm.observers([0, 1, 2, 3]).tolist() == [3, 7, 19, 40]
    assert lm.observers([1]).tolist() == [7, 40] and lm.observers([3, 3]).tolist() == [3, 19]
    assert lm.observers([4]).tolist() == [] and lm.observers([]).tolist() == []
    expect(mc, mc.E_CAP, lambda: lm.observers([0, 1], cap=2))
    assert lm.observers_count.value == 3
    expect(mc, mc.E_STATE, lambda: lm.observers([0, 5]))
    expect(mc, mc.E_ARG, lambda: lm.observers([4096]))


# ---------------------------------------------------------------------------------------------------------------------------
# what is refused is refused before anything runs
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(mc, voc):
    kf = K.keyframe(64, 3)
    n = len(kf[2])
    lm, db = make(mc, voc, -1, Lm.probe_of(Lm.pool()[0][:3]), max_landmarks=16)
    e = db.add(*kf)
    lm.set([0, 1, 2], Lc.random_points(np.random.default_rng(0), 3), np.zeros((3, 3)))
    mi = np.ones((n + 2, 2), np.int32)
    mi[1] = -1                                                            # feature 1 has no view
    ok = mc.obs_frame(5, mi, [(0, 0, 0), (1, 0, 0)])
    lm.observe(ok, [0, 1], [0, 2], db=db, entry=e, mono=[1, 0])
    before = Lc.snapshot(lm, [0, 1, 2])

    def refused(code, fn):
        expect(mc, code, fn)
        assert Lc.snapshot(lm, [0, 1, 2]) == before

    for mode in (mc.OBS_UPDATE, mc.OBS_RECORD):
        refused(mc.E_ARG, lambda: lm.observe(ok, [0, 16], [0, 0], mode=mode))                 # ids outside the store
        refused(mc.E_ARG, lambda: lm.observe(ok, [0, -1], [0, 0], mode=mode))
        refused(mc.E_ARG, lambda: lm.observe(ok, [0, 2], [0, n + 2], mode=mode))              # feat outside the frame
        refused(mc.E_ARG, lambda: lm.observe(ok, [0, 2], [0, -1], mode=mode))
        refused(mc.E_ARG, lambda: lm.observe(ok, [0, 2], [0, 1], mode=mode))                  # a feature with no view
        refused(mc.E_ARG, lambda: lm.observe(ok, [0, 2], [0, n], mode=mode, db=db, entry=e))  # a row outside the entry
        refused(mc.E_ARG, lambda: lm.observe(ok, [0, 2], [0, 0], mode=mode, db=db, entry=e + 1))
        refused(mc.E_STATE, lambda: lm.observe(ok, [0, 3], [0, 0], mode=mode))                # a slot without a point
    refused(mc.E_ARG, lambda: lm.observe(ok, [0], [0], mode=2))
    refused(mc.E_ARG, lambda: lm.observe(mc.obs_frame(-1, mi, [(0, 0, 0), (1, 0, 0)]), [0], [0]))
    for ncams in (0, 17):
        bad = mc.obs_frame(5, mi, [(0, 0, 0), (1, 0, 0)])
        bad.struct.ncams = ncams
        refused(mc.E_ARG, lambda: lm.observe(bad, [0], [0]))
    refused(mc.E_ARG, lambda: lm.update_points([0, 16], ZERO * 2))
    refused(mc.E_STATE, lambda: lm.update_points([0, 3], ZERO * 2))
    refused(mc.E_ARG, lambda: lm.delete([0, 1, 0]))                                            # an id twice
    refused(mc.E_ARG, lambda: lm.delete([0, 16]))
    refused(mc.E_STATE, lambda: lm.delete([0, 3]))
    refused(mc.E_CAP, lambda: lm.delete([0, 1], cap=1))
    refused(mc.E_ARG, lambda: lm.set_rays([0, 16], [1, 1]))
    refused(mc.E_ARG, lambda: lm.set_rays([0, 1], [1, -1]))
    refused(mc.E_STATE, lambda: lm.set_rays([0, 3], [1, 1]))
    refused(mc.E_ARG, lambda: lm.observations(16))
    assert lm.observe(ok, [], []).tolist() == [] and lm.update_points([], np.zeros((0, 3)))[0].tolist() == []
    lm.set_rays([2, 2], [4, 6])                                                                # the last occurrence holds
    assert lm.observations(2) == (6, [])
    with pytest.raises(ValueError):
        mc.obs_frame(0, np.ones((2, 17), np.int32), [(0, 0, 0)] * 17)


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded life cycle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncams", [1, 4, 8])
def test_life_cycle(mc, voc, ncams):
    ref, stats, _ = Lc.life_cycle(mc, [store(mc, voc)], ncams)
    Lc.life_cycle_is_rich(stats)
    assert len(ref.mapPoints) > 150 and max(l.n_rays for l in ref.mapPoints.values()) >= (3 if ncams == 1 else 8)
