"""The local map (mcorb_lmap_*: FrontEnd::searchLocalMap2's candidates, frustum test, transform, InterMatchingBow and camera filter)
on the host-only store (device -1, with a host-only vocabulary and database), against the plain-Python restatement of
tests/lmap_ref.py and against hand-derived answers, everything exact.  No GPU is needed."""
import collections

import numpy as np
import pytest

import kfdb_cases as K
import lmap_cases as Lc
import lmap_ref as R
import mcorb

RESULT_FIELDS = ("new_lids", "cam_masks", "ind1", "ind2", "matches")


def host_voc():
    return mcorb.ORBVocabulary(device=-1).create(**K.vocabulary())


def make(mc, voc, device, probe, landmarks=None, max_landmarks=4096, max_candidates=4096, max_feats=600):
    """a store holding `landmarks` (lids, pts, normals, descs, mono) and a database whose probe slot 0 holds the frame `probe`"""
    db = mc.ORBDatabase(voc, device=device, max_entries=2, max_words=600, max_feats=max_feats)
    db.reserve_probes(2)
    db.set_probe(0, *probe)
    lm = mc.LocalMap(voc, device=device, max_landmarks=max_landmarks, max_candidates=max_candidates)
    if landmarks is not None:
        lm.set(*landmarks)
    return lm, db


def ref_store(landmarks):
    lids, pts, nrm, desc, mono = landmarks
    return {int(l): (pts[i], nrm[i], desc[i], bool(mono[i])) for i, l in enumerate(lids)}


def free(n, cam=0):
    """matched_cur / mono_cur / cam_cur of a probe whose n features are all unmatched, mono and seen by camera `cam`"""
    return np.zeros(n, np.uint8), np.ones(n, np.uint8), np.full(n, cam, np.int32)


def as_dict(res):
    return {f: getattr(res, f) for f in RESULT_FIELDS}


def same_result(got, want, what=""):
    got = as_dict(got) if not isinstance(got, dict) else got
    want = as_dict(want) if not isinstance(want, dict) else want
    for f in RESULT_FIELDS:
        assert got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


def one_mask(mc, lm, db, view, lid):
    res = lm.search(Lc.to_view(mc, view), [lid], [], db, 0, *free(len(db.get_probe(0)[2])), levelsup=K.LEVELSUP)
    assert len(res.new_lids) == (1 if len(res.cam_masks) else 0) and (not len(res.new_lids) or res.new_lids[0] == lid)
    return int(res.cam_masks[0]) if len(res.cam_masks) else 0


def gate_rows():
    """every hand-derived (view, pt, normal, mask) row of lmap_cases"""
    v, rows = Lc.gate_cases()
    out = [(n, v, p, q, w) for n, p, q, w in rows] + list(Lc.normal_cases())
    v, rows = Lc.coverage_cases()
    return out + [(n, v, p, q, w) for n, p, q, w in rows]


def probe3():
    """a three-feature probe frame from the vocabulary"""
    return Lc.probe_of(Lc.pool()[0][:3])


def test_round_trip_null_arrays_and_errors():
    lm, db = make(mcorb, host_voc(), -1, probe3(), max_landmarks=16)
    rng = np.random.default_rng(0)
    lids = np.array([3, 0, 15], np.int32)
    pts, nrm, desc = rng.normal(size=(3, 3)), rng.normal(size=(3, 3)), rng.integers(0, 256, (3, 32), dtype=np.uint8)
    lm.set(lids, pts, nrm)                                  # no descriptor yet
    p, q, d, mono = lm.get(0)
    assert p.tobytes() == pts[1].tobytes() and q.tobytes() == nrm[1].tobytes() and d is None and mono is False
    lm.set(lids, desc=desc, mono=[1, 0, 1])                 # NULL points and normals keep the old ones
    for i, l in enumerate(lids):
        p, q, d, mono = lm.get(int(l))
        assert p.tobytes() == pts[i].tobytes() and q.tobytes() == nrm[i].tobytes() and np.array_equal(d, desc[i]) and mono == bool([1, 0, 1][i])
    lm.set([0], pt3d=[[1.0, 2.0, 3.0]])                     # only the point changes
    p, q, d, mono = lm.get(0)
    assert p.tolist() == [1.0, 2.0, 3.0] and q.tobytes() == nrm[1].tobytes() and np.array_equal(d, desc[1]) and mono is False
    lm.set([5, 5], [[1, 1, 1], [2, 2, 2]], [[0, 0, 1], [0, 1, 0]])     # of an id given twice the last entry holds
    assert lm.get(5)[0].tolist() == [2.0, 2.0, 2.0] and lm.get(5)[1].tolist() == [0.0, 1.0, 0.0]
    lm.set([], np.zeros((0, 3)), np.zeros((0, 3)))
    for bad, code in (((16,), mcorb.E_ARG), ((-1,), mcorb.E_ARG)):
        with pytest.raises(mcorb.McorbError) as ei:
            lm.set(list(bad), [[0, 0, 0]], [[0, 0, 1]])
        assert ei.value.code == code
    with pytest.raises(mcorb.McorbError) as ei:             # a slot that was never set needs a point and a normal ...
        lm.set([3, 7], desc=desc[:2])
    assert ei.value.code == mcorb.E_STATE
    assert np.array_equal(lm.get(3)[2], desc[0])            # ... and nothing of the batch was stored
    for l, code in ((7, mcorb.E_STATE), (16, mcorb.E_ARG), (-1, mcorb.E_ARG)):
        with pytest.raises(mcorb.McorbError) as ei:
            lm.get(l)
        assert ei.value.code == code
    with pytest.raises(mcorb.McorbError) as ei:             # a host-only store needs a host-only vocabulary; no GPU is touched
        mcorb.LocalMap(host_voc(), device=0)
    assert ei.value.code == mcorb.E_ARG


def test_set_desc_from_entry_equals_set():
    voc = host_voc()
    kf = K.keyframe(64, 3)
    lm, db = make(mcorb, voc, -1, probe3(), max_landmarks=200)
    lm2 = mcorb.LocalMap(voc, device=-1, max_landmarks=200, max_candidates=8)
    e = db.add(*kf)
    n = len(kf[2])
    rng = np.random.default_rng(1)
    feats = rng.permutation(n)[:40].astype(np.int32)
    feats[5] = feats[4]                                     # one feature into two slots
    lids = rng.permutation(200)[:40].astype(np.int32)
    mono = rng.integers(0, 2, 40).astype(np.uint8)
    pts, nrm = rng.normal(size=(40, 3)), rng.normal(size=(40, 3))
    lm.set(lids[:30], pts[:30], nrm[:30])
    lm.set_desc_from_entry(db, e, lids, feats, mono)        # ten of the slots have no point yet
    lm.set(lids[30:], pts[30:], nrm[30:])
    stored = db.entry(e)[2]
    lm2.set(lids, pts, nrm, stored[feats], mono)
    for l in lids:
        a, b = lm.get(int(l)), lm2.get(int(l))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    lm.set_desc_from_entry(db, e, lids[:3], feats[:3])      # mono = NULL keeps the flags
    assert [lm.get(int(l))[3] for l in lids[:3]] == [bool(m) for m in mono[:3]]
    for args, code in (((e, [0], [n]), mcorb.E_ARG), ((e, [0], [-1]), mcorb.E_ARG), ((e, [200], [0]), mcorb.E_ARG), ((e + 1, [0], [0]), mcorb.E_ARG)):
        with pytest.raises(mcorb.McorbError) as ei:
            lm.set_desc_from_entry(db, *args)
        assert ei.value.code == code


def test_candidate_walk():
    """duplicates inside one keyframe and across keyframes, -1 entries, members of matched_lids; an empty list"""
    d = Lc.pool()[0]
    view, land = Lc.front_store(d[:12], lid0=20)
    lm, db = make(mcorb, host_voc(), -1, Lc.probe_of(d[:12]), land)
    kf1, kf2, kf3 = [25, -1, 21, 25, 30], [-1, 21, 22, 31, 22], [20, 30, 29]
    matched = [30, 29, 20 + 11]
    res = lm.search(Lc.to_view(mcorb, view), kf1 + kf2 + kf3, matched, db, 0, *free(12), levelsup=K.LEVELSUP)
    assert res.new_lids.tolist() == [25, 21, 22, 20] == R.candidates(kf1 + kf2 + kf3, matched)
    same_result(res, R.search(view, ref_store(land), kf1 + kf2 + kf3, matched, K.vocabulary(), db.get_probe(0)[1], d[:12], *free(12), K.LEVELSUP))
    assert sorted(zip(res.ind1.tolist(), res.ind2.tolist())) == [(0, 5), (1, 1), (2, 2), (3, 0)]      # each finds its own row of the probe
    for neigh, m in (([], []), ([-1, -1], []), ([25, 25], [25]), ([], [25])):
        res = lm.search(Lc.to_view(mcorb, view), neigh, m, db, 0, *free(12), levelsup=K.LEVELSUP)
        assert all(len(getattr(res, f)) == 0 for f in RESULT_FIELDS) and res.matches.shape == (0, 2)
    assert lm.last_timing()[2] == 0
    with pytest.raises(mcorb.McorbError) as ei:             # a candidate that was never set
        lm.search(Lc.to_view(mcorb, view), [25, 19], [], db, 0, *free(12), levelsup=K.LEVELSUP)
    assert ei.value.code == mcorb.E_STATE
    for neigh, m in (([4096], []), ([-2], []), ([25], [-1]), ([25], [4096])):
        with pytest.raises(mcorb.McorbError) as ei:
            lm.search(Lc.to_view(mcorb, view), neigh, m, db, 0, *free(12), levelsup=K.LEVELSUP)
        assert ei.value.code == mcorb.E_ARG


@pytest.mark.parametrize("row", gate_rows(), ids=lambda r: r[0])
def test_gate(row):
    """every gate at its boundary, one landmark per case: the hand-derived mask, which the restatement also gives"""
    name, view, pt, nrm, want = row
    d = Lc.pool()[0]
    lm, db = make(mcorb, host_voc(), -1, probe3(), ([9], [pt], [nrm], d[:1], [1]), max_landmarks=16)
    assert R.cull(view, pt, nrm) == want
    assert one_mask(mcorb, lm, db, view, 9) == want


def scene_landmarks(ncams, n=2000, seed=0):
    """the random scene's landmarks with descriptors that are near copies of a 257-row probe pool, and the probe frame"""
    view, pts, nrm = Lc.random_scene(ncams, n, seed)
    rng = np.random.default_rng(7 + seed)
    base = Lc.pool()[0][:257]
    desc = np.array([Lc.flip(rng, base[i % 257], 12) for i in range(n)], np.uint8)
    lids = rng.permutation(4096)[:n].astype(np.int32)
    mono = (rng.random(n) < 0.7).astype(np.uint8)
    cur = ((rng.random(257) < 0.2).astype(np.uint8), (rng.random(257) < 0.7).astype(np.uint8), rng.integers(0, ncams, 257).astype(np.int32))
    return view, (lids, pts, nrm, desc, mono), Lc.probe_of(base), cur


def test_random_scene_is_not_vacuous():
    """before agreement on the random scene means anything: at least 5 % of its (landmark, camera) pairs end at each gate and at
    least 20 % pass all of them"""
    view, pts, nrm = Lc.random_scene(4)
    c = collections.Counter(R.camera_verdict(view, cam, [float(x) for x in p], [float(x) for x in q]) for p, q in zip(pts, nrm) for cam in view["cams"])
    total = sum(c.values())
    assert total == 8000
    for gate in (R.Z_GATE, R.NORMAL_GATE, R.BOUNDS_GATE):
        assert c[gate] >= 0.05 * total, (gate, c)
    assert c[R.SEEN] >= 0.20 * total, c


@pytest.mark.parametrize("ncams", [1, 4, mcorb._lib.MAX_CAMS])
def test_rigs_on_the_random_scene(ncams):
    n = 2000 if ncams == 4 else 400
    view, land, probe, cur = scene_landmarks(ncams, n)
    lm, db = make(mcorb, host_voc(), -1, probe, land)
    rng = np.random.default_rng(3)
    neigh = np.concatenate([land[0], rng.choice(land[0], n // 4), np.full(n // 10, -1, np.int32)])[rng.permutation(n + n // 4 + n // 10)]
    matched = land[0][::17]
    for ratio in (0.85, 1.0):
        res = lm.search(Lc.to_view(mcorb, view), neigh, matched, db, 0, *cur, levelsup=K.LEVELSUP, max_neighbor_ratio=ratio)
        same_result(res, R.search(view, ref_store(land), neigh, matched, K.vocabulary(), probe[1], probe[2], *cur, K.LEVELSUP, ratio), (ncams, ratio))
    assert len(res.new_lids) > n // 8 and len(res.ind1) > 50 and 0 < len(res.matches) < len(res.ind1)
    assert len(set(res.cam_masks.tolist())) >= min(ncams, 3)      # several different camera sets


def test_shared_nodes_of_every_size():
    """shared nodes with 0, 1, 2, 63, 64 and 65 features on either side; the landmarks' FeatureVector is transform()'s"""
    A, probe = Lc.sized_frames()
    view, land = Lc.front_store(A, lid0=100)
    lm, db = make(mcorb, host_voc(), -1, probe, land)
    nb = len(probe[2])
    for ratio in (0.85, 1.0):
        res = lm.search(Lc.to_view(mcorb, view), land[0], [], db, 0, *free(nb), levelsup=K.LEVELSUP, max_neighbor_ratio=ratio)
        want = R.search(view, ref_store(land), land[0], [], K.vocabulary(), probe[1], probe[2], *free(nb), K.LEVELSUP, ratio)
        same_result(res, want, ratio)
    assert res.new_lids.tolist() == land[0].tolist() and sorted(len(f) for f in want["fv"].values()) == sorted(a for a, _ in Lc.NODE_SIZES if a)
    assert len(res.ind1) > 60 and np.array_equal(res.matches, np.stack([res.ind1, res.ind2], axis=1))


def test_get_matches_dist_ratio_branches():
    A, probe, levelsup = Lc.branch_frames()
    view, land = Lc.front_store(A)
    lm, db = make(mcorb, host_voc(), -1, probe, land)
    nb = len(probe[2])
    got = {}
    for ratio in (0.85, 1.0):
        res = lm.search(Lc.to_view(mcorb, view), land[0], [], db, 0, *free(nb), levelsup=levelsup, max_neighbor_ratio=ratio)
        same_result(res, R.search(view, ref_store(land), land[0], [], K.vocabulary(), probe[1], probe[2], *free(nb), levelsup, ratio), ratio)
        got[ratio] = set(zip(res.ind1.tolist(), res.ind2.tolist()))
    (_, fa, _), (_, fb, _) = K.match_pair()
    # K.match_pair()'s lists in A / B order without node 20 and the lists that have no A: positions of the rows here
    posA, posB, a, b = {}, {}, 0, 0
    for nid in sorted(fa):
        if nid == 20 or not fa[nid]:
            continue
        posA[nid] = list(range(a, a + len(fa[nid])))
        a += len(fa[nid])
        if nid in fb:
            posB[nid] = list(range(b, b + len(fb[nid])))
            b += len(fb[nid])
    want = {(posA[3][0], posB[3][0]), (posA[4][0], posB[4][0]), (posA[7][1], posB[7][0]), (posA[8][0], posB[8][0]), (posA[9][0], posB[9][0]),
            (posA[10][0], posB[10][0])}
    # (node 21, two of each, is left to the restatement); the hand-derived rest:
    assert {p for p in got[0.85] if p[0] not in posA[21]} == {p for p in want if p[0] not in posA[21]}
    # at 1.0 also 5 / 5 (the first of the equal rows) and 18 / 20
    assert {p for p in got[1.0] - got[0.85] if p[0] not in posA[21]} == {(posA[6][0], posB[6][0]), (posA[14][0], posB[14][0])}


def test_small_probes_and_nothing_accepted():
    d = Lc.pool()[0]
    view, land = Lc.front_store(d[:8])
    voc = host_voc()
    for nprobe in (0, 1):
        probe = Lc.probe_of(d[:nprobe])
        lm, db = make(mcorb, voc, -1, probe, land)
        res = lm.search(Lc.to_view(mcorb, view), land[0], [], db, 0, *free(nprobe), levelsup=K.LEVELSUP)
        same_result(res, R.search(view, ref_store(land), land[0], [], K.vocabulary(), probe[1], probe[2], *free(nprobe), K.LEVELSUP))
        assert len(res.new_lids) == 8 and len(res.ind1) == nprobe
    behind = (land[0], -land[1], land[2], land[3], land[4])      # every landmark behind the camera: status 0, empty outputs
    lm.set(*behind)
    res = lm.search(Lc.to_view(mcorb, view), land[0], [], db, 0, *free(1), levelsup=K.LEVELSUP)
    assert all(len(getattr(res, f)) == 0 for f in RESULT_FIELDS) and lm.last_timing()[2] == 8
    with pytest.raises(mcorb.McorbError) as ei:             # probe slot 1 was never set
        lm.search(Lc.to_view(mcorb, view), land[0], [], db, 1, *free(1), levelsup=K.LEVELSUP)
    assert ei.value.code == mcorb.E_STATE


def test_filter_conditions_one_at_a_time():
    """four landmarks that each match their own probe feature; two cameras, landmark 3 is seen by camera 0 only"""
    d = Lc.pool()[0][:4]
    view = Lc.view_of([Lc.cam(), Lc.cam(t=(600.0, 0.0, 0.0))])
    pts = np.array([[100.0, 100.0, 1.0]] * 3 + [[700.0, 100.0, 1.0]])
    land = (np.arange(4, dtype=np.int32), pts, np.tile(np.array(Lc.UP), (4, 1)), d, np.array([1, 1, 0, 1], np.uint8))
    lm, db = make(mcorb, host_voc(), -1, Lc.probe_of(d), land)

    def run(matched_cur, mono_cur, cam_cur):
        res = lm.search(Lc.to_view(mcorb, view), land[0], [], db, 0, matched_cur, mono_cur, cam_cur, levelsup=K.LEVELSUP)
        same_result(res, R.search(view, ref_store(land), land[0], [], K.vocabulary(), db.get_probe(0)[1], d, matched_cur, mono_cur, cam_cur, K.LEVELSUP))
        assert res.cam_masks.tolist() == [3, 3, 3, 1] and sorted(zip(res.ind1.tolist(), res.ind2.tolist())) == [(i, i) for i in range(4)]
        return sorted(res.matches[:, 0].tolist())

    assert run([0] * 4, [1] * 4, [0] * 4) == [0, 1, 3]            # the landmark's mono flag (landmark 2)
    assert run([0, 1, 0, 0], [1] * 4, [0] * 4) == [0, 3]          # matched_cur
    assert run([0] * 4, [0, 1, 1, 1], [0] * 4) == [1, 3]          # mono_cur
    assert run([0] * 4, [1] * 4, [1, 1, 1, 1]) == [0, 1]          # the camera: landmark 3 is not seen by camera 1
    assert run([0] * 4, [1] * 4, [1, -1, 0, 0]) == [0, 3]         # no camera at all
    lm.set([2], mono=[1])
    land[4][2] = 1
    assert run([0] * 4, [1] * 4, [0] * 4) == [0, 1, 2, 3]


def test_caps():
    d = Lc.pool()[0][:6]
    view, land = Lc.front_store(d)
    lm, db = make(mcorb, host_voc(), -1, Lc.probe_of(d), land, max_candidates=6)
    v = Lc.to_view(mcorb, view)
    full = lm.search(v, land[0], [], db, 0, *free(6), levelsup=K.LEVELSUP, caps=(6, 6, 6))
    assert len(full.new_lids) == len(full.ind1) == len(full.matches) == 6
    for caps in ((5, 6, 6), (6, 5, 6), (6, 6, 5), (0, 0, 0)):
        with pytest.raises(mcorb.McorbError) as ei:
            lm.search(v, land[0], [], db, 0, *free(6), levelsup=K.LEVELSUP, caps=caps)
        assert ei.value.code == mcorb.E_CAP and [c.value for c in lm.counts] == [6, 6, 6]      # the needed counts
    lm.set([6], [[640.0, 360.0, 1.0]], [Lc.UP], d[:1], [1])
    with pytest.raises(mcorb.McorbError) as ei:             # seven candidates in a store made for six
        lm.search(v, list(land[0]) + [6], [], db, 0, *free(6), levelsup=K.LEVELSUP)
    assert ei.value.code == mcorb.E_CAP and [c.value for c in lm.counts] == [0, 0, 0]
    same_result(lm.search(v, list(land[0]) + [6], [6], db, 0, *free(6), levelsup=K.LEVELSUP), full)     # ... six once one is matched already
    lm.set([7], [[640.0, 360.0, 1.0]], [Lc.UP])             # accepted, but without a descriptor
    with pytest.raises(mcorb.McorbError) as ei:
        lm.search(v, [7], [], db, 0, *free(6), levelsup=K.LEVELSUP)
    assert ei.value.code == mcorb.E_STATE
    lm.set([7], [[640.0, 360.0, -1.0]])                     # ... which only matters when it is accepted
    assert len(lm.search(v, [7], [], db, 0, *free(6), levelsup=K.LEVELSUP).new_lids) == 0


def test_known_answer():
    """Three landmarks, two cameras with K = identity that differ in t.x (0 and 600), 1280 x 720, worked out by hand.
    lid 7 at (100, 100, 1): x = 100 in camera 0, 700 in camera 1 -> cameras {0, 1}; lid 3 at (700, 100, 1): 700 and 1300 > 1250
    -> camera {0}; lid 11 at (100, 100, -1): z < 0 in both -> dropped.  The probe holds lid 3's descriptor, lid 7's and a third
    row, so accepted landmark 0 (lid 7) matches feature 1 and landmark 1 (lid 3) feature 0 at distance 0.  Every feature is mono
    and unmatched; features 0 and 1 are seen by camera 1: (0, 1) survives, (1, 0) does not -- lid 3 is seen by camera 0 only."""
    d = Lc.pool()[0]
    D7, D3, D11, X = d[10], d[11], d[12], d[13]
    view = Lc.view_of([Lc.cam(), Lc.cam(t=(600.0, 0.0, 0.0))])
    land = (np.array([7, 3, 11], np.int32), np.array([[100.0, 100.0, 1.0], [700.0, 100.0, 1.0], [100.0, 100.0, -1.0]]),
            np.tile(np.array(Lc.UP), (3, 1)), np.stack([D7, D3, D11]), np.ones(3, np.uint8))
    lm, db = make(mcorb, host_voc(), -1, Lc.probe_of(np.stack([D3, D7, X])), land)
    res = lm.search(Lc.to_view(mcorb, view), [7, -1, 3, 11, 7], [], db, 0, [0, 0, 0], [1, 1, 1], [1, 1, 0], levelsup=K.LEVELSUP)
    assert res.new_lids.tolist() == [7, 3] and res.cam_masks.tolist() == [3, 1]
    assert res.cam_ids(0) == [0, 1] and res.cam_ids(1) == [0]
    assert sorted(zip(res.ind1.tolist(), res.ind2.tolist())) == [(0, 1), (1, 0)]
    assert res.matches.tolist() == [[0, 1]]


def test_lf_mono_cam_helper():
    lf = np.zeros(3, mcorb._lib.LF_DTYPE)
    lf["match_index"] = -1
    lf["match_index"][0, 2] = 5
    lf["match_index"][1, 0] = 1
    lf["match_index"][1, 3] = 4
    lf["mono"] = [1, 0, 1]
    mono, cam = mcorb.lf_mono_cam(lf)
    assert mono.tolist() == [1, 0, 1] and cam.tolist() == [2, 0, -1]
