"""The local map on the device (device >= 0: points, normals and descriptors in HBM, k_lmap_cull, the gathered rows through
k_bow_descend and k_kfdb_best2) against the host-only store, vocabulary and database (device -1) on the same inputs, bit for bit:
masks, lists and orders; on the inputs of test_lmap_cpu.py."""
import numpy as np
import pytest

import kfdb_cases as K
import lmap_cases as Lc
import lmap_ref as R
import oracle_lib as O
from test_gpu_live_lf import calib, frames
from test_kfdb_probe_cpu import same_frame
from test_lmap_cpu import RESULT_FIELDS, free, gate_rows, make, ref_store, same_result, scene_landmarks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    """the small vocabulary on the device and host-only"""
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def both(mc, vocs, probe, landmarks, **kw):
    (lm_d, db_d), (lm_h, db_h) = make(mc, vocs[0], 0, probe, landmarks, **kw), make(mc, vocs[1], -1, probe, landmarks, **kw)
    return (lm_d, db_d), (lm_h, db_h)


@pytest.fixture(scope="module")
def scene(mc, vocs):
    view, land, probe, cur = scene_landmarks(4, 2000)
    return view, land, probe, cur, both(mc, vocs, probe, land)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_candidate_counts(mc, scene, n):
    """the wave and workgroup edges of k_lmap_cull (256 lanes) and of the order-preserving compaction behind it"""
    view, land, probe, cur, ((lm_d, db_d), (lm_h, db_h)) = scene
    v = Lc.to_view(mc, view)
    neigh = land[0][100:100 + n]
    got = lm_d.search(v, neigh, [], db_d, 0, *cur, levelsup=K.LEVELSUP)
    same_result(got, lm_h.search(v, neigh, [], db_h, 0, *cur, levelsup=K.LEVELSUP), n)
    assert lm_d.last_timing()[2] == n
    if n >= 63:
        assert 0 < len(got.new_lids) < n


def test_boundary_cases_in_one_launch(mc, vocs):
    """every hand-derived gate case of the CPU file, all cases of a view in one launch"""
    views = {}
    for name, view, pt, nrm, want in gate_rows():
        views.setdefault(id(view), (view, []))[1].append((name, pt, nrm, want))
    d = Lc.pool()[0]
    assert len(views) == 4
    for view, rows in views.values():
        n = len(rows)
        land = (np.arange(n, dtype=np.int32), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]), d[:n], np.ones(n, np.uint8))
        (lm_d, db_d), (lm_h, db_h) = both(mc, vocs, Lc.probe_of(d[:3]), land, max_landmarks=64)
        got = lm_d.search(Lc.to_view(mc, view), land[0], [], db_d, 0, *free(3), levelsup=K.LEVELSUP)
        want = [(i, r[3]) for i, r in enumerate(rows) if r[3]]
        assert list(zip(got.new_lids.tolist(), got.cam_masks.tolist())) == want, [r[0] for r in rows]
        same_result(got, lm_h.search(Lc.to_view(mc, view), land[0], [], db_h, 0, *free(3), levelsup=K.LEVELSUP))
        for i in range(n):                                   # the points and normals came back from HBM as they were given
            p, q, dd, _ = lm_d.get(i)
            assert p.tobytes() == land[1][i].tobytes() and q.tobytes() == land[2][i].tobytes() and np.array_equal(dd, d[i])


def test_random_scene(mc, vocs, scene):
    """about 2000 candidates over 4 cameras with points on both sides of every gate (test_lmap_cpu.py checks that): the device
    equals the host-only store and the restatement; the landmarks' FeatureVector is mcorb_vocab_transform's"""
    view, land, probe, cur, ((lm_d, db_d), (lm_h, db_h)) = scene
    v = Lc.to_view(mc, view)
    rng = np.random.default_rng(3)
    neigh = np.concatenate([land[0], rng.choice(land[0], 500), np.full(200, -1, np.int32)])[rng.permutation(2700)]
    matched = land[0][::17]
    for ratio in (0.85, 1.0):
        got = lm_d.search(v, neigh, matched, db_d, 0, *cur, levelsup=K.LEVELSUP, max_neighbor_ratio=ratio)
        same_result(got, lm_h.search(v, neigh, matched, db_h, 0, *cur, levelsup=K.LEVELSUP, max_neighbor_ratio=ratio), ratio)
    want = R.search(view, ref_store(land), neigh, matched, K.vocabulary(), probe[1], probe[2], *cur, K.LEVELSUP, 1.0)
    same_result(got, want)
    assert lm_d.last_timing()[2] == 2000 - len(matched) and len(got.new_lids) > 1000 and len(got.ind1) > 100 and len(got.matches) > 10
    assert len(set(got.cam_masks.tolist())) > 6
    us = lm_d.last_timing()
    assert us[0] > 0 and us[1] > 0
    where = {int(l): i for i, l in enumerate(land[0])}
    _, fv = vocs[0].transform(land[3][[where[int(l)] for l in got.new_lids]], K.LEVELSUP)
    assert sorted(fv) == sorted(want["fv"]) and all(np.array_equal(fv[k], want["fv"][k]) for k in fv)


def test_sized_nodes_and_branches(mc, vocs):
    for A, probe, levelsup in (Lc.sized_frames() + (K.LEVELSUP,), Lc.branch_frames()):
        view, land = Lc.front_store(A, lid0=50)
        (lm_d, db_d), (lm_h, db_h) = both(mc, vocs, probe, land)
        nb = len(probe[2])
        for ratio in (0.85, 1.0):
            got = lm_d.search(Lc.to_view(mc, view), land[0], [], db_d, 0, *free(nb), levelsup=levelsup, max_neighbor_ratio=ratio)
            same_result(got, lm_h.search(Lc.to_view(mc, view), land[0], [], db_h, 0, *free(nb), levelsup=levelsup, max_neighbor_ratio=ratio))
        assert len(got.ind1) > 5


def test_searches_whose_second_half_shrinks(mc, vocs):
    """the cull accepts nothing (every candidate behind the camera: no gather, no descent, no search) and the accepted landmarks
    share no FeatureVector node with the probe (the gather and the descent run, k_kfdb_best2 has no item), for 1 and 65
    candidates: the device equals the host-only store, and a search with matches behind them is not disturbed"""
    d, node = Lc.pool()
    nodes = sorted(set(node.tolist()))
    A, B = d[node == nodes[0]][:65], d[node == nodes[1]][:40]
    view, land = Lc.front_store(A, lid0=7)
    behind = (land[0], land[1] * np.array([1.0, 1.0, -1.0]), land[2], land[3], land[4])
    v = Lc.to_view(mc, view)
    for landmarks, probe, accepted, matches in ((behind, Lc.probe_of(A), False, False), (land, Lc.probe_of(B), True, False),
                                                (land, Lc.probe_of(A), True, True)):
        (lm_d, db_d), (lm_h, db_h) = both(mc, vocs, probe, landmarks)
        nb = len(probe[2])
        for n in (1, 65):
            got = lm_d.search(v, land[0][:n], [], db_d, 0, *free(nb), levelsup=K.LEVELSUP)
            same_result(got, lm_h.search(v, land[0][:n], [], db_h, 0, *free(nb), levelsup=K.LEVELSUP), n)
            assert len(got.new_lids) == (n if accepted else 0) and lm_d.last_timing()[2] == n
            assert (len(got.ind1) > 0) == matches


def test_rig_frames_entry_to_store_and_probe(mc):
    """set_desc_from_entry from an entry written by add_rig_frame, a search whose probe was set by set_probe_rig_frame, and the
    entry and the probe read back unchanged after it"""
    C, W, H, F, levelsup = 4, 320, 240, 2, 2
    vd = O.make_vocabulary(10, 4, seed=3)
    voc_d, voc_h = mc.ORBVocabulary().create(**vd), mc.ORBVocabulary(device=-1).create(**vd)
    rig = mc.Rig(C, W, H, F, 1, nfeatures=300)
    rig.set_vocabulary(voc_d, levelsup=levelsup)
    rig.set_lf(*calib(C, W, H))
    rig.upload(frames(mc, F, C, W, H, f0=11))
    rig.extract(F * C)
    caps = dict(max_entries=2, max_words=2048, max_feats=2048)
    db_d, db_h = mc.ORBDatabase(voc_d, device=0, **caps), mc.ORBDatabase(voc_h, device=-1, **caps)
    for db in (db_d, db_h):
        db.reserve_probes(1)
        assert db.add_rig_frame(rig, 0) == 0
        db.set_probe_rig_frame(0, rig, 1)
    lf0, lf1 = rig.lf_features(0)[0], rig.lf_features(1)[0]
    n0, n1 = len(lf0), len(lf1)
    assert n0 > 50 and n1 > 50
    rng = np.random.default_rng(9)
    feats = rng.permutation(n0).astype(np.int32)                      # every LF feature of the keyframe is a landmark
    lids = rng.permutation(3000)[:n0].astype(np.int32)
    view, _ = Lc.coverage_cases()                                     # four cameras, K = identity, t.x = 0, 100, 200, 300
    pts = np.stack([rng.uniform(-300, 1500, n0), rng.uniform(0, 720, n0), np.ones(n0)], axis=1)
    mono0 = (lf0["mono"][feats] != 0).astype(np.uint8)
    lm_d, lm_h = mc.LocalMap(voc_d, device=0, max_landmarks=3000, max_candidates=n0), mc.LocalMap(voc_h, device=-1, max_landmarks=3000, max_candidates=n0)
    before = db_d.entry(0), db_d.get_probe(0)
    for lm, db in ((lm_d, db_d), (lm_h, db_h)):
        lm.set(lids, pts, np.tile(np.array(Lc.UP), (n0, 1)))
        lm.set_desc_from_entry(db, 0, lids, feats, mono0)
    for i in range(0, n0, 7):
        a, b = lm_d.get(int(lids[i])), lm_h.get(int(lids[i]))
        assert np.array_equal(a[2], lf0["desc"][feats[i]]) and np.array_equal(a[2], b[2]) and a[3] == b[3] == bool(mono0[i])
    with pytest.raises(mc.McorbError) as ei:                          # a database on another device
        lm_d.set_desc_from_entry(db_h, 0, lids[:1], feats[:1])
    assert ei.value.code == mc.E_ARG
    mono1, cam1 = mc.lf_mono_cam(lf1)
    matched = (rng.random(n1) < 0.1).astype(np.uint8)
    v = Lc.to_view(mc, view)
    got = lm_d.search(v, lids, [], db_d, 0, matched, mono1, cam1, levelsup=levelsup)
    same_result(got, lm_h.search(v, lids, [], db_h, 0, matched, mono1, cam1, levelsup=levelsup))
    with pytest.raises(mc.McorbError) as ei:
        lm_d.search(v, lids, [], db_h, 0, matched, mono1, cam1, levelsup=levelsup)
    assert ei.value.code == mc.E_ARG
    assert len(got.new_lids) > n0 // 3 and len(got.ind1) > 10 and len(got.matches) > 0
    same_frame(db_d.entry(0), before[0])
    same_frame(db_d.get_probe(0), before[1])
    same_frame(db_d.get_probe(0), (rig.lf_bow(1)[0], rig.lf_bow(1)[1], lf1["desc"]))
    rig.close()
