"""The landmarks' life on the device (device >= 0: k_lmap_observe, k_lmap_update, n_rays in HBM) against the host-only store
(device -1) and the restatement (landmark_ref.py) on the same inputs, bit for bit: doubles as raw bytes, every integer and list.

On the commit before these calls existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_landmark.py`)."""
import numpy as np
import pytest

import kfdb_cases as K
import landmark_cases as Lc
import landmark_ref as R
import lmap_cases as Lm
import oracle_lib as O
from landmark_cases import bits, frame, to_obs
from test_gpu_live_lf import calib, frames
from test_kfdb_probe_cpu import same_frame
from test_landmark_cpu import check_gate, run_gate
from test_lmap_cpu import free, make, same_result

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def stores(mc, vocs, max_landmarks=4096):
    return [mc.LocalMap(voc, device=dev, max_landmarks=max_landmarks, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.mark.parametrize("n", SIZES)
def test_observe_item_counts(mc, vocs, n):
    """the wave and workgroup edges of k_lmap_observe (256 lanes) on a 4-camera rig; about half of the landmarks have observations
    already, so first and later observations mix within every wave"""
    b = Lc.batch(n, 4, n)
    ref = Lc.run_batch(mc, stores(mc, vocs), *b)
    if n >= 63:
        first = sum(len(l.KFs) == 1 for l in ref.mapPoints.values())
        assert n // 5 < first < n and len({l.n_rays for l in ref.mapPoints.values()}) >= 6


@pytest.mark.parametrize("n", SIZES)
def test_update_item_counts(mc, vocs, n):
    """the edges of k_lmap_update: corrections on both sides of the gate"""
    rng = np.random.default_rng(n)
    nl = max(n, 1)
    pts = Lc.random_points(rng, nl)
    lids = rng.permutation(4096)[:nl].astype(np.int32)
    sel = rng.permutation(nl)[:n]
    d = rng.normal(size=(n, 3))
    new = pts[sel] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([0.5, 4.9, 5.1, 8.0], (n, 1))
    out = []
    for lm in stores(mc, vocs):
        lm.set(lids, pts, np.zeros_like(pts))
        upd, diff = lm.update_points(lids[sel], new)
        out.append((upd.tolist(), bits(diff), Lc.snapshot(lm, lids)))
    assert out[0] == out[1]
    ref = R.GlobalMap()
    for l, p in zip(lids, pts):
        ref.insert(int(l), p)
    want = [ref.update_landmark(l, p) for l, p in zip(lids[sel], new)]
    assert out[0][0] == [w[0] for w in want] and out[0][1] == bits([w[1] for w in want])
    if n >= 63:
        assert 0.2 * n < sum(out[0][0]) < 0.8 * n


def test_camera_masks_in_one_launch(mc, vocs):
    """rigs of 1, 4 and 8 cameras; every feature count of views from one to all cameras, and every single camera, in one launch"""
    for ncams in (1, 4, 8):
        rng = np.random.default_rng(ncams)
        masks = sorted({(1 << k) - 1 for k in range(1, ncams + 1)} | {1 << c for c in range(ncams)} | {int(m) for m in rng.integers(1, 1 << ncams, 40)})
        mi = np.array([[c if (m >> c) & 1 else -1 for c in range(ncams)] for m in masks], np.int32)
        fr = frame(2, mi, rng.uniform(-1, 1, (ncams, 3)))
        n = 3 * len(masks)
        pts = Lc.random_points(rng, n)
        old = [Lc.random_frame(rng, 1, ncams, 40, blind=0.0)]
        had = np.arange(n) % 2 == 0
        feats = (np.arange(n) % len(masks)).astype(np.int32)
        ref = Lc.run_batch(mc, stores(mc, vocs), pts, old, had, fr, np.arange(n, dtype=np.int32), feats)
        assert max(l.n_rays for l in ref.mapPoints.values()) >= ncams + 1


def test_repeated_ids_across_workgroups(mc, vocs):
    """ids two and three times in a batch of 600, with occurrences on either side of item 256: the rounds; against the host-only
    store, the restatement, and the same items sent one call each"""
    rng = np.random.default_rng(12)
    n = 600
    pts, old, had, fr, _, _ = Lc.batch(300, 4, 77)
    lids = np.concatenate([np.arange(300), np.arange(100, 300), np.arange(250, 350) % 300]).astype(np.int32)   # 250 .. 299 three times
    lids[255], lids[257] = 7, 7                                           # and one id on both sides of the workgroup edge
    feats = rng.choice(Lc.seen_feats(fr), n).astype(np.int32)
    both = stores(mc, vocs)
    ref = Lc.run_batch(mc, both, pts, old, had, fr, lids, feats)
    assert max(len(l.KFs) for l in ref.mapPoints.values()) >= 5
    assert both[0].last_landmark_timing()[0] > 0
    one = stores(mc, vocs)[0]                                             # the same items, one call each
    Lc.run_batch(mc, [one], pts, old, had, fr, lids[:0], feats[:0])
    obs = to_obs(mc, fr)
    for l, f in zip(lids.tolist(), feats.tolist()):
        one.observe(obs, [l], [f])
    Lc.same_map(mc, one, ref)
    # update_points with the same shape of batch
    d = rng.normal(size=(n, 3)) * rng.choice([0.3, 2.0, 4.0], (n, 1))
    new = pts[lids] + d
    want = [ref.update_landmark(l, p) for l, p in zip(lids, new)]
    for lm in both:
        upd, diff = lm.update_points(lids, new)
        assert upd.tolist() == [w[0] for w in want] and bits(diff) == bits([w[1] for w in want])
        Lc.same_map(mc, lm, ref)
    assert 0.05 * n < sum(not w[0] for w in want) < 0.6 * n


def test_batches_where_a_chain_shrinks(mc, vocs):
    """the calls whose submission shrinks to one piece or to none, device against host-only, bit for bit: observe that records
    only (no kernel, no entry: nothing is queued), one item, and every id twice; update_points, set_rays and delete with one item
    and with every id twice (delete refuses that on both, and nothing changes)"""
    rng = np.random.default_rng(41)
    ncams, n = 4, 6
    pts = Lc.random_points(rng, n)
    lids = np.arange(20, 20 + n, dtype=np.int32)
    fr = [Lc.random_frame(rng, 1 + k, ncams, 30, blind=0.0) for k in range(3)]
    twice = np.concatenate([lids, lids[::-1]])
    step = {len(sel): rng.choice([0.5, 8.0], (len(sel), 1)) for sel in (lids[:1], twice)}
    out = []
    for lm in stores(mc, vocs):
        lm.set(lids, pts, np.zeros_like(pts))
        got = [lm.observe(to_obs(mc, fr[0]), lids[:1], [3]).tolist()]                              # one item
        got.append(lm.observe(to_obs(mc, fr[1]), lids, np.arange(n), mode=mc.OBS_RECORD).tolist())   # nothing queued
        got.append(lm.observe(to_obs(mc, fr[1]), lids[:1], [7], mode=mc.OBS_RECORD).tolist())
        got.append(lm.observe(to_obs(mc, fr[2]), twice, np.arange(2 * n)).tolist())                # every id twice
        got.append(Lc.snapshot(lm, lids))
        for sel in (lids[:1], twice):
            new = pts[sel - 20] + step[len(sel)]
            upd, diff = lm.update_points(sel, new)
            got.append((upd.tolist(), bits(diff)))
            lm.set_rays(sel, np.arange(len(sel)) + 2)
            got.append(Lc.snapshot(lm, lids))
        Lc.expect(mc, mc.E_ARG, lambda: lm.delete(twice))
        got.append(Lc.snapshot(lm, lids))
        got.append(lm.delete(lids[:1]))
        Lc.expect(mc, mc.E_STATE, lambda: lm.get(int(lids[0])))
        got.append(Lc.snapshot(lm, lids[1:]))
        out.append(got)
    assert out[0] == out[1]
    assert out[0][3][:n] != out[0][3][n:] and len(out[0][-2]) == 5


def test_gate_values_in_one_launch(mc, vocs):
    """every gate row of the CPU file; the rows of one max_diff share a launch"""
    both = stores(mc, vocs)
    out = []
    for lm in both:
        rows, o = run_gate(mc, lm, lid0=100)
        check_gate(rows, o)
        out.append([(u, bits(d), bits(p)) for u, d, p in o])
    assert out[0] == out[1]
    us = both[0].last_landmark_timing()
    assert us[1] > 0
    assert both[0].update_points([], np.zeros((0, 3)))[0].tolist() == [] and both[0].last_landmark_timing() == us


def test_rig_frame_entry_to_observe(mc):
    """observe with a database entry written by add_rig_frame: the descriptors equal the entry's rows and the host-only store's,
    and entry and probe read back unchanged"""
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
    lf0 = rig.lf_features(0)[0]
    rng = np.random.default_rng(9)
    feats = rng.permutation(np.flatnonzero((lf0["match_index"][:, :C] != -1).any(axis=1))).astype(np.int32)
    n0 = len(feats)
    assert n0 > 50
    lids = rng.permutation(3000)[:n0].astype(np.int32)
    lids[5] = lids[2]                                                     # one landmark twice
    pts = Lc.random_points(rng, n0)
    mono = (lf0["mono"][feats] != 0).astype(np.uint8)
    fr = mc.obs_frame(0, lf0, rng.uniform(-1, 1, (C, 3)))
    lm_d, lm_h = mc.LocalMap(voc_d, device=0, max_landmarks=3000, max_candidates=16), mc.LocalMap(voc_h, device=-1, max_landmarks=3000, max_candidates=16)
    before = db_d.entry(0), db_d.get_probe(0)
    for lm, db in ((lm_d, db_d), (lm_h, db_h)):
        lm.set(lids, pts, np.zeros_like(pts))
        lm.observe(fr, lids, feats, db=db, entry=0, mono=mono)
    assert Lc.snapshot(lm_d, lids) == Lc.snapshot(lm_h, lids)
    for i in [2] + list(range(0, n0, 5)):
        want = feats[5] if i == 2 else feats[i]
        assert np.array_equal(lm_d.get(int(lids[i]))[2], lf0["desc"][want])
    with pytest.raises(mc.McorbError) as ei:                              # a database on another device
        lm_d.observe(fr, lids[:1], feats[:1], db=db_h, entry=0)
    assert ei.value.code == mc.E_ARG
    same_frame(db_d.entry(0), before[0])
    same_frame(db_d.get_probe(0), before[1])
    rig.close()


def test_life_cycle_then_search(mc, vocs):
    """the seeded life cycle on the 4-camera rig on both stores; then the survivors get descriptors and are searched"""
    pool = Lm.pool()[0]
    probe = Lm.probe_of(pool[:257])
    (lm_d, db_d), (lm_h, db_h) = make(mc, vocs[0], 0, probe), make(mc, vocs[1], -1, probe)
    ref, stats, sc = Lc.life_cycle(mc, [lm_d, lm_h], 4)
    Lc.life_cycle_is_rich(stats)
    us = lm_d.last_landmark_timing()
    assert us[0] > 0 and us[1] > 0
    assert lm_d.observe(mc.obs_frame(99, [[1, 1, 1, 1]], np.zeros((4, 3))), [], []).tolist() == []
    assert lm_d.update_points([], np.zeros((0, 3)))[0].tolist() == [] and lm_d.last_landmark_timing() == us
    alive = np.array(sorted(ref.mapPoints), np.int32)
    rng = np.random.default_rng(8)
    desc = np.array([Lm.flip(rng, pool[i % 257], 10) for i in range(len(alive))], np.uint8)
    pose = np.linalg.inv(np.vstack([np.hstack([sc["Rcw"], sc["tcw"].reshape(3, 1)]), [0, 0, 0, 1]]))
    view = mc.lmap_view(sc["Rcw"], sc["tcw"], [np.eye(3)], [np.zeros(3)], [sc["K"][0]], [pose[:3, 3]], 640, 480)
    res = []
    for lm, db in ((lm_d, db_d), (lm_h, db_h)):
        lm.set(alive, desc=desc, mono=np.ones(len(alive), np.uint8))
        res.append(lm.search(view, alive, alive[:5], db, 0, *free(257), levelsup=K.LEVELSUP))
    same_result(res[0], res[1])
    assert len(res[0].new_lids) > 20 and len(res[0].ind1) > 0
