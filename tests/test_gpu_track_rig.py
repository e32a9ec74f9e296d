"""Fast tracking on a frame of a rig slot (LocalMap.track_rig_frame: k_track_points, k_track_project, k_track_match with the slot's
descriptors in HBM, k_track_compact) against the same frame read back with Rig.features and handed to LocalMap.track on the device
store, to LocalMap.track on the host-only store and to the restatement (track_ref.py); track_rig_frame on a host-only store must
give the same again.  Bit for bit: floats as raw bytes, every integer and list, no tolerance and no excluded case.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_track_rig.py`):
LocalMap has no track_rig_frame."""
import numpy as np
import pytest

import kfdb_cases as K
import oracle_lib as O
import track_cases as T
import track_rig_cases as S
from test_gpu_live_lf import frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def stores(mc, vocs, store, max_landmarks=4096, max_candidates=1024):
    out = [mc.LocalMap(voc, device=dev, max_landmarks=max_landmarks, max_candidates=max_candidates) for voc, dev in zip(vocs, (0, -1))]
    for lm in out:
        T.fill(lm, store)
    return out


def check(mc, lms, rig, frame, store, lids, slot=0, vacuous_ok=False, **kw):
    """the five answers of one frame -> (track_rig_frame's on the device store as lists, the restatement, the frame's arrays)"""
    recs, xy, ds = S.slot_frame(rig, frame, slot)
    v = S.view_of(rig)
    ref = S.restated(v, store, xy, ds, lids, **kw)
    if not vacuous_ok:
        S.assert_not_vacuous(ref, xy)
    view = T.to_view(mc, v)
    want = [lm.track(view, xy, ds, lids, **kw) for lm in lms]
    got = [lm.track_rig_frame(view, rig, frame, lids, slot=slot, **kw) for lm in lms]
    first = T.as_lists(got[0])
    T.same(first, T.ref_lists(ref, store), "slot entry, device store, against the restatement")
    for r, what in ((want[0], "track on the device store"), (want[1], "track on the host-only store"),
                    (got[1], "the slot entry on the host-only store")):
        T.same(first, T.as_lists(r), "slot entry, device store, against " + what)
        assert r.n_candidates == got[0].n_candidates
    return first, ref, (recs, xy, ds)


def extracted(mc, C, W, H, F, nfeatures, images=None, **kw):
    rig = mc.Rig(C, W, H, F, 1, nfeatures=nfeatures, **kw)
    rig.upload(images if images is not None else frames(mc, F, C, W, H))
    rig.extract(F * C)
    return rig


def test_frames_and_image_bases(mc, vocs):
    """three frames in one job: frames 1 and 2 read the slot's rows from a non-zero image base.  One store, built from the
    keypoints of all three, so the answers differ by the frame alone"""
    C, W, H, F = 4, 320, 240, 3
    rig = extracted(mc, C, W, H, F, 300)
    rng = np.random.default_rng(1)
    store, lids = S.landmarks(rng, [S.slot_frame(rig, f) for f in range(F)], W, H)
    lms = stores(mc, vocs, store)
    got = [check(mc, lms, rig, f, store, lids)[0] for f in range(F)]
    for f in (1, 2):
        assert got[f]["best"] != got[0]["best"] and got[f]["matches"] != got[0]["matches"]
    rig.close()


@pytest.mark.parametrize("C", [1, 4])
def test_one_frame_job(mc, vocs, C):
    """a one-frame job is a small batch, whose selection words may live in host-mapped memory; and a rig of one camera"""
    W, H = 320, 240
    rig = extracted(mc, C, W, H, 1, 300)
    rng = np.random.default_rng(2 + C)
    store, lids = S.landmarks(rng, [S.slot_frame(rig, 0)], W, H)
    check(mc, stores(mc, vocs, store), rig, 0, store, lids)
    rig.close()


@pytest.mark.parametrize("selection,graph", [(1, 0), (2, 0), (2, 1)], ids=["host", "gpu", "gpu-graph"])
def test_every_selection_path(mc, vocs, selection, graph):
    """the selection on the host and in k_select leave the slot's words in different places (the control block's host side, its
    device mirror), a small batch and one with result copies do, and so does a job replayed from its graph; a match job that
    follows the extraction points the slot's control view at the device mirror, which a small host-selected batch never filled"""
    C, W, H = 2, 320, 240
    for F in (1, 5):
        rig = mc.Rig(C, W, H, F, 1, nfeatures=300, selection=selection)
        rig.set_graph(graph)
        for f0 in (3, 0):                                                     # the second job is the replay
            rig.upload(frames(mc, F, C, W, H, f0=f0))
            rig.extract(F * C)
        rng = np.random.default_rng(40 + F)
        store, lids = S.landmarks(rng, [S.slot_frame(rig, F - 1)], W, H)
        lms = stores(mc, vocs, store)
        first = check(mc, lms, rig, F - 1, store, lids)[0]
        rig.match(F)
        assert check(mc, lms, rig, F - 1, store, lids)[0] == first
        rig.close()


def test_counts_per_camera(mc, vocs):
    """one frame whose cameras have 0 keypoints (an all-zero image), a handful (a blank image with one small patch), an ordinary
    number, and more than one LDS tile of k_track_match; the best match of one landmark is a keypoint of index >= 1024"""
    C, W, H = 4, 640, 480
    full = mc.synth_rig_frame(0, C, 0, W, H)
    patch = np.zeros((H, W), np.uint8)
    patch[H // 2:H // 2 + 12, W // 2:W // 2 + 12] = 255
    part = np.zeros((H, W), np.uint8)
    part[100:260, 200:400] = full[100:260, 200:400]
    rig = extracted(mc, C, W, H, 1, 2000, images=[np.zeros((H, W), np.uint8), patch, part, full])
    recs, xy, ds = S.slot_frame(rig, 0)
    assert len(xy[0]) == 0 and 1 <= len(xy[1]) <= 9 and len(xy[2]) > 9 and len(xy[3]) > mc._lib.TRACK_TILE
    rng = np.random.default_rng(7)
    store, lids = S.landmarks(rng, [(recs, xy, ds)], W, H, per_cam=10)
    paired = {k for p in S.same_pixel_pairs(recs[3]) for k in p}
    far = next(k for k in range(len(xy[3]) - 1, 1023, -1) if k not in paired)
    lid = len(store)
    store[lid] = ((float(xy[3][far][0]), float(xy[3][far][1]), 1.0), ds[3][far])
    lids = lids + [lid]
    got, _, _ = check(mc, stores(mc, vocs, store), rig, 0, store, lids)
    at = [l for l, _, _ in got["proj"][3]].index(lid)
    assert far >= 1024 and got["best"][3][at] == (far, 0)
    assert got["best"][0] == [(-1, 10000)] * len(got["proj"][0]) and got["matches"][0] == []
    rig.close()


def test_sees_the_slot_and_the_store_as_they_are(mc, vocs):
    """nothing of the slot is cached: after an upload and extraction of other images into the slot the call answers for the new
    frame; points moved by update_points and descriptors written by set_desc_from_entry just before the call are seen"""
    C, W, H = 4, 320, 240
    rig = extracted(mc, C, W, H, 1, 300)
    rng = np.random.default_rng(11)
    old = S.slot_frame(rig, 0)
    rig.upload(frames(mc, 1, C, W, H, f0=5))
    rig.extract(C)
    new = S.slot_frame(rig, 0)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(old[1], new[1]))
    store, lids = S.landmarks(rng, [old, new], W, H)
    lms = stores(mc, vocs, store)
    first, _, (recs, xy, ds) = check(mc, lms, rig, 0, store, lids)
    # the store changes under the same slot: a database entry's descriptors become the landmarks', the points move
    n = len(store)
    allk = np.concatenate(ds)
    new_desc = np.array([T.desc_at(allk[int(rng.integers(0, len(allk)))], int(rng.integers(0, 6)), rng) for _ in range(n)], np.uint8)
    moved = np.array([store[i][0] for i in range(n)]) + np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), np.zeros(n)], axis=1)
    feats = rng.permutation(n).astype(np.int32)
    bow, fv = O.bow_transform(K.vocabulary(), new_desc, K.LEVELSUP)
    for lm, voc, dev in zip(lms, vocs, (0, -1)):
        db = mc.ORBDatabase(voc, device=dev, max_entries=2, max_words=600, max_feats=600)
        entry = db.add(bow, fv, new_desc)
        lm.set_desc_from_entry(db, entry, np.arange(n, dtype=np.int32), feats)
        upd, _ = lm.update_points(np.arange(n, dtype=np.int32), moved, max_diff=1e9)
        assert upd.all()
    store2 = {i: (tuple(moved[i].tolist()), new_desc[feats[i]]) for i in range(n)}
    second, _, _ = check(mc, lms, rig, 0, store2, lids, vacuous_ok=True)
    assert second["proj"] != first["proj"] and second["best"] != first["best"]
    rig.close()


def test_errors_leave_the_store_alone(mc, vocs):
    L = mc._lib
    C, W, H, F = 2, 320, 240, 2
    rig = extracted(mc, C, W, H, F, 300)
    rng = np.random.default_rng(13)
    store, lids = S.landmarks(rng, [S.slot_frame(rig, 1)], W, H)
    bare = len(store)
    view = T.to_view(mc, S.view_of(rig))
    for lm in stores(mc, vocs, store):
        lm.set([bare], [[1.0, 2.0, 1.0]], [[0.0, 0.0, 1.0]])                  # a point, no descriptor
        watched = sorted(store)[::7] + [bare]
        before = T.snapshot(lm, watched)
        for code, call in ((L.E_STATE, lambda: lm.track_rig_frame(view, rig, F, lids)),           # a frame beyond the job
                           (L.E_STATE, lambda: lm.track_rig_frame(view, rig, -1, lids)),
                           (L.E_ARG, lambda: lm.track_rig_frame(T.to_view(mc, T.flat_view(ncams=C + 1)), rig, 1, lids)),
                           (L.E_ARG, lambda: lm.track_rig_frame(view, rig, 1, lids, slot=1)),     # the rig has one slot
                           (L.E_ARG, lambda: lm.track_rig_frame(view, None, 1, lids)),
                           (L.E_STATE, lambda: lm.track_rig_frame(view, rig, 1, lids + [bare]))):
            err = T.expect(mc, code, call)
            assert err.n_candidates == 0 and not any(err.n_proj) and not any(err.n_match)
        full = lm.track_rig_frame(view, rig, 1, lids)
        n_proj, n_match = [len(a) for a in full.proj_lid], [len(a) for a in full.match_kp]
        assert min(n_proj) > 1 and min(n_match) > 1
        for caps in ((max(n_proj) - 1, max(n_match)), (max(n_proj), max(n_match) - 1), (0, 0)):
            err = T.expect(mc, L.E_CAP, lambda: lm.track_rig_frame(view, rig, 1, lids, caps=caps))
            assert (err.n_candidates, err.n_proj, err.n_match) == (full.n_candidates, n_proj, n_match)
        assert T.as_lists(lm.track_rig_frame(view, rig, 1, lids, caps=(max(n_proj), max(n_match)))) == T.as_lists(full)
        assert T.snapshot(lm, watched) == before
    rig.close()


def test_timing4(mc, vocs):
    C, W, H = 2, 320, 240
    rig = extracted(mc, C, W, H, 1, 300)
    rng = np.random.default_rng(17)
    recs, xy, ds = S.slot_frame(rig, 0)
    store, lids = S.landmarks(rng, [(recs, xy, ds)], W, H)
    lm = stores(mc, vocs, store)[0]
    view = T.to_view(mc, S.view_of(rig))
    assert lm.last_track_timing4() == (0.0, 0.0, 0.0, 0.0)
    lm.track_rig_frame(view, rig, 0, lids)
    us = lm.last_track_timing4()
    assert all(t > 0 for t in us) and us[1:3] == lm.last_track_timing()
    lm.track_rig_frame(view, rig, 0, [-1, -1])                                # no candidate: nothing is launched
    assert lm.last_track_timing4() == us
    lm.track(view, xy, ds, lids)                                              # the host-array entry runs no k_track_points
    us = lm.last_track_timing4()
    assert us[0] == 0.0 and all(t > 0 for t in us[1:]) and us[1:3] == lm.last_track_timing()
    rig.close()
