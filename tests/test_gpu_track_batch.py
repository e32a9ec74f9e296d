"""Fast tracking of all frames of a rig slot's job in one submission (LocalMap.track_rig_frames, track_rig_frames_submit,
track_frames_wait: the seven k_track_* kernels, the frame in the grid's z).  Frame f of a batched call must be, bit for bit,
what track_rig_frame gives for (views[f], frames[f], lids[f]) on the device store, what it gives on a host-only store, and what
the restatement (track_ref.py) gives on the frame read back with Rig.features; the batch on a host-only store must give the same
again.  Floats as raw bytes, every integer and list, no tolerance and no excluded case.  assert_not_vacuous runs on the
restatement alone, per frame, before anything is compared (a frame that a case gives 0 or 1 candidates on purpose has nothing to
be non-vacuous about and is exempt, by name).

On the commit before the batch existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_track_batch.py`):
LocalMap has no track_rig_frames."""
import numpy as np
import pytest

import kfdb_cases as K
import oracle_lib as O
import track_cases as T
import track_rig_cases as S
from test_gpu_live_lf import frames

pytestmark = pytest.mark.gpu

W, H = 320, 240
NFEATURES_BIG = 2000  # the keypoint extremes: at nfeatures 2000 the synthetic 320 x 240 image gives 1 495 keypoints, more than one tile


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


def extracted(mc, C, w, h, F, nfeatures, images=None):
    rig = mc.Rig(C, w, h, F, 1, nfeatures=nfeatures)
    rig.upload(images if images is not None else frames(mc, F, C, w, h))
    rig.extract(F * C)
    return rig


def shifted(rig, t0=(0.0, 0.0)):
    """the flat view of track_rig_cases moved by a whole-pixel t0: a landmark made from a keypoint projects t0 beside it"""
    return T.view([T.cam() for _ in range(rig.ncams)], rig.w + S.MARGIN[0], rig.h + S.MARGIN[1], t0=(float(t0[0]), float(t0[1]), 0.0))


SHIFTS = [(0, 0), (2, -1), (-1, 2)]


def frame_landmarks(rng, rig, which, **kw):
    """one store with landmarks of their own for every frame of `which` -> (store, the ids per frame)"""
    store, lidss = {}, []
    for f in which:
        st, lids = S.landmarks(rng, [S.slot_frame(rig, f)], rig.w, rig.h, **kw)
        off = len(store)
        store.update({off + l: v for l, v in st.items()})
        lidss.append([l if l < 0 else l + off for l in lids])
    return store, lidss


def check(mc, lms, rig, vs, which, lidss, store, vacuous_ok=(), **kw):
    """a batch against its oracles, frame by frame -> the batch's results on the device store as lists"""
    views = [T.to_view(mc, v) for v in vs]
    refs = []
    for f, (v, frame, lids) in enumerate(zip(vs, which, lidss)):
        recs, xy, ds = S.slot_frame(rig, frame)
        ref = S.restated(v, store, xy, ds, lids, **kw)
        if f not in vacuous_ok:
            S.assert_not_vacuous(ref, xy)
        refs.append(T.ref_lists(ref, store))
    singles = [[lm.track_rig_frame(view, rig, frame, lids, **kw) for view, frame, lids in zip(views, which, lidss)] for lm in lms]
    got = [lm.track_rig_frames(views, rig, which, lidss, **kw) for lm in lms]
    assert all(len(g) == len(which) for g in got)
    first = [T.as_lists(r) for r in got[0]]
    for f in range(len(which)):
        what = "frame %d of the batch (frame %d of the job), device store, against " % (f, which[f])
        T.same(first[f], refs[f], what + "the restatement")
        for r, who in ((singles[0][f], "track_rig_frame on the device store"), (singles[1][f], "track_rig_frame on the host-only store"),
                       (got[1][f], "the batch on the host-only store")):
            T.same(first[f], T.as_lists(r), what + who)
            assert r.n_candidates == got[0][f].n_candidates, what + who
    return first


@pytest.fixture(scope="module")
def job3(mc, vocs):
    """a 4-camera rig with a 3-frame job, a store with landmarks of every frame, the ids per frame, the two stores"""
    rig = extracted(mc, 4, W, H, 3, 300)
    store, lidss = frame_landmarks(np.random.default_rng(101), rig, range(3))
    yield rig, store, lidss, stores(mc, vocs, store)
    rig.close()


def test_three_frames_in_one_call(mc, job3):
    rig, store, lidss, lms = job3
    got = check(mc, lms, rig, [shifted(rig, t) for t in SHIFTS], [0, 1, 2], lidss, store)
    for f in (1, 2):
        assert got[f]["proj"] != got[0]["proj"] and got[f]["best"] != got[0]["best"] and got[f]["matches"] != got[0]["matches"]


def test_frame_order_and_repeats(mc, job3):
    rig, store, lidss, lms = job3
    got = check(mc, lms, rig, [shifted(rig, t) for t in SHIFTS], [2, 0, 2], [lidss[2], lidss[0], lidss[2]], store)
    assert got[0]["proj"] != got[2]["proj"]                                    # frame 2 twice, from two views


def test_frames_are_isolated(mc, vocs):
    """frames 0 and 1 of the job hold the same images and are tracked with one view and one id list: whatever two frames could
    share -- a de-duplication table, a row base, a count -- both answers are the single call's"""
    C = 4
    rig = extracted(mc, C, W, H, 2, 300, images=frames(mc, 1, C, W, H) * 2)
    store, lids = S.landmarks(np.random.default_rng(102), [S.slot_frame(rig, 0)], W, H)
    lms = stores(mc, vocs, store)
    v = shifted(rig)
    single = T.as_lists(lms[0].track_rig_frame(T.to_view(mc, v), rig, 0, lids))
    got = check(mc, lms, rig, [v, v], [0, 1], [lids, lids], store)
    for f in (0, 1):
        for k in ("proj", "best", "matches", "pts"):
            assert got[f][k] == single[k], ("frame %d of two identical frames differs from the single call in %s: a table or a row base "
                                           "shared between the frames loses matches in one of them" % (f, k))
    rig.close()


def test_candidate_counts_257_0_1(mc, vocs):
    """257 candidates are one more than a workgroup of the compaction and the de-duplication; the frame in the middle has none, is
    touched by no kernel and has zero counts; the last has one.  Then every frame without a candidate: nothing is launched"""
    C = 4
    rig = extracted(mc, C, W, H, 3, 300)
    store, lids = S.landmarks(np.random.default_rng(103), [S.slot_frame(rig, 0)], W, H, per_cam=60)
    surplus = len(store) - 257
    assert 0 <= surplus < 60, len(store)                                       # dropped from camera 0's 60 single landmarks
    ids257 = sorted(store)[surplus:]
    one = [ids257[0]]
    lms = stores(mc, vocs, store)
    vs = [shifted(rig)] * 3
    got = check(mc, lms, rig, vs, [0, 1, 2], [ids257 + [-1, ids257[5]], [-1, -1], one], store, vacuous_ok=(1, 2))
    assert [g["n_candidates"] for g in got] == [257, 0, 1]
    assert got[1]["proj"] == [[]] * C and got[1]["matches"] == [[]] * C
    us = lms[0].last_track_timing5()
    assert all(t > 0 for t in us)
    views = [T.to_view(mc, v) for v in vs]
    none = lms[0].track_rig_frames(views, rig, [0, 1, 2], [[-1], [], [-1, -1]])
    assert [r.n_candidates for r in none] == [0, 0, 0] and all(len(p) == 0 for r in none for p in r.proj_lid)
    assert lms[0].last_track_timing5() == us
    rig.close()


def test_last_frame_without_candidates(mc, job3):
    """a 2-frame batch whose second frame has no candidate: the submission's rows end with the first frame's"""
    rig, store, lidss, lms = job3
    got = check(mc, lms, rig, [shifted(rig, t) for t in SHIFTS[:2]], [0, 1], [lidss[0], [-1]], store, vacuous_ok=(1,))
    assert got[0]["n_candidates"] > 0 and got[1]["n_candidates"] == 0 and got[1]["proj"] == [[]] * 4 and got[1]["matches"] == [[]] * 4


def test_keypoint_extremes(mc, vocs):
    """a 2-frame job whose first frame has a camera without keypoints (an all-zero image), one with a handful (a blank image with
    one patch) and one with more than one LDS tile of k_track_match; a landmark's match is a keypoint of the second tile"""
    C, w, h = 3, W, H
    full = mc.synth_rig_frame(0, 4, 0, w, h)
    patch = np.zeros((h, w), np.uint8)
    patch[h // 2:h // 2 + 12, w // 2:w // 2 + 12] = 255
    second = []                                                                # ordinary cameras: a part of an image each
    for img in frames(mc, 1, C, w, h, f0=1):
        part = np.zeros((h, w), np.uint8)
        part[60:180, 80:240] = img[60:180, 80:240]
        second.append(part)
    rig = extracted(mc, C, w, h, 2, NFEATURES_BIG, images=[np.zeros((h, w), np.uint8), patch, full] + second)
    recs, xy, ds = S.slot_frame(rig, 0)                                        # (asserts nsel < kcap for every image)
    second_n = [len(a) for a in S.slot_frame(rig, 1)[1]]
    assert all(n > 9 for n in second_n), second_n
    assert len(xy[0]) == 0 and 1 <= len(xy[1]) <= 9 and len(xy[2]) > mc._lib.TRACK_TILE, [len(a) for a in xy]
    rng = np.random.default_rng(104)
    store, lidss = frame_landmarks(rng, rig, [0, 1], per_cam=10)
    paired = {k for p in S.same_pixel_pairs(recs[2]) for k in p}
    far = next(k for k in range(len(xy[2]) - 1, mc._lib.TRACK_TILE - 1, -1) if k not in paired)
    lid = len(store)
    store[lid] = ((float(xy[2][far][0]), float(xy[2][far][1]), 1.0), ds[2][far])
    lidss[0] = lidss[0] + [lid]
    got = check(mc, stores(mc, vocs, store), rig, [shifted(rig), shifted(rig, (2, 1))], [0, 1], lidss, store)
    at = [l for l, _, _ in got[0]["proj"][2]].index(lid)
    assert far >= mc._lib.TRACK_TILE and got[0]["best"][2][at] == (far, 0)
    assert got[0]["best"][0] == [(-1, 10000)] * len(got[0]["proj"][0]) and got[0]["matches"][0] == []
    rig.close()


@pytest.mark.parametrize("C", [1, 4])
def test_small_batch(mc, vocs, C):
    """a one-frame job is a small batch, whose selection words may live in host-mapped memory, which k_track_points reads
    there; a match job that follows points the slot's control view at the device mirror, which such a batch never filled (a rig
    of one camera has no pair to match)"""
    rig = extracted(mc, C, W, H, 1, 300)
    store, lids = S.landmarks(np.random.default_rng(105 + C), [S.slot_frame(rig, 0)], W, H)
    lms = stores(mc, vocs, store)
    first = check(mc, lms, rig, [shifted(rig)], [0], [lids], store)
    if C > 1:
        rig.match(1)
        assert check(mc, lms, rig, [shifted(rig)], [0], [lids], store) == first
    rig.close()


def test_frame_cap(mc, job3):
    rig, store, lidss, lms = job3
    L = mc._lib
    nf = L.TRACK_MAX_FRAMES
    assert nf == 32
    vs = [shifted(rig, SHIFTS[f % 3]) for f in range(nf + 1)]
    which = [f % 3 for f in range(nf + 1)]
    few = [[l for l in lidss[f % 3] if l >= 0][f:f + 12] + [-1] for f in range(nf + 1)]
    check(mc, lms, rig, vs[:nf], which[:nf], few[:nf], store, vacuous_ok=range(nf))
    views = [T.to_view(mc, v) for v in vs]
    for lm in lms:
        err = T.expect(mc, L.E_ARG, lambda: lm.track_rig_frames(views, rig, which, few))
        assert len(err.n_candidates) == nf + 1 and no_counts(err)
        T.expect(mc, L.E_ARG, lambda: lm.track_rig_frames_submit(views, rig, which, few))
        T.expect(mc, L.E_STATE, lambda: lm.track_frames_wait())


def test_sees_the_store_as_it_is(mc, vocs):
    """points moved by update_points and descriptors written by set_desc_from_entry just before the call are seen by every frame"""
    C = 4
    rig = extracted(mc, C, W, H, 3, 300)
    rng = np.random.default_rng(106)
    store, lidss = frame_landmarks(rng, rig, range(3))
    lms = stores(mc, vocs, store)
    vs = [shifted(rig, t) for t in SHIFTS]
    first = check(mc, lms, rig, vs, [0, 1, 2], lidss, store)
    n = len(store)
    allk = np.concatenate([d for f in range(3) for d in S.slot_frame(rig, f)[2]])
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
    second = check(mc, lms, rig, vs, [0, 1, 2], lidss, store2, vacuous_ok=range(3))
    for f in range(3):
        assert second[f]["proj"] != first[f]["proj"] and second[f]["best"] != first[f]["best"]
    rig.close()


def no_counts(err):
    return not any(err.n_candidates) and not any(any(p) for p in err.n_proj) and not any(any(p) for p in err.n_match)


def test_refusals_leave_the_store_alone(mc, vocs):
    L = mc._lib
    C, F = 2, 3
    rig = extracted(mc, C, W, H, F, 300)
    store, lidss = frame_landmarks(np.random.default_rng(107), rig, range(F))
    bare = len(store)
    vs = [shifted(rig, t) for t in SHIFTS]
    views = [T.to_view(mc, v) for v in vs]
    other = T.to_view(mc, T.flat_view(ncams=C + 1))
    lms = stores(mc, vocs, store)
    small = stores(mc, vocs, store, max_candidates=max(len(set(l) - {-1}) for l in lidss) - 1)
    for lm, tight in zip(lms + small, (False, False, True, True)):
        lm.set([bare], [[1.0, 2.0, 1.0]], [[0.0, 0.0, 1.0]])                  # a point, no descriptor
        watched = sorted(store)[::7] + [bare]
        before = T.snapshot(lm, watched)
        if tight:                                                             # one frame has one candidate too many
            cases = [(L.E_CAP, views, [0, 1, 2], lidss)]
        else:
            cases = [(L.E_STATE, views, [0, 1, F], lidss),                    # a frame beyond the job as the last of three
                     (L.E_STATE, views, [0, -1, 2], lidss),                   # a negative frame
                     (L.E_STATE, views, [0, 1, 2], [lidss[0], lidss[1] + [bare], lidss[2]]),   # no descriptor, the middle frame only
                     (L.E_ARG, [views[0], other, views[2]], [0, 1, 2], lidss),                 # a view of another camera count
                     (L.E_ARG, [], [], [])]                                   # nf = 0
        for code, vw, which, ids in cases:
            err = T.expect(mc, code, lambda: lm.track_rig_frames(vw, rig, which, ids))
            assert len(err.n_candidates) == len(which) and no_counts(err), (code, which)
            T.expect(mc, L.E_STATE, lambda: lm.track_frames_wait())
            T.expect(mc, code, lambda: lm.track_rig_frames_submit(vw, rig, which, ids))
            T.expect(mc, L.E_STATE, lambda: lm.track_frames_wait())
        if not tight:                                                         # a decreasing lid_first, through the C entry
            va = (L.TrackView * 3)(*views)
            fa = np.arange(3, dtype=np.int32)
            la = np.array([l for l in lidss[0] if l >= 0][:9], np.int32)
            firsts = np.array([0, 6, 3, 9], np.int32)
            outs = (L.TrackOut * 3)()
            for o in outs:
                o.n_candidates, o.n_proj[0], o.n_match[1] = 7, 7, 7
            code = lm.L.mcorb_lmap_track_rig_frames(lm.h, va, rig.h_rig, 0, fa.ctypes.data, 3, la.ctypes.data, firsts.ctypes.data,
                                                    10000.0, 20, 0, outs)
            assert code == L.E_ARG
            assert all(o.n_candidates == 0 and not any(o.n_proj) and not any(o.n_match) for o in outs)
            assert lm.L.mcorb_lmap_track_rig_frames_submit(lm.h, va, rig.h_rig, 0, fa.ctypes.data, 3, la.ctypes.data,
                                                           firsts.ctypes.data, 10000.0, 20, 0) == L.E_ARG
            T.expect(mc, L.E_STATE, lambda: lm.track_frames_wait())
        assert T.snapshot(lm, watched) == before
    # the frames together may have more candidates than max_candidates: each of these has fewer
    cut = [[l for l in ids if l >= 0][:20] for ids in lidss]
    roomy = stores(mc, vocs, store, max_candidates=25)
    assert sum(len(set(c)) for c in cut) > 25
    check(mc, roomy, rig, vs, [0, 1, 2], cut, store, vacuous_ok=range(3))
    rig.close()


def test_short_caps(mc, job3):
    """caps too short for one camera of one frame: MCORB_E_CAP, every frame's counts set, no array written"""
    rig, store, lidss, lms = job3
    L = mc._lib
    views = [T.to_view(mc, shifted(rig, t)) for t in SHIFTS]
    for lm in lms:
        full = lm.track_rig_frames(views, rig, [0, 1, 2], lidss)
        n_proj, n_match = [[len(a) for a in r.proj_lid] for r in full], [[len(a) for a in r.match_kp] for r in full]
        top_p, top_m = max(max(p) for p in n_proj), max(max(m) for m in n_match)
        assert min(min(m) for m in n_match) < top_m                            # (top_p, top_m - 1) is short for some cameras only
        for caps in ((top_p - 1, top_m), (top_p, top_m - 1), (0, 0)):
            err = T.expect(mc, L.E_CAP, lambda: lm.track_rig_frames(views, rig, [0, 1, 2], lidss, caps=caps))
            assert (err.n_candidates, err.n_proj, err.n_match) == ([r.n_candidates for r in full], n_proj, n_match)
            assert all(not a.any() for r in err.outputs for a in r.values()), "an output array was written"
            lm.track_rig_frames_submit(views, rig, [0, 1, 2], lidss)
            err = T.expect(mc, L.E_CAP, lambda: lm.track_frames_wait(caps=caps))
            assert (err.n_candidates, err.n_proj, err.n_match) == ([r.n_candidates for r in full], n_proj, n_match)
            assert all(not a.any() for r in err.outputs for a in r.values()), "an output array was written"
            T.expect(mc, L.E_STATE, lambda: lm.track_frames_wait())
        again = lm.track_rig_frames(views, rig, [0, 1, 2], lidss, caps=(top_p, top_m))
        assert [T.as_lists(r) for r in again] == [T.as_lists(r) for r in full]


def test_the_pair(mc, vocs, job3):
    rig, store, lidss, lms = job3
    L = mc._lib
    views = [T.to_view(mc, shifted(rig, t)) for t in SHIFTS]
    db = mc.ORBDatabase(vocs[0], device=0, max_entries=2, max_words=600, max_feats=600)
    eye = np.eye(3)
    sview = mc.lmap_view(eye, np.zeros(3), [eye], [np.zeros(3)], [eye], [np.zeros(3)], 640, 480)
    some = np.array(sorted(store)[:3], np.int32)
    for lm in lms:
        want = [T.as_lists(r) for r in lm.track_rig_frames(views, rig, [0, 1, 2], lidss)]
        # the caller's arrays are free after the submission
        mine = [T.to_view(mc, shifted(rig, t)) for t in SHIFTS]
        ids = [np.array(l, np.int32) for l in lidss]
        which = np.array([0, 1, 2], np.int32)
        assert lm.track_rig_frames_submit(mine, rig, which, ids) is None
        for v in mine:
            v.rows = 1
        for a in ids:
            a[...] = 1
        which[...] = 0
        assert [T.as_lists(r) for r in lm.track_frames_wait()] == want
        T.expect(mc, L.E_STATE, lambda: lm.track_frames_wait())               # the wait cleared it
        # while pending
        before = T.snapshot(lm, some)
        lm.track_rig_frames_submit(views, rig, [0, 1, 2], lidss)
        xy, ds = S.slot_frame(rig, 0)[1:]
        for what, call in (("a second batch", lambda: lm.track_rig_frames_submit(views, rig, [0, 1, 2], lidss)),
                           ("a synchronous batch", lambda: lm.track_rig_frames(views, rig, [0, 1, 2], lidss)),
                           ("track_submit", lambda: lm.track_submit(views[0], xy, ds, lidss[0])),
                           ("track", lambda: lm.track(views[0], xy, ds, lidss[0])),
                           ("update_points", lambda: lm.update_points(some, np.ones((3, 3)), max_diff=1e9))) + \
                ((("search", lambda: lm.search(sview, some, [], db, 0, [], [], [])),) if lm is lms[0] else ()):
            with pytest.raises(mc.McorbError) as ei:
                call()
            assert ei.value.code == L.E_STATE, (what, ei.value)
        assert len(lm.last_track_timing5()) == 5
        assert [T.as_lists(r) for r in lm.track_frames_wait()] == want
        assert T.snapshot(lm, some) == before
        # track_wait serves no batch of more than one frame, and leaves nothing pending
        lm.track_rig_frames_submit(views, rig, [0, 1, 2], lidss)
        T.expect(mc, L.E_STATE, lambda: lm.track_wait())
        T.expect(mc, L.E_STATE, lambda: lm.track_frames_wait())
        T.expect(mc, L.E_STATE, lambda: lm.track_wait())
        # a single submission is a batch of one
        lm.track_rig_frame_submit(views[1], rig, 1, lidss[1])
        one = lm.track_frames_wait()
        lm.track_rig_frame_submit(views[1], rig, 1, lidss[1])
        assert len(one) == 1 and T.as_lists(one[0]) == T.as_lists(lm.track_wait()) == want[1]
        # and a batch of one frame is served by track_wait
        lm.track_rig_frames_submit(views[2:], rig, [2], lidss[2:])
        assert T.as_lists(lm.track_wait()) == want[2]
        # without the points
        lm.track_rig_frames_submit(views, rig, [0, 1, 2], lidss, want_pts=False)
        got = lm.track_frames_wait()
        assert all(r.match_pt is None for r in got)
        for r in got:
            r.match_pt = [np.array([store[int(l)][0] for l in m], np.float64).reshape(-1, 3) for m in r.match_lid]
        assert [T.as_lists(r) for r in got] == want


def test_destroy_with_a_batch_pending(mc, vocs, job3):
    rig, store, lidss, _ = job3
    views = [T.to_view(mc, shifted(rig, t)) for t in SHIFTS]
    lm, host = stores(mc, vocs, store)
    want = [T.as_lists(r) for r in host.track_rig_frames(views, rig, [0, 1, 2], lidss)]
    lm.track_rig_frames_submit(views, rig, [0, 1, 2], lidss)
    lm.close()                                                                # waits for the stream, then frees what the kernels write
    lm = stores(mc, vocs, store)[0]
    assert [T.as_lists(r) for r in lm.track_rig_frames(views, rig, [0, 1, 2], lidss)] == want


def test_timing(mc, vocs, job3):
    rig, store, lidss, _ = job3
    views = [T.to_view(mc, shifted(rig, t)) for t in SHIFTS]
    lm = stores(mc, vocs, store)[0]
    assert lm.last_track_timing5() == (0.0, 0.0, 0.0, 0.0, 0.0)
    lm.track_rig_frames(views, rig, [0, 1, 2], lidss)
    us = lm.last_track_timing5()
    assert all(t > 0 for t in us) and us[:4] == lm.last_track_timing4() and us[1:3] == lm.last_track_timing()
