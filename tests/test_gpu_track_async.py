"""The submit / wait pair of fast tracking on a device store (LocalMap.track_submit, track_rig_frame_submit, track_wait): the
submission returns with every kernel on the store's stream -- the de-duplication included -- and the wait hands out what the
synchronous call gives, bit for bit; that in turn equals the host-only store's answer and the restatement (track_ref.py).  While a
call is pending the store refuses everything but the timing getters.

On the commit before the pair existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_track_async.py`):
LocalMap has no track_submit and no track_wait."""
import numpy as np
import pytest

import kfdb_cases as K
import track_cases as T
import track_dedup_cases as D
import track_ref as R
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


@pytest.fixture(scope="module")
def seeded(mc):
    """the seeded 4-camera scene and its restatement, computed once"""
    v, store, kps, descs, lids = T.scene(4)
    assert D.ordinary(kps)                                                    # the restatement can convert every coordinate
    ref = R.track(v, store, [a.tolist() for a in kps], descs, lids)
    assert ref["stats"]["replaced"] > 0 and ref["stats"]["rejected"] > 0
    return v, store, kps, descs, lids, T.ref_lists(ref, store)


def extracted(mc, C, W, H, F, nfeatures):
    rig = mc.Rig(C, W, H, F, 1, nfeatures=nfeatures)
    rig.upload(frames(mc, F, C, W, H))
    rig.extract(F * C)
    return rig


def test_host_arrays(mc, vocs, seeded):
    v, store, kps, descs, lids, want = seeded
    view = T.to_view(mc, v)
    for lm in stores(mc, vocs, store):
        sync = lm.track(view, kps, descs, lids)
        assert lm.track_submit(view, kps, descs, lids) is None
        got = lm.track_wait()
        T.same(T.as_lists(got), want, "submit + wait against the restatement")
        T.same(T.as_lists(got), T.as_lists(sync), "submit + wait against the synchronous call")
        assert got.n_candidates == sync.n_candidates == len(store)


@pytest.mark.parametrize("F,frame", [(3, 1), (1, 0)], ids=["frame 1 of 3", "one-frame small batch"])
def test_rig_slot(mc, vocs, F, frame):
    """a 4-camera 320 x 240 rig with the twins of track_rig_cases: frame 1 of a 3-frame job (a non-zero image base), and a
    one-frame job, whose selection words may live in host-mapped memory"""
    C, W, H = 4, 320, 240
    rig = extracted(mc, C, W, H, F, 300)
    recs, xy, ds = S.slot_frame(rig, frame)
    store, lids = S.landmarks(np.random.default_rng(20 + F), [(recs, xy, ds)], W, H)
    v = S.view_of(rig)
    assert D.ordinary(xy)
    ref = S.restated(v, store, xy, ds, lids)
    S.assert_not_vacuous(ref, xy)
    want = T.ref_lists(ref, store)
    view = T.to_view(mc, v)
    for lm in stores(mc, vocs, store):
        sync = lm.track_rig_frame(view, rig, frame, lids)
        lm.track_rig_frame_submit(view, rig, frame, lids)
        got = lm.track_wait()
        T.same(T.as_lists(got), want, "slot entry, submit + wait, against the restatement")
        T.same(T.as_lists(got), T.as_lists(sync), "slot entry, submit + wait, against the synchronous call")
        T.same(T.as_lists(got), T.as_lists(lm.track(view, xy, ds, lids)), "slot entry against the host arrays")
    rig.close()


def test_the_callers_arrays_are_free_after_submit(mc, vocs, seeded):
    v, store, kps, descs, lids, want = seeded
    lm = stores(mc, vocs, store)[0]
    view = T.to_view(mc, v)
    xy = [np.array(a, np.float32) for a in kps]
    ds = [np.array(d, np.uint8) for d in descs]
    ids = np.array(lids, np.int32)
    lm.track_submit(view, xy, ds, ids)
    for a in xy + ds:
        a[...] = 9
    ids[...] = 1
    view.rows = 1
    T.same(T.as_lists(lm.track_wait()), want, "arrays overwritten between submit and wait")


def test_state_rules(mc, vocs, seeded):
    L = mc._lib
    v, store, kps, descs, lids, want = seeded
    lm = stores(mc, vocs, store)[0]
    view = T.to_view(mc, v)
    db = mc.ORBDatabase(vocs[0], device=0, max_entries=2, max_words=600, max_feats=600)
    eye = np.eye(3)
    sview = mc.lmap_view(eye, np.zeros(3), [eye], [np.zeros(3)], [eye], [np.zeros(3)], 640, 480)
    watched = sorted(store)[::40]
    before = T.snapshot(lm, watched)
    some = np.array(watched[:3], np.int32)
    T.expect(mc, L.E_STATE, lambda: lm.track_wait())                          # nothing was submitted
    lm.track_submit(view, kps, descs, lids)
    for what, call in (("a second submission", lambda: lm.track_submit(view, kps, descs, lids)),
                       ("track", lambda: lm.track(view, kps, descs, lids)),
                       ("set", lambda: lm.set(some, np.zeros((3, 3)), np.zeros((3, 3)))),
                       ("update_points", lambda: lm.update_points(some, np.ones((3, 3)), max_diff=1e9)),
                       ("delete", lambda: lm.delete(some)),
                       ("search", lambda: lm.search(sview, some, [], db, 0, [], [], []))):
        with pytest.raises(mc.McorbError) as ei:
            call()
        assert ei.value.code == L.E_STATE, (what, ei.value)
    assert len(lm.last_track_timing5()) == 5                                  # the getters answer while a call is pending
    got = lm.track_wait()
    T.expect(mc, L.E_STATE, lambda: lm.track_wait())                          # the wait cleared it
    T.same(T.as_lists(got), want, "the pending call's result, after the refused calls")
    assert T.snapshot(lm, watched) == before, "the store changed under the refused calls"


def test_a_refused_submit_leaves_nothing_pending(mc, vocs):
    L = mc._lib
    C, W, H, F = 2, 320, 240, 2
    rig = extracted(mc, C, W, H, F, 300)
    store, lids = S.landmarks(np.random.default_rng(31), [S.slot_frame(rig, 1)], W, H)
    view = T.to_view(mc, S.view_of(rig))
    lm = stores(mc, vocs, store)[0]
    bare = len(store)
    lm.set([bare], [[1.0, 2.0, 1.0]], [[0.0, 0.0, 1.0]])                      # a point, no descriptor
    want = T.as_lists(lm.track_rig_frame(view, rig, 1, lids))
    for code, call in ((L.E_STATE, lambda: lm.track_rig_frame_submit(view, rig, 1, lids + [bare])),
                       (L.E_STATE, lambda: lm.track_rig_frame_submit(view, rig, F, lids)),        # a frame beyond the job
                       (L.E_ARG, lambda: lm.track_rig_frame_submit(view, None, 1, lids))):
        T.expect(mc, code, call)
        T.expect(mc, L.E_STATE, lambda: lm.track_wait())
    lm.track_rig_frame_submit(view, rig, 1, lids)
    T.same(T.as_lists(lm.track_wait()), want, "a submission after the refused ones")
    rig.close()


def test_without_points(mc, vocs, seeded):
    v, store, kps, descs, lids, want = seeded
    lm = stores(mc, vocs, store)[0]
    lm.track_submit(T.to_view(mc, v), kps, descs, lids, want_pts=False)
    got = lm.track_wait()
    assert got.match_pt is None
    got.match_pt = [np.array([store[int(l)][0] for l in m], np.float64).reshape(-1, 3) for m in got.match_lid]
    T.same(T.as_lists(got), want, "want_pts=False, the points apart")


def test_destroy_with_a_call_pending(mc, vocs, seeded):
    v, store, kps, descs, lids, want = seeded
    view = T.to_view(mc, v)
    lm = stores(mc, vocs, store)[0]
    lm.track_submit(view, kps, descs, lids)
    lm.close()                                                                # waits for the stream, then frees what the kernels write
    lm = stores(mc, vocs, store)[0]
    T.same(T.as_lists(lm.track(view, kps, descs, lids)), want, "a fresh store")


def test_two_stores_on_one_slot(mc, vocs):
    """two stores with pending calls on frames 0 and 2 of one slot's job, waited for in reverse order: each has its own stream
    and scratch, and both only read the slot"""
    C, W, H, F = 4, 320, 240, 3
    rig = extracted(mc, C, W, H, F, 300)
    view = T.to_view(mc, S.view_of(rig))
    jobs = []
    for frame in (0, 2):
        store, lids = S.landmarks(np.random.default_rng(50 + frame), [S.slot_frame(rig, frame)], W, H)
        dev, host = stores(mc, vocs, store)
        jobs.append((dev, frame, lids, T.as_lists(host.track_rig_frame(view, rig, frame, lids))))
    for dev, frame, lids, _ in jobs:
        dev.track_rig_frame_submit(view, rig, frame, lids)
    for dev, frame, lids, want in reversed(jobs):
        T.same(T.as_lists(dev.track_wait()), want, "frame %d against the host-only store" % frame)
    assert jobs[0][3]["best"] != jobs[1][3]["best"]
    rig.close()
