"""The submit / wait pair of fast tracking and the pixel of a keypoint where no GPU is needed: on a host-only store (device -1)
LocalMap.track_submit runs the serial path to its end and keeps the result, LocalMap.track_wait hands it out -- equal, bit for
bit, to LocalMap.track and to the restatement (track_ref.py) -- and the state rules hold as on a device store.  The conversion
of a keypoint coordinate to its pixel, which the host tail and k_track_dedup_min share, at the values where (int) of a float is
not defined.

On the commit before the pair existed every test of this file fails (`python -m pytest tests/test_track_async_cpu.py`):
LocalMap has no track_submit, track_wait or last_track_timing5 and the library has no mcorb_host_track_pixel."""
import numpy as np
import pytest

import kfdb_cases as K
import track_cases as T
import track_dedup_cases as D
import track_ref as R

INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def store_of(mc, voc, store, max_landmarks=1024, max_candidates=1024):
    lm = mc.LocalMap(voc, device=-1, max_landmarks=max_landmarks, max_candidates=max_candidates)
    T.fill(lm, store)
    return lm


def seeded(mc):
    v, store, kps, descs, lids = T.scene(2, seed=3, n_landmarks=90, n_twins=60)
    return v, T.to_view(mc, v), store, kps, descs, lids


def test_the_pixel_of_a_coordinate(mc):
    """truncation toward zero below 2^31 in magnitude, INT32_MIN from there on and for a NaN"""
    px = mc._lib.load().mcorb_host_track_pixel
    big = float(np.nextafter(np.float32(2.0 ** 31), np.float32(0)))           # 2^31 - 128, the greatest float below 2^31
    assert big == 2.0 ** 31 - 128
    for v, want in ((-0.5, 0), (0.5, 0), (-1.0, -1), (-1.5, -1), (10.9, 10), (big, 2 ** 31 - 128), (-big, -(2 ** 31 - 128)),
                    (2.0 ** 31, INT32_MIN), (-2.0 ** 31, INT32_MIN), (3e9, INT32_MIN), (-3e9, INT32_MIN), (float("nan"), INT32_MIN),
                    (float("inf"), INT32_MIN), (float("-inf"), INT32_MIN)):
        assert px(v) == want, (v, px(v), want)


def test_pixels_in_the_list(mc, voc):
    """the host-only store's serial list through the shared function: (-0.5, -0.5) and (0.3, 0.2) are one pixel, (-1.0, -1.0) is
    another; keypoints at 3e9, -3e9 and inf are one pixel (INT32_MIN, 7) -- they are reached with max_d2 = inf only -- and a
    keypoint with a NaN coordinate is no neighbour of any query, so it never reaches the list"""
    px = mc._lib.load().mcorb_host_track_pixel
    assert px(-0.5) == px(0.3) == px(0.2) == 0 and px(-1.0) == -1 and px(3e9) == px(-3e9) == px(float("inf")) == INT32_MIN
    kps = [(-0.5, -0.5), (0.3, 0.2), (-1.0, -1.0)]
    store, xy, ds, lids = D.scene(kps, [(0, 5, (0.0, 0.0)), (1, 3, (0.0, 0.0)), (2, 4, (0.0, 0.0)), (2, 4, (0.0, 0.0)), (2, 6, (0.0, 0.0))])
    got, ref = T.run(mc, store_of(mc, voc, store), T.flat_view(), store, [xy], [ds], lids)
    assert got["best"][0] == [(0, 5), (1, 3), (2, 4), (2, 4), (2, 6)] and got["matches"][0] == [(1, 1, 3), (2, 2, 4)]
    assert (ref["stats"]["replaced"], ref["stats"]["rejected"]) == (1, 2)

    nan = float("nan")
    kps = [(3e9, 7.2), (-3e9, 7.9), (float("inf"), 7.5), (nan, 7.0), (12.0, nan), (50.0, 7.0)]
    at = (10.0, 7.0)
    store, xy, ds, lids = D.scene(kps, [(0, 5, at), (1, 3, at), (2, 3, at), (3, 0, at), (4, 0, at), (5, 2, at)])
    assert not D.ordinary([xy])
    lm = store_of(mc, voc, store)
    res = T.as_lists(lm.track(T.to_view(mc, T.flat_view()), [xy], [ds], lids, max_d2=float("inf")))
    assert res["best"][0] == [(0, 5), (1, 3), (2, 3), (-1, 10000), (-1, 10000), (5, 2)]
    assert res["matches"][0] == [(1, 1, 3), (5, 5, 2)]
    res = T.as_lists(lm.track(T.to_view(mc, T.flat_view()), [xy], [ds], lids))   # the default radius reaches keypoint 5 alone
    assert res["matches"][0] == [(5, 5, 2)]


def test_submit_then_wait_is_track(mc, voc):
    v, view, store, kps, descs, lids = seeded(mc)
    lm = store_of(mc, voc, store)
    want = T.as_lists(lm.track(view, kps, descs, lids))
    ref = R.track(v, store, [a.tolist() for a in kps], descs, lids)
    T.same(want, T.ref_lists(ref, store), "track against the restatement")
    assert ref["stats"]["replaced"] > 0 and ref["stats"]["rejected"] > 0
    assert lm.track_submit(view, kps, descs, lids) is None
    got = lm.track_wait()
    T.same(T.as_lists(got), want, "submit + wait against track")
    assert got.n_candidates == want["n_candidates"]
    assert lm.last_track_timing5() == (0.0, 0.0, 0.0, 0.0, 0.0)


def test_the_callers_arrays_are_free_after_submit(mc, voc):
    v, view, store, kps, descs, lids = seeded(mc)
    lm = store_of(mc, voc, store)
    want = T.as_lists(lm.track(view, kps, descs, lids))
    xy = [np.array(a, np.float32) for a in kps]
    ds = [np.array(d, np.uint8) for d in descs]
    ids = np.array(lids, np.int32)
    lm.track_submit(view, xy, ds, ids)
    for a in xy + ds:
        a[...] = 7
    ids[...] = 0
    view.cols = 1
    T.same(T.as_lists(lm.track_wait()), want, "overwritten arrays")


def test_state_rules(mc, voc):
    L = mc._lib
    v, view, store, kps, descs, lids = seeded(mc)
    lm = store_of(mc, voc, store)
    watched = sorted(store)[::9]
    before = T.snapshot(lm, watched)
    T.expect(mc, L.E_STATE, lambda: lm.track_wait())                          # nothing was submitted
    lm.track_submit(view, kps, descs, lids)
    some = np.array(watched[:3], np.int32)
    for call in (lambda: lm.track_submit(view, kps, descs, lids),
                 lambda: lm.track(view, kps, descs, lids),
                 lambda: lm.track_rig_frame(view, None, 0, lids),
                 lambda: lm.set(some, np.zeros((3, 3)), np.zeros((3, 3))),
                 lambda: lm.update_points(some, np.ones((3, 3)), max_diff=1e9),
                 lambda: lm.delete(some),
                 lambda: lm.get(int(some[0]))):
        T.expect(mc, L.E_STATE, call)
    assert lm.last_track_timing4() == (0.0, 0.0, 0.0, 0.0)                    # the getters answer while a call is pending
    got = lm.track_wait()
    T.expect(mc, L.E_STATE, lambda: lm.track_wait())                          # the wait cleared it
    assert T.snapshot(lm, watched) == before
    T.same(T.as_lists(got), T.as_lists(lm.track(view, kps, descs, lids)), "the pending call's result")


def test_a_refused_submit_leaves_nothing_pending(mc, voc):
    L = mc._lib
    v, view, store, kps, descs, lids = seeded(mc)
    lm = store_of(mc, voc, store)
    bare = len(store)
    lm.set([bare], [[1.0, 2.0, 1.0]], [[0.0, 0.0, 1.0]])                      # a point, no descriptor
    small = store_of(mc, voc, store, max_candidates=8)
    for who, code, call in ((lm, L.E_STATE, lambda: lm.track_submit(view, kps, descs, lids + [bare])),
                            (lm, L.E_ARG, lambda: lm.track_submit(view, kps, descs, lids + [5000])),
                            (lm, L.E_ARG, lambda: lm.track_submit(view, kps, descs, lids, max_hamming=-1)),
                            (lm, L.E_ARG, lambda: lm.track_rig_frame_submit(view, None, 0, lids)),
                            (small, L.E_CAP, lambda: small.track_submit(view, kps, descs, lids))):
        T.expect(mc, code, call)
        T.expect(mc, L.E_STATE, lambda: who.track_wait())
    assert lm.track(view, kps, descs, lids).n_candidates == len(store)


def test_wait_outputs(mc, voc):
    """want_pts=False gives no match_pt; a call without candidates is pending and its wait gives zero counts; short caps are
    MCORB_E_CAP with every count set, and the wait that failed left nothing pending"""
    L = mc._lib
    v, view, store, kps, descs, lids = seeded(mc)
    lm = store_of(mc, voc, store)
    full = lm.track(view, kps, descs, lids)
    lm.track_submit(view, kps, descs, lids, want_pts=False)
    got = lm.track_wait()
    assert got.match_pt is None
    assert [a.tolist() for a in got.match_lid] == [a.tolist() for a in full.match_lid]
    lm.track_submit(view, kps, descs, [-1, -1])
    T.expect(mc, L.E_STATE, lambda: lm.get(0))
    got = lm.track_wait()
    assert got.n_candidates == 0 and all(len(a) == 0 for a in got.proj_lid + got.match_kp)
    n_proj, n_match = [len(a) for a in full.proj_lid], [len(a) for a in full.match_kp]
    assert min(n_match) > 1
    for caps in ((max(n_proj) - 1, max(n_match)), (max(n_proj), max(n_match) - 1), (0, 0)):
        lm.track_submit(view, kps, descs, lids)
        err = T.expect(mc, L.E_CAP, lambda: lm.track_wait(caps=caps))
        assert (err.n_candidates, err.n_proj, err.n_match) == (full.n_candidates, n_proj, n_match)
        T.expect(mc, L.E_STATE, lambda: lm.track_wait())
    lm.track_submit(view, kps, descs, lids)
    T.same(T.as_lists(lm.track_wait(caps=(max(n_proj), max(n_match)))), T.as_lists(full), "exact caps")


def test_destroy_with_a_call_pending(mc, voc):
    v, view, store, kps, descs, lids = seeded(mc)
    lm = store_of(mc, voc, store)
    lm.track_submit(view, kps, descs, lids)
    lm.close()
    lm = store_of(mc, voc, store)
    assert lm.track(view, kps, descs, lids).n_candidates == len(store)
