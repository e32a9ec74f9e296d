"""The pose refinement behind fast tracking (LocalMap.set_track_refine, last_track_pose): with the option on, every tracking
submission -- track, track_rig_frame, the submit / wait pair, track_rig_frames -- also runs k_pose_refine per frame in the same
submission, on observations the kernel builds from the frame's de-duplicated matches.  The defining property is the oracle: frame
f's result is bit for bit what refine_pose returns on that frame's match_kp -> pt, match_lid and camera arrays -- on the device
store, on the host-only store and in the restatement (pose_ref.py).  The octave is 0: querryEachFrame's bestMatches carry none.

The rig is 320 x 240 with track_rig_cases' landmarks: made from the frame's keypoints, so with the flat view every residual is
exactly zero; the views of frames 1 and 2 are moved by whole pixels (the pose has something to undo) and three landmarks per
frame are moved 6 px beside their keypoint (chi2 = 36 > 5.991: culled).  Both are shown on the restatement alone first.

On the commit before the option existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_track_refine.py`):
LocalMap has no refine_pose and no set_track_refine."""
import numpy as np
import pytest

import kfdb_cases as K
import pose_cases as PC
import pose_ref as P
import track_cases as T
import track_rig_cases as S
from test_gpu_track_batch import SHIFTS, H, W, extracted, frame_landmarks, shifted, stores

pytestmark = pytest.mark.gpu

INV = PC.INV_SIGMA2
MOVED = 3            # landmarks per frame whose point is moved 6 px beside the keypoint it was made from


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture(scope="module")
def job3(mc, vocs):
    """a 4-camera rig with a 3-frame job; a store with landmarks of every frame, three per frame moved; the ids per frame; the
    device store and the host-only store; per frame the view, the frame read back, and the restatement of the tracking call
    and of the refinement"""
    assert hasattr(mc.LocalMap, "set_track_refine")
    rig = extracted(mc, 4, W, H, 3, 300)
    store, lidss = frame_landmarks(np.random.default_rng(131), rig, range(3))
    for lids in lidss:
        first = min(l for l in lids if l >= 0)
        for l in range(first, first + MOVED):
            (x, y, z), d = store[l]
            store[l] = ((x + 6.0, y, z), d)
    lms = stores(mc, vocs, store)
    vs = [shifted(rig, t) for t in SHIFTS]
    frames = [S.slot_frame(rig, f) for f in range(3)]
    tracked = [S.restated(vs[f], store, frames[f][1], frames[f][2], lidss[f]) for f in range(3)]
    refs = [restated_pose(vs[f], store, frames[f][1], tracked[f]["matches"]) for f in range(3)]
    yield dict(rig=rig, store=store, lidss=lidss, lms=lms, vs=vs, frames=frames, tracked=tracked, refs=refs)
    rig.close()


def restated_pose(v, store, xy, matches):
    """the refinement of a frame in the restatement: the observations are the matches, the cameras back to back"""
    obs = [(c, float(xy[c][kp][0]), float(xy[c][kp][1]), 0, [float(x) for x in store[lid][0]]) for c, m in enumerate(matches) for kp, lid, _ in m]
    return P.refine(v["cams"], P.pose_of_view(v["R0"], v["t0"]), obs, INV)


def check_pose(mc, lms, v, xy, res, got, ref, what):
    """got = last_track_pose(f) of a call whose TrackResult is res: equal to refine_pose on res's arrays on both stores, and to
    the restatement"""
    view = T.to_view(mc, v)
    cam = np.concatenate([np.full(len(res.match_kp[c]), c, np.int32) for c in range(len(xy))])
    uv = np.concatenate([xy[c][res.match_kp[c]].reshape(-1, 2) for c in range(len(xy))]).astype(np.float32)
    lids = np.concatenate(res.match_lid).astype(np.int32)
    R0, t0 = mc.pose_of_view(view)
    PC.same(PC.as_ref(got), ref, what + " against the restatement")
    for lm, who in zip(lms, ("device store", "host-only store")):
        want = lm.refine_pose(view, R0, t0, cam, uv, np.zeros(len(cam), np.int32), INV, lids=lids)
        PC.same(PC.as_ref(got), PC.as_ref(want), what + " against refine_pose on the %s" % who)
    assert got.n_obs == len(cam)


def test_restatement_is_not_vacuous(job3):
    """first on the restatement alone: every frame has a culled observation and frames 1 and 2 move their pose"""
    for f, ref in enumerate(job3["refs"]):
        init = P.pose_of_view(job3["vs"][f]["R0"], job3["vs"][f]["t0"])
        assert sum(len(m) for m in job3["tracked"][f]["matches"]) > 40
        assert MOVED <= len(ref["inliers"]) - ref["n_inliers"] < len(ref["inliers"]) // 2, (f, ref["n_inliers"])
        if f > 0:
            assert ref["status"] == P.CONVERGED and not P.same_bits(ref["t"], init[1]), f
            assert max(abs(a) for a in init[1]) >= 1.0 and max(abs(a) for a in ref["t"]) < 0.01                # (it undoes the shift)


@pytest.mark.parametrize("entry", ["track", "track_rig_frame", "track_submit", "track_rig_frame_submit"])
def test_single_entries(mc, job3, entry):
    """each single entry, synchronous or the pair, on every frame: last_track_pose against its three oracles, and the
    TrackResult equal to the one with the option off"""
    rig, lms = job3["rig"], job3["lms"]
    for f in range(3):
        v, (recs, xy, ds), lids = job3["vs"][f], job3["frames"][f], job3["lidss"][f]
        view = T.to_view(mc, v)
        for lm, who in zip(lms, ("device store", "host-only store")):
            def run():
                if entry == "track":
                    return lm.track(view, xy, ds, lids)
                if entry == "track_rig_frame":
                    return lm.track_rig_frame(view, rig, f, lids)
                if entry == "track_submit":
                    lm.track_submit(view, xy, ds, lids)
                else:
                    lm.track_rig_frame_submit(view, rig, f, lids)
                return lm.track_wait()
            lm.set_track_refine(None)
            off = run()
            lm.set_track_refine(INV)
            on = run()
            got = lm.last_track_pose()
            T.same(T.as_lists(on), T.as_lists(off), "%s, frame %d, %s: the TrackResult with the option on" % (entry, f, who))
            T.same(T.as_lists(on), T.ref_lists(job3["tracked"][f], job3["store"]), "%s, frame %d, %s" % (entry, f, who))
            check_pose(mc, lms, v, xy, on, got, job3["refs"][f], "%s, frame %d, %s:" % (entry, f, who))
            lm.set_track_refine(None)


def test_three_frames_in_one_call(mc, job3):
    rig, lms = job3["rig"], job3["lms"]
    views = [T.to_view(mc, v) for v in job3["vs"]]
    for which in ([0, 1, 2], [2, 0, 2]):
        for lm, who in zip(lms, ("device store", "host-only store")):
            lm.set_track_refine(None)
            off = lm.track_rig_frames([views[f] for f in which], rig, which, [job3["lidss"][f] for f in which])
            lm.set_track_refine(INV)
            on = lm.track_rig_frames([views[f] for f in which], rig, which, [job3["lidss"][f] for f in which])
            for k, f in enumerate(which):
                T.same(T.as_lists(on[k]), T.as_lists(off[k]), "frame %d of %s, %s: the TrackResult with the option on" % (k, which, who))
                check_pose(mc, lms, job3["vs"][f], job3["frames"][f][1], on[k], lm.last_track_pose(k), job3["refs"][f],
                           "frame %d of %s, %s:" % (k, which, who))
            with pytest.raises(mc.McorbError) as e:
                lm.last_track_pose(3)
            assert e.value.code == mc.E_ARG
            # the pair
            lm.track_rig_frames_submit([views[f] for f in which], rig, which, [job3["lidss"][f] for f in which])
            lm.track_frames_wait()
            for k, f in enumerate(which):
                PC.same(PC.as_ref(lm.last_track_pose(k)), job3["refs"][f], "frame %d of %s, %s, the pair" % (k, which, who))
            lm.set_track_refine(None)


def test_frames_without_matches(mc, job3):
    """no candidate at all (nothing is launched), candidates that are all behind the rig, an empty frame in the middle of a
    batch and one at the end of a 2-frame batch (the refinement's rows end with the first frame's): NO_OBS with the view's pose"""
    rig, lms, store = job3["rig"], job3["lms"], job3["store"]
    behind = [l for l, ((x, y, z), d) in store.items() if z < 0]
    assert len(behind) >= 4
    views = [T.to_view(mc, v) for v in job3["vs"]]
    for lm in lms:
        lm.set_track_refine(INV)
        for lids in ([], behind):
            res = lm.track_rig_frame(views[1], rig, 1, lids)
            got = lm.last_track_pose()
            want = P.pose_of_view(job3["vs"][1]["R0"], job3["vs"][1]["t0"])
            assert sum(len(m) for m in res.match_kp) == 0
            assert got.status == P.NO_OBS and got.n_obs == 0 and got.n_inliers == 0 and got.iterations == (0, 0)
            assert P.same_bits(got.R.tolist(), want[0]) and P.same_bits(got.t.tolist(), want[1])
        lm.track_rig_frames(views, rig, [0, 1, 2], [job3["lidss"][0], [], job3["lidss"][2]])
        assert lm.last_track_pose(1).status == P.NO_OBS
        for f in (0, 2):
            PC.same(PC.as_ref(lm.last_track_pose(f)), job3["refs"][f], "frame %d beside an empty one" % f)
        two = lm.track_rig_frames(views[:2], rig, [0, 1], [job3["lidss"][0], [-1]])
        assert two[1].n_candidates == 0 and lm.last_track_pose(1).status == P.NO_OBS
        T.same(T.as_lists(two[0]), T.ref_lists(job3["tracked"][0], store), "frame 0 in front of an empty last frame")
        PC.same(PC.as_ref(lm.last_track_pose(0)), job3["refs"][0], "frame 0 in front of an empty last frame")
        lm.track_rig_frames(views, rig, [0, 1, 2], [[], [], []])
        assert [lm.last_track_pose(f).status for f in range(3)] == [P.NO_OBS] * 3
        lm.set_track_refine(None)


def test_state_rules(mc, vocs, job3):
    """last_track_pose is MCORB_E_STATE before any call, with the option off and while a call is pending"""
    rig = job3["rig"]
    view = T.to_view(mc, job3["vs"][0])
    for lm in stores(mc, vocs, job3["store"]):
        def state_error(what):
            with pytest.raises(mc.McorbError) as e:
                lm.last_track_pose()
            assert e.value.code == mc.E_STATE, what

        state_error("before any call")
        lm.track_rig_frame(view, rig, 0, job3["lidss"][0])
        state_error("the option is off")
        lm.set_track_refine(INV)
        state_error("the last call ran without the option")
        lm.track_rig_frame_submit(view, rig, 0, job3["lidss"][0])
        state_error("pending")
        with pytest.raises(mc.McorbError) as e:
            lm.set_track_refine(None)
        assert e.value.code == mc.E_STATE
        lm.track_wait()
        PC.same(PC.as_ref(lm.last_track_pose()), job3["refs"][0], "after the wait")
        # an explicit refinement in between does not disturb it
        PC.refine(mc, lm, PC.flat_rig(), PC.IDENT, PC.huber_rows())
        PC.same(PC.as_ref(lm.last_track_pose()), job3["refs"][0], "after a refine_pose")
        lm.set_track_refine(None)
        lm.track_rig_frame(view, rig, 0, job3["lidss"][0])
        state_error("the option is off again")
