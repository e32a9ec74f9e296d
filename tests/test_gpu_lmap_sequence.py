"""Every call of the local map that keeps scratch of its own, one after the other on ONE device store and on a host-only twin:
track from host arrays, track_rig_frames (2 frames), refine_pose, ransac_pose with its refinement (both solvers),
triangulate_new, triangulate_neighbours (2 neighbours), observe / update_points, search, relative_pose, align_pose (mode 1 from
points, mode 0 from landmark ids), essential_pose and initialize, bundle_adjust (points and landmark ids), retriangulate (report,
apply, a search over the survivors), and relative_pose_polished and essential_pose_polished right behind their unpolished calls
(they share `in`, `h_out` and `h_flags` with them) -- three times over, small, about four times larger, small again, so that every grow-only buffer is grown by one call and then used again, by that call and, where the
buffers are shared, by the others.  Every result equals the twin's bit for bit (floats as raw bytes); after each call its timing
getter gives a finite, non-negative number for every span that ran, and the span of k_track_points reads exactly 0 for the frame
from host arrays -- also right behind a rig slot's frames.  What this is aimed at: two calls on one buffer, or a group's reserve
given one call site's counts at the other.  2 cameras, tens of landmarks, a few hundred keypoints, 16 .. 64 hypotheses."""
import math

import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
import ba_cases as BC
import ba_ref as B
import ess_cases as EC
import ess_polish_cases as EPC
import init_cases as Ic
import init_ref as IR
import kfdb_cases as K
import landmark_cases as Lc
import lmap_cases as Lm
import mapping_cases as Mc
import mapping_new_cases as Nc
import pose_cases as PC
import rel_cases as RC
import rel_polish_cases as RPC
import retri_cases as RTC
import retri_ref as RT
import sac_cases as SC
import sac_rig_cases as SR
import track_cases as T
from test_gpu_init import same as same_init, same_store as same_init_store
from test_gpu_track_batch import extracted, frame_landmarks, shifted
from test_lmap_cpu import make, same_result, scene_landmarks
from test_retri_cpu import record_observations

pytestmark = pytest.mark.gpu

C = 2
MAXL = 8192
# where each call keeps its landmarks: (host-array tracking, the rig frames', refine_pose, ransac_pose central / rig, the neighbours' old
# landmarks are the scene's own 3000 .., new ids of triangulate_neighbours / triangulate_new, observe, search, align_pose's frame-1
# points, initialize's new ids: 160 per round, bundle_adjust's points, retriangulate's landmarks: 150 per round)
AT = dict(track=0, frames=600, pose=1300, sac=1800, sac_rig=2400, neigh_new=4200, new_new=5200, observe=6200, search=7400, align=2600,
          init=7700, ba=6750, retri=6920)
#        landmarks twins  per_cam  pose  sac  thin  hyp  neighbours      old  new  observe  search
SIZES = [(40, 20, 8, 12, 20, 3, 16, (16, 12), 8, 24, 30, 60),
         (160, 80, 32, 48, 80, 12, 64, (64, 48), 32, 96, 120, 240),
         (40, 20, 8, 12, 20, 3, 16, (16, 12), 8, 24, 30, 60)]


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


def moved(store, lids, off):
    return {l + off: v for l, v in store.items()}, [l if l < 0 else l + off for l in lids]


def spans_ok(us):
    us = [us] if isinstance(us, float) else list(us)
    assert all(math.isfinite(u) and u >= 0.0 for u in us), us
    return us


def same_fields(a, b, fields, what):
    for f in fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, f)


def same_sac(a, b, what):
    same_fields(a, b, ("R", "t", "sac_R", "sac_t", "inliers", "sample"), what)
    for f in ("status", "used", "n_inliers", "n_matches", "sac_n_inliers", "best_hypothesis", "n_models", "n_consensus"):
        assert getattr(a, f) == getattr(b, f), (what, f)
    same_fields(a.refine, b.refine, ("R", "t", "cost_initial", "cost_final", "iterations"), what + ", refinement")
    assert (a.refine.status, a.refine.n_inliers, a.refine.n_obs) == (b.refine.status, b.refine.n_inliers, b.refine.n_obs), what


def frames_of_the_slot(mc, both, rig, rnd, per_cam, what):
    fstore, lidss = frame_landmarks(np.random.default_rng(200 + rnd), rig, range(2), per_cam=per_cam)
    fstore = {l + AT["frames"]: v_ for l, v_ in fstore.items()}
    lidss = [[l if l < 0 else l + AT["frames"] for l in ls] for ls in lidss]
    views = [T.to_view(mc, shifted(rig, t)) for t in ((0, 0), (2, -1))]
    got = []
    for lm in both:
        T.fill(lm, fstore)
        got.append([T.as_lists(r) for r in lm.track_rig_frames(views, rig, [0, 1], lidss)])
    for f in range(2):
        T.same(got[0][f], got[1][f], what + "track_rig_frames, frame %d" % f)
        assert sum(len(m) for m in got[0][f]["matches"]) > 0
    us = spans_ok(both[0].last_track_timing5())
    assert us[0] > 0 and us[4] > 0



def one_round(mc, lm_d, db_d, lm_h, db_h, rig, rnd, size):
    nl, ntw, per_cam, npose, nsac, nthin, hyp, nneigh, nold, nnew, nobs, nsearch = size
    both = (lm_d, lm_h)
    what = "round %d, " % rnd

    # track from host arrays
    v, store, kps, descs, lids = T.scene(C, seed=rnd, n_landmarks=nl, n_twins=ntw)
    store, lids = moved(store, lids, AT["track"])
    xy, ds = T.kp_arrays(kps, descs)
    got = []
    for lm in both:
        T.fill(lm, store)
        got.append(T.as_lists(lm.track(T.to_view(mc, v), xy, ds, lids)))
    T.same(got[0], got[1], what + "track")
    assert sum(len(m) for m in got[0]["matches"]) > 0 and got[0]["n_candidates"] == len(store)
    us = spans_ok(lm_d.last_track_timing5())
    assert us[0] == 0.0, "k_track_points did not run for a frame from host arrays"
    assert us[1] > 0 and us[2] > 0

    # two frames of the rig slot's job in one submission
    frames_of_the_slot(mc, both, rig, rnd, per_cam, what)

    # refine_pose, ids and points
    cams, truth, init, obs, _ = PC.scene(C, nlm=npose, seed=5 + rnd)
    for form in ("lids", "pts"):
        got = [PC.as_ref(PC.refine(mc, lm, cams, init, obs, form=form, first_lid=AT["pose"])) for lm in both]
        PC.same(got[0], got[1], what + "refine_pose, " + form)
        assert got[0]["n_inliers"] > 0
        spans_ok(lm_d.last_pose_timing())
    # ransac_pose with its refinement, both solvers
    cams, truth, obs, match, _ = SC.scene(C, nlm=nsac, seed=3 + rnd, per_match=2)
    got = [SC.run(mc, lm, cams, obs, match=match, max_iterations=hyp, refine=(PC.INV_SIGMA2,), form="lids", first_lid=AT["sac"]) for lm in both]
    same_sac(got[0], got[1], what + "ransac_pose, central")
    assert got[0].status == mc.SAC_OK
    us, nh = lm_d.last_ransac_timing()
    assert nh == hyp and len(spans_ok(us)) == 3
    cams, truth, obs, match, _ = SR.thin_scene(C, per_cam=nthin, seed=3 + rnd)
    got = [SR.run(mc, lm, cams, obs, max_iterations=hyp, refine=(PC.INV_SIGMA2,), form="lids", first_lid=AT["sac_rig"]) for lm in both]
    same_sac(got[0], got[1], what + "ransac_pose, rig")
    assert got[0].status == mc.SAC_OK
    spans_ok(lm_d.last_ransac_timing()[0])

    # triangulate_new
    sc = Nc.scene(C, n=nnew, seed=1 + rnd)
    sc["next_lid"] = AT["new_new"] + 300 * rnd
    got = [Nc.run_scene(mc, lm, sc) for lm in both]
    Nc.same(got[0], got[1], what + "triangulate_new")
    assert got[0].n_triangulated > 0
    us, launched = lm_d.last_triangulate_new_timing()
    assert launched > 0 and spans_ok(us)

    # triangulate_neighbours, two neighbours
    sc = Mc.scene(C, sizes=nneigh, seed=1 + rnd, n_old=nold)
    sc["next_lid"] = AT["neigh_new"] + 300 * rnd
    got = []
    for lm in both:
        Mc.fill_store(lm, sc["store"])
        got.append(Mc.run_scene(mc, lm, sc))
    same_fields(got[0], got[1], ("inliers", "verdict", "new_lid", "pt3d", "normal", "dist2", "cos_parallax", "neigh_skipped", "depth_vec",
                                 "lids_cur"), what + "triangulate_neighbours")
    assert got[0].n_triangulated == got[1].n_triangulated > 0 and got[0].next_lid == got[1].next_lid
    for a, b in zip(got[0].lids_neigh, got[1].lids_neigh):
        assert a.tolist() == b.tolist()
    us_tri, us_depth, launched, depths = lm_d.last_triangulate_timing()
    assert launched > 0 and depths > 0 and spans_ok((us_tri, us_depth))

    # observe and update_points: both stores against the restatement, which makes them equal
    lid0 = AT["observe"] + 200 * rnd
    b = Lc.batch(nobs, C, rnd, lid0=lid0)
    Lc.run_batch(mc, list(both), *b, lid0=lid0)
    lids = b[4]
    new = b[0][lids - lid0] + np.random.default_rng(rnd).choice([0.5, 4.9, 5.1, 8.0], (len(lids), 1)) * np.array([[0.6, 0.0, 0.8]])
    got = [lm.update_points(lids, new) for lm in both]
    assert got[0][0].tolist() == got[1][0].tolist() and got[0][1].tobytes() == got[1][1].tobytes() and 0 < got[0][0].sum() < len(lids)
    assert Lc.snapshot(lm_d, lids) == Lc.snapshot(lm_h, lids)
    spans_ok(lm_d.last_landmark_timing())

    # search
    view, land, probe, cur = scene_landmarks(C, nsearch, seed=rnd)
    land = (AT["search"] + np.arange(nsearch, dtype=np.int32),) + tuple(land[1:])
    got = []
    for lm, db in ((lm_d, db_d), (lm_h, db_h)):
        lm.set(*land)
        got.append(lm.search(Lm.to_view(mc, view), land[0], [], db, 0, *cur, levelsup=K.LEVELSUP))
    same_result(got[0], got[1], what + "search")
    assert len(got[0].new_lids) > 0
    us = lm_d.last_timing()
    assert us[2] == nsearch and spans_ok(us[:2])

    # relative_pose: as many matches as the tracking scene has landmarks
    cams, truth, matches, _ = RC.scene(C, nl, 5 + rnd, moved=0.0)
    got = [RC.run(mc, lm, cams, matches, max_iterations=hyp, seed=rnd) for lm in both]
    same_fields(got[0], got[1], ("R", "t", "inliers", "sample"), what + "relative_pose")
    for f in ("status", "n_inliers", "n_matches", "best_hypothesis", "n_models"):
        assert getattr(got[0], f) == getattr(got[1], f), (what, "relative_pose", f)
    assert got[0].status == mc.REL_OK and got[0].n_inliers > 17
    us, nh = lm_d.last_relative_timing()
    assert nh == hyp and len(spans_ok(us)) == 3
    # .. and its polish on the same matches: the same `in`, `h_out` and `h_flags`, the polish's own scratch behind them
    plain = got
    got = [RPC.run(mc, lm, cams, matches, max_iterations=hyp, seed=rnd) for lm in both]
    same_fields(got[0][0], got[1][0], ("R", "t", "inliers", "sample"), what + "relative_pose_polished")
    for f in ("status", "n_inliers", "n_matches", "best_hypothesis", "n_models"):
        assert getattr(got[0][0], f) == getattr(got[1][0], f), (what, "relative_pose_polished", f)
    RPC.same_polish(got[0][1], got[1][1], what + "relative_pose_polished")
    assert got[0][0].status == mc.REL_OK and got[0][1].R.tobytes() == plain[0].R.tobytes() and got[0][1].rounds_run >= 1, "the polish began from the winner"
    us, nh = lm_d.last_relative_timing4()
    assert nh == hyp and len(spans_ok(us)) == 4 and us[3] > 0

    # align_pose: mode 1 from points, mode 0 from the store's landmarks
    truth, p1, p2, _ = AC.scene(n=nobs, seed=7 + rnd, moved=nobs // 10)
    got = [AC.run(mc, lm, p1, p2, max_iterations=hyp, seed=rnd) for lm in both]
    AC.same_results(got[0], got[1], what + "align_pose, sac")
    assert got[0].status == AR.OK and got[0].used == AR.USED_FIT and got[0].n_inliers > 3 and math.isfinite(got[0].mean_error)
    us, nh = lm_d.last_align_timing()
    assert nh == hyp and len(spans_ok(us)) == 4
    lids = AT["align"] + np.arange(nobs, dtype=np.int32)
    got = []
    for lm in both:
        lm.set(lids, p1, np.zeros_like(p1))
        got.append(AC.run(mc, lm, None, p2, mode=AR.ALL, lids1=lids))
    AC.same_results(got[0], got[1], what + "align_pose, all, lids1")
    AC.same_results(got[0], AC.run(mc, lm_h, p1, p2, mode=AR.ALL), what + "align_pose, all, lids1 against pts1")
    assert got[0].status == AR.OK and math.isfinite(got[0].mean_error)
    spans_ok(lm_d.last_align_timing()[0])

    # essential_pose
    truth, matches, _ = EC.scene("general", n=nl, seed=9 + rnd, noise=0.1)
    got = [EC.run(mc, lm, matches, max_iterations=hyp, seed=rnd) for lm in both]
    EC.same_stores(got[0], got[1], what + "essential_pose")
    assert got[0].status == mc.ESS_OK and got[0].n_inliers > 5
    for x, y in zip(lm_d.last_essential_counts(), lm_h.last_essential_counts()):
        assert x.tobytes() == y.tobytes(), what + "essential_pose, the slots"
    us, nh = lm_d.last_essential_timing()
    assert nh == hyp and len(spans_ok(us)) == 4
    # .. and its polish on the same matches
    got = [EPC.run(mc, lm, matches, max_iterations=hyp, seed=rnd) for lm in both]
    EC.same_stores(got[0][0], got[1][0], what + "essential_pose_polished")
    EPC.same_polish(got[0][1], got[1][1], what + "essential_pose_polished")
    assert got[0][0].status == mc.ESS_OK and got[0][1].rounds_run >= 1
    us, nh = lm_d.last_essential_timing5()
    assert nh == hyp and len(spans_ok(us)) == 5 and us[4] > 0

    # initialize: init_cases.py's two-camera scene, its ids in a range of its own
    sc = Ic.scene(C, n=nsearch, seed=3 + rnd)
    sc["next_lid"] = AT["init"] + 160 * rnd
    sc["prev"]["lids"][sc["prev"]["lids"] == 7] = sc["next_lid"] + 159
    got = [Ic.run_scene(mc, lm, sc) for lm in both]
    same_init(got[0], got[1], what + "initialize")
    new = got[0].new_lid[got[0].new_lid >= 0]
    assert got[0].status == (IR.DONE if nsearch >= 240 else IR.FEW), "the large round initializes, the small ones have too few matches"
    assert len(new) == (got[0].n_triangulated if got[0].status == IR.DONE else 0)
    assert len(new) == 0 or (sc["next_lid"] <= new.min() and new.max() < sc["next_lid"] + 159)
    same_init_store(lm_d, lm_h, new, what + "initialize")
    us = lm_d.last_initialize_timing()
    assert us[3] == int(sc["flags"].sum()) and spans_ok(us[:3])

    # bundle_adjust, points and ids: as many landmarks as the tracking scene
    sc = BC.scene(nkf=4, ncams=C, nlm=nl, nfixed=2, seed=30 + rnd, max_views=3)
    for form in ("pts", "lids"):
        got = [BC.run(mc, lm, sc, max_iterations=6, form=form, first_lid=AT["ba"]) for lm in both]
        same_fields(got[0], got[1], ("R", "t", "pts", "inliers", "cost_initial", "cost_final"), what + "bundle_adjust, " + form)
        for f in ("status", "iterations", "n_inliers", "n_obs"):
            assert getattr(got[0], f) == getattr(got[1], f), (what, "bundle_adjust", form, f)
        assert got[0].status in (B.CONVERGED, B.MAX_ITER) and got[0].cost_final < got[0].cost_initial and got[0].n_obs == len(sc["obs"])
        us, idle = lm_d.last_ba_timing()
        assert len(spans_ok(us)) == 7 and us[0] > 0

    # retriangulate: report, apply with a cap that holds every pair, a search over the survivors.  The landmarks are a search
    # scene's, with descriptors; every second one keeps that scene's point, far from where its views put it (VALID_REJECTED: it
    # stays where the search sees it), every fifth has a NaN keypoint (DEGENERATE: apply deletes it)
    view, land, probe, cur = scene_landmarks(C, nobs, seed=10 + rnd)
    lids = AT["retri"] + 150 * rnd + np.arange(nobs, dtype=np.int32)
    sc = RTC.synth(4, C, [2 + j % 4 for j in range(nobs)], seed=20 + rnd)
    sc["pts"] = [land[1][j].tolist() if j % 2 else p for j, p in enumerate(sc["pts"])]
    for j in range(2, nobs, 5):
        i = next(i for i, o in enumerate(sc["obs"]) if o[2] == j)
        sc["obs"][i] = sc["obs"][i][:3] + (float("nan"), 1.0)
    fields = ("pts", "diff_norm", "n_views", "verdict")
    for lm in both:
        lm.set(lids, np.array(sc["pts"]), *land[2:])
        record_observations(mc, lm, lids)
    got = [RTC.run(mc, lm, sc, lids=lids) for lm in both]
    same_fields(got[0], got[1], fields, what + "retriangulate, report")
    assert got[0].counts == got[1].counts and got[0].n_pairs == got[1].n_pairs > 0 and got[0].launched
    assert min(got[0].counts[v] for v in (RT.VALID_UPDATED, RT.VALID_REJECTED, RT.DEGENERATE)) > 0, got[0].counts
    assert Lc.snapshot(lm_d, lids) == Lc.snapshot(lm_h, lids)
    assert len(spans_ok(lm_d.last_retri_timing())) == 2
    report = got[0]
    got = [RTC.run(mc, lm, sc, lids=lids, apply=True, cap=2 * nobs) for lm in both]
    same_fields(got[0], got[1], fields, what + "retriangulate, apply")
    same_fields(got[0], report, fields, what + "retriangulate, apply against report")
    assert got[0].counts == got[1].counts and got[0].pairs == got[1].pairs and len(got[0].pairs) == got[0].n_pairs == report.n_pairs
    alive = lids[[v not in RT.FAILED for v in got[0].verdict.tolist()]]
    assert 0 < len(alive) < nobs and Lc.snapshot(lm_d, alive) == Lc.snapshot(lm_h, alive)
    spans_ok(lm_d.last_retri_timing())
    got = [lm.search(Lm.to_view(mc, view), alive, [], db, 0, *cur, levelsup=K.LEVELSUP) for lm, db in ((lm_d, db_d), (lm_h, db_h))]
    same_result(got[0], got[1], what + "search over the survivors")
    assert len(got[0].new_lids) > 0 and set(got[0].new_lids.tolist()) <= set(alive.tolist())
    us = lm_d.last_timing()
    assert us[2] == len(alive) and spans_ok(us[:2])


def test_every_call_three_times_on_one_store(mc):
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    probe = scene_landmarks(C, 8)[2]
    (lm_d, db_d), (lm_h, db_h) = [make(mc, voc, dev, probe, max_landmarks=MAXL, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]
    rig = extracted(mc, C, 320, 240, 2, 300)
    try:
        for rnd, size in enumerate(SIZES):
            one_round(mc, lm_d, db_d, lm_h, db_h, rig, rnd, size)
    finally:
        rig.close()
