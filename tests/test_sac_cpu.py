"""The absolute rig pose by RANSAC on the host-only store (device -1): mcorb_lmap_ransac_pose against the plain-Python
restatement (sac_ref.py) and against answers written out by hand.  Bit for bit, floats as raw bytes, but for the one comparison
of the minimal solver, which states its tolerance.  No GPU.

On the commit before this call existed every test of this file fails (`python -m pytest tests/test_sac_cpu.py`): LocalMap has
no ransac_pose."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import kfdb_cases as K
import pose_cases as PC
import pose_ref as P
import sac_cases as SC
import sac_ref as S
import track_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture()
def lm(mc, voc):
    assert hasattr(mc.LocalMap, "ransac_pose")
    return mc.LocalMap(voc, device=-1, max_landmarks=4096, max_candidates=1024)


@pytest.fixture(scope="module")
def scenes(mc):
    """the seeded scenes of 1, 4 and 8 cameras and their restatements, computed once"""
    assert hasattr(mc.LocalMap, "ransac_pose")
    out = {}
    for ncams in (1, 4, 8):
        cams, truth, obs, match, moved = SC.scene(ncams)
        out[ncams] = (cams, truth, obs, match, moved, S.ransac(cams, obs, SC.THRESHOLD, SC.solver_of(mc, cams), match, 100, 0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the minimal solver (the one comparison of this file with a tolerance)
# ---------------------------------------------------------------------------------------------------------------------------
def test_solver_recovers_the_generating_pose(mc):
    """4 000 seeded cases (rotations up to 3.1 rad, translation N(0, 1) per axis, three points at depth 2 - 10 within +-0.5 x
    +-0.4 normalised).  A case is included iff the numpy solver alone (polyroots + Kabsch) recovers the generating pose to 1e-8
    (max |dR_ij|, |dt| / max(1, |t|)); at most 1 % may be left out.  On every included case one of mcorb_sac_solve's poses
    recovers it to 1e-6 -- two decades of margin, because a closed-form quartic loses digits that eigenvalue roots keep -- and
    every pose it returns scores below 1e-12 on its own three points.  Measured: 13 of 4 000 left out (0.33 %), worst error of
    mcorb_sac_solve on the included ones 2.1e-8, worst own score 6.6e-14"""
    assert hasattr(mc, "sac_solve")
    cases = SC.solver_cases()
    assert len(cases) == 4000
    cc = PC.to_cams(mc, [cases[0][0]])
    left, worst, worst_self = 0, 0.0, 0.0
    for cam, truth, uv, X in cases:
        f = [S.bearing(cam, u, v) for u, v in uv]
        alone = min([S.pose_distance(S.rig_pose(cam, R_, t_), truth) for R_, t_ in S.numpy_p3p(f, X)], default=math.inf)
        got = mc.sac_solve(cc, 0, uv, X)
        assert len(got) <= 4
        for R_, t_ in got:
            own = float(mc.sac_eval(cc, R_, t_, [0] * 3, uv, X).max())
            worst_self = max(worst_self, own)
            assert own < 1e-12, (own, uv)
        if not alone <= 1e-8:
            left += 1
            continue
        d = min([S.pose_distance(p, truth) for p in got], default=math.inf)
        worst = max(worst, d)
        assert d <= 1e-6, (d, alone, uv, X)
    print("left out %d of %d, worst error %.3g, worst own score %.3g" % (left, len(cases), worst, worst_self))
    assert left <= 0.01 * len(cases)


def test_solver_hook_degenerate(mc):
    """three collinear points, and two equal points: no pose, and nothing but finite numbers ever comes back"""
    cc = PC.to_cams(mc, PC.flat_rig())
    assert mc.sac_solve(cc, 0, [[0.0, 0.0], [0.1, 0.0], [0.2, 0.0]], [[0.0, 0.0, 4.0], [0.4, 0.0, 4.0], [0.8, 0.0, 4.0]]) == []
    assert mc.sac_solve(cc, 0, [[0.0, 0.0], [0.0, 0.0], [0.2, 0.1]], [[0.0, 0.0, 4.0], [0.0, 0.0, 4.0], [0.8, 0.4, 4.0]]) == []
    assert mc.sac_threshold(640.0) == 1.0 - math.cos(math.atan(math.sqrt(2.0) * 0.5 / 640.0))


# ---------------------------------------------------------------------------------------------------------------------------
# sampling, on the bits
# ---------------------------------------------------------------------------------------------------------------------------
def test_draws():
    """the splitmix64 finaliser against its published first outputs: seed 0 yields 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4"""
    assert S.draw(0, 0, 0) == 0xE220A8397B1DCDAF
    assert S.draw(0x9E3779B97F4A7C15, 0, 0) == 0x6E789E6AA1B965F4
    assert S.draw(5, 3, 7) == S.draw(5 + 0x9E3779B97F4A7C15 * 55, 0, 0)


def check(mc, lm, cams, obs, what, threshold=SC.THRESHOLD, match=None, max_iterations=100, seed=0, forms=("pts", "lids")):
    ref = S.ransac(cams, obs, threshold, SC.solver_of(mc, cams), match, max_iterations, seed)
    for form in forms:
        SC.same_plain(SC.run(mc, lm, cams, obs, threshold, match, max_iterations, seed, form=form), ref, "%s, %s" % (what, form))
    return ref


def test_four_in_one_camera_and_ties(mc, lm):
    """S = 4 in one camera: every hypothesis draws the same set, in its own order.  Every model has all four as inliers, so all
    counts tie and the lowest hypothesis with a model wins"""
    obs = SC.square()
    ref = check(mc, lm, PC.flat_rig(), obs, "S = 4", threshold=1e-9)
    assert ref["status"] == S.OK and ref["n_inliers"] == 4 and all(ref["inliers"])
    assert all(sorted(s) == [0, 1, 2, 3] for s, m in zip(ref["samples"], ref["models"]) if m is not None)
    assert len(set(tuple(s) for s in ref["samples"])) > 4
    with_model = [h for h, c in enumerate(ref["counts"]) if c is not None]
    assert len(with_model) >= 2 and all(ref["counts"][h] == 4 for h in with_model) and ref["best"] == with_model[0]


def test_no_model_and_no_obs(mc, lm):
    obs = SC.square()[:3]
    ref = check(mc, lm, PC.flat_rig(), obs, "S = 3")
    assert ref["status"] == S.NO_MODEL and ref["n_models"] == 0
    got = SC.run(mc, lm, PC.flat_rig(), obs)
    assert P.same_bits(got.R.tolist(), S.IDENT[0]) and got.t.tolist() == [0.0] * 3 and not got.inliers.any() and len(got.inliers) == 3
    assert got.best_hypothesis == -1 and got.sample == (-1,) * 4
    ref = check(mc, lm, PC.flat_rig(), [], "S = 0", forms=("pts",))
    assert ref["status"] == S.NO_OBS
    got = SC.run(mc, lm, PC.flat_rig(), [])
    assert got.status == S.NO_OBS and got.n_matches == 0 and len(got.inliers) == 0 and P.same_bits(got.R.tolist(), S.IDENT[0])
    # with a refinement asked for: NO_OBS from the identity, and used stays 0
    got = SC.run(mc, lm, PC.flat_rig(), [], refine=(PC.INV_SIGMA2,))
    assert got.status == S.NO_OBS and got.used == 0 and got.refine.status == P.NO_OBS
    got = SC.run(mc, lm, PC.flat_rig(), obs, refine=(PC.INV_SIGMA2,))
    assert got.status == S.NO_MODEL and got.used == 0 and not got.inliers.any() and P.same_bits(got.R.tolist(), S.IDENT[0])


def test_a_camera_with_three_and_one_with_five(mc, lm):
    """a hypothesis whose first draw lands in the camera with 3 consensus observations has no model; the others do"""
    rig = PC.flat_rig(2)
    five = SC.square(cam=1) + [(1, 0.375, 0.375, 0, [1.5, 1.5, 4.0])]
    obs = [SC.square(cam=0)[0], five[0], SC.square(cam=0)[1], five[1], five[2], SC.square(cam=0)[2], five[3], five[4]]
    ref = check(mc, lm, rig, obs, "3 + 5", threshold=1e-9)
    in0 = [h for h, s in enumerate(ref["samples"]) if obs[s[0]][0] == 0]
    assert 10 < len(in0) < 90 and all(ref["models"][h] is None and ref["samples"][h][1:] == [-1] * 3 for h in in0)
    assert all(obs[i][0] == 1 for h, s in enumerate(ref["samples"]) if h not in in0 for i in s)
    assert ref["status"] == S.OK and ref["n_inliers"] == 8 and ref["n_models"] <= 100 - len(in0)


def test_duplicates_exhaust_the_draws(mc, lm):
    """S = 4: a hypothesis whose 15 further draws never name three other members has no model.  The first seed for which
    that happens among 100 hypotheses is found on the restatement"""
    obs = SC.square()
    cons = list(range(4))
    seed = next(sd for sd in range(64) if any(not S.sample(sd, h, obs, cons)[1] for h in range(100)))
    ref = check(mc, lm, PC.flat_rig(), obs, "duplicates", threshold=1e-9, seed=seed)
    out = [h for h in range(100) if not S.sample(seed, h, obs, cons)[1]]
    assert out and all(ref["models"][h] is None and -1 in ref["samples"][h] for h in out)
    assert ref["n_models"] <= 100 - len(out) and ref["status"] == S.OK


@pytest.mark.parametrize("per_match", [1, 2, 16])
def test_match_forms(mc, lm, per_match):
    """1, 2 and 16 observations per match: the consensus set is the first of each, the flags are per match"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=40, seed=7, per_match=per_match)
    ref = check(mc, lm, cams, obs, "%d per match" % per_match, match=match)
    nm = match[-1] + 1
    assert ref["n_consensus"] == nm and len(obs) >= nm * per_match and ref["status"] == S.OK
    if per_match == 1:      # and without the array every observation is its own match
        own = check(mc, lm, cams, obs, "no match array", match=None)
        assert own["n_consensus"] == len(obs) >= nm
    # match indices need not be dense
    sparse = [3 * k + 5 for k in match]
    SC.same_plain(SC.run(mc, lm, cams, obs, match=sparse), ref, "sparse match indices")


# ---------------------------------------------------------------------------------------------------------------------------
# the threshold, a NaN score
# ---------------------------------------------------------------------------------------------------------------------------
def threshold_rows(mc):
    """-> (rig, obs, seed, k, score, model): six observations of the flat rig, one hypothesis.  Observation 4 is a little off
    and observation 5 a placeholder; the seed is the first whose only hypothesis draws neither, so the model does not depend
    on them.  Observation 5's point is then put at the model's translation, bit for bit: with the flat rig's camera at the body's
    origin q is (0, 0, 0) there and the score 0 / 0"""
    rig = PC.flat_rig()
    obs = SC.square() + [(0, 0.3125, 0.0625, 0, [1.26, 0.24, 4.0]), (0, 0.0, 0.0, 0, [0.0, 0.0, 3.0])]
    seed = next(sd for sd in range(256) if sorted(S.sample(sd, 0, obs, list(range(6)))[0]) == [0, 1, 2, 3])
    ref = S.ransac(rig, obs, 1e-3, SC.solver_of(mc, rig), None, 1, seed)
    assert ref["status"] == S.OK
    model = (ref["R"], ref["t"])
    obs[5] = (0, 0.0, 0.0, 0, list(model[1]))
    sc = S.obs_score(rig, model, obs[4])
    assert 1e-7 < sc < 1e-3 and S.obs_score(rig, model, obs[5]) != S.obs_score(rig, model, obs[5])
    return rig, obs, seed, sc, model


def test_threshold_is_strict_and_nan_is_no_inlier(mc, lm):
    rig, obs, seed, sc, model = threshold_rows(mc)
    cc = PC.to_cams(mc, rig)
    cam, uv, octave, pts = PC.arrays(obs)
    hook = mc.sac_eval(cc, model[0], model[1], cam, uv, pts)
    assert S.bits(float(hook[4])) == S.bits(sc) and math.isnan(hook[5])
    assert all(S.bits(float(hook[i])) == S.bits(S.obs_score(rig, model, obs[i])) for i in range(5))
    at = check(mc, lm, rig, obs, "threshold = the score", threshold=sc, max_iterations=1, seed=seed)
    above = check(mc, lm, rig, obs, "threshold = the next double", threshold=S.next_up(sc), max_iterations=1, seed=seed)
    assert at["flags"] == [True] * 4 + [False, False] and above["flags"] == [True] * 5 + [False]
    assert at["n_inliers"] == 4 and above["n_inliers"] == 5
    wide = check(mc, lm, rig, obs, "a wide threshold", threshold=1.5, max_iterations=1, seed=seed)
    assert wide["flags"] == [True] * 5 + [False]      # the NaN is not an inlier at any threshold


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded scene
# ---------------------------------------------------------------------------------------------------------------------------
# the pose error of the restatement against the truth (max |dR_ij|, |dt| in m), read from the restatement alone; the pass
# mark is ten times the reading
READ = {1: (2.37e-4, 1.56e-3), 4: (3.55e-4, 7.3e-4), 8: (1.65e-4, 2.24e-3)}


@pytest.mark.parametrize("ncams", [1, 4, 8])
def test_seeded_scene(mc, lm, scenes, ncams):
    """200 landmarks at depth 2 - 10 around an outward-facing rig, fx = fy = 500, principal point (640, 360), projections with N(0,
    0.1 px) rounded to float, 40 % moved by 50 px, 100 hypotheses, the reference's threshold at 640.  On the restatement alone:
    the winner's inliers are exactly the unmoved matches, and at least three hypotheses sampled no moved observation (read: 9,
    9 and 13).  Then the library equals the restatement on the bits and passes at ten times the error the restatement reads"""
    cams, truth, obs, match, moved, ref = scenes[ncams]
    cons = S.consensus(obs, match)[0]
    assert len(cons) == 200 and 0.3 < sum(moved[i] for i in cons) / 200 < 0.5
    assert ref["status"] == S.OK
    assert all(ref["flags"][i] == (not moved[i]) for i in cons) and ref["n_inliers"] == sum(not moved[i] for i in cons)
    clean = sum(1 for s, m in zip(ref["samples"], ref["models"]) if m is not None and not any(moved[i] for i in s))
    err = SC.pose_error((ref["R"], ref["t"]), truth)
    print("restatement, %d cameras: %d clean hypotheses, %.3g in R, %.3g m" % (ncams, clean, err[0], err[1]))
    assert clean >= 3
    assert err[0] <= READ[ncams][0] and err[1] <= READ[ncams][1]
    for form in ("pts", "lids"):
        got = SC.run(mc, lm, cams, obs, match=match, form=form)
        SC.same_plain(got, ref, "seeded scene, %d cameras, %s" % (ncams, form))
        err = SC.pose_error((got.R.tolist(), got.t.tolist()), truth)
        assert err[0] <= 10 * READ[ncams][0] and err[1] <= 10 * READ[ncams][1]


@pytest.mark.parametrize("ncams", [1, 4, 8])
def test_seeded_scene_with_refinement(mc, lm, scenes, ncams):
    """used = 1, and the refinement part is mcorb_lmap_refine_pose called explicitly on the same observations from the returned
    RANSAC pose, bit for bit"""
    cams, truth, obs, match, moved, sac = scenes[ncams]
    _, ref, final = S.ransac_refine(cams, obs, SC.THRESHOLD, SC.solver_of(mc, cams), PC.INV_SIGMA2, match, 100, 0)
    got = SC.run(mc, lm, cams, obs, match=match, refine=(PC.INV_SIGMA2,))
    SC.same(got, sac, "with refinement")
    SC.same_final(got, final, "with refinement")
    assert got.used == 1 and got.n_inliers >= got.sac_n_inliers
    explicit = PC.refine(mc, lm, cams, (got.sac_R.tolist(), got.sac_t.tolist()), obs)
    for f in ("R", "t", "cost_initial", "cost_final"):
        assert P.same_bits(np.asarray(getattr(got.refine, f)).tolist(), np.asarray(getattr(explicit, f)).tolist()), f
    assert (got.refine.status, got.refine.iterations, got.refine.n_inliers, got.refine.n_obs) == \
        (explicit.status, explicit.iterations, explicit.n_inliers, explicit.n_obs)
    assert P.same_bits(got.R.tolist(), explicit.R.tolist()) and P.same_bits(got.t.tolist(), explicit.t.tolist())
    first = sac["first"]
    assert got.inliers.tolist() == [bool(explicit.inliers[first[k]:first[k + 1]].all()) for k in range(len(first) - 1)]
    PC.same(dict(PC.as_ref(explicit)), ref, "the restatement's refinement")
    e0, e1 = SC.pose_error((got.sac_R, got.sac_t), truth), SC.pose_error((got.R, got.t), truth)
    assert e1[1] < e0[1]


def test_refinement_culls_a_match_the_ransac_kept(mc, lm):
    """the rule of FrontEnd.cpp:4786.  No observation is far off, eight are 5 px off and the threshold is wide (1 - cos of about
    16 px at f = 500), so the RANSAC keeps every match; the refinement's chi2 cull (5.991 px^2 at octave 0) drops the eight.
    The RANSAC's inlier matches outnumber the refinement's: its pose and flags are the answer, used = 0"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=60, seed=9, moved=0.0)
    obs = [(c, PC.f32(kx + 5.0) if i % 9 == 4 and i < 72 else kx, ky, 0, X) for i, (c, kx, ky, o, X) in enumerate(obs)]
    thr = 1.0 - math.cos(16.0 / 500.0)
    sac, ref, final = S.ransac_refine(cams, obs, thr, SC.solver_of(mc, cams), PC.INV_SIGMA2, match, 100, 0)
    assert sac["status"] == S.OK and sac["n_inliers"] == sac["n_consensus"]
    assert 0 < sum(not v for v in ref["inliers"]) <= 8 and final["used"] == 0
    got = SC.run(mc, lm, cams, obs, thr, match=match, refine=(PC.INV_SIGMA2,))
    SC.same(got, sac, "the 4786 case")
    SC.same_final(got, final, "the 4786 case")
    assert got.used == 0 and got.inliers.all() and got.refine.n_inliers < len(obs)
    assert P.same_bits(got.R.tolist(), got.sac_R.tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def read_back(lm, lids):
    return [(p.tobytes(), q.tobytes()) for p, q, _, _ in (lm.get(int(l)) for l in lids)]


def check_refusals(mc, lm):
    cams, truth, obs, match, moved = SC.scene(4, nlm=20, seed=7, per_match=2)
    lids = PC.fill_points(lm, obs)
    before = read_back(lm, lids)
    cam, uv, octave, pts = PC.arrays(obs)
    cc = PC.to_cams(mc, cams)
    ref = S.ransac(cams, obs, SC.THRESHOLD, SC.solver_of(mc, cams), match, 100, 0)

    def refused(code, pending=False, **kw):
        a = dict(cams=cc, cam=cam, uv=uv, octave=octave, threshold=SC.THRESHOLD, lids=lids, match=match)
        a.update(kw)
        with pytest.raises(mc.McorbError) as e:
            lm.ransac_pose(**a)
        assert e.value.code == code, (kw.keys(), e.value)
        assert pending or read_back(lm, lids) == before

    bad = cam.copy()
    bad[7] = 4
    refused(mc.E_ARG, cam=bad)
    bad[7] = -1
    refused(mc.E_ARG, cam=bad)
    bad = octave.copy()
    bad[3] = 16
    refused(mc.E_ARG, octave=bad)
    bad[3] = len(PC.INV_SIGMA2)
    refused(mc.E_ARG, octave=bad, refine=mc.pose_params(PC.INV_SIGMA2))
    bad[3] = -1
    refused(mc.E_ARG, octave=bad)
    bad = lids.copy()
    bad[5] = 4096
    refused(mc.E_ARG, lids=bad)
    bad[5] = -1
    refused(mc.E_ARG, lids=bad)
    refused(mc.E_ARG, pts=pts)                      # both
    refused(mc.E_ARG, lids=None)                    # neither
    for thr in (0.0, -1e-7, float("nan"), float("inf")):
        refused(mc.E_ARG, threshold=thr)
    refused(mc.E_ARG, max_iterations=0)
    refused(mc.E_ARG, max_iterations=1025)
    bad = list(match)
    bad[6], bad[7] = bad[7] + 1, bad[6]
    assert bad[7] < bad[6]
    refused(mc.E_ARG, match=bad)
    refused(mc.E_ARG, match=[k - 1 for k in match])
    refused(mc.E_ARG, refine=mc.pose_params(PC.INV_SIGMA2, 0))
    refused(mc.E_ARG, refine=mc.pose_params(PC.INV_SIGMA2, 101))
    refused(mc.E_ARG, refine=mc.pose_params([1.0] * 17))
    bad = lids.copy()
    bad[5] = 3000                                   # a slot that was never set
    refused(mc.E_STATE, lids=bad)
    # bad counts, through the C entry
    res, par = mc._lib.SacResultC(), mc._lib.SacParams()
    par.threshold, par.max_iterations = SC.THRESHOLD, 100
    for n, ncams in ((-1, 4), (20, 0), (20, 17)):
        code = lm.L.mcorb_lmap_ransac_pose(lm.h, n, cam.ctypes.data, uv.ctypes.data, octave.ctypes.data, None, lids.ctypes.data, None, ncams,
                                           C.addressof(cc.cams), C.byref(par), None, C.byref(res), None)
        assert code == mc.E_ARG, (n, ncams)
    assert read_back(lm, lids) == before
    # while a tracking call is pending
    v = T.to_view(mc, T.flat_view())
    lm.track_submit(v, [np.zeros((0, 2), np.float32)], [np.zeros((0, 32), np.uint8)], [])
    refused(mc.E_STATE, pending=True)
    lm.track_wait()
    assert read_back(lm, lids) == before
    # and it runs after all that
    SC.same_plain(lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match), ref, "after the refusals")
    assert read_back(lm, lids) == before


def test_refusals(mc, lm):
    check_refusals(mc, lm)


# ---------------------------------------------------------------------------------------------------------------------------
# the header's host path as a stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_under_asan_ubsan(mc, lm, scenes, tmp_path):
    """tests/cpp/test_sac_sanitize.cpp (its own main, -fsanitize=address,undefined) runs sac_run_serial on the 8-camera scene:
    no report, and every record -- the pick, the flags, and the model, sample and count of each of the 100 hypotheses -- equals
    the library's result and the restatement"""
    cams, truth, obs, match, moved, ref = scenes[8]
    exe = str(tmp_path / "test_sac_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_sac_sanitize.cpp"),
                           "-o", exe])
    cons = S.consensus(obs, match)[0]
    n, Sn, H, ncams = len(obs), len(cons), 100, len(cams)
    by_cam = [[i for i in cons if obs[i][0] == c] for c in range(ncams)]
    cam_first = [0]
    for c in range(ncams):
        cam_first.append(cam_first[-1] + len(by_cam[c]))
    blob = struct.pack("<4idQ", ncams, n, Sn, H, SC.THRESHOLD, 0)
    for c in cams:
        blob += struct.pack("<17d", *[v for row in c["R"] for v in row], *c["t"], c["fx"], c["fy"], c["s"], c["u0"], c["v0"])
    blob += b"".join(struct.pack("<2f2i", o[1], o[2], o[0], o[3]) for o in obs)
    blob += b"".join(struct.pack("<3d", *o[4]) for o in obs)
    blob += struct.pack("<%di" % Sn, *cons) + struct.pack("<%di" % (ncams + 1), *cam_first)
    blob += struct.pack("<%di" % Sn, *[i for own in by_cam for i in own])
    (tmp_path / "in.bin").write_bytes(blob)
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bad=0" in out.stdout and not out.stderr, out.stdout + out.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == 128 + n + 4 * H + 128 * H
    R_, t_ = struct.unpack("<9d", raw[:72]), struct.unpack("<3d", raw[72:96])
    status, n_in, best, n_models, *sample = struct.unpack("<8i", raw[96:128])
    flags = list(raw[128:128 + n])
    counts = struct.unpack("<%di" % H, raw[128 + n:128 + n + 4 * H])
    got = SC.run(mc, lm, cams, obs, match=match)
    assert struct.pack("<9d", *got.sac_R.reshape(9)) == raw[:72] and struct.pack("<3d", *got.sac_t) == raw[72:96]
    assert (status, n_in, best, n_models, tuple(sample)) == (got.status, got.sac_n_inliers, got.best_hypothesis, got.n_models, got.sample)
    assert [bool(flags[i]) for i in cons] == got.inliers.tolist() and flags == [int(v) for v in ref["flags"]]
    assert P.same_bits([list(R_[0:3]), list(R_[3:6]), list(R_[6:9])], ref["R"]) and P.same_bits(list(t_), ref["t"])
    for h in range(H):
        rec = raw[128 + n + 4 * H + 128 * h:128 + n + 4 * H + 128 * (h + 1)]
        valid, *smp = struct.unpack("<5i", rec[96:116])
        assert smp == ref["samples"][h] and bool(valid) == (ref["models"][h] is not None), h
        if valid:
            assert counts[h] == ref["counts"][h], h
            m = struct.unpack("<12d", rec[:96])
            assert P.same_bits([list(m[0:3]), list(m[3:6]), list(m[6:9])], ref["models"][h][0]) and P.same_bits(list(m[9:12]), ref["models"][h][1]), h
