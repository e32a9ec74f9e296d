"""The RANSAC with the rig solver (LocalMap.ransac_pose(..., solver="rig"), MCORB_SAC_SOLVER_RIG) on the host-only store (device
-1): against the plain-Python restatement (sac_rig_ref.py on sac_ref.py) and against the true pose of seeded scenes.  Bit for bit,
floats as raw bytes, but for the one comparison of the solver, which states its tolerance.  No GPU.

On the commit before the solver existed every test of this file fails (`python -m pytest tests/test_sac_rig_cpu.py`): ransac_pose
has no `solver`."""
import ctypes as C
import inspect
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
import sac_rig_cases as RC
import sac_rig_ref as R
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
    assert "solver" in inspect.signature(mc.LocalMap.ransac_pose).parameters
    return mc.LocalMap(voc, device=-1, max_landmarks=4096, max_candidates=1024)


@pytest.fixture(scope="module")
def scenes(mc):
    """the thin scenes (16 x 3 and 8 x 3 observations) and section 9i's seeded scenes (1, 4 and 8 cameras, 200 landmarks) with
    their restatements, computed once"""
    assert "solver" in inspect.signature(mc.LocalMap.ransac_pose).parameters
    out = {}
    for ncams in (16, 8):
        cams, truth, obs, match, moved = RC.thin_scene(ncams)
        out["thin", ncams] = (cams, truth, obs, match, moved, R.ransac(cams, obs, SC.THRESHOLD, RC.solver_of(mc, cams), match, 100, 0))
    for ncams in (1, 4, 8):
        cams, truth, obs, match, moved = SC.scene(ncams)
        out["seeded", ncams] = (cams, truth, obs, match, moved, R.ransac(cams, obs, SC.THRESHOLD, RC.solver_of(mc, cams), match, 100, 0))
    return out


def check(mc, lm, cams, obs, what, threshold=SC.THRESHOLD, match=None, max_iterations=100, seed=0, forms=("pts", "lids")):
    ref = R.ransac(cams, obs, threshold, RC.solver_of(mc, cams), match, max_iterations, seed)
    for form in forms:
        got = RC.run(mc, lm, cams, obs, "rig", threshold, match, max_iterations, seed, form=form)
        SC.same_plain(got, ref, "%s, %s" % (what, form))
    return ref


# ---------------------------------------------------------------------------------------------------------------------------
# the solver (the one comparison of this file with a tolerance)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncams", [1, 4, 8])
def test_solver_recovers_the_generating_pose(mc, ncams):
    """4 000 seeded noise-free cases per rig (RC.solver_cases: test_sac_cpu.py's, over outward-facing rigs of 1, 4 and 8 cameras
    at 0.2 m offsets, each observation's camera drawn for it, repeats allowed).  A case is included iff the independent solver
    alone (polyroots, 20 Newton steps through numpy.linalg.solve, Kabsch through numpy.linalg.svd) recovers the generating pose
    to 1e-8 (max |dR_ij|, |dt| / max(1, |t|)); at most 5 % may be left out, which is a condition.  On every included case one of
    mcorb_sac_solve_rig's poses recovers it to 1e-6, and every pose it returns on any case scores below 1e-12 on its own three
    points.  Measured, 1 / 4 / 8 cameras: 0, 193 and 150 of 4 000 left out (0 %, 4.8 %, 3.8 %); worst error on the included ones
    6.5e-12, 8.9e-12 and 2.5e-12; worst own score 4.4e-16 on all three.  (With 8 Newton steps instead of the library's 20
    three included cases of the 4-camera rig and four of the 8-camera rig are missed: section 9i.)"""
    assert hasattr(mc, "sac_solve_rig")
    cams, cases = RC.solver_cases(ncams)
    assert len(cases) == 4000
    cc = PC.to_cams(mc, cams)
    left, worst, worst_self = 0, 0.0, 0.0
    for truth, ci, uv, X in cases:
        c, d = RC.rays(cams, ci, uv)
        alone = min([S.pose_distance(p, truth) for p in R.numpy_rig(c, d, X)], default=math.inf)
        got = mc.sac_solve_rig(cc, ci, uv, X)
        assert len(got) <= 4
        for R_, t_ in got:
            own = float(mc.sac_eval(cc, R_, t_, ci, uv, X).max())
            worst_self = max(worst_self, own)
            assert own < 1e-12, (own, ci, uv)
        if not alone <= 1e-8:
            left += 1
            continue
        dist = min([S.pose_distance(p, truth) for p in got], default=math.inf)
        worst = max(worst, dist)
        assert dist <= 1e-6, (dist, alone, ci, uv, X)
    print("%d cameras: left out %d of %d, worst error %.3g, worst own score %.3g" % (ncams, left, len(cases), worst, worst_self))
    assert left <= 0.05 * len(cases)


def test_solver_hook_one_camera_and_degenerate(mc):
    """three observations of one camera: the rig solver's poses are the central solver's up to Newton's polish (1e-9); three
    collinear points and two equal points give no pose; a camera outside the rig is refused"""
    cam, truth, uv, X = SC.solver_cases(n=1)[0]
    cc = PC.to_cams(mc, [cam])
    central, rig = mc.sac_solve(cc, 0, uv, X), mc.sac_solve_rig(cc, [0, 0, 0], uv, X)
    assert len(central) == len(rig) >= 1
    for a, b in zip(central, rig):
        assert S.pose_distance(b, a) < 1e-9
    cc = PC.to_cams(mc, PC.flat_rig(2))
    assert mc.sac_solve_rig(cc, [0, 1, 0], [[0.0, 0.0], [0.1, 0.0], [0.2, 0.0]], [[0.0, 0.0, 4.0], [0.4, 0.0, 4.0], [0.8, 0.0, 4.0]]) == []
    assert mc.sac_solve_rig(cc, [0, 0, 1], [[0.0, 0.0], [0.0, 0.0], [0.2, 0.1]], [[0.0, 0.0, 4.0], [0.0, 0.0, 4.0], [0.8, 0.4, 4.0]]) == []
    for bad in ([0, 2, 0], [-1, 0, 0]):
        with pytest.raises(mc.McorbError) as e:
            mc.sac_solve_rig(cc, bad, [[0.0, 0.0], [0.1, 0.0], [0.2, 0.1]], [[0.0, 0.0, 4.0], [0.4, 0.0, 4.0], [0.8, 0.4, 4.0]])
        assert e.value.code == mc.E_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# sampling, on the bits
# ---------------------------------------------------------------------------------------------------------------------------
def one_per_camera():
    """four observations, one in each camera of the 4-camera rig, no noise and nothing moved"""
    cams, truth, obs, match, moved = RC.thin_scene(4, per_cam=1, moved=0.0, noise=0.0)
    assert [o[0] for o in obs] == [0, 1, 2, 3]
    return cams, truth, obs


def test_four_observations_over_four_cameras(mc, lm):
    """S = 4 spread one per camera: the central solver has no camera with four observations and answers NO_MODEL, the rig solver
    answers OK with all four as inliers near the true pose"""
    cams, truth, obs = one_per_camera()
    got = RC.run(mc, lm, cams, obs, "central")
    assert got.status == S.NO_MODEL and got.n_models == 0 and not got.inliers.any()
    assert got.sac_R.tobytes() == RC.run(mc, lm, cams, obs, 0).sac_R.tobytes()       # (the number and the name)
    ref = check(mc, lm, cams, obs, "one per camera")
    assert ref["status"] == S.OK and ref["n_inliers"] == 4 and all(ref["inliers"])
    assert all(sorted(s) == [0, 1, 2, 3] for s, m in zip(ref["samples"], ref["models"]) if m is not None)
    err = SC.pose_error((ref["R"], ref["t"]), truth)
    assert err[0] < 1e-5 and err[1] < 1e-4, err          # (exact points, keypoints rounded to float: some 1e-5 px)
    assert RC.run(mc, lm, cams, obs, mc.SAC_SOLVER_RIG).sac_R.tobytes() == RC.run(mc, lm, cams, obs, "rig").sac_R.tobytes()


def test_too_few_observations(mc, lm):
    cams, truth, obs = one_per_camera()
    ref = check(mc, lm, cams, obs[:3], "S = 3")
    assert ref["status"] == S.NO_MODEL and ref["n_models"] == 0 and all(-1 in s for s in ref["samples"])
    got = RC.run(mc, lm, cams, obs[:3])
    assert P.same_bits(got.R.tolist(), S.IDENT[0]) and got.t.tolist() == [0.0] * 3 and not got.inliers.any() and len(got.inliers) == 3
    assert got.best_hypothesis == -1 and got.sample == (-1,) * 4
    ref = check(mc, lm, cams, [], "S = 0", forms=("pts",))
    assert ref["status"] == S.NO_OBS
    got = RC.run(mc, lm, cams, [])
    assert got.status == S.NO_OBS and got.n_matches == 0 and len(got.inliers) == 0 and P.same_bits(got.R.tolist(), S.IDENT[0])


def test_duplicates_exhaust_the_draws(mc, lm):
    """S = 4: a hypothesis whose 16 draws never name four different members has no model.  The first seed for which that
    happens among 100 hypotheses is found on the restatement"""
    cams, truth, obs = one_per_camera()
    cons = list(range(4))
    seed = next(sd for sd in range(64) if any(not R.sample(sd, h, obs, cons)[1] for h in range(100)))
    ref = check(mc, lm, cams, obs, "duplicates", seed=seed)
    out = [h for h in range(100) if not R.sample(seed, h, obs, cons)[1]]
    assert out and all(ref["models"][h] is None and -1 in ref["samples"][h] for h in out)
    assert ref["n_models"] <= 100 - len(out) and ref["status"] == S.OK


def test_sample_walk_crosses_cameras():
    """the walk itself: the first member is draw 0's, every member is a consensus observation, and the samples of a rig with
    one observation per camera span cameras (the central walk's never do)"""
    obs = [(c, 0.0, 0.0, 0, [0.0, 0.0, 1.0]) for c in range(8)]
    cons = list(range(8))
    for h in range(50):
        s, complete = R.sample(7, h, obs, cons)
        assert complete and len(set(s)) == 4 and s[0] == cons[S.draw(7, h, 0) % 8]
        assert not S.sample(7, h, obs, cons)[1]


# ---------------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------------
# the pose error of the restatement against the truth (max |dR_ij|, |dt| in m), read from the restatement alone; the pass mark of
# the library is ten times the reading
READ_THIN = {16: (1.49e-4, 1.95e-3), 8: (2.80e-4, 2.34e-3)}
READ_SEEDED = {1: (2.37e-4, 1.56e-3), 4: (2.65e-4, 1.12e-3), 8: (2.34e-4, 1.02e-3)}


def scene_checks(mc, lm, scenes, kind, ncams, read):
    cams, truth, obs, match, moved, ref = scenes[kind, ncams]
    cons = S.consensus(obs, match)[0]
    assert 0.3 < sum(moved[i] for i in cons) / len(cons) < 0.5
    assert ref["status"] == S.OK
    assert all(ref["flags"][i] == (not moved[i]) for i in cons) and ref["n_inliers"] == sum(not moved[i] for i in cons)
    clean = sum(1 for s, m in zip(ref["samples"], ref["models"]) if m is not None and not any(moved[i] for i in s))
    err = SC.pose_error((ref["R"], ref["t"]), truth)
    print("restatement, %s, %d cameras: %d models, %d clean hypotheses, %.3g in R, %.3g m" % (kind, ncams, ref["n_models"], clean, err[0], err[1]))
    assert clean >= 3
    assert err[0] <= read[0] and err[1] <= read[1]
    for form in ("pts", "lids"):
        got = RC.run(mc, lm, cams, obs, match=match, form=form)
        SC.same_plain(got, ref, "%s scene, %d cameras, %s" % (kind, ncams, form))
        err = SC.pose_error((got.R.tolist(), got.t.tolist()), truth)
        assert err[0] <= 10 * read[0] and err[1] <= 10 * read[1]
    return cams, obs, match, cons, ref


@pytest.mark.parametrize("ncams", [16, 8])
def test_thin_scene(mc, lm, scenes, ncams):
    """ncams x 3 observations, no camera with four (RC.thin_scene, seed 3: the first tried), 40 % moved by 50 px, 100
    hypotheses, the reference's threshold at 640.  The central solver answers NO_MODEL.  On the restatement alone the rig
    solver's winner has exactly the unmoved observations as inliers and at least three hypotheses sampled no moved observation
    (read: 10 and 12); the library equals the restatement on the bits and passes at ten times the error the restatement reads"""
    cams, obs, match, cons, ref = scene_checks(mc, lm, scenes, "thin", ncams, READ_THIN[ncams])
    assert len(cons) == 3 * ncams and max(sum(1 for o in obs if o[0] == c) for c in range(ncams)) == 3
    got = RC.run(mc, lm, cams, obs, "central", match=match)
    assert got.status == S.NO_MODEL and got.n_models == 0 and got.best_hypothesis == -1 and not got.inliers.any()


@pytest.mark.parametrize("ncams", [1, 4, 8])
def test_seeded_scene(mc, lm, scenes, ncams):
    """section 9i's seeded scenes (200 landmarks, 40 % moved) with the rig solver, checked as test_sac_cpu.py checks them with the
    central one (read: 9, 9 and 18 hypotheses that sampled no moved observation); the samples of the 4- and 8-camera rigs do
    span cameras"""
    cams, obs, match, cons, ref = scene_checks(mc, lm, scenes, "seeded", ncams, READ_SEEDED[ncams])
    assert len(cons) == 200
    spans = sum(1 for s in ref["samples"] if len(set(obs[i][0] for i in s)) > 1)
    assert spans == 0 if ncams == 1 else spans > 50


def test_more_than_one_root_survives(mc, scenes):
    """the pick by the fourth point is exercised: among the scenes' hypotheses at least one has two or more surviving roots, and
    in at least one of those the pick is not the first root"""
    many, later = 0, 0
    for cams, truth, obs, match, moved, ref in scenes.values():
        solve = RC.solver_of(mc, cams)
        for s in ref["samples"]:
            cand = R.candidates(cams, obs, s, solve)
            if len(cand) >= 2:
                many += 1
                pick = R.model(cams, obs, s, solve)
                later += 0 if P.same_bits(pick[0], cand[0][0][0]) and P.same_bits(pick[1], cand[0][0][1]) else 1
    print("%d hypotheses with two or more roots, the pick is a later root in %d" % (many, later))
    assert many >= 1 and later >= 1


@pytest.mark.parametrize("per_match", [1, 2, 16])
def test_match_forms(mc, lm, per_match):
    """1, 2 and 16 observations per match: the consensus set is the first of each, the flags are per match"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=40, seed=7, per_match=per_match)
    ref = check(mc, lm, cams, obs, "%d per match" % per_match, match=match)
    nm = match[-1] + 1
    assert ref["n_consensus"] == nm and len(obs) >= nm * per_match and ref["status"] == S.OK
    assert all(i in S.consensus(obs, match)[0] for s in ref["samples"] for i in s)
    if per_match == 1:
        own = check(mc, lm, cams, obs, "no match array", match=None)
        assert own["n_consensus"] == len(obs) >= nm
    SC.same_plain(RC.run(mc, lm, cams, obs, match=[3 * k + 5 for k in match]), ref, "sparse match indices")


@pytest.mark.parametrize("kind, ncams", [("thin", 16), ("seeded", 4)])
def test_with_refinement(mc, lm, scenes, kind, ncams):
    """the defining property: the refinement part is mcorb_lmap_refine_pose called explicitly on the same observations from the
    returned RANSAC pose, bit for bit, and the rule of :4786 is the restatement's"""
    cams, truth, obs, match, moved, sac = scenes[kind, ncams]
    _, ref, final = R.ransac_refine(cams, obs, SC.THRESHOLD, RC.solver_of(mc, cams), PC.INV_SIGMA2, match, 100, 0)
    got = RC.run(mc, lm, cams, obs, match=match, refine=(PC.INV_SIGMA2,))
    SC.same(got, sac, "with refinement")
    SC.same_final(got, final, "with refinement")
    explicit = PC.refine(mc, lm, cams, (got.sac_R.tolist(), got.sac_t.tolist()), obs)
    for f in ("R", "t", "cost_initial", "cost_final"):
        assert P.same_bits(np.asarray(getattr(got.refine, f)).tolist(), np.asarray(getattr(explicit, f)).tolist()), f
    assert (got.refine.status, got.refine.iterations, got.refine.n_inliers, got.refine.n_obs) == \
        (explicit.status, explicit.iterations, explicit.n_inliers, explicit.n_obs)
    PC.same(dict(PC.as_ref(explicit)), ref, "the restatement's refinement")
    if got.used:
        assert P.same_bits(got.R.tolist(), explicit.R.tolist()) and P.same_bits(got.t.tolist(), explicit.t.tolist())
    else:
        assert P.same_bits(got.R.tolist(), got.sac_R.tolist())
    assert kind == "thin" or got.used == 1


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def check_refusals(mc, lm):
    """a solver that is none: MCORB_E_ARG before anything runs, the store read back unchanged; a pending tracking call; then both
    solvers still run"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=20, seed=7, per_match=2)
    lids = PC.fill_points(lm, obs)
    before = [(p.tobytes(), q.tobytes()) for p, q, _, _ in (lm.get(int(l)) for l in lids)]
    cam, uv, octave, pts = PC.arrays(obs)
    cc = PC.to_cams(mc, cams)

    def unchanged():
        return [(p.tobytes(), q.tobytes()) for p, q, _, _ in (lm.get(int(l)) for l in lids)] == before

    for bad in (-1, 2):
        with pytest.raises(mc.McorbError) as e:
            lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match, solver=bad)
        assert e.value.code == mc.E_ARG and unchanged(), bad
        # and through the C entry
        res, par = mc._lib.SacResultC(), mc._lib.SacParams()
        par.threshold, par.max_iterations, par.solver = SC.THRESHOLD, 100, bad
        code = lm.L.mcorb_lmap_ransac_pose(lm.h, len(cam), cam.ctypes.data, uv.ctypes.data, octave.ctypes.data, None, lids.ctypes.data, None,
                                           len(cams), C.addressof(cc.cams), C.byref(par), None, C.byref(res), None)
        assert code == mc.E_ARG and unchanged(), bad
    with pytest.raises(KeyError):
        lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match, solver="gp3p")
    assert C.sizeof(mc._lib.SacParams) == 24 and mc._lib.SacParams.solver.offset == 20
    # the other refusals hold with the rig solver as they do without
    with pytest.raises(mc.McorbError) as e:
        lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match, solver="rig", max_iterations=1025)
    assert e.value.code == mc.E_ARG and unchanged()
    # while a tracking call is pending: MCORB_E_STATE, as for the central solver
    lm.track_submit(T.to_view(mc, T.flat_view()), [np.zeros((0, 2), np.float32)], [np.zeros((0, 32), np.uint8)], [])
    with pytest.raises(mc.McorbError) as e:
        lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match, solver="rig")
    assert e.value.code == mc.E_STATE
    lm.track_wait()
    assert unchanged()
    SC.same_plain(lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match, solver="rig"),
                  R.ransac(cams, obs, SC.THRESHOLD, RC.solver_of(mc, cams), match, 100, 0), "rig, after the refusals")
    SC.same_plain(lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match),
                  S.ransac(cams, obs, SC.THRESHOLD, SC.solver_of(mc, cams), match, 100, 0), "central, after the refusals")
    assert unchanged()


def test_refusals(mc, lm):
    check_refusals(mc, lm)


# ---------------------------------------------------------------------------------------------------------------------------
# the header's host path as a stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_under_asan_ubsan(mc, lm, scenes, tmp_path):
    """tests/cpp/test_sac_rig_sanitize.cpp (its own main, -fsanitize=address,undefined) runs sac_run_serial with the rig solver on
    the 16 x 3 scene: no report, and every record -- the pick, the flags, and the model, sample and count of each of the 100
    hypotheses -- equals the library's result and the restatement"""
    cams, truth, obs, match, moved, ref = scenes["thin", 16]
    exe = str(tmp_path / "test_sac_rig_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_sac_rig_sanitize.cpp"),
                           "-o", exe])
    cons = S.consensus(obs, match)[0]
    n, Sn, H, ncams = len(obs), len(cons), 100, len(cams)
    blob = struct.pack("<4idQ", ncams, n, Sn, H, SC.THRESHOLD, 0)
    for c in cams:
        blob += struct.pack("<17d", *[v for row in c["R"] for v in row], *c["t"], c["fx"], c["fy"], c["s"], c["u0"], c["v0"])
    blob += b"".join(struct.pack("<2f2i", o[1], o[2], o[0], o[3]) for o in obs)
    blob += b"".join(struct.pack("<3d", *o[4]) for o in obs)
    blob += struct.pack("<%di" % Sn, *cons)
    (tmp_path / "in.bin").write_bytes(blob)
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bad=0" in out.stdout and not out.stderr, out.stdout + out.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == 128 + n + 4 * H + 128 * H
    R_, t_ = struct.unpack("<9d", raw[:72]), struct.unpack("<3d", raw[72:96])
    status, n_in, best, n_models, *sample = struct.unpack("<8i", raw[96:128])
    flags = list(raw[128:128 + n])
    counts = struct.unpack("<%di" % H, raw[128 + n:128 + n + 4 * H])
    got = RC.run(mc, lm, cams, obs, match=match)
    assert struct.pack("<9d", *got.sac_R.reshape(9)) == raw[:72] and struct.pack("<3d", *got.sac_t) == raw[72:96]
    assert (status, n_in, best, n_models, tuple(sample)) == (got.status, got.sac_n_inliers, got.best_hypothesis, got.n_models, got.sample)
    assert [bool(flags[i]) for i in cons] == got.inliers.tolist() and flags == [int(v) for v in ref["flags"]]
    assert P.same_bits([list(R_[0:3]), list(R_[3:6]), list(R_[6:9])], ref["R"]) and P.same_bits(list(t_), ref["t"])
    lib_count, lib_valid = lm.last_ransac_counts()
    for h in range(H):
        rec = raw[128 + n + 4 * H + 128 * h:128 + n + 4 * H + 128 * (h + 1)]
        valid, *smp = struct.unpack("<5i", rec[96:116])
        assert smp == ref["samples"][h] and bool(valid) == (ref["models"][h] is not None) == bool(lib_valid[h]), h
        assert counts[h] == lib_count[h], h
        if valid:
            assert counts[h] == ref["counts"][h], h
            m = struct.unpack("<12d", rec[:96])
            assert P.same_bits([list(m[0:3]), list(m[3:6]), list(m[6:9])], ref["models"][h][0]) and P.same_bits(list(m[9:12]), ref["models"][h][1]), h
