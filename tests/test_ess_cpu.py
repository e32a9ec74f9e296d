"""The pose of one camera between two frames by five-point RANSAC on the host-only store (device -1):
mcorb_lmap_essential_pose against the restatement (ess_ref.py) and against answers written out by hand.  Bit for bit, floats as
raw bytes, but for the comparisons of the solver and of the decomposition with numpy's, which state their tolerances.  No GPU.

On the commit before this call existed every test of this file fails (`python -m pytest tests/test_ess_cpu.py`): LocalMap has
no essential_pose."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import ess_cases as EC
import ess_ref as ER
import init_cases as Ic
import kfdb_cases as K
import pose_cases as PC
import rel_ref as RR
import track_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb.LocalMap, "essential_pose")
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture()
def lm(mc, voc):
    return mc.LocalMap(voc, device=-1, max_landmarks=4096, max_candidates=1024)


# the seeds EC.first_seed finds, recorded
SEED = {("general", 0.0): 1, ("general", 0.1): 1, ("coplanar", 0.0): 2, ("coplanar", 0.1): 0, ("forward", 0.0): 2, ("forward", 0.1): 0}
H = 500


@pytest.fixture(scope="module")
def scenes(mc):
    """the seeded scenes, noise-free and with N(0, 0.1 px), and their restatements at 500 hypotheses, computed once"""
    out = {}
    for key, seed in SEED.items():
        truth, matches, moved = EC.scene(key[0], seed=seed, noise=key[1])
        out[key] = (truth, matches, moved, ER.ransac(EC.CAM, matches, EC.solver_of(mc), max_iterations=H))
    return out


def check(mc, lm, matches, what, **kw):
    ref = ER.ransac(EC.CAM, matches, EC.solver_of(mc), **kw)
    EC.same(EC.run(mc, lm, matches, **kw), ref, what)
    if ref["status"] != ER.NO_OBS:
        EC.same_counts(lm, ref, what)
    return ref


def split(five):
    return [m[0:2] for m in five], [m[2:4] for m in five]


# ---------------------------------------------------------------------------------------------------------------------------
# the five-point solver (comparisons with a tolerance)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["general", "coplanar"])
def test_solver_recovers_the_generating_matrix(mc, kind):
    """2 000 seeded noise-free samples per kind (EC.solver_cases).  A sample is included iff the numpy solver alone (SVD null space,
    numpy.linalg.det, numpy.roots, lstsq) has the true E, up to sign and with |E|_F^2 = 2, among its models to 1e-8 (max |dE_ij|); at
    most 5 % may be left out.  On every included sample mcorb_ess_solve has it to 1e-6.
    Measured: 2 and 24 of 2 000 left out (0.1 %, 1.2 %); worst error of mcorb_ess_solve on the included ones 2.2e-11 and 5.6e-11.
    (With the determinant's polynomial taken at the 11 nodes in [-2, 2] only, without the second pass at the scale of the roots,
    one general sample whose ten roots all lie within 0.2 of zero had no model at all.)"""
    cases = EC.solver_cases(kind)
    assert len(cases) == 2000
    cc = EC.to_cam(mc)
    left, worst = 0, 0.0
    for (R, t), five in cases:
        E = ER.true_E(R, t)
        if not ER.E_distance(ER.numpy_solve5(EC.CAM, five), E) <= 1e-8:
            left += 1
            continue
        d = ER.E_distance(mc.ess_solve(cc, *split(five)), E)
        worst = max(worst, d)
        assert d <= 1e-6, (d, five)
    print("%s: left out %d of %d, worst error %.3g" % (kind, left, len(cases), worst))
    assert left <= 0.05 * len(cases)


def test_models_satisfy_their_sample_and_the_cubics(mc):
    """every model of the hook: |E|_F^2 = 2, its five rows d1^T E d2 and its ten cubics (2 E E^T E - tr(E E^T) E, det E) below the
    header's 1e-9, evaluated here with numpy; the roots come in ascending z; at most 10 models"""
    cc = EC.to_cam(mc)
    n_models = 0
    for kind in ("general", "coplanar"):
        for _, five in EC.solver_cases(kind)[:300]:
            models, z = mc.ess_solve(cc, *split(five), with_roots=True)
            assert len(models) <= 10 and z == sorted(z) and len(set(z)) == len(z)
            d1 = np.array([ER.bearing(*ER.normalise(EC.CAM, m[0], m[1])) for m in five])
            d2 = np.array([ER.bearing(*ER.normalise(EC.CAM, m[2], m[3])) for m in five])
            for E in models:
                n_models += 1
                assert abs((E * E).sum() - 2.0) <= 1e-12
                assert np.abs(np.einsum("ia,ab,ib->i", d1, E, d2)).max() < 1e-9
                assert np.abs(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E).max() < 1e-9 and abs(np.linalg.det(E)) < 1e-9
    assert n_models >= 600 * 2


def test_a_nan_keypoint_has_no_model(mc):
    cc = EC.to_cam(mc)
    _, five = EC.solver_cases("general")[0]
    assert len(mc.ess_solve(cc, *split(five))) >= 1
    for j in range(5):
        for k in range(4):
            bad = [list(m) for m in five]
            bad[j][k] = float("nan")
            assert mc.ess_solve(cc, *split(bad)) == []
    # five times the same match: the rows have rank 1, no finite model
    assert mc.ess_solve(cc, *split([five[0]] * 5)) == []


def test_decompose_contains_the_generating_pose(mc):
    """on an exact [t]x R of any scale the four candidates contain (R, t / |t|) to 1e-12, are rotations to 1e-12, and are, as a
    set, numpy's four from the SVD of E to 1e-9; the hook equals the restatement on the bits"""
    rng = np.random.default_rng(4)
    for k in range(200):
        R, t = EC.random_pose(rng, forward=k % 5 == 0)
        E = ER.true_E(R, t) * rng.uniform(0.1, 10.0) * (1 if k % 2 else -1)
        Rp, Rm, th = mc.ess_decompose(E)
        ref = ER.decompose([float(v) for v in E.reshape(9)])
        assert EC.pack(Rp.reshape(9)) == EC.pack(ref[0]) and EC.pack(Rm.reshape(9)) == EC.pack(ref[1]) and EC.pack(th) == EC.pack(ref[2])
        cands = [(Rp, th), (Rm, th), (Rp, -th), (Rm, -th)]
        assert min(max(np.abs(Rc - R).max(), np.abs(tc - t / np.linalg.norm(t)).max()) for Rc, tc in cands) <= 1e-12
        for Rc in (Rp, Rm):
            assert np.abs(Rc @ Rc.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rc) - 1.0) <= 1e-12
        for Rn, tn in ER.numpy_decompose(E):
            assert min(max(np.abs(Rc - Rn).max(), np.abs(tc - tn).max()) for Rc, tc in cands) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------------------
# sampling, on the bits
# ---------------------------------------------------------------------------------------------------------------------------
def test_draws_and_walk():
    """the walk of section 9j's hand-worked example cut to 5 draws: the raw indices 3, 3, 3, 0, 0 of S = 20 pick 3; 4 (3 is taken);
    5 (3, 4 are taken); 0; 1 (0 is taken).  The draws are relative_pose's: the splitmix64 finaliser at 1 + 32 h + j"""
    assert RR.draw(0, 0, 0) == 0xE220A8397B1DCDAF
    assert RR.walk([3, 3, 3, 0, 0]) == [3, 4, 5, 0, 1]
    assert RR.walk([0] * 5) == list(range(5)) and RR.walk([4, 3, 2, 1, 0]) == [4, 3, 2, 1, 0]
    for n in (5, 6, 40, 1000):
        for h in range(50):
            s, ok = ER.sample(9, h, n)
            assert ok and len(set(s)) == 5 and all(0 <= i < n for i in s)
            assert s == RR.walk([RR.draw(9, h, j) % (n - j) for j in range(5)])
    assert ER.sample(9, 0, 4) == ([-1] * 5, False)


def test_none_four_five_and_six(mc, lm):
    """S = 0: NO_OBS.  S = 4: no hypothesis has a model.  S = 5: every hypothesis draws the same set in its own order; at a
    threshold far above the rounding every model of every hypothesis counts all five, and hypothesis 0's root 0 wins.  S = 6"""
    truth, matches, moved = EC.scene("general", n=6, seed=3, moved=0.0)
    ref = check(mc, lm, [], "S = 0")
    assert ref["status"] == ER.NO_OBS
    got = EC.run(mc, lm, [])
    assert got.status == ER.NO_OBS and got.n_matches == 0 and len(got.inliers) == 0 and got.R.tolist() == ER.IDENT and got.sample == (-1,) * 5
    ref = check(mc, lm, matches[:4], "S = 4", max_iterations=20)
    assert ref["status"] == ER.NO_MODEL and ref["n_models"] == 0 and ref["samples"][3] == [-1] * 5
    got = EC.run(mc, lm, matches[:4], max_iterations=20)
    assert got.R.tolist() == ER.IDENT and got.t.tolist() == [0.0] * 3 and not got.inliers.any() and len(got.inliers) == 4
    assert (got.best_hypothesis, got.best_root, got.n_inliers, got.n_ransac_inliers, got.cheirality) == (-1, -1, 0, 0, (0, 0, 0, 0))
    ref = check(mc, lm, matches[:5], "S = 5", max_iterations=40)
    assert all(sorted(s) == list(range(5)) for s in ref["samples"]) and len(set(tuple(s) for s in ref["samples"])) > 1
    assert ref["status"] == ER.OK and (ref["best"], ref["root"]) == (0, 0) and ref["n_ransac_inliers"] == 5
    assert all(c == 5 for c, v in zip(ref["counts"], ref["valid"]) if v) and ref["n_models"] >= 40
    ref = check(mc, lm, matches, "S = 6", max_iterations=40)
    assert ref["status"] == ER.OK and ref["n_ransac_inliers"] == 6 and ER.pose_error((ref["R"], ref["t"]), truth)[0] < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
# the gates: the Sampson threshold, the depths of the vote
# ---------------------------------------------------------------------------------------------------------------------------
def gate_rows(mc):
    """-> (matches, model E as 9, k, its Sampson value): 40 matches with N(0, 0.1 px), one hypothesis; k is a match outside the
    sample whose value some threshold_px reaches exactly (a square reaches about every other double)"""
    truth, matches, moved = EC.scene("general", n=40, seed=11, moved=0.0, noise=0.1)
    ref = ER.ransac(EC.CAM, matches, EC.solver_of(mc), max_iterations=1)
    assert ref["status"] == ER.OK
    for k in range(40):
        s = ER.sampson(ref["E"], ER.point(EC.CAM, matches[k]))
        if k in ref["sample"] or not 1e-12 < s < 1e-4:
            continue
        try:
            px = Ic.solve(lambda v: ER.threshold2(EC.CAM, v), 1e-6, 100.0, s)
        except AssertionError:
            continue
        return matches, ref["E"], k, s, px
    raise AssertionError("no match's value is a threshold's square")


def test_score_forms_agree(mc, scenes):
    """the restatement's vector form and the mcorb_ess_eval hook equal its scalar form on the bits, at the winner and at the truth"""
    truth, matches, moved, ref = scenes[("general", 0.1)]
    pts = [ER.point(EC.CAM, m) for m in matches]
    cols = tuple(np.array([p[k] for p in pts]) for k in range(4))
    uv1, uv2 = [m[0:2] for m in matches], [m[2:4] for m in matches]
    for E in (ref["E"], [float(v) for v in ER.true_E(*truth).reshape(9)]):
        many, hook = ER.sampson_many(E, cols), mc.ess_eval(EC.to_cam(mc), E, uv1, uv2)
        for i, p in enumerate(pts):
            assert ER.bits(float(many[i])) == ER.bits(ER.sampson(E, p)) == ER.bits(float(hook[i])), i


def test_threshold_is_strict_and_nan_is_no_inlier(mc, lm):
    matches, E, k, s, px = gate_rows(mc)
    assert ER.threshold2(EC.CAM, px) == s
    hook = mc.ess_eval(EC.to_cam(mc), E, [m[0:2] for m in matches], [m[2:4] for m in matches])
    assert ER.bits(float(hook[k])) == ER.bits(s)
    at = check(mc, lm, matches, "threshold = the value", threshold_px=px, max_iterations=1)
    above = check(mc, lm, matches, "the next double", threshold_px=math.nextafter(px, math.inf), max_iterations=1)
    assert not at["ransac_inliers"][k] and above["ransac_inliers"][k] and above["n_ransac_inliers"] == at["n_ransac_inliers"] + 1
    # a NaN row: no inlier at any threshold, and no model for a hypothesis that draws it
    matches[7] = (matches[7][0], float("nan"), matches[7][2], matches[7][3])
    wide = check(mc, lm, matches, "a NaN row", threshold_px=1e4, max_iterations=60)
    assert wide["status"] == ER.OK and not wide["ransac_inliers"][7] and wide["n_ransac_inliers"] == 39
    drew = [h for h, smp in enumerate(wide["samples"]) if 7 in smp]
    assert len(drew) >= 3 and all(wide["roots"][h] == 0 for h in drew)


def test_distance_is_strict_in_either_camera(mc, lm, scenes):
    """distance_thresh equal to an inlier's depth in camera 1, then in camera 2: the match is out; at the next double above it is
    in; one call each, against the restatement on the bits"""
    truth, matches, moved, ref = scenes[("general", 0.1)]
    assert ref["status"] == ER.OK
    R, t = ER.candidate(ref["cands"], ref["winner"])
    z = [ER.depths(R, t, ER.point(EC.CAM, m)) for m in matches]
    (cands, depth) = mc.ess_decompose(ref["E"], EC.to_cam(mc), [m[0:2] for m in matches], [m[2:4] for m in matches])
    for i in range(len(matches)):
        assert (ER.bits(float(depth[i, ref["winner"], 0])), ER.bits(float(depth[i, ref["winner"], 1]))) == (ER.bits(z[i][0]), ER.bits(z[i][1]))
    for cam in (0, 1):
        k = max((i for i in range(len(matches)) if ref["inliers"][i] and z[i][cam] > z[i][1 - cam]), key=lambda i: z[i][cam])
        d = z[k][cam]
        at = check(mc, lm, matches, "distance = the depth", distance=d, max_iterations=H)
        above = check(mc, lm, matches, "the next double", distance=math.nextafter(d, math.inf), max_iterations=H)
        assert not at["inliers"][k] and above["inliers"][k] and at["ransac_inliers"][k]
        assert above["n_inliers"] == at["n_inliers"] + 1 and above["n_ransac_inliers"] == at["n_ransac_inliers"] == ref["n_ransac_inliers"]


def test_depth_zero_is_out_in_either_camera(mc):
    """a match that crosses the plane z = 0 of a camera.  Camera 1: with R = I and t = (0.6, 0, -0.8) camera 1's centre is seen by
    camera 2 at u = 266.5; a frame-2 keypoint that moves along the row through that point takes the midpoint through camera 1's
    centre and its depth there through zero.  Camera 2: with t = (0.6, 0, 0.8) camera 2's centre is seen by camera 1 at u = 1016.5
    and the frame-1 keypoint moves.  The two neighbouring doubles of the keypoint between which the depth changes sign are found
    by bisection; the hook's depths equal the restatement's on the bits on both sides, the other camera's depth is positive on
    both, and the side whose depth is not > 0 fails the test"""
    cc = EC.to_cam(mc)
    v = EC.CAM["v0"]
    for cam, t, lo, hi in ((0, np.array([0.6, 0.0, -0.8]), 260.0, 270.0), (1, np.array([0.6, 0.0, 0.8]), 1010.0, 1020.0)):
        E = [float(w) for w in ER.true_E(np.eye(3), t).reshape(9)]
        cands = ER.decompose(E)
        c = next(k for k in range(4) if max(ER.pose_error(ER.candidate(cands, k), (np.eye(3), t))) < 1e-12)
        Rc, tc = ER.candidate(cands, c)

        def match(u):
            return (641.5 + 50.0, v, u, v) if cam == 0 else (u, v, 641.5 - 50.0, v)

        def z_of(u):
            return ER.depths(Rc, tc, ER.point(EC.CAM, match(u)))

        pos = z_of(lo)[cam] > 0.0
        assert pos != (z_of(hi)[cam] > 0.0)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid in (lo, hi):
                break
            if (z_of(mid)[cam] > 0.0) == pos:
                lo = mid
            else:
                hi = mid
        assert hi == math.nextafter(lo, math.inf)
        for u in (lo, hi):
            m = match(u)
            (_, depth) = mc.ess_decompose(E, cc, [m[0:2]], [m[2:4]])
            zr = z_of(u)
            assert (ER.bits(float(depth[0, c, 0])), ER.bits(float(depth[0, c, 1]))) == (ER.bits(zr[0]), ER.bits(zr[1]))
            assert 0.0 < zr[1 - cam] < 50.0 and abs(zr[cam]) < 1e-9
        assert ER.in_front(z_of(lo), 50.0) == pos and ER.in_front(z_of(hi), 50.0) == (not pos)
    assert not ER.in_front((0.0, 1.0), 50.0) and not ER.in_front((1.0, 0.0), 50.0) and not ER.in_front((float("nan"), 1.0), 50.0)


def test_a_cheirality_tie_goes_to_the_lowest_candidate(mc, lm, scenes):
    """a distance below every depth: all four counts are 0, candidate 0 = (R+, t^) wins, no flag is set and the status is still OK"""
    truth, matches, moved, ref = scenes[("general", 0.1)]
    tie = check(mc, lm, matches, "a tie of four zeros", distance=1e-3, max_iterations=H)
    assert tie["status"] == ER.OK and tie["cheirality"] == [0, 0, 0, 0] and tie["winner"] == 0 and tie["n_inliers"] == 0
    assert tie["n_ransac_inliers"] == ref["n_ransac_inliers"] and not any(tie["inliers"])
    assert EC.pack(tie["R"]) == EC.pack(tie["cands"][0]) and EC.pack(tie["t"]) == EC.pack(tie["cands"][2])
    assert ER.key(7, 3, 2) > ER.key(7, 3, 3) > ER.key(7, 4, 0) > ER.key(6, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded scenes
# ---------------------------------------------------------------------------------------------------------------------------
# the pose error of the restatement against the truth with N(0, 0.1 px) (max |dR_ij|, |dt^|), read from the restatement alone; the
# library's pass mark is ten times the reading
READ = {"general": (6.54e-4, 9.62e-3), "coplanar": (1.48e-3, 9.99e-3), "forward": (1.59e-3, 1.22e-2)}
# noise-free: the keypoints are rounded to float, 6e-5 px at 1 000 px or 1.2e-7 on the normalised points; the five-point problem
# of these scenes amplifies that by up to 1e3
EXACT = 1e-4


def test_first_seeds_are_recorded():
    for (kind, noise), seed in SEED.items():
        assert EC.first_seed(kind, noise) == seed, (kind, noise)


@pytest.mark.parametrize("kind", EC.KINDS)
def test_seeded_scene_noise_free(mc, lm, scenes, kind):
    """one camera, 200 matches, 10 % moved by 50 px in frame 2, 500 hypotheses, threshold_px = 1, keypoints rounded to float and
    nothing else.  On the restatement alone: no moved match is an inlier at the true pose, no gate quantity lies within 1e-6
    relative of its gate, the returned inliers are exactly the unmoved matches and the pose is the truth with t normalised.
    Then the library equals the restatement on the bits"""
    truth, matches, moved, ref = scenes[(kind, 0.0)]
    assert len(matches) == 200 and 10 <= sum(moved) <= 30
    inl, near = EC.near_gate(truth, matches)
    assert not near and not any(i and mv for i, mv in zip(inl, moved))
    assert ref["status"] == ER.OK and ref["inliers"] == [not v for v in moved] and ref["n_inliers"] == 200 - sum(moved)
    err = ER.pose_error((ref["R"], ref["t"]), truth)
    print("restatement, %s, noise-free: %.3g in R, %.3g in t^" % (kind, err[0], err[1]))
    assert err[0] <= EXACT and err[1] <= EXACT
    EC.same(EC.run(mc, lm, matches, max_iterations=H), ref, kind)
    EC.same_counts(lm, ref, kind)


@pytest.mark.parametrize("kind", EC.KINDS)
def test_seeded_scene_with_noise(mc, lm, scenes, kind):
    """the same with N(0, 0.1 px) on every keypoint: at least 95 % of the unmoved matches are inliers and no moved match is.  The
    library equals the restatement on the bits and passes at ten times the errors the restatement reads.  The coplanar scene (nine
    points in ten on one plane) returns OK with the right pose, which a linear eight-point solver cannot"""
    truth, matches, moved, ref = scenes[(kind, 0.1)]
    inl, near = EC.near_gate(truth, matches)
    assert not near and not any(i and mv for i, mv in zip(inl, moved))
    unmoved = [i for i, v in enumerate(moved) if not v]
    assert ref["status"] == ER.OK
    assert sum(ref["inliers"][i] for i in unmoved) >= 0.95 * len(unmoved) and not any(ref["inliers"][i] for i, v in enumerate(moved) if v)
    err = ER.pose_error((ref["R"], ref["t"]), truth)
    print("restatement, %s, 0.1 px: %d of %d unmoved, %.3g in R, %.3g in t^" % (kind, sum(ref["inliers"][i] for i in unmoved), len(unmoved),
                                                                               err[0], err[1]))
    assert err[0] <= READ[kind][0] and err[1] <= READ[kind][1]
    got = EC.run(mc, lm, matches, max_iterations=H)
    EC.same(got, ref, kind)
    EC.same_counts(lm, ref, kind)
    err = ER.pose_error((got.R, got.t), truth)
    assert got.status == mc.ESS_OK and err[0] <= 10 * READ[kind][0] and err[1] <= 10 * READ[kind][1]


# ---------------------------------------------------------------------------------------------------------------------------
# the bootstrap of a one-camera rig, end to end
# ---------------------------------------------------------------------------------------------------------------------------
def bootstrap(mc, lm):
    """essential_pose on the mono matches of init_cases' one-camera scene, its (R, t) and flags into initialize"""
    sc = Ic.scene(1)
    cam = mc.pose_cams([np.eye(3)], [np.zeros(3)], [sc["K"][0]])

    def kp(frame, feat):
        r = frame["kps"][0][frame["match_index"][feat][0]]
        return (r["x"], r["y"])

    uv1 = np.array([kp(sc["prev"], q) for q, _ in sc["matches"]], np.float32)
    uv2 = np.array([kp(sc["cur"], t) for _, t in sc["matches"]], np.float32)
    ess = lm.essential_pose(cam, uv1, uv2, threshold_px=1.0, max_iterations=H)
    assert ess.status == mc.ESS_OK and abs(np.linalg.norm(ess.t) - 1.0) <= 1e-12
    err = ER.pose_error((ess.R, ess.t), (sc["R"], sc["t"]))
    assert err[0] <= EXACT and err[1] <= EXACT
    got = Ic.run_scene(mc, lm, dict(sc, R=ess.R, t=ess.t, flags=ess.inliers & sc["flags"]))
    assert got.status == mc.INIT_DONE and got.scaled and got.n_triangulated > 50
    acc = got.new_lid >= 0
    depth = sorted(got.dist2[acc].tolist())[int(acc.sum()) // 2]
    assert depth == got.median_scene_depth and depth * (1.0 / got.median_scene_depth) == 1.0
    assert abs(np.linalg.norm(got.t_out) * got.median_scene_depth - 1.0) <= 1e-12
    return ess, got


def test_bootstrap_end_to_end(mc, lm):
    bootstrap(mc, lm)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def read_back(lm, lids):
    return [(p.tobytes(), q.tobytes()) for p, q, _, _ in (lm.get(int(l)) for l in lids)]


def check_refusals(mc, lm):
    truth, matches, moved = EC.scene("general", n=30, seed=2)
    lids = np.arange(10, 40, dtype=np.int32)
    pts = np.random.default_rng(1).normal(size=(30, 3))
    lm.set(lids, pts, np.zeros_like(pts))
    before = read_back(lm, lids)
    uv1, uv2 = EC.arrays(matches)
    cc = EC.to_cam(mc)
    ref = ER.ransac(EC.CAM, matches, EC.solver_of(mc), max_iterations=100)

    def refused(code, pending=False, cam=cc, **kw):
        a = dict(uv1=uv1, uv2=uv2, threshold_px=1.0, distance_thresh=50.0, max_iterations=100)
        a.update(kw)
        with pytest.raises(mc.McorbError) as e:
            lm.essential_pose(cam, **a)
        assert e.value.code == code, (kw.keys(), e.value)
        assert pending or read_back(lm, lids) == before

    for bad in (0.0, -1e-7, float("nan"), float("inf")):
        refused(mc.E_ARG, threshold_px=bad)
        refused(mc.E_ARG, distance_thresh=bad)
        for name in ("fx", "fy"):
            refused(mc.E_ARG, cam=PC.to_cams(mc, [dict(EC.CAM, **{name: bad})]))
    refused(mc.E_ARG, max_iterations=0)
    refused(mc.E_ARG, max_iterations=mc.ESS_MAX_ITERATIONS + 1)
    # NULLs and a bad count, through the C entry
    res, par = mc._lib.EssResultC(), mc._lib.EssParams()
    par.threshold_px, par.distance_thresh, par.max_iterations = 1.0, 50.0, 100
    good = [lm.h, 30, uv1.ctypes.data, uv2.ctypes.data, C.addressof(cc.cams), C.byref(par), C.byref(res), None]
    for at, v in ((0, None), (2, None), (3, None), (4, None), (5, None), (6, None), (1, -1)):
        args = list(good)
        args[at] = v
        assert lm.L.mcorb_lmap_essential_pose(*args) == mc.E_ARG, at
    assert lm.L.mcorb_lmap_essential_pose(*good) == mc.OK     # (inlier may be NULL)
    ns = C.c_int(0)
    assert lm.L.mcorb_lmap_last_essential_counts(lm.h, None, None, None, 0, C.byref(ns)) == mc.E_CAP and ns.value == 1000
    assert read_back(lm, lids) == before
    # while a tracking call is pending
    v = T.to_view(mc, T.flat_view())
    lm.track_submit(v, [np.zeros((0, 2), np.float32)], [np.zeros((0, 32), np.uint8)], [])
    refused(mc.E_STATE, pending=True)
    lm.track_wait()
    assert read_back(lm, lids) == before
    # and it runs after all that
    EC.same(lm.essential_pose(cc, uv1, uv2, max_iterations=100), ref, "after the refusals")
    assert read_back(lm, lids) == before


def test_refusals(mc, lm):
    check_refusals(mc, lm)


# ---------------------------------------------------------------------------------------------------------------------------
# the header's host path as a stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_under_asan_ubsan(mc, lm, scenes, tmp_path):
    """tests/cpp/test_ess_sanitize.cpp (its own main, -fsanitize=address,undefined) runs ess_run_serial on the noisy general scene:
    no report, and every record -- the result, the flags, and the model, count and sample of each of the 5 000 slots and 500
    hypotheses -- equals the library's result and the restatement on the bytes"""
    truth, matches, moved, ref = scenes[("general", 0.1)]
    exe = str(tmp_path / "test_ess_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_ess_sanitize.cpp"),
                           "-o", exe])
    n = len(matches)
    blob = struct.pack("<2i7dQ", n, H, EC.CAM["fx"], EC.CAM["fy"], EC.CAM["s"], EC.CAM["u0"], EC.CAM["v0"], 1.0, 50.0, 0)
    blob += b"".join(struct.pack("<4f", *m) for m in matches)
    (tmp_path / "in.bin").write_bytes(blob)
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bad=0" in out.stdout and not out.stderr, out.stdout + out.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == 232 + n + 4 * 10 * H + 4 * 5 * H + 80 * 10 * H
    got = EC.run(mc, lm, matches, max_iterations=H)
    assert raw[:168] == got.R.tobytes() + got.t.tobytes() + got.E.tobytes() == EC.pack(ref["R"]) + EC.pack(ref["t"]) + EC.pack(ref["E"])
    status, n_ransac, n_in, best, root, *rest = struct.unpack("<16i", raw[168:232])
    assert (status, n_ransac, n_in, best, root) == (got.status, got.n_ransac_inliers, got.n_inliers, got.best_hypothesis, got.best_root)
    assert tuple(rest[0:5]) == got.sample and rest[5] == got.n_models == ref["n_models"] and tuple(rest[6:10]) == got.cheirality
    at = 232
    assert [bool(v) for v in raw[at:at + n]] == got.inliers.tolist() == ref["inliers"]
    at += n
    count, valid, models = lm.last_essential_counts()
    assert raw[at:at + 40 * H] == count.tobytes() == struct.pack("<%di" % (10 * H), *ref["counts"])
    at += 40 * H
    assert list(struct.unpack("<%di" % (5 * H), raw[at:at + 20 * H])) == [i for s in ref["samples"] for i in s]
    at += 20 * H
    for s in range(10 * H):
        rec = raw[at + 80 * s:at + 80 * (s + 1)]
        assert rec[:72] == models[s].tobytes() == EC.pack(ref["models"][s]) and struct.unpack("<i", rec[72:76])[0] == int(valid[s]) == int(ref["valid"][s]), s
