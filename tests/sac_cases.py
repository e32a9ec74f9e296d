"""Inputs and helpers of the RANSAC tests (test_sac_cpu.py, test_gpu_sac.py): the solver's seeded cases, outward-facing rigs, the
seeded scene with a known true pose, rows written out by hand, and the comparison of a LocalMap.ransac_pose result against the
restatement (sac_ref.py), floats as raw bytes with no tolerance."""
import math

import numpy as np

import pose_cases as PC
import pose_ref as P
import sac_ref as S
import track_cases as T

NAMES = {S.OK: "OK", S.NO_OBS: "NO_OBS", S.NO_MODEL: "NO_MODEL"}
K02 = 640.0
THRESHOLD = 1.0 - math.cos(math.atan(math.sqrt(2.0) * 0.5 / K02))     # the reference's expression at u0 = 640


def outward_rig(ncams):
    """ncams cameras facing outwards around the body's y axis, 0.2 m from its origin; fx = fy = 500, principal point (640, 360)"""
    cams = []
    for c in range(ncams):
        a = 2 * math.pi * c / ncams
        R_ = PC.rot([0.0, 1.0, 0.0], a)
        cams.append(T.cam(PC.rows_of(R_), [float(v) for v in R_ @ np.array([0.0, 0.0, 0.2])], fx=500.0, fy=500.0, u0=640.0, v0=360.0))
    return cams


def lists(pose):
    return PC.rows_of(pose[0]), [float(v) for v in np.asarray(pose[1]).reshape(3)]


def solver_of(mc, cams):
    """the `solve` argument of the restatement: mcorb_sac_solve on three observations of camera c"""
    cc = PC.to_cams(mc, cams)

    def solve(c, three):
        return [lists(p) for p in mc.sac_solve(cc, c, [[o[1], o[2]] for o in three], [o[4] for o in three])]
    return solve


def solver_cases(n=4000, seed=11):
    """-> [(cam, truth (R, t as numpy), uv: 3 x (u, v) floats, X: 3 x 3)]: rotations up to 3.1 rad about a random axis, translation
    N(0, 1) per axis, three points at depth 2 - 10 whose normalised coordinates lie within +-0.5 x +-0.4.  The keypoints are
    rounded to float first and the points are placed on their rays, so a case has no noise: the generating pose solves it to
    the last bits"""
    rng = np.random.default_rng(seed)
    cam = T.cam(PC.rows_of(PC.rot([0.2, 1.0, 0.1], 0.3)), (0.1, -0.05, 0.02), fx=500.0, fy=480.0, s=0.3, u0=640.0, v0=360.0)
    Rc, tc = np.asarray(cam["R"]), np.asarray(cam["t"])
    out = []
    for _ in range(n):
        Rwb, twb = PC.rot(rng.normal(size=3), rng.uniform(0, 3.1)), rng.normal(size=3)
        Rwc, twc = Rwb @ Rc, Rwb @ tc + twb
        uv, X = [], []
        for _k in range(3):
            x, y, z = rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), rng.uniform(2, 10)
            u, v = PC.f32(cam["fx"] * x + cam["s"] * y + cam["u0"]), PC.f32(cam["fy"] * y + cam["v0"])
            f = np.asarray(S.bearing(cam, u, v))
            X.append(Rwc @ (f / f[2] * z) + twc)
            uv.append((u, v))
        out.append((cam, (Rwb, twb), uv, np.array(X)))
    return out


def scene(ncams=4, nlm=200, seed=3, moved=0.4, noise=0.1, per_match=1):
    """-> (cams, truth, obs, match, is_moved): nlm landmarks at depth 2 - 10 around an outward-facing rig at the pose `truth`, each
    placed in the view of one camera and observed by every camera that has it in front and inside 1280 x 720; the projections
    are rounded to float after N(0, noise px) is added, and a fraction `moved` of the landmarks have their observations moved by
    50 px in a random direction.  A landmark is a match; per_match > 1 repeats its first observation (the further copies are
    outside the consensus set)"""
    rng = np.random.default_rng(seed)
    cams = outward_rig(ncams)
    Rt = PC.rot([0.3, -0.2, 1.0], 0.7)
    tt = np.array([1.5, -0.7, 0.3])
    truth = (PC.rows_of(Rt), [float(v) for v in tt])
    obs, match, is_moved = [], [], []
    k = 0
    for _ in range(nlm):
        c0 = int(rng.integers(ncams))
        z = rng.uniform(2, 10)
        q = np.array([rng.uniform(-1.2, 1.2) * z, rng.uniform(-0.68, 0.68) * z, z])
        pb = np.asarray(cams[c0]["R"]) @ q + np.asarray(cams[c0]["t"])
        X = [float(v) for v in Rt @ pb + tt]
        mv = rng.random() < moved
        seen = 0
        for c in range(ncams):
            qc = P.transform_to(cams[c]["R"], cams[c]["t"], P.transform_to(truth[0], truth[1], X))
            if qc[2] <= 0.5:
                continue
            px, py = PC.project(cams, truth, c, X)
            if not (0 <= px <= 1280 and 0 <= py <= 720):
                continue
            px, py = px + rng.normal(scale=noise), py + rng.normal(scale=noise)
            if mv:
                a = rng.uniform(0, 2 * math.pi)
                px, py = px + 50 * math.cos(a), py + 50 * math.sin(a)
            for _r in range(per_match if seen == 0 else 1):
                obs.append((c, PC.f32(px), PC.f32(py), int(rng.integers(4)), X))
                match.append(k)
                is_moved.append(mv)
            seen += 1
        k += 1 if seen else 0
    return cams, truth, obs, match, is_moved


def pose_error(pose, truth):
    """(max |dR_ij|, |dt| in m)"""
    return (float(np.max(np.abs(np.asarray(pose[0]) - np.asarray(truth[0])))),
            float(np.linalg.norm(np.asarray(pose[1]) - np.asarray(truth[1]))))


def run(mc, lm, cams, obs, threshold=THRESHOLD, match=None, max_iterations=100, seed=0, refine=None, form="pts", first_lid=0):
    """LocalMap.ransac_pose on the observations, points given (form "pts") or read from the store (form "lids")"""
    cam, uv, octave, pts = PC.arrays(obs)
    kw = dict(pts=pts) if form == "pts" else dict(lids=PC.fill_points(lm, obs, first_lid))
    return lm.ransac_pose(PC.to_cams(mc, cams), cam, uv, octave, threshold, match=match, max_iterations=max_iterations, seed=seed,
                          refine=None if refine is None else mc.pose_params(*refine), **kw)


def same(got, ref, what=""):
    """a SacResult's RANSAC part against sac_ref.ransac's dict"""
    assert got.status == ref["status"], (what, "status", NAMES[got.status], NAMES[ref["status"]])
    assert P.same_bits(got.sac_R.tolist(), ref["R"]) and P.same_bits(got.sac_t.tolist(), ref["t"]), (what, "model", got.sac_R, ref["R"])
    assert got.best_hypothesis == ref["best"], (what, "best", got.best_hypothesis, ref["best"])
    assert list(got.sample) == list(ref["sample"]), (what, "sample", got.sample, ref["sample"])
    assert got.sac_n_inliers == ref["n_inliers"], (what, "count", got.sac_n_inliers, ref["n_inliers"])
    assert got.n_models == ref["n_models"], (what, "n_models", got.n_models, ref["n_models"])
    assert got.n_consensus == ref["n_consensus"] and got.n_matches == ref["n_consensus"], (what, "n_consensus")


def same_final(got, final, what=""):
    assert got.used == final["used"], (what, "used", got.used, final["used"])
    assert P.same_bits(got.R.tolist(), final["R"]) and P.same_bits(got.t.tolist(), final["t"]), (what, "final pose")
    assert got.n_inliers == final["n_inliers"], (what, "n_inliers", got.n_inliers, final["n_inliers"])
    assert got.inliers.tolist() == [bool(v) for v in final["inliers"]], (what, "inliers")


def same_plain(got, ref, what=""):
    """without refinement: the answer is the RANSAC's"""
    same(got, ref, what)
    same_final(got, dict(used=0, R=ref["R"], t=ref["t"], n_inliers=ref["n_inliers"], inliers=ref["inliers"]), what)


# ---------------------------------------------------------------------------------------------------------------------------
# rows written out by hand: the flat rig (fx = fy = 1, identity), so a keypoint (x, y) has the bearing (x, y, 1) / |.|
# ---------------------------------------------------------------------------------------------------------------------------
def square(ncam=1, cam=0, z=4.0, octave=0):
    """four exact observations of one camera at the identity pose: points (x, y, 1) * z seen at (x, y)"""
    return [(cam, x, y, octave, [x * z, y * z, z]) for x, y in ((0.25, 0.125), (-0.25, 0.25), (0.125, -0.375), (-0.375, -0.125))]
