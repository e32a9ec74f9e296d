"""Inputs and helpers of the relative pose tests (test_rel_cpu.py, test_gpu_rel.py): the solver's seeded noise-free cases, the
seeded two-frame scene with a known true pose, rows written out by hand, and the comparison of a LocalMap.relative_pose result
against the restatement (rel_ref.py), floats as raw bytes with no tolerance.

A match is (cam1, u1, v1, cam2, u2, v2); a pose is (R, t) = b1_T_b2: X_b1 = R X_b2 + t."""
import math

import numpy as np

import pose_cases as PC
import pose_ref as P
import rel_ref as RR
import sac_cases as SC

NAMES = {RR.OK: "OK", RR.NO_OBS: "NO_OBS", RR.NO_MODEL: "NO_MODEL"}
K02 = 640.0
THRESHOLD = 2.0 * SC.THRESHOLD     # the reference's expression (FrontEnd.cpp:4604) at u0 = 640
W, H = 1280, 720

outward_rig = SC.outward_rig     # ncams cameras facing outwards, 0.2 m from the body's origin, fx = fy = 500, (640, 360)


def rig_arrays(cams):
    return (np.array([c["R"] for c in cams]), np.array([c["t"] for c in cams]), np.array([c["fx"] for c in cams]),
            np.array([c["fy"] for c in cams]), np.array([c["u0"] for c in cams]), np.array([c["v0"] for c in cams]))


def first_camera(rig, Xb):
    """-> (the first camera that has the body-frame point in front (z > 0.5) and inside the image, its projection in double) or
    None.  The rigs here have no skew"""
    Rc, tc, fx, fy, u0, v0 = rig
    q = np.einsum("cji,cj->ci", Rc, Xb[None, :] - tc)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * q[:, 0] / q[:, 2] + u0, fy * q[:, 1] / q[:, 2] + v0
    ok = (q[:, 2] > 0.5) & (u >= 0) & (u <= W) & (v >= 0) & (v <= H)
    c = int(np.argmax(ok))
    return (c, float(u[c]), float(v[c])) if ok[c] else None


def random_pose(rng, rot_sigma=0.1, t_sigma=0.3):
    w = rng.normal(scale=rot_sigma, size=3)
    return PC.rot(w, float(np.linalg.norm(w))), rng.normal(scale=t_sigma, size=3)


def exact_match(rng, cams, rig, R, t):
    """one noise-free match: a keypoint of a random camera of frame 1, rounded to float FIRST, the point put on its ray at depth
    2 - 10, and its projection in double into the first camera of frame 2 that sees it.  (Frame 2's keypoint stays a double: a
    point cannot lie on two rays through float keypoints at a given pose, and 6e-5 px of rounding at u = 640 is 1e-7 rad, far
    above the 1e-8 the solver is held to; the hooks take doubles for this reason)"""
    while True:
        c1 = int(rng.integers(len(cams)))
        u1, v1 = PC.f32(rng.uniform(40, W - 40)), PC.f32(rng.uniform(20, H - 20))
        f = np.asarray(RR.S.bearing(cams[c1], u1, v1))
        Xb1 = np.asarray(cams[c1]["R"]) @ (f / f[2] * rng.uniform(2, 10)) + np.asarray(cams[c1]["t"])
        seen = first_camera(rig, R.T @ (Xb1 - t))
        if seen is not None:
            return (c1, u1, v1) + seen


def solver_cases(ncams, n=4000, seed=17):
    """-> (cams, [(truth (R, t as numpy), 17 matches)]): rotation N(0, 0.1 rad) per axis, translation N(0, 0.3 m) per axis"""
    rng = np.random.default_rng(seed + ncams)
    cams = outward_rig(ncams)
    rig = rig_arrays(cams)
    out = []
    for _ in range(n):
        R, t = random_pose(rng)
        out.append(((R, t), [exact_match(rng, cams, rig, R, t) for _k in range(RR.SAMPLE)]))
    return cams, out


TRUTH = (PC.rot([0.3, -0.2, 1.0], 0.15), np.array([0.25, -0.1, 0.3]))


def scene(ncams=8, n=200, seed=0, moved=0.1, noise=0.1):
    """-> (cams, truth, matches, is_moved): n matches between two frames of an outward-facing rig, frame 2 at b1_T_b2 = TRUTH; a
    match is a point at depth 2 - 10 in a random camera of frame 1 and in the first camera of frame 2 that sees it; both keypoints
    get N(0, noise px) and are rounded to float; a fraction `moved` of the matches have their frame-2 keypoint moved by 50 px in
    a random direction"""
    rng = np.random.default_rng(1000 + seed)
    cams = outward_rig(ncams)
    rig = rig_arrays(cams)
    R, t = TRUTH
    matches, is_moved = [], []
    while len(matches) < n:
        c1, u1, v1, c2, u2, v2 = exact_match(rng, cams, rig, R, t)
        mv = bool(rng.random() < moved)
        e = rng.normal(scale=1.0, size=4) * noise
        a = rng.uniform(0, 2 * math.pi)
        if mv:
            u2, v2 = u2 + 50 * math.cos(a), v2 + 50 * math.sin(a)
        matches.append((c1, PC.f32(u1 + e[0]), PC.f32(v1 + e[1]), c2, PC.f32(u2 + e[2]), PC.f32(v2 + e[3])))
        is_moved.append(mv)
    return cams, (PC.rows_of(R), [float(v) for v in t]), matches, is_moved


def first_seed(ncams=8, n=200, moved=0.1, noise=0.1, threshold=THRESHOLD, limit=64):
    """the first seed of scene() for which no moved match is an inlier at the true pose (on the restatement's score)"""
    for seed in range(limit):
        cams, truth, matches, mv = scene(ncams, n, seed, moved, noise)
        if not any(RR.score(cams, truth, m) < threshold for m, v in zip(matches, mv) if v):
            return seed
    raise AssertionError("no seed")


def pose_error(pose, truth):
    """(max |dR_ij|, |dt| in m)"""
    return SC.pose_error(pose, truth)


def arrays(matches):
    cam1 = np.array([m[0] for m in matches], np.int32)
    uv1 = np.array([[m[1], m[2]] for m in matches], np.float32).reshape(-1, 2)
    cam2 = np.array([m[3] for m in matches], np.int32)
    uv2 = np.array([[m[4], m[5]] for m in matches], np.float32).reshape(-1, 2)
    return cam1, uv1, cam2, uv2


def arrays64(matches):
    cam1, _, cam2, _ = arrays(matches)
    return (cam1, np.array([[m[1], m[2]] for m in matches], np.float64).reshape(-1, 2), cam2,
            np.array([[m[4], m[5]] for m in matches], np.float64).reshape(-1, 2))


def solver_of(mc, cams):
    """the `solve` argument of the restatement: mcorb_rel_solve on 17 matches -> (R rows, t) or None"""
    cc = PC.to_cams(mc, cams)

    def solve(seventeen):
        got = mc.rel_solve(cc, *arrays64(seventeen))
        return None if got is None else SC.lists(got)
    return solve


def run(mc, lm, cams, matches, threshold=THRESHOLD, max_iterations=100, seed=0):
    return lm.relative_pose(PC.to_cams(mc, cams), *arrays(matches), threshold, max_iterations=max_iterations, seed=seed)


def same(got, ref, what=""):
    """a RelResult against rel_ref.ransac's dict"""
    assert got.status == ref["status"], (what, "status", NAMES[got.status], NAMES[ref["status"]])
    assert P.same_bits(got.R.tolist(), ref["R"]) and P.same_bits(got.t.tolist(), ref["t"]), (what, "model", got.R, ref["R"])
    assert got.best_hypothesis == ref["best"], (what, "best", got.best_hypothesis, ref["best"])
    assert list(got.sample) == list(ref["sample"]), (what, "sample", got.sample, ref["sample"])
    assert got.n_inliers == ref["n_inliers"], (what, "count", got.n_inliers, ref["n_inliers"])
    assert got.n_models == ref["n_models"], (what, "n_models", got.n_models, ref["n_models"])
    assert got.n_matches == len(ref["inliers"]), (what, "n_matches")
    assert got.inliers.tolist() == [bool(v) for v in ref["inliers"]], (what, "inliers")


def same_counts(lm, ref, what=""):
    """the counts of all hypotheses through the read-back"""
    count, valid = lm.last_relative_counts()
    assert valid.tolist() == [m is not None for m in ref["models"]], (what, "models")
    assert count.tolist() == [c or 0 for c in ref["counts"]], (what, "counts")


def same_stores(a, b, what=""):
    """two results of the library (device store, host-only store), doubles as raw bytes"""
    for k in ("R", "t"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)
    for k in ("status", "n_matches", "n_inliers", "best_hypothesis", "sample", "n_models"):
        assert getattr(a, k) == getattr(b, k), (what, k)
    assert a.inliers.tolist() == b.inliers.tolist(), what
