"""Inputs of the essential-pose tests (test_ess_cpu.py, test_gpu_ess.py): the camera, seeded five-point samples and seeded
scenes of one camera in two frames, and the helpers that compare the library's result with the restatement (ess_ref.py).  A match
is (u1, v1, u2, v2); the truth (R, t) is c1_T_c2: X_c1 = R X_c2 + t."""
import math
import struct

import numpy as np

import ess_ref as ER
import pose_cases as PC
import track_cases as T

CAM = T.cam(fx=500.0, fy=503.0, s=0.25, u0=641.5, v0=358.25)
KINDS = ("general", "coplanar", "forward")


def to_cam(mc):
    return PC.to_cams(mc, [CAM])


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, float) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def project(X):
    """a point of the camera's frame -> its keypoint in double"""
    x, y = X[0] / X[2], X[1] / X[2]
    return CAM["fx"] * x + CAM["s"] * y + CAM["u0"], CAM["fy"] * y + CAM["v0"]


def unproject(u, v, z):
    x, y = ER.normalise(CAM, u, v)
    return np.array([x * z, y * z, z])


def random_pose(rng, forward=False, min_baseline=0.0):
    """rotation N(0, 0.1 rad) per axis, translation N(0, 0.3) per axis (drawn again while shorter than min_baseline) or, forward,
    along the optical axis"""
    R = rodrigues(rng.normal(0.0, 0.1, 3))
    t = np.array([0.02, -0.01, 0.5]) if forward else rng.normal(0.0, 0.3, 3)
    while np.linalg.norm(t) < min_baseline:
        t = rng.normal(0.0, 0.3, 3)
    return R, t


def depths(rng, kind, uv, off_plane=0):
    """the depth of frame 1's keypoints: 2 - 10, or on a random plane at depth about 6 (off_plane: every off_plane-th point keeps
    a depth of 2 - 10)"""
    free = rng.uniform(2.0, 10.0, len(uv))
    if kind != "coplanar":
        return free
    nrm = np.array([rng.normal(0.0, 0.3), rng.normal(0.0, 0.3), 1.0])
    plane = np.array([6.0 / (nrm @ np.array([*ER.normalise(CAM, u, v), 1.0])) for u, v in uv])
    if off_plane:
        plane[::off_plane] = free[::off_plane]
    return plane


def exact_matches(rng, kind, n, R, t, z2=None, off_plane=0):
    """n noise-free matches: frame 1's keypoints rounded to float first and the points put on their rays, frame 2's keypoints the
    projections in double; z2 (a list): receives the depths in frame 2"""
    uv1 = np.stack([rng.uniform(100.0, 1180.0, n), rng.uniform(60.0, 660.0, n)], 1).astype(np.float32).astype(np.float64)
    out = []
    for (u, v), z in zip(uv1, depths(rng, kind, uv1, off_plane)):
        X2 = R.T @ (unproject(u, v, z) - t)
        out.append((float(u), float(v), *[float(w) for w in project(X2)]))
        if z2 is not None:
            z2.append(float(X2[2]))
    return out


_SOLVER = {}


def solver_cases(kind, count=2000):
    """count seeded noise-free five-point samples: rotation N(0, 0.1 rad) per axis, translation N(0, 0.3), depth 2 - 10 (general) or
    the five points on a random plane at depth about 6 (coplanar) -> [((R, t), five matches)]"""
    if kind not in _SOLVER:
        rng = np.random.default_rng({"general": 11, "coplanar": 12}[kind])
        out = []
        while len(out) < count:
            R, t = random_pose(rng)
            z2 = []
            five = exact_matches(rng, kind, 5, R, t, z2)
            if min(z2) > 0.5:     # (in front of the second camera too)
                out.append(((R, t), five))
        _SOLVER[kind] = out
    return _SOLVER[kind][:count]


def scene(kind, n=200, seed=0, moved=0.1, noise=0.0):
    """-> (truth (R, t), matches as floats, is_moved): n matches of one camera, a fraction `moved` of frame 2's keypoints moved by 50
    px in a random direction, N(0, noise px) on every keypoint, all rounded to float.  The baseline is at least 0.3, so that
    every depth (2 - 10) stays inside recoverPose's 50 baselines.  In the coplanar scene every tenth point is off the plane: points
    that are all on one plane have two essential matrices -- the two physical solutions of the plane's homography -- which
    nothing but a point off the plane tells apart"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + seed)
    R, t = random_pose(rng, forward=kind == "forward", min_baseline=0.3)
    ms = exact_matches(rng, kind, n, R, t, off_plane=10)
    is_moved = [bool(v) for v in rng.random(n) < moved]
    out = []
    for m, mv in zip(ms, is_moved):
        u1, v1, u2, v2 = m
        if mv:
            a = rng.uniform(0.0, 2.0 * math.pi)
            u2, v2 = u2 + 50.0 * math.cos(a), v2 + 50.0 * math.sin(a)
        e = rng.normal(0.0, noise, 4) if noise else np.zeros(4)
        out.append(tuple(PC.f32(w) for w in (u1 + e[0], v1 + e[1], u2 + e[2], v2 + e[3])))
    return (R, t), out, is_moved


CLEAR_PX = 5.0     # a moved match stays this far from its epipolar line at the true pose


def near_gate(truth, matches, threshold_px=1.0, distance=50.0, rel=1e-6):
    """on the restatement alone, at the true pose: (which matches are inliers -- at CLEAR_PX in place of the threshold: a moved
    match 2 px from its epipolar line is an inlier of a pose that fits every other match within the threshold --, whether a
    gate quantity -- a Sampson value against the threshold, a depth against 0 or the distance -- lies within `rel` relative of
    its gate)"""
    R, t = truth
    E = [float(v) for v in ER.true_E(R, t).reshape(9)]
    th = [float(v) for v in t / np.linalg.norm(t)]
    thr2 = ER.threshold2(CAM, threshold_px)
    inl, near = [], False
    for m in matches:
        p = ER.point(CAM, m)
        s = ER.sampson(E, p)
        z = ER.depths([float(v) for v in np.asarray(R).reshape(9)], th, p)
        inl.append(s < ER.threshold2(CAM, CLEAR_PX) and ER.in_front(z, distance))
        near = near or abs(s - thr2) <= rel * thr2 or any(abs(v) <= rel or abs(v - distance) <= rel * distance for v in z)
    return inl, near


def first_seed(kind, noise):
    """the first seed whose scene has no moved match among the inliers at the true pose and no gate quantity near its gate"""
    for seed in range(50):
        truth, matches, moved = scene(kind, seed=seed, noise=noise)
        inl, near = near_gate(truth, matches)
        if not near and not any(i and mv for i, mv in zip(inl, moved)):
            return seed
    raise AssertionError("no seed")


def solver_of(mc):
    cc = to_cam(mc)
    return lambda five: [E.reshape(9).tolist() for E in mc.ess_solve(cc, [m[0:2] for m in five], [m[2:4] for m in five])]


def arrays(matches):
    a = np.array(matches, np.float32).reshape(-1, 4)
    return a[:, 0:2].copy(), a[:, 2:4].copy()


def run(mc, lm, matches, threshold_px=1.0, distance=50.0, max_iterations=100, seed=0):
    uv1, uv2 = arrays(matches)
    return lm.essential_pose(to_cam(mc), uv1, uv2, threshold_px, distance, max_iterations, seed)


def pack(v):
    return struct.pack("<%dd" % len(v), *v)


def same(got, ref, what):
    """the library's result against the restatement, doubles as raw bytes"""
    assert got.status == ref["status"], what
    assert pack(got.R.reshape(9)) == pack(ref["R"]) and pack(got.t) == pack(ref["t"]) and pack(got.E.reshape(9)) == pack(ref["E"]), what
    assert (got.n_ransac_inliers, got.n_inliers, got.best_hypothesis, got.best_root) == (ref["n_ransac_inliers"], ref["n_inliers"], ref["best"],
                                                                                        ref["root"]), what
    assert list(got.sample) == ref["sample"] and got.n_models == ref["n_models"] and list(got.cheirality) == ref["cheirality"], what
    assert got.inliers.tolist() == ref["inliers"] and got.n_matches == len(ref["inliers"]), what


def same_counts(lm, ref, what):
    count, valid, models = lm.last_essential_counts()
    assert count.tolist() == ref["counts"] and valid.tolist() == ref["valid"], what
    assert models.tobytes() == b"".join(pack(m) for m in ref["models"]), what


def same_stores(a, b, what):
    """two results of the library (device store, host-only store), doubles as raw bytes"""
    for k in ("R", "t", "E"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)
    for k in ("status", "n_matches", "n_ransac_inliers", "n_inliers", "best_hypothesis", "best_root", "sample", "n_models", "cheirality"):
        assert getattr(a, k) == getattr(b, k), (what, k)
    assert a.inliers.tolist() == b.inliers.tolist(), what
