"""Inputs and helpers of the pose refinement tests (test_pose_cpu.py, test_gpu_pose.py, test_gpu_track_refine.py): rigs as the
plain dicts pose_ref.py reads, a seeded scene with a known true pose, rows written out by hand, and the comparison of a
LocalMap.refine_pose result against the restatement, floats as raw bytes with no tolerance."""
import math

import numpy as np

import pose_ref as P
import track_cases as T

EYE = T.EYE
NAMES = {P.NO_OBS: "NO_OBS", P.NO_STEP: "NO_STEP", P.CONVERGED: "CONVERGED", P.MAX_ITER: "MAX_ITER"}


def rot(axis, angle):
    """a rotation matrix (Rodrigues; input data only, never part of what is compared)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def rows_of(M):
    return [[float(v) for v in row] for row in np.asarray(M, np.float64).reshape(3, 3)]


def rig(ncams, skew=True):
    """a forward-looking rig: camera c a little to the side of the body's origin and turned a little, 640 x 480 calibrations
    that differ per camera, with skew"""
    cams = []
    for c in range(ncams):
        side = c - (ncams - 1) / 2.0
        R_ = rot([0.2, 1.0, 0.1], 0.04 * side) @ rot([1.0, 0.0, 0.3], 0.01 * c)
        cams.append(T.cam(rows_of(R_), (0.12 * side, 0.01 * c, 0.005 * c), fx=520.0 + 3 * c, fy=515.0 - 2 * c, s=0.4 * c if skew else 0.0,
                          u0=320.5 + c, v0=240.25 - c))
    return cams


def flat_rig(ncams=1):
    """fx = fy = 1, u0 = v0 = 0, identity: with the identity pose a point (X, Y, 1) projects to exactly (X, Y)"""
    return [T.cam() for _ in range(ncams)]


def to_cams(mc, cams):
    K = [[[c["fx"], c["s"], c["u0"]], [0.0, c["fy"], c["v0"]], [0.0, 0.0, 1.0]] for c in cams]
    return mc.pose_cams([c["R"] for c in cams], [c["t"] for c in cams], K)


def project(cams, pose, cam, X):
    """the calibrated projection of X through the restatement (the residual against a keypoint at the origin)"""
    r, _ = P.residual(cams[cam], pose, X, 0.0, 0.0, want_j=False)
    return r


def f32(v):
    return float(np.float32(v))


def scene(ncams=4, nlm=200, seed=5, moved=0.2, off=(0.05, 0.2), noct=4):
    """-> (cams, truth, init, obs, is_moved): nlm landmarks in front of a rig at the pose `truth`, every one observed by every
    camera that has it in front and inside 640 x 480, the projections rounded to float, a fraction `moved` of them moved by 50 px;
    init is off by off[0] rad and off[1] m"""
    rng = np.random.default_rng(seed)
    cams = rig(ncams)
    Rt = rot([0.3, -0.2, 1.0], 0.4)
    tt = np.array([1.5, -0.7, 0.3])
    truth = (rows_of(Rt), [float(v) for v in tt])
    Ri = Rt @ rot(rng.normal(size=3), off[0])
    d = rng.normal(size=3)
    init = (rows_of(Ri), [float(v) for v in tt + off[1] * d / np.linalg.norm(d)])
    obs, is_moved = [], []
    for _ in range(nlm):
        pb = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 12)])
        X = [float(v) for v in Rt @ pb + tt]
        for c in range(ncams):
            px, py = project(cams, truth, c, X)
            if not (0 <= px <= 640 and 0 <= py <= 480):
                continue
            mv = rng.random() < moved
            if mv:
                a = rng.uniform(0, 2 * math.pi)
                px, py = px + 50 * math.cos(a), py + 50 * math.sin(a)
            obs.append((c, f32(px), f32(py), int(rng.integers(noct)), X))
            is_moved.append(mv)
    return cams, truth, init, obs, is_moved


INV_SIGMA2 = [1.0 / (1.2 ** (2 * l)) for l in range(8)]     # GetInverseScaleSigmaSquares() at scaleFactor 1.2


def pose_error(pose, truth):
    """(rotation angle in rad, translation distance in m) between two poses"""
    dR = np.asarray(pose[0]).T @ np.asarray(truth[0])
    w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])     # sin(angle) * axis: exact near zero
    ang = math.asin(min(1.0, float(np.linalg.norm(w))))
    return ang, float(np.linalg.norm(np.asarray(pose[1]) - np.asarray(truth[1])))


def arrays(obs):
    cam = np.array([o[0] for o in obs], np.int32)
    uv = np.array([[o[1], o[2]] for o in obs], np.float32).reshape(-1, 2)
    octave = np.array([o[3] for o in obs], np.int32)
    pts = np.array([o[4] for o in obs], np.float64).reshape(-1, 3)
    return cam, uv, octave, pts


def as_ref(res):
    """a PoseResult as the restatement's dict, for same()"""
    return dict(R=res.R.tolist(), t=res.t.tolist(), status=res.status, iterations=tuple(res.iterations), cost_initial=res.cost_initial,
                cost_final=res.cost_final, inliers=res.inliers.tolist(), n_inliers=res.n_inliers)


def same(got, want, what=""):
    """got, want: dicts as pose_ref.refine returns them; floats as raw bytes"""
    assert got["status"] == want["status"], (what, "status", NAMES[got["status"]], NAMES[want["status"]])
    assert tuple(got["iterations"]) == tuple(want["iterations"]), (what, "iterations", got["iterations"], want["iterations"])
    for f in ("R", "t", "cost_initial", "cost_final"):
        assert P.same_bits(got[f], want[f]), (what, f, got[f], want[f])
    assert [bool(v) for v in got["inliers"]] == [bool(v) for v in want["inliers"]], (what, "inliers")
    assert got["n_inliers"] == want["n_inliers"], (what, "n_inliers")


def fill_points(lm, obs, first_lid=0):
    """the observations' points into slots first_lid .. of a store -> the lids"""
    lids = np.arange(first_lid, first_lid + len(obs), dtype=np.int32)
    if len(obs):
        pts = np.array([o[4] for o in obs], np.float64).reshape(-1, 3)
        lm.set(lids, pts, np.zeros_like(pts))
    return lids


def refine(mc, lm, cams, init, obs, inv_sigma2=INV_SIGMA2, max_iterations=25, form="pts", first_lid=0):
    """LocalMap.refine_pose on the observations, points given (form "pts") or read from the store (form "lids")"""
    cam, uv, octave, pts = arrays(obs)
    kw = dict(pts=pts) if form == "pts" else dict(lids=fill_points(lm, obs, first_lid))
    return lm.refine_pose(to_cams(mc, cams), init[0], init[1], cam, uv, octave, inv_sigma2, max_iterations=max_iterations, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# rows written out by hand: the flat rig at the identity pose, q = X
# ---------------------------------------------------------------------------------------------------------------------------
IDENT = (EYE, [0.0, 0.0, 0.0])


def z_rows(with_nan=True):
    """observations whose q.z is 0.0, -0.0, 1e-300, -1e-300 and NaN, among ordinary ones a few pixels off"""
    obs = [(0, 3.0, 4.0, 0, [3.5, 4.25, 1.0]), (0, -2.0, 1.0, 0, [-4.5, 2.5, 2.0]), (0, 7.0, -3.0, 0, [20.0, -10.0, 3.0]),
           (0, 0.5, 0.5, 0, [1.0, 0.5, 1.5]), (0, -1.0, -1.0, 0, [-1.0, -1.5, 1.25]), (0, 2.0, 2.0, 0, [9.0, 8.0, 4.0]),
           (0, 1.0, 2.0, 0, [1.0, 2.0, 0.0]), (0, 1.0, 2.0, 0, [1.0, 2.0, -0.0]), (0, 1.0, 2.0, 0, [1.0, 2.0, 1e-300]),
           (0, 1.0, 2.0, 0, [1.0, 2.0, -1e-300])]
    if with_nan:
        obs.append((0, 1.0, 2.0, 0, [1.0, 2.0, float("nan")]))
    return obs


def huber_rows():
    """e exactly k and one ulp either side: the point (x, 0, 1) against a keypoint at the origin has r = (x, 0) and
    e = sqrt(x * x) = x"""
    k = P.HUBER_K
    return [(0, 0.0, 0.0, 0, [x, 0.0, 1.0]) for x in (math.nextafter(k, 0.0), k, math.nextafter(k, 10.0))]


def chi2_rows():
    """-> (obs, inv_sigma2, expected inlier flags).  Pairs of observations of one point whose keypoints lie 2 px either side of
    its projection: r = (-2, 0) and (2, 0) with equal Jacobians, so g is exactly zero, no trial is ever better and the cull
    runs at the initial pose with r.r = 4.  Octave 0: chi2 is exactly 5.991 (kept); 1: the next double above (culled); 2: 4
    (kept); 3: 8 (culled)"""
    inv = [5.991 / 4.0, math.nextafter(5.991, 10.0) / 4.0, 1.0, 2.0]
    obs, flags = [], []
    for octave, (x, y) in enumerate([(10.0, 5.0), (-7.0, 3.0), (2.0, -9.0), (-4.0, -6.0)]):
        for dx in (2.0, -2.0):
            obs.append((0, x + dx, y, octave, [x, y, 1.0]))
            flags.append(octave in (0, 2))
    return obs, inv, flags
