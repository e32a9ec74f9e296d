"""Inputs and helpers of the re-triangulation tests (test_retri_cpu.py, test_gpu_retri.py, scripts/retri_rate.py): seeded scenes
with a chosen number of views per landmark, scenes written out by hand whose answer is exact, and the comparison of a
LocalMap.retriangulate result against the restatement (retri_ref.py), floats as raw bytes with no tolerance.

A scene is a dict: cams (pose_ref.py's rig), poses (list of (R rows, t)), moved (per keyframe), pts (the landmarks' current
points), truth_pts, obs (list of (kf, cam, lm, kx, ky))."""
import math

import numpy as np

import ba_cases as BC
import landmark_cases as Lc
import pose_cases as PC
import pose_ref as P
import retri_ref as R
import track_cases as T

VIEW_COUNTS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 257]      # the fold's lane and trip boundaries; 257 spans more than 16 keyframes
LANDMARK_COUNTS = [0, 1, 3, 4, 5, 63, 64, 65, 257]        # the group, wave and workgroup boundaries


def forward_rig(ncams, skew=0.0, fx=700.0):
    """cameras that all look along the body's z, a little apart and a little turned, so that every camera of every keyframe has
    every landmark in front"""
    cams = []
    for c in range(ncams):
        side = c - (ncams - 1) / 2.0
        R_ = PC.rot([0.2, 1.0, 0.1], 0.02 * side) @ PC.rot([1.0, 0.0, 0.3], 0.005 * c)
        cams.append(T.cam(PC.rows_of(R_), (0.05 * side, 0.01 * (c % 3), 0.002 * c), fx=fx + 3 * c, fy=fx - 2 * c, s=skew * (c + 1),
                          u0=320.5 + c, v0=240.25 - c))
    return cams


def synth(nkf, ncams, views, seed, skew=0.0, used_kfs=None, moved=None, noise=0.5, pt_off=0.05, spacing=0.05):
    """landmark j has views[j] observations in distinct (keyframe, camera) pairs drawn from used_kfs (all keyframes by default)
    x the cameras; the keyframes stand `spacing` m apart along x with small turns; moved: per keyframe (all by default)"""
    rng = np.random.default_rng(seed)
    cams = forward_rig(ncams, skew)
    poses = []
    for k in range(nkf):
        Rk = PC.rot([0.1, 1.0, 0.05], 0.002 * (k % 50)) @ PC.rot([1.0, 0.0, 0.0], 0.01 * (k % 3))
        poses.append((PC.rows_of(Rk), [spacing * (k % 64) + 0.01 * (k // 64), 0.02 * (k % 2), 0.01 * (k % 5)]))
    used = list(range(nkf)) if used_kfs is None else list(used_kfs)
    pairs = [(k, c) for k in used for c in range(ncams)]
    truth, pts, obs = [], [], []
    for j, nv in enumerate(views):
        assert nv <= len(pairs)
        X = [float(rng.uniform(-1.5, 3.0)), float(rng.uniform(-1.0, 1.0)), float(rng.uniform(4.0, 8.0))]
        truth.append(X)
        d = rng.normal(size=3)
        pts.append([float(v) for v in np.asarray(X) + pt_off * d / np.linalg.norm(d)])
        for i in rng.choice(len(pairs), nv, replace=False):
            k, c = pairs[int(i)]
            px, py = PC.project(cams, poses[k], c, X)
            obs.append((k, c, j, PC.f32(px + noise * rng.normal()), PC.f32(py + noise * rng.normal())))
    perm = rng.permutation(len(obs))      # the caller's order is not the sorted one
    obs = [obs[i] for i in perm]
    return dict(cams=cams, poses=poses, moved=[True] * nkf if moved is None else list(moved), pts=pts, truth_pts=truth, obs=obs)


def from_ba(sc, poses=None, moved=None):
    """a bundle adjustment scene (ba_cases.py) as a re-triangulation scene: the octave leaves"""
    out = dict(cams=sc["cams"], poses=list(sc["poses"] if poses is None else poses), pts=sc["pts"], truth_pts=sc["truth_pts"],
               obs=[o[:5] for o in sc["obs"]])
    out["moved"] = [not f for f in sc["fixed"]] if moved is None else list(moved)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the exact scene: identity rotations, fx = fy = 100, u0 = 160, v0 = 120, every keypoint the exact projection of the origin.
# Every DLT row then has a fourth component of exactly zero, G's last row and column are exactly zero, no rotation touches them,
# and X = (0, 0, 0) * (1.0 / 1.0) on the bits
# ---------------------------------------------------------------------------------------------------------------------------
def exact_cam(R_=T.EYE):
    return T.cam(R_, (0.0, 0.0, 0.0), fx=100.0, fy=100.0, s=0.0, u0=160.0, v0=120.0)


MINUS = [[-1.0, -0.0, -0.0], [-0.0, -1.0, -0.0], [-0.0, -0.0, -1.0]]      # not a rotation: every product of a view's z is -0.0
EXACT_VIEWS = [([0.0, 0.0, -2.0], 160.0, 120.0), ([2.0, 0.0, -2.0], 60.0, 120.0), ([0.0, 2.0, -2.0], 160.0, 20.0)]


def exact_scene(extra=(), pt=(0.0, 0.0, 0.0), order=None):
    """one landmark at the origin seen from the three EXACT_VIEWS (camera 0, identity) and from `extra`: a list of (centre,
    camera, kx, ky) keyframes.  Cameras: 0 the identity, 1 MINUS.  order: the keyframe index of every view, by default as listed"""
    views = [(c, 0, u, v) for c, u, v in EXACT_VIEWS] + list(extra)
    order = list(range(len(views))) if order is None else order
    poses = [None] * len(views)
    obs = []
    for (centre, cam, u, v), k in zip(views, order):
        poses[k] = (T.EYE, [float(x) for x in centre])
        obs.append((k, cam, 0, float(u), float(v)))
    return dict(cams=[exact_cam(), exact_cam(MINUS)], poses=poses, moved=[True] * len(views), pts=[list(pt)], truth_pts=[[0.0] * 3], obs=obs)


AT_ORIGIN = ([0.0, 0.0, 0.0], 0, 7.0, 9.0)          # z = +0.0 exactly: behind
AT_ORIGIN_MINUS = ([0.0, 0.0, 0.0], 1, 7.0, 9.0)    # z = -0.0 exactly: behind


# ---------------------------------------------------------------------------------------------------------------------------
# running and comparing
# ---------------------------------------------------------------------------------------------------------------------------
def arrays(obs):
    kf = np.array([o[0] for o in obs], np.int32)
    cam = np.array([o[1] for o in obs], np.int32)
    lm = np.array([o[2] for o in obs], np.int32)
    uv = np.array([[o[3], o[4]] for o in obs], np.float32).reshape(-1, 2)
    return kf, cam, lm, uv


def fill(store, sc, first_lid=0):
    """the scene's current points into slots first_lid .., with a normal, so that apply mode may delete them"""
    lids = np.arange(first_lid, first_lid + len(sc["pts"]), dtype=np.int32)
    if len(lids):
        p = np.array(sc["pts"], np.float64).reshape(-1, 3)
        store.set(lids, p, np.tile(np.array([0.0, 0.0, 1.0]), (len(lids), 1)))
    return lids


def run(mc, store, sc, lids=None, first_lid=0, **kw):
    """LocalMap.retriangulate on a scene whose points were put into the store (fill) unless lids says where they are"""
    if lids is None:
        lids = fill(store, sc, first_lid)
    kf, cam, lm, uv = arrays(sc["obs"])
    return store.retriangulate(PC.to_cams(mc, sc["cams"]), [p[0] for p in sc["poses"]], [p[1] for p in sc["poses"]], sc["moved"], lids,
                               kf, cam, lm, uv, **kw)


REF_KEYS = dict(rank_tol="rank_tol", landmark_distance_threshold="far_threshold", dynamic_outlier_threshold="outlier_threshold",
                max_diff="max_diff")


def ref(sc, detail=False, **kw):
    return R.retriangulate(sc["cams"], sc["poses"], sc["moved"], sc["pts"], sc["obs"], detail=detail,
                           **{REF_KEYS[k]: v for k, v in kw.items() if k in REF_KEYS})


def same(got, want, what=""):
    """a RetriResult against the restatement's dict; floats as raw bytes"""
    assert got.verdict.tolist() == want["verdict"], (what, "verdict", [R.NAMES[v] for v in got.verdict], [R.NAMES[v] for v in want["verdict"]])
    assert got.n_views.tolist() == want["n_views"], (what, "n_views")
    assert got.counts == want["counts"], (what, "counts", got.counts, want["counts"])
    assert got.pts.tobytes() == np.array(want["pts"], np.float64).reshape(-1, 3).tobytes(), (what, "pts", got.pts, want["pts"])
    assert got.diff_norm.tobytes() == np.array(want["diff_norm"], np.float64).tobytes(), (what, "diff_norm", got.diff_norm, want["diff_norm"])


def both_ways(mc, stores, sc, what, **kw):
    """every store (the host-only one, or the device store and the host-only one) against the restatement -> the restatement"""
    want = ref(sc, **kw)
    for k, store in enumerate(stores):
        before = Lc.snapshot(store, fill(store, sc))
        got = run(mc, store, sc, **kw)
        same(got, want, "%s, store %d" % (what, k))
        assert Lc.snapshot(store, range(len(sc["pts"]))) == before, (what, "report mode wrote the store")
    return want


def svd_points(sc):
    """numpy.linalg.svd of every landmark's design (the DLT rows on the restatement's views) -> per landmark X or None"""
    order = R.sort_obs(sc["obs"])
    rows = [[] for _ in sc["pts"]]
    for i in order:
        kf, cam, j, kx, ky = sc["obs"][i]
        a, b = R.rows(R.view(sc["cams"][cam], sc["poses"][kf]), kx, ky)
        rows[j] += [a, b]
    out = []
    for r in rows:
        if len(r) < 4:
            out.append(None)
            continue
        v = np.linalg.svd(np.array(r))[2][-1]
        out.append(v[:3] / v[3])
    return out


def svd_difference(sc):
    """the largest relative difference |X - X_svd| / |X_svd| between the restatement and numpy's SVD over the scene's landmarks"""
    want = ref(sc)
    worst = 0.0
    for X, Y in zip(want["pts"], svd_points(sc)):
        if Y is not None:
            worst = max(worst, float(np.linalg.norm(np.array(X) - Y) / np.linalg.norm(Y)))
    return worst


def truth_error(sc, pts, verdict):
    """the largest distance of a valid landmark's point from the truth"""
    return max(math.dist(p, t) for p, t, v in zip(pts, sc["truth_pts"], verdict) if v in (R.VALID_UPDATED, R.VALID_REJECTED))
