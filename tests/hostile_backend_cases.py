"""Degenerate and hostile inputs of the back end and of mapping (test_hostile_backend_cpu.py, test_gpu_hostile_backend.py,
scripts/header_coverage.py): one table of named rows per call -- bundle_adjust, retriangulate, refine_pose, triangulate_new,
triangulate_neighbours, initialize -- built from the family's *_cases.py helpers, seeded, at the smallest shape at which the
launch has a full unit and a partly filled one.  What a bootstrap or a diverged back end hands these calls: a window that did not
move or only rotated, every landmark one point, on one line through two camera centres, on one plane, a landmark at a camera
centre, keypoints at the principal point, repeated, given twice, overflowed, infinite and NaN, an R that is no rotation, a
non-finite number in each operand position, and points and translations scaled until a square is subnormal or infinite.

A row changes floating-point values and which observations exist, never an index, a count or an id beyond what the entry
accepts.  A row is (name, scene or arguments ..., keywords of the call).  The tables are built once and never changed by a test."""
import functools
import math

import numpy as np

import ba_cases as BC
import init_cases as Ic
import mapping_cases as Mc
import mapping_new_cases as Nc
import pose_cases as PC
import pose_ref as P
import retri_cases as RC
import retri_ref as R

INF, NAN = math.inf, math.nan
NLM = 68                      # a wave of k_ba_linearize and four lanes of the next; four workgroups of k_retri_solve and a part of the fifth
SCALES = (1e-160, 1e-155, 1e-150, 1e150, 1e155, 1e160)
BAD = (("NaN", NAN), ("inf", INF))
# the front end's calls triangulate by a DLT on [R | t] and keypoints: scaling the translations alone unbalances its design long
# before a square overflows.  Where the verdict counts of the well-posed rows change, found on the restatement, a decade apart
EDGES = ((1e-28, 1e-27), (1e8, 1e9), (1e87, 1e88))
FRONT_SCALES = SCALES + tuple(k for e in EDGES for k in e)


def f32(v):
    """a double as the float the call receives: overflow gives inf"""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(v))


def names(rows):
    return [r[0] for r in rows]


def row_of(rows, name):
    return rows[names(rows).index(name)]


# ---------------------------------------------------------------------------------------------------------------------------
# what a row does to a scene of ba_cases.py / retri_cases.py: cams, poses, pts, obs = (kf, cam, lm, kx, ky[, octave])
# ---------------------------------------------------------------------------------------------------------------------------
def centre(sc, kf, cam, poses=None):
    """the camera's centre in the world: R_kf t_cam + t_kf"""
    Rk, tk = (poses or sc["poses"])[kf]
    return np.asarray(Rk) @ np.asarray(sc["cams"][cam]["t"], np.float64) + np.asarray(tk)


def depth(sc, pose, cam, X):
    """the point's z in the camera"""
    c = sc["cams"][cam]
    return P.transform_to(c["R"], c["t"], P.transform_to(pose[0], pose[1], X))[2]


def reobserved(sc, poses=None, pts=None, start=None, cams=None, pairs=None):
    """the scene with its landmarks at `pts` (by default the true points) seen from `poses`: landmark j keeps its number of
    observations and their octaves, and has them in the pairs of keyframe and camera that have it at least 0.2 m in front, taken
    in turn (so twice where there are fewer such pairs than observations); a landmark in front of nothing keeps its pairs; with `pairs`
    every landmark has its observations in those, in turn, wherever it lies.
    Every keypoint is the projection rounded to float.  Without `poses` the scene keeps its initial poses and is seen from the
    true ones; the landmarks' current points start at `start`, by default as far from pts as the scene's are from the truth"""
    sc = dict(sc, cams=sc["cams"] if cams is None else cams)
    given = poses is not None
    poses = list(poses if given else sc.get("truth_poses", sc["poses"]))
    pts = [list(map(float, p)) for p in (sc["truth_pts"] if pts is None else pts)]
    mine = [[] for _ in pts]
    for i, o in enumerate(sc["obs"]):
        mine[o[2]].append(i)
    obs = list(sc["obs"])
    for j, idx in enumerate(mine):
        front = pairs or [(k, c) for k in range(len(poses)) for c in range(len(sc["cams"])) if depth(sc, poses[k], c, pts[j]) > 0.2]
        for n, i in enumerate(idx):
            k, c = front[n % len(front)] if front else obs[i][:2]
            px, py = PC.project(sc["cams"], poses[k], c, pts[j])
            obs[i] = (k, c, j, f32(px), f32(py)) + obs[i][5:]
    off = [np.asarray(p) - np.asarray(t) for p, t in zip(sc["pts"], sc["truth_pts"])]
    start = [list(np.asarray(p) + d) for p, d in zip(pts, off)] if start is None else [list(p) for p in start]
    return dict(sc, poses=poses if given else sc["poses"], truth_pts=pts, pts=start, obs=obs)


def with_uv(sc, fn):
    """fn(i, observation) -> (kx, ky)"""
    return dict(sc, obs=[o[:3] + tuple(f32(v) for v in fn(i, o)) + o[5:] for i, o in enumerate(sc["obs"])])


def with_pose(sc, k, R_=None, t=None):
    poses = list(sc["poses"])
    poses[k] = ([list(r) for r in (poses[k][0] if R_ is None else R_)], list(poses[k][1] if t is None else t))
    return dict(sc, poses=poses)


def with_entry(sc, what, k, value):
    """one entry of pose k's R (what "R": row 1, column 2), of its t (entry 1) or of point k (entry 2) replaced"""
    if what == "pt":
        pts = [list(p) for p in sc["pts"]]
        pts[k][2] = value
        return dict(sc, pts=pts)
    R_, t = [list(r) for r in sc["poses"][k][0]], list(sc["poses"][k][1])
    if what == "R":
        R_[1][2] = value
    else:
        t[1] = value
    return with_pose(sc, k, R_, t)


def scaled(sc, k):
    """points, the keyframes' translations and the rig's lever arms times k: the same images"""
    cams = [dict(c, t=[v * k for v in c["t"]]) for c in sc["cams"]]
    out = dict(sc, cams=cams, poses=[(p[0], [v * k for v in p[1]]) for p in sc["poses"]], pts=[[v * k for v in p] for p in sc["pts"]])
    if "truth_pts" in sc:
        out["truth_pts"] = [[v * k for v in p] for p in sc["truth_pts"]]
    return out


def times(M, k):
    return [[v * k for v in r] for r in M]


REFLECT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]


def generic_rows(base, free, fixed, pp):
    """the rows every call of a window of keyframes takes: base a scene, free / fixed the index of a pose the call may and may
    not move (for retriangulate: of a moved and of an unmoved keyframe), pp(cam) the camera's principal point
    -> [(name, scene)]"""
    nkf = len(base["poses"])
    rows = [("well posed", base)]
    rows.append(("no keyframe moved", reobserved(base, [base["poses"][0]] * nkf, start=base["pts"])))
    rows.append(("pure rotation", reobserved(base, [(p[0], base["poses"][0][1]) for p in base["poses"]], start=base["pts"])))
    one = [base["truth_pts"][0]] * len(base["pts"])
    rows.append(("every landmark the same point", reobserved(base, pts=one)))
    # (the camera that looks most along the way from its centre in the first keyframe to its centre in the last; every landmark is
    # seen from these two centres alone: every ray is the line)
    true = base.get("truth_poses", base["poses"])
    ncams = len(base["cams"])
    if nkf > 1:
        ends = [((0, c), (nkf - 1, c)) for c in range(ncams)]
    else:       # (one keyframe: the centres of two of its cameras)
        ends = [((0, c), (0, (c + 1) % ncams)) for c in range(ncams)]
    ends = [(a, b, centre(base, *a, true), centre(base, *b, true)) for a, b in ends]
    a, b, c0, c1 = max(ends, key=lambda e: depth(base, true[e[0][0]], e[0][1], e[2] + 3.0 * (e[3] - e[2])))
    line = [list(c1 + (2.0 + 0.25 * j) * (c1 - c0) / np.linalg.norm(c1 - c0)) for j in range(len(base["pts"]))]
    rows.append(("points on the line through two camera centres", reobserved(base, pts=line, pairs=[a, b])))
    plane = [[p[0], 0.5, p[2]] for p in base["truth_pts"]]
    rows.append(("points on one plane", reobserved(base, pts=plane)))
    # (the centre of the camera of the landmark's first observation, every fourth landmark)
    first = {}
    for o in base["obs"]:
        first.setdefault(o[2], o)
    at = [list(centre(base, first[j][0], first[j][1])) if j % 4 == 1 and j in first else p for j, p in enumerate(base["pts"])]
    rows.append(("landmarks at a camera centre", dict(base, pts=at)))
    rows.append(("every keypoint at its principal point", with_uv(base, lambda i, o: pp(o[1]))))
    rows.append(("one keypoint repeated", with_uv(base, lambda i, o: base["obs"][0][3:5])))
    rows.append(("observations given twice", dict(base, obs=base["obs"] + base["obs"][::5])))
    rows.append(("keypoints times 1e30", with_uv(base, lambda i, o: (o[3] * 1e30, o[4] * 1e30))))
    rows.append(("keypoints times 1e36, all inf", with_uv(base, lambda i, o: (o[3] * 1e36, o[4] * 1e36))))
    rows.append(("a third of the keypoints inf", with_uv(base, lambda i, o: (o[3], o[4]) if i % 3 else (INF, o[4]) if i % 2 else (o[3], -INF))))
    for col in (0, 1):
        rows.append(("NaN in keypoint column %d" % col,
                     with_uv(base, lambda i, o, col=col: (o[3], o[4]) if i % 5 else ((NAN, o[4]), (o[3], NAN))[col])))
    rows.append(("every keypoint NaN", with_uv(base, lambda i, o: (NAN, o[4]))))
    for word, v in BAD:
        for what in ("R", "t"):
            for who, k in (("fixed", fixed), ("free", free)):
                if k is not None:
                    rows.append(("%s in %s of a %s pose" % (word, what, who), with_entry(base, what, k, v)))
        rows.append(("%s in one point" % word, with_entry(base, "pt", 3, v)))
    rows.append(("R times 2", with_pose(base, free, times(base["poses"][free][0], 2.0))))
    rows.append(("R a reflection", with_pose(base, free, (np.asarray(base["poses"][free][0]) @ np.asarray(REFLECT)).tolist())))
    rows.append(("R zero", with_pose(base, free, times(base["poses"][free][0], 0.0))))
    for k in SCALES:
        rows.append(("points and translations times %g" % k, scaled(base, k)))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# bundle_adjust: 4 keyframes, 2 of them fixed, 4 cameras, 68 landmarks of at most 3 views, 8 iterations
# ---------------------------------------------------------------------------------------------------------------------------
BA_ITERATIONS = 8


def mirrored(sc, which):
    """the landmarks `which` (current and true point) mirrored at the centre of the first keyframe that sees them: behind every
    camera that has an observation of them"""
    first = {}
    for o in sc["obs"]:
        first.setdefault(o[2], o[0])
    pts, truth = [list(p) for p in sc["pts"]], [list(p) for p in sc["truth_pts"]]
    for j in which:
        if j in first:
            c = np.asarray(sc["poses"][first[j]][1])
            pts[j], truth[j] = list(2 * c - np.asarray(pts[j])), list(2 * c - np.asarray(truth[j]))
    return dict(sc, pts=pts, truth_pts=truth)


def all_cameras_scene():
    """a rig of 16 cameras that all look forwards: landmark 0 has an observation in every camera of every keyframe, 64 in one
    lane of k_ba_linearize beside lanes of 2 and 3"""
    sc = BC.scene(nkf=4, ncams=16, nlm=NLM, nfixed=2, seed=63, max_views=3)
    truth = [[0.4, 0.1, 5.0]] + sc["truth_pts"][1:]
    obs = [o for o in sc["obs"] if o[2] != 0] + [(k, c, 0, 0.0, 0.0, (k + c) % len(sc["sigma"])) for k in range(4) for c in range(16)]
    start = [[0.45, 0.05, 5.1]] + sc["pts"][1:]
    return reobserved(dict(sc, obs=obs), poses=sc["truth_poses"], pts=truth, start=start, cams=RC.forward_rig(16, fx=160.0))


@functools.lru_cache(None)
def ba_rows():
    """-> [(name, scene of ba_cases.py, keywords: max_iterations)]"""
    base = BC.scene(nkf=4, ncams=4, nlm=NLM, nfixed=2, seed=61, max_views=3)
    cams = base["cams"]
    rows = [(n, sc, {}) for n, sc in generic_rows(base, free=2, fixed=1, pp=lambda c: (cams[c]["u0"], cams[c]["v0"]))]
    for s in (1e-300, 1e300):
        rows.append(("sigma %g" % s, dict(base, sigma=[s] * len(base["sigma"])), {}))
    rows.append(("no fixed keyframe", dict(base, fixed=[False] * 4), {}))
    rows.append(("every landmark behind every camera", mirrored(base, range(NLM)), {}))
    rows.append(("inactive landmarks between active ones", mirrored(base, range(1, NLM, 2)), {}))
    rows.append(("one landmark in all 64 cameras", all_cameras_scene(), {}))
    rows.append(("well posed, 100 iterations", base, dict(max_iterations=100)))
    rows.append(("well posed, 1 iteration", base, dict(max_iterations=1)))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# retriangulate: 4 keyframes, 4 cameras, 68 landmarks of 2, 3, 15, 16 and 17 views (the seventeenth a second observation in
# one of the 16 pairs of keyframe and camera), report mode
# ---------------------------------------------------------------------------------------------------------------------------
RETRI_VIEWS = [(2, 3, 15, 16, 17)[j % 5] for j in range(NLM)]
RETRI_ON = dict(landmark_distance_threshold=7.5, dynamic_outlier_threshold=3.0)


def retri_scene(views, seed, cams=None, pairs=None, noise=0.5, pt_off=0.05, moved=None):
    """retri_cases.synth with view counts above the number of pairs: landmark j's observations are drawn from `pairs` (all 16 of
    keyframe and camera by default) without repetition while they last, then with; every keyframe but the second moved"""
    rng = np.random.default_rng(seed)
    cams = RC.forward_rig(4) if cams is None else cams
    poses = RC.synth(4, 4, [], seed)["poses"]
    pairs = [(k, c) for k in range(4) for c in range(4)] if pairs is None else pairs
    truth, pts, obs = [], [], []
    for j, nv in enumerate(views):
        X = [float(rng.uniform(-1.5, 3.0)), float(rng.uniform(-1.0, 1.0)), float(rng.uniform(4.0, 8.0))]
        truth.append(X)
        d = rng.normal(size=3)
        pts.append([float(v) for v in np.asarray(X) + pt_off * d / np.linalg.norm(d)])
        mine = [pairs[int(i)] for i in rng.permutation(len(pairs))]
        while len(mine) < nv:
            mine.append(pairs[int(rng.integers(len(pairs)))])
        for k, c in mine[:nv]:
            px, py = PC.project(cams, poses[k], c, X)
            obs.append((k, c, j, f32(px + noise * rng.normal()), f32(py + noise * rng.normal())))
    perm = rng.permutation(len(obs))
    return dict(cams=cams, poses=poses, moved=[True, False, True, True] if moved is None else moved, pts=pts, truth_pts=truth,
                obs=[obs[i] for i in perm])


def lane_scene():
    """camera 3 looks backwards and only landmarks 0 and 1 have an observation in it, in keyframe 3: the last in the order of
    (keyframe, camera).  Landmark 0 has 16 views, the failing one is lane 15's; landmark 1 has 17, the failing one is
    observation 16, the second trip of lane 0.  Every other landmark lies in cameras 0 .. 2"""
    cams = RC.forward_rig(4)
    back = (np.asarray(cams[3]["R"]) @ PC.rot([0.0, 1.0, 0.0], math.pi)).tolist()
    cams = cams[:3] + [dict(cams[3], R=back)]
    front = [(k, c) for k in range(4) for c in range(3)]
    sc = retri_scene([15, 16] + RETRI_VIEWS[2:], 72, cams=cams, pairs=front)
    obs = list(sc["obs"])
    for j in (0, 1):
        px, py = PC.project(cams, sc["poses"][3], 3, sc["truth_pts"][j])
        obs.append((3, 3, j, f32(px), f32(py)))
    return dict(sc, obs=obs)


@functools.lru_cache(None)
def retri_rows():
    """-> [(name, scene of retri_cases.py, keywords of RC.run / RC.ref)]: every row once with the far and outlier checks off
    and once with both on"""
    base = retri_scene(RETRI_VIEWS, 71)
    cams = base["cams"]
    plain = generic_rows(base, free=2, fixed=1, pp=lambda c: (cams[c]["u0"], cams[c]["v0"]))
    # every view of landmarks 5, 6 and 9 (2, 3 and 17 views) has a NaN keypoint: every error of theirs is NaN
    plain.append(("landmarks whose errors are all NaN", with_uv(base, lambda i, o: (NAN, NAN) if o[2] in (5, 6, 9) else (o[3], o[4]))))
    plain.append(("the first failing observation in lane 15 and in observation 16", lane_scene()))
    # the current points far from where the landmarks are: VALID_REJECTED
    plain.append(("current points 6 m off", dict(base, pts=[[p[0], p[1] + 6.0, p[2]] if j % 2 else p for j, p in enumerate(base["pts"])])))
    # landmarks of one observation, and of none, among the others: FEW_VIEWS
    plain.append(("landmarks of one view", dict(base, obs=[o for i, o in enumerate(base["obs"])
                                                         if o[2] % 7 or o == next(p for p in base["obs"] if p[2] == o[2])])))
    rows = []
    for name, sc in plain:
        rows.append((name, sc, {}))
        rows.append((name + ", far and outlier checks on", sc, dict(RETRI_ON)))
    rows.append(("well posed, max_diff 0", base, dict(max_diff=0.0)))
    rows.append(("well posed, max_diff inf", base, dict(max_diff=INF)))
    rows.append(("well posed, rank_tol 0", base, dict(rank_tol=0.0)))
    rows.append(("well posed, rank_tol inf", base, dict(rank_tol=INF)))
    rows.append(("well posed, thresholds 1e-300", base, dict(landmark_distance_threshold=1e-300, dynamic_outlier_threshold=1e-300)))
    rows.append(("well posed, thresholds inf", base, dict(landmark_distance_threshold=INF, dynamic_outlier_threshold=INF)))
    return rows


def failed(ref):
    """the restatement ends a landmark in a failed verdict: the row runs in apply mode as well"""
    return any(v in R.FAILED for v in ref["verdict"])


# ---------------------------------------------------------------------------------------------------------------------------
# refine_pose: 4 cameras, 68 observations; a row is a window of one keyframe whose pose is free
# ---------------------------------------------------------------------------------------------------------------------------
NOBS = 68


def pose_args(sc):
    """a window of one keyframe -> (cams, init, obs) of pose_cases.py"""
    return sc["cams"], sc["poses"][0], [(o[1], o[3], o[4], o[5], sc["pts"][o[2]]) for o in sc["obs"]]


@functools.lru_cache(None)
def pose_rows():
    """-> [(name, cams, init, obs, keywords of PC.refine / P.refine)]"""
    cams, truth, init, obs, _ = PC.scene(4, nlm=24, seed=81, moved=0.1)
    obs = obs[:NOBS]
    assert len(obs) == NOBS
    index, pts = {}, []
    for o in obs:
        if id(o[4]) not in index:
            index[id(o[4])] = len(pts)
            pts.append(list(o[4]))
    base = dict(cams=cams, poses=[init], truth_poses=[truth], pts=pts, truth_pts=[list(p) for p in pts],
                obs=[(0, o[0], index[id(o[4])], o[1], o[2], o[3]) for o in obs])
    rows = [(n, *pose_args(sc), {}) for n, sc in generic_rows(base, free=0, fixed=None, pp=lambda c: (cams[c]["u0"], cams[c]["v0"]))
            if n != "pure rotation"]
    rows.append(("the initial pose the true one", *pose_args(dict(base, poses=[truth])), {}))
    for word, v in (("0", 0.0), ("inf", INF), ("1e-300", 1e-300), ("1e300", 1e300)):
        rows.append(("inv_sigma2 %s" % word, *pose_args(base), dict(inv_sigma2=[v] * len(PC.INV_SIGMA2))))
    rows.append(("well posed, 1 iteration", *pose_args(base), dict(max_iterations=1)))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the front end's three calls read frames of mapping_cases.py: match_index, keypoints, proj = [R | t] and centre_w per camera,
# twc.  What a row does to a frame
# ---------------------------------------------------------------------------------------------------------------------------
NMATCH = 68
NCAMS = 4


def frame_uv(fr, fn):
    """fn(camera, index, x, y) -> (x, y), rounded to float"""
    kps = []
    for c, a in enumerate(fr["kps"]):
        a = a.copy()
        for i in range(len(a)):
            x, y = fn(c, i, float(a[i]["x"]), float(a[i]["y"]))
            a[i]["x"], a[i]["y"] = f32(x), f32(y)
        kps.append(a)
    return dict(fr, kps=kps)


def frame_geom(fr, fn_R=None, fn_t=None):
    """fn_R(camera, R) -> the rotation part of proj; fn_t(v) -> every translation: proj's last column, centre_w, twc"""
    proj, cw, twc = [np.array(p, np.float64) for p in fr["proj"]], [np.array(c, np.float64) for c in fr["centre_w"]], np.array(fr["twc"], np.float64)
    if fn_R is not None:
        for c in range(len(proj)):
            proj[c][:, :3] = fn_R(c, proj[c][:, :3])
    if fn_t is not None:
        for c in range(len(proj)):
            proj[c][:, 3] = fn_t(proj[c][:, 3])
            cw[c] = fn_t(cw[c])
        twc = fn_t(twc)
    return dict(fr, proj=proj, centre_w=cw, twc=twc)


def frame_entry(fr, what, value):
    """one entry of camera 1's R (row 1, column 2), of its t (entry 1), of its centre (entry 0) or of twc (entry 2) replaced"""
    proj, cw, twc = [np.array(p, np.float64) for p in fr["proj"]], [np.array(c, np.float64) for c in fr["centre_w"]], np.array(fr["twc"], np.float64)
    if what == "R":
        proj[1][1, 2] = value
    elif what == "t":
        proj[1][1, 3] = value
    elif what == "centre":
        cw[1][0] = value
    else:
        twc[2] = value
    return dict(fr, proj=proj, centre_w=cw, twc=twc)


def build_frames(rig, poses_a, pose_b, pts, seed, octave=None, n_old=0):
    """frames of mapping_cases.py at the poses (4 x 4, body in world): one per pose of poses_a, and b; every frame sees every
    point, each in a seeded choice of cameras, the keypoints exact projections rounded to float.  With n_old every frame of
    poses_a also has that many features with landmarks 3000 .. of a store, 3 .. 8 m in front of it.
    -> ([frame a], b, [matches (feature of a, feature of b)], store, [the 4 x 4 per camera of a], those of b)"""
    rng = np.random.default_rng(seed)
    Ks, rig_T = rig
    gb = Mc.frame_geometry(pose_b, rig_T)
    b = Mc.FrameBuilder(gb, Ks)
    feats = []
    with np.errstate(all="ignore"):
        for X in pts:
            feats.append(b.add(np.asarray(X, np.float64), Mc.pick_cams(len(Ks), rng, False), rng, octave))
        frames, matches, store, fulls = [], [], {}, []
        for pose in poses_a:
            g = Mc.frame_geometry(pose, rig_T)
            fa = Mc.FrameBuilder(g, Ks)
            ms = [(fa.add(np.asarray(X, np.float64), Mc.pick_cams(len(Ks), rng, False), rng, octave), t) for X, t in zip(pts, feats)]
            for _ in range(n_old):
                X = pose[:3, :3] @ np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 8)]) + pose[:3, 3]
                fa.add(X, Mc.pick_cams(len(Ks), rng, False), rng, lid=3000 + len(store))
                store[3000 + len(store)] = X
            frames.append(fa.done())
            matches.append(np.array(ms, np.int32).reshape(-1, 2))
            fulls.append(g["full"])
    return frames, b.done(), matches, store, fulls, gb["full"]


def the_rig(seed):
    return Mc.make_rig(NCAMS, np.random.default_rng(seed))


POSE_A = Mc.T4(Mc.rot(0.02, -0.03, 0.01), np.array([0.03, -0.02, 0.01]))
POSE_B = Mc.T4(Mc.rot(-0.04, 0.05, 0.02), np.array([1.0, 0.04, -0.03]))
POSE_C = Mc.T4(Mc.rot(0.03, 0.02, -0.05), np.array([-1.3, 0.05, 0.06]))


def cloud(n, seed, mid):
    rng = np.random.default_rng(seed)
    return [mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 15)]) for _ in range(n)]


def geometries(n, seed, pose_a=POSE_A, pose_b=POSE_B):
    """-> rig, [(name, pose of frame a, pose of frame b, points)]: the rows that place frames and points"""
    rig = the_rig(seed)
    mid = 0.5 * (pose_a[:3, 3] + pose_b[:3, 3])
    pts = cloud(n, seed + 1, mid)
    ca, cb = Mc.frame_geometry(pose_a, rig[1])["centre_w"][0], Mc.frame_geometry(pose_b, rig[1])["centre_w"][0]
    d = (cb - ca) / np.linalg.norm(cb - ca)
    turned = Mc.T4(pose_b[:3, :3], pose_a[:3, 3])          # pure rotation: b's body where a's is
    out = [("the second frame did not move", pose_a, pose_a, pts),
           ("pure rotation", pose_a, turned, pts),
           ("every match the same point", pose_a, pose_b, [pts[0]] * n),
           ("points on the line through two camera centres", pose_a, pose_b, [cb + (2.0 + 0.25 * j) * d for j in range(n)]),
           ("points on one plane", pose_a, pose_b, [np.array([p[0], 0.5, p[2]]) for p in pts]),
           ("points at a camera centre", pose_a, pose_b, [ca if j % 4 == 1 else cb if j % 4 == 3 else p for j, p in enumerate(pts)]),
           ("every match behind", pose_a, pose_b, [np.array([p[0], p[1], mid[2] - (p[2] - mid[2])]) for p in pts])]
    return rig, out


def two_frame_rows(base, both, one, n, seed, rebuilt, pose_a=POSE_A, pose_b=POSE_B):
    """the rows of a call that reads frames: base the well-posed scene; both(fn) -> base with fn(frame) in place of every
    frame, one(fn) -> with fn(frame) in place of the current frame; rebuilt(rig, name, pose a, pose b, points) -> the scene of
    other frames -> [(name, scene)]"""
    K = base["K"]
    rows = [("well posed", base)]
    rig, geo = geometries(n, seed, pose_a, pose_b)
    for name, pa, pb, pts in geo:
        rows.append((name, rebuilt(rig, name, pa, pb, pts)))
    rows.append(("every keypoint at its principal point", both(lambda fr: frame_uv(fr, lambda c, i, x, y: (K[c][0][2], K[c][1][2])))))
    rows.append(("one keypoint repeated", both(lambda fr: frame_uv(fr, lambda c, i, x, y: (300.0, 200.0)))))
    twice = lambda m: np.concatenate([m, m[::5]])
    rows.append(("matches given twice", dict(base, matches=[twice(m) for m in base["matches"]] if isinstance(base["matches"], list) else twice(base["matches"]))))
    rows.append(("keypoints times 1e30", both(lambda fr: frame_uv(fr, lambda c, i, x, y: (x * 1e30, y * 1e30)))))
    rows.append(("keypoints times 1e36, all inf", both(lambda fr: frame_uv(fr, lambda c, i, x, y: (x * 1e36, y * 1e36)))))
    rows.append(("a third of the keypoints inf", both(lambda fr: frame_uv(fr, lambda c, i, x, y: (x, y) if i % 3 else (INF, y) if i % 2 else (x, -INF)))))
    for col in (0, 1):
        rows.append(("NaN in keypoint column %d" % col,
                     both(lambda fr, col=col: frame_uv(fr, lambda c, i, x, y: (x, y) if i % 5 else ((NAN, y), (x, NAN))[col]))))
    rows.append(("every keypoint NaN", both(lambda fr: frame_uv(fr, lambda c, i, x, y: (NAN, y)))))
    for word, v in BAD:
        for what in ("R", "t", "centre", "twc"):
            rows.append(("%s in %s of the current frame" % (word, what), one(lambda fr, what=what, v=v: frame_entry(fr, what, v))))
    rows.append(("R times 2", one(lambda fr: frame_geom(fr, lambda c, R_: R_ * 2.0))))
    rows.append(("R a reflection", one(lambda fr: frame_geom(fr, lambda c, R_: np.asarray(REFLECT) @ R_))))
    rows.append(("R zero", one(lambda fr: frame_geom(fr, lambda c, R_: R_ * 0.0))))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# triangulate_new
# ---------------------------------------------------------------------------------------------------------------------------
def new_scaled(sc, k):
    fn = lambda fr: frame_geom(fr, fn_t=lambda v: v * k)
    return dict(sc, cur=fn(sc["cur"]), prev=fn(sc["prev"]))


@functools.lru_cache(None)
def new_rows():
    """-> [(name, scene of mapping_new_cases.py, keywords)]; frame a is the previous keyframe, frame b the current frame"""
    base = Nc.scene(NCAMS, n=NMATCH, seed=91)

    def rebuilt(rig, name, pa, pb, pts):
        a, b, matches = build_frames(rig, [pa], pb, pts, 93)[:3]
        return dict(base, K=np.array(rig[0]), prev=a[0], cur=b, matches=matches[0])

    rows = two_frame_rows(base, lambda fn: dict(base, prev=fn(base["prev"]), cur=fn(base["cur"])), lambda fn: dict(base, cur=fn(base["cur"])),
                          NMATCH, 92, rebuilt)
    for k in FRONT_SCALES:
        rows.append(("translations times %g" % k, new_scaled(base, k)))
    for word, v in (("0", 0.0), ("inf", INF), ("1e-30", 1e-30), ("1e30", 1e30)):
        rows.append(("inv_sigma2 %s" % word, dict(base, inv_sigma2=np.full(Nc.NLEVELS, v, np.float32))))
    return [(n, sc, {}) for n, sc in rows]


# ---------------------------------------------------------------------------------------------------------------------------
# triangulate_neighbours: two neighbours of 68 and 66 matches, 12 landmarks of the store in each (the baseline gate's depths)
# ---------------------------------------------------------------------------------------------------------------------------
def neigh_scaled(sc, k):
    fn = lambda fr: frame_geom(fr, fn_t=lambda v: v * k)
    return dict(sc, cur=fn(sc["cur"]), neigh=[fn(f) for f in sc["neigh"]], store={l: np.asarray(p) * k for l, p in sc["store"].items()},
                tcw=np.asarray(sc["tcw"]) * k)


def neigh_store(sc, fn):
    """fn(n, landmark id, point) -> point, n counting the store's landmarks in the order of their ids"""
    return dict(sc, store={l: np.asarray(fn(n, l, np.asarray(sc["store"][l], np.float64)), np.float64) for n, l in enumerate(sorted(sc["store"]))})


def neigh_one_landmark(sc, keep):
    """the first neighbour's features without their landmarks, but for `keep`: a depth list of one"""
    fr = sc["neigh"][0]
    lids = np.where(fr["lids"] == keep, fr["lids"], -1).astype(np.int32)
    return dict(sc, neigh=[dict(fr, lids=lids)] + list(sc["neigh"][1:]))


@functools.lru_cache(None)
def neigh_rows():
    """-> [(name, scene of mapping_cases.py, keywords)]; frame a is a neighbour, frame b the current frame"""
    base = Mc.scene(NCAMS, sizes=(NMATCH, NMATCH - 2), seed=101, zero_f=-1, n_old=12)

    def rebuilt(rig, name, pa, pb, pts):
        still = name == "the second frame did not move"
        frames, b, matches, store, fulls, full_b = build_frames(rig, [pa, pa if still else POSE_C], pb, pts, 103, n_old=12)
        matches[1] = matches[1][:NMATCH - 2]
        Ks = rig[0]
        with np.errstate(all="ignore"):
            F21 = [np.array([[Mc.fundamental(full_b[cc], full[cn], Ks[cc], Ks[cn]) for cn in range(NCAMS)] for cc in range(NCAMS)]) for full in fulls]
        Tcw = np.linalg.inv(pb)
        return dict(base, K=np.array(Ks), cur=b, neigh=frames, matches=matches, F21=F21, store=store, Rcw=Tcw[:3, :3].copy(), tcw=Tcw[:3, 3].copy())

    rows = two_frame_rows(base, lambda fn: dict(base, cur=fn(base["cur"]), neigh=[fn(f) for f in base["neigh"]]),
                          lambda fn: dict(base, cur=fn(base["cur"])), NMATCH, 102, rebuilt)
    first = sorted(l for l in base["neigh"][0]["lids"].tolist() if l in base["store"])
    rows.append(("a neighbour whose depths are all NaN", neigh_store(base, lambda n, l, p: p * NAN if l in first else p)))
    # one landmark in the first neighbour: its depth is the list and the median.  Near (its own point), and 1e6 times as far:
    # the baseline is less than a hundredth of the median then, the neighbour is skipped
    rows.append(("a neighbour with one depth", neigh_one_landmark(base, first[0])))
    rows.append(("a neighbour with one depth, far", neigh_store(neigh_one_landmark(base, first[0]), lambda n, l, p: p * 1e6 if l == first[0] else p)))
    # a NaN among finite depths: where the sort leaves it is not stated (a NaN compares false both ways), so the row holds only
    # that both stores and the restatement sort alike; the neighbour's other 11 depths are one value, the median whatever the order
    rows.append(("a neighbour whose depths are one value and a NaN", neigh_store(base, lambda n, l, p: p * NAN if l == first[0] else base["store"][first[1]] if l in first else p)))
    rows.append(("a third of the store's points inf", neigh_store(base, lambda n, l, p: p if n % 3 else np.array([p[0], p[1], INF if n % 2 else -INF]))))
    for word, v in BAD:
        R_, t = np.array(base["Rcw"]), np.array(base["tcw"])
        R_[2, 1], t[2] = v, v
        rows.append(("%s in Rcw" % word, dict(base, Rcw=R_)))
        rows.append(("%s in tcw" % word, dict(base, tcw=t)))
        F = [np.array(f) for f in base["F21"]]
        F[0][:, :, 1, 1] = v
        rows.append(("%s in every F of a neighbour" % word, dict(base, F21=F)))
    rows.append(("F times 1e30", dict(base, F21=[np.array(f) * 1e30 for f in base["F21"]])))
    rows.append(("F times 1e-30", dict(base, F21=[np.array(f) * 1e-30 for f in base["F21"]])))
    for k in FRONT_SCALES:
        rows.append(("points and translations times %g" % k, neigh_scaled(base, k)))
    for word, v in (("0", 0.0), ("inf", INF), ("1e-30", 1e-30), ("1e30", 1e30)):
        rows.append(("inv_sigma2 %s" % word, dict(base, inv_sigma2=np.full(Mc.NLEVELS, v, np.float32))))
    return [(n, sc, {}) for n, sc in rows]


# ---------------------------------------------------------------------------------------------------------------------------
# initialize: the first NINIT matches of init_cases.py's scene of seed 3, all flags set -- the smallest count at which that scene
# ends DONE (more than 50 landmarks), test_hostile_backend_cpu.py holds it to that on the restatement
# ---------------------------------------------------------------------------------------------------------------------------
NINIT = 70


def init_scaled(sc, k):
    fn = lambda fr: frame_geom(fr, fn_t=lambda v: v * k)
    return dict(sc, cur=fn(sc["cur"]), prev=fn(sc["prev"]), t=np.asarray(sc["t"]) * k, body=np.asarray(sc["body"]) * k,
                min_baseline=sc["min_baseline"] * k)


def init_entry(sc, what, value):
    R_, t, body = np.array(sc["R"], np.float64), np.array(sc["t"], np.float64), np.array(sc["body"], np.float64)
    if what == "R":
        R_[1, 2] = value
    elif what == "t":
        t[1] = value
    else:
        body[1][0] = value
    return dict(sc, R=R_, t=t, body=body)


@functools.lru_cache(None)
def init_rows():
    """-> [(name, scene of init_cases.py, keywords)]; frame a is lf_prev at the identity, frame b the current frame at T"""
    base = Ic.cut(Ic.scene(NCAMS, n=300, seed=3), NINIT)
    T = Mc.T4(np.asarray(base["R"]), np.asarray(base["t"]))

    def rebuilt(rig, name, pa, pb, pts):
        a, b, matches = build_frames(rig, [pa], pb, pts, 113)[:3]
        return dict(base, K=np.array(rig[0]), prev=a[0], cur=b, matches=matches[0], flags=np.ones(len(pts), bool), R=pb[:3, :3].copy(),
                    t=pb[:3, 3].copy(), body=np.array([np.linalg.inv(M)[:3, 3] for M in rig[1]]))

    rows = two_frame_rows(base, lambda fn: dict(base, prev=fn(base["prev"]), cur=fn(base["cur"])), lambda fn: dict(base, cur=fn(base["cur"])),
                          NINIT, 112, rebuilt, np.eye(4), T)
    # (the frame that did not move and the one that only turned have no baseline: the call ends BASELINE before a launch; with
    # min_baseline -1 the loop runs on them)
    for name in ("the second frame did not move", "pure rotation"):
        rows.append((name + ", no baseline gate", dict(row_of(rows, name)[1], min_baseline=-1.0)))
    rows.append(("matches given twice, flags too", dict(base, matches=np.concatenate([base["matches"], base["matches"][::5]]),
                                                       flags=np.concatenate([base["flags"], base["flags"][::5]]))))
    rows = [r for r in rows if r[0] != "matches given twice"]
    for word, v in BAD:
        for what in ("R", "t", "body"):
            rows.append(("%s in %s of the call" % (word, what), init_entry(base, what, v)))
        for what in ("R", "t"):
            rows.append(("%s in %s of the previous frame" % (word, what), dict(base, prev=frame_entry(base["prev"], what, v))))
        # every camera of the previous frame: every parallax is NaN, the median runs over NaN alone
        rows.append(("%s in every R of the previous frame" % word,
                     dict(base, prev=frame_geom(base["prev"], lambda c, R_, v=v: np.where(np.arange(9).reshape(3, 3) == 5, v, R_)))))
    for k in FRONT_SCALES:
        rows.append(("translations times %g, min_baseline too" % k, init_scaled(base, k)))
    for word, v in (("0", 0.0), ("inf", INF), ("1e-30", 1e-30), ("1e30", 1e30)):
        rows.append(("inv_sigma2 %s" % word, dict(base, inv_sigma2=np.full(Mc.NLEVELS, v, np.float32))))
    for word, v in (("0", 0.0), ("inf", INF), ("1e-300", 1e-300)):
        rows.append(("min_baseline %s" % word, dict(base, min_baseline=v)))
    return [(n, sc, {}) for n, sc in rows]
