"""Degenerate and hostile inputs of the pose RANSACs (test_hostile_cpu.py, test_gpu_hostile.py, scripts/header_coverage.py): one
table of named rows per call -- essential_pose, relative_pose, align_pose, ransac_pose (both solvers) -- built from the family's
*_cases.py helpers, seeded, at N = 64 matches or pairs and H = 64 hypotheses, the smallest shape at which a wave of hypotheses and
a partly filled tile both exist; 8 cameras for relative_pose, 4 for ransac_pose.  What a front end hands these calls during a
bootstrap: a camera that has not moved, pure rotation, every match the same point, collinear and coplanar points, overflowed,
infinite and NaN keypoints, and inputs scaled until an intermediate product is subnormal.

A row is (name, arguments ..., keywords of the call).  The tables are built once and never changed by a test."""
import functools
import math

import numpy as np

import align_cases as AC
import ess_cases as EC
import pose_cases as PC
import rel_cases as RC
import rel_ref as RR
import sac_cases as SC
import sac_ref as S

N, H = 64, 64
INF, NAN = math.inf, math.nan
SEEDS = (1 << 32, (1 << 63) + 1, 2 ** 64 - 1)     # what only the upper half of the job's seed tells apart from 0, 1 and 2^32 - 1


def f32(v):
    """a double as the float the call receives: overflow gives inf"""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------------------
# essential_pose: a match is (u1, v1, u2, v2)
# ---------------------------------------------------------------------------------------------------------------------------
def ess_two_frames(R, t, uv1, depth):
    """frame 1's keypoints uv1 at the depths -> matches with frame 2's keypoints at the pose (R, t) = c1_T_c2, rounded to float"""
    out = []
    for (u, v), z in zip(uv1, depth):
        X2 = R.T @ (EC.unproject(u, v, z) - t)
        out.append((f32(u), f32(v), *[f32(w) for w in EC.project(X2)]))
    return out


@functools.lru_cache(None)
def ess_rows():
    """-> [(name, matches, keywords of EC.run / ER.ransac)]"""
    truth, base, moved = EC.scene("general", n=N, seed=0, noise=0.1)
    R, t = truth
    rng = np.random.default_rng(7)
    uv1 = [(m[0], m[1]) for m in base]
    rows = [("well posed", base, {})]
    # (frame 1 of the scene of seed 2: among its samples are roots whose (x, y) is not finite -- a zero pivot of C(z) -- and
    # Gauss-Newton steps to a value that is not finite; the scene of seed 0 has neither)
    still = EC.scene("general", n=N, seed=2, noise=0.1)[1]
    rows.append(("zero motion", [(m[0], m[1], m[0], m[1]) for m in still], {}))
    rows.append(("pure rotation", ess_two_frames(EC.rodrigues([0.05, -0.08, 0.03]), np.zeros(3), uv1, rng.uniform(2.0, 10.0, N)), {}))
    rows.append(("one match 64 times", [base[0]] * N, {}))
    rows.append(("two matches alternating", [base[i % 2] for i in range(N)], {}))
    # a line of space seen in both frames: a line in both images
    line = [np.array([-3.0, -1.0, 4.0]) + s * np.array([0.1, 0.03, 0.05]) for s in range(N)]
    rows.append(("collinear", [(*[f32(w) for w in EC.project(X)], *[f32(w) for w in EC.project(R.T @ (X - t))]) for X in line], {}))
    rows.append(("keypoints times 1e30", [tuple(f32(w * 1e30) for w in m) for m in base], {}))
    rows.append(("keypoints times 1e36, all inf", [tuple(f32(w * 1e36) for w in m) for m in base], {}))
    rows.append(("a third of the rows inf", [m if i % 3 else ((INF,) + m[1:] if i % 2 else m[:3] + (-INF,)) for i, m in enumerate(base)], {}))
    # (a threshold that nothing misses: a model of a sample with a NaN member is counted on rows with a NaN)
    rows.append(("NaN in every column, wide threshold", [m if i % 5 else m[:(i // 5) % 4] + (NAN,) + m[(i // 5) % 4 + 1:] for i, m in enumerate(base)],
                 dict(threshold_px=1e4)))
    rows.append(("every row NaN", [(NAN, m[1], m[2], m[3]) for m in base], {}))
    pp = (f32(EC.CAM["u0"]), f32(EC.CAM["v0"]))
    rows.append(("half the rows at the principal point", [m if i % 2 else pp + pp for i, m in enumerate(base)], {}))
    plane = EC.exact_matches(np.random.default_rng(8), "coplanar", N, R, t, off_plane=0)
    rows.append(("all on one plane", [tuple(f32(w) for w in m) for m in plane], {}))
    # frame 2 is frame 1 shifted by whole pixels: x2 = x1 + const, the rank of the sample's five equations drops
    rows.append(("a shift of the image", [(m[0], m[1], f32(m[0] + 16.0), f32(m[1] - 8.0)) for m in base], {}))
    # keypoints on a lattice of 4 x 4 pixels around the principal point: samples with repeated and mirrored members
    rows.append(("a lattice around the principal point", [(f32(pp[0] + 64.0 * (i % 4 - 1.5)), f32(pp[1] + 64.0 * (i // 4 % 4 - 1.5)),
                                                            f32(pp[0] + 64.0 * (i % 4 - 1.5) + (i // 16)), f32(pp[1] + 64.0 * (i // 4 % 4 - 1.5)))
                                                           for i in range(N)], {}))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# relative_pose: a match is (cam1, u1, v1, cam2, u2, v2)
# ---------------------------------------------------------------------------------------------------------------------------
NCAMS_REL = 8


def rel_scene(R, t, seed, only_cam0=False, ncams=NCAMS_REL):
    """N noise-free matches of RC.exact_match at the pose (R, t), the keypoints rounded to float"""
    rng = np.random.default_rng(seed)
    cams = RC.outward_rig(ncams)
    rig = RC.rig_arrays(cams)
    out = []
    while len(out) < N:
        m = RC.exact_match(rng, cams, rig, R, t)
        if not only_cam0 or (m[0] == 0 and m[3] == 0):
            out.append((m[0], f32(m[1]), f32(m[2]), m[3], f32(m[4]), f32(m[5])))
    return out


def rel_scaled(m, k):
    return (m[0], f32(m[1] * k), f32(m[2] * k), m[3], f32(m[4] * k), f32(m[5] * k))


@functools.lru_cache(None)
def rel_rows():
    """-> [(name, cams, matches, keywords of RC.run / RR.ransac)]"""
    cams, truth, base, moved = RC.scene(NCAMS_REL, N, 0, moved=0.1)
    Rt, tt = np.asarray(RC.TRUTH[0]), np.asarray(RC.TRUTH[1])
    rows = [("well posed", cams, base, {})]
    rows.append(("zero motion", cams, [m[:3] + m[:3] for m in base], {}))
    rows.append(("pure translation", cams, rel_scene(np.eye(3), tt, 1), {}))
    rows.append(("pure rotation", cams, rel_scene(Rt, np.zeros(3), 2), {}))
    rows.append(("one match 64 times", cams, [base[0]] * N, {}))
    rows.append(("two matches alternating", cams, [base[i % 2] for i in range(N)], {}))
    rows.append(("all matches in camera 0", cams, rel_scene(Rt, tt, 3, only_cam0=True), {}))
    rows.append(("keypoints times 1e30", cams, [rel_scaled(m, 1e30) for m in base], {}))
    rows.append(("keypoints times 1e36, all inf", cams, [rel_scaled(m, 1e36) for m in base], {}))
    rows.append(("every fifth row inf", cams, [m if i % 5 else (m[0], INF, m[2], m[3], m[4], -INF) for i, m in enumerate(base)], {}))
    rows.append(("NaN in every column, wide threshold", cams,
                 [m if i % 5 else tuple(NAN if k == (1, 2, 4, 5)[(i // 5) % 4] else w for k, w in enumerate(m)) for i, m in enumerate(base)],
                 dict(threshold=1.5)))
    rows.append(("every row NaN", cams, [(m[0], NAN) + m[2:] for m in base], {}))
    # every keypoint at its camera's principal point: every ray is a camera's axis, at most 8 distinct rows of the 17
    rows.append(("every keypoint at the principal point", cams, [(m[0], 640.0, 360.0, m[3], 640.0, 360.0) for m in base], {}))
    # a rig whose cameras all sit at the body's origin: central, the scale is not observable
    central = [dict(c, t=[0.0, 0.0, 0.0]) for c in cams]
    rows.append(("every camera at the body's origin", central, base, {}))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# align_pose: pair i is (p1[i], p2[i]); every row runs in both modes
# ---------------------------------------------------------------------------------------------------------------------------
def _pairs(p1, p2):
    return np.ascontiguousarray(p1, np.float64).reshape(-1, 3), np.ascontiguousarray(p2, np.float64).reshape(-1, 3)


@functools.lru_cache(None)
def align_rows():
    """-> [(name, p1, p2, keywords of AC.run / AC.ref without the mode)]"""
    truth, p1, p2, moved = AC.scene(n=N, seed=0, moved=6)
    R, t = np.asarray(AC.TRUTH[0]), np.asarray(AC.TRUTH[1])
    s = np.arange(N, dtype=np.float64)[:, None]
    rows = [("well posed", p1, p2, {})]
    rows.append(("zero motion", p2.copy(), p2, {}))
    rows.append(("coincident", *_pairs(np.tile(p2[:1] @ R.T + t, (N, 1)), np.tile(p2[:1], (N, 1))), {}))
    line = np.array([0.5, -1.0, 3.0]) + s * np.array([0.0625, 0.03125, 0.125])
    rows.append(("on a line", *_pairs(line @ R.T + t, line), {}))
    plane = p2 * np.array([1.0, 1.0, 0.0]) + np.array([0.0, 0.0, 5.0])
    rows.append(("on a plane", *_pairs(plane @ R.T + t, plane), {}))
    rows.append(("times 1e200", p1 * 1e200, p2 * 1e200, {}))
    rows.append(("times 1e-200", p1 * 1e-200, p2 * 1e-200, {}))
    # (p1 - R p2 - t scales with the points, so the limits do: the squares of the distances are subnormal, the fit is valid)
    rows.append(("times 1e-158, the limits too", p1 * 1e-158, p2 * 1e-158, dict(threshold=AC.THRESHOLD * 1e-158, inlier_dist=AC.INLIER_DIST * 1e-158)))
    bad1, bad2 = p1.copy(), p2.copy()
    bad1[0::7, 0], bad2[3::7, 2], bad1[5::7, 1] = INF, -INF, NAN
    rows.append(("inf and NaN rows", bad1, bad2, {}))
    rows.append(("every row NaN", *_pairs(np.where(np.arange(3) == 1, NAN, p1), p2), {}))
    rows.append(("a reflection", *_pairs((p2 * np.array([1.0, 1.0, -1.0])) @ R.T + t, p2), {}))
    # three distinct points, each 21 or 22 times: every sample is complete, most are coincident or collinear
    three = p2[np.arange(N) % 3]
    rows.append(("three points repeated", *_pairs(three @ R.T + t, three), {}))
    # no pair is within the threshold of any model, its own sample's included: the winner is hypothesis 0 with no inlier, and the
    # refit over no pair is refused
    rows.append(("a threshold that nothing meets", p1, p2, dict(threshold=1e-300)))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# ransac_pose: an observation is (cam, u, v, octave, X); every row runs with both solvers and in both forms
# ---------------------------------------------------------------------------------------------------------------------------
NCAMS_SAC = 4


def sac_prefix(obs, match, n_matches):
    n = next((i for i, k in enumerate(match) if k >= n_matches), len(obs))
    return obs[:n], match[:n]


def sac_thin(cams, seed):
    """N landmarks, each seen by one camera of the rig `cams` at SC.scene's pose, noise-free, the keypoints rounded to float"""
    rng = np.random.default_rng(seed)
    Rt, tt = PC.rot([0.3, -0.2, 1.0], 0.7), np.array([1.5, -0.7, 0.3])
    truth = (PC.rows_of(Rt), [float(v) for v in tt])
    obs = []
    for i in range(N):
        c = i % len(cams)
        z = rng.uniform(2, 10)
        q = np.array([rng.uniform(-1.0, 1.0) * z, rng.uniform(-0.55, 0.55) * z, z])
        X = [float(v) for v in Rt @ (np.asarray(cams[c]["R"]) @ q + np.asarray(cams[c]["t"])) + tt]
        px, py = PC.project(cams, truth, c, X)
        obs.append((c, f32(px), f32(py), 0, X))
    return obs


def sac_points(obs, fn):
    return [(o[0], o[1], o[2], o[3], [float(v) for v in fn(i, np.asarray(o[4], np.float64))]) for i, o in enumerate(obs)]


@functools.lru_cache(None)
def sac_rows():
    """-> [(name, cams, obs, match or None, keywords of SC.run / S.ransac)]"""
    cams, truth, obs, match, moved = SC.scene(NCAMS_SAC, nlm=80, seed=13)
    obs, match = sac_prefix(obs, match, N)
    assert match[-1] + 1 == N
    rows = [("well posed", cams, obs, match, {})]
    rows.append(("one observation 64 times", cams, [obs[0]] * N, None, {}))
    own = [o for o in obs if o[0] == obs[0][0]]
    rows.append(("one landmark under many keypoints", cams, [(o[0], o[1], o[2], o[3], obs[0][4]) for o in (own * N)[:N]], None, {}))
    rows.append(("points on a line", cams, sac_points(obs, lambda i, X: np.asarray(obs[0][4]) + i * np.array([0.125, 0.0625, -0.03125])), match, {}))
    rows.append(("points at the origin", cams, sac_points(obs, lambda i, X: X * 0.0), match, {}))
    rows.append(("points times 1e200", cams, sac_points(obs, lambda i, X: X * 1e200), match, {}))
    rows.append(("points times 1e-200", cams, sac_points(obs, lambda i, X: X * 1e-200), match, {}))
    # every second row is observation 0: samples with a repeated member among samples without one
    # (without the match array a landmark that two cameras see is two matches: the rig solver draws one point twice)
    rows.append(("every observation its own match", cams, obs[:N], None, {}))
    # every second row is one observation, of a camera that holds enough others for complete samples: samples that hold one point
    # twice, under two indices, among samples that hold it once -- two equal points make Grunert's quartic biquadratic (q == 0)
    window = obs[14:14 + N]
    rows.append(("half the rows one observation", cams, [o if i % 2 else window[0] for i, o in enumerate(window)], None, {}))
    rows.append(("keypoints times 1e30", cams, [(o[0], f32(o[1] * 1e30), f32(o[2] * 1e30), o[3], o[4]) for o in obs], match, {}))
    rows.append(("keypoints times 1e36, all inf", cams, [(o[0], f32(o[1] * 1e36), f32(o[2] * 1e36), o[3], o[4]) for o in obs], match, {}))
    bad = []
    for i, o in enumerate(obs):
        X = list(o[4])
        if i % 11 == 3:
            X[i % 3] = NAN if i % 2 else INF
        bad.append((o[0], INF if i % 7 == 0 else o[1], -INF if i % 7 == 4 else NAN if i % 13 == 5 else o[2], o[3], X))
    rows.append(("inf and NaN rows", cams, bad, match, {}))
    rows.append(("every point NaN", cams, sac_points(obs, lambda i, X: X * NAN), match, {}))
    central = [dict(c, t=[0.0, 0.0, 0.0]) for c in cams]
    thin = sac_thin(central, 5)
    rows.append(("every camera at the body's origin", central, thin, None, {}))
    # a central rig's problem scales with its points.  At 1e-155 every hypothesis still has its model, at 1e-165 none has: at 1e-160
    # the squares of the distances between the points are subnormal, 14 (central) and 10 (rig) of the 64 hypotheses keep a model
    rows.append(("central rig, points times 1e-160", central, sac_points(thin, lambda i, X: X * 1e-160), None, {}))
    rows.append(("one observation per landmark, offset rig", cams, sac_thin(cams, 6), None, {}))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the well-posed row of each call, for the seeds
# ---------------------------------------------------------------------------------------------------------------------------
def well_posed(rows):
    assert rows[0][0] == "well posed"
    return rows[0]
