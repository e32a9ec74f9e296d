"""Inputs and helpers of the point-cloud alignment tests (test_align_cpu.py, test_gpu_align.py): the solver's seeded cases, the
seeded scene with a known true pose, rows written out by hand, and the comparison of a LocalMap.align_pose result against the
restatement (align_ref.py), floats as raw bytes with no tolerance.

A pose is (R, t) = b1_T_b2: X_1 = R X_2 + t; pair i is (p1[i], p2[i])."""
import math

import numpy as np

import align_ref as AR
import pose_cases as PC
import pose_ref as P
import rel_cases as RC
import sac_cases as SC

NAMES = {AR.OK: "OK", AR.NO_OBS: "NO_OBS", AR.NO_MODEL: "NO_MODEL"}
THRESHOLD, INLIER_DIST = 0.2, 0.1     # the reference's values (FrontEnd.cpp:4480, :4504)
TRUTH = RC.TRUTH


def cayley(w):
    """the rotation of the Cayley parameters w: a = w / 2, ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a)"""
    a = 0.5 * np.asarray(w, np.float64)
    aa = float(a @ a)
    ax = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return ((1.0 - aa) * np.eye(3) + 2.0 * np.outer(a, a) + 2.0 * ax) / (1.0 + aa)


def cloud(rng, n):
    """n points of frame 2: x in +-4, y in +-3, depth 2 - 10"""
    return np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(2, 10, n)], axis=1)


def solver_cases(npts, count, seed, noise=0.0):
    """-> [(truth (R, t), p1, p2)]: rotation Cayley of N(0, 0.05) per axis, translation N(0, 0.3 m) per axis, p1 = R p2 + t (+
    N(0, noise) per axis)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        R, t = cayley(rng.normal(scale=0.05, size=3)), rng.normal(scale=0.3, size=3)
        p2 = cloud(rng, npts)
        p1 = p2 @ R.T + t
        if noise:
            p1 = p1 + rng.normal(scale=noise, size=p1.shape)
        out.append(((R, t), p1, p2))
    return out


def scene(n=200, seed=0, moved=20, noise=0.02, step=1.0):
    """-> (truth, p1, p2, is_moved): n pairs at b1_T_b2 = TRUTH; the first `moved` pairs of a seeded permutation have p1 moved by
    `step` m in a seeded direction, the others get N(0, noise m) per axis on p1"""
    rng = np.random.default_rng(2000 + seed)
    R, t = TRUTH
    p2 = cloud(rng, n)
    p1 = p2 @ np.asarray(R).T + np.asarray(t)
    is_moved = np.zeros(n, bool)
    is_moved[rng.permutation(n)[:moved]] = True
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    e = rng.normal(scale=noise, size=(n, 3)) if noise else np.zeros((n, 3))
    p1 = np.where(is_moved[:, None], p1 + step * direction, p1 + e)
    return (PC.rows_of(R), [float(v) for v in t]), np.ascontiguousarray(p1), np.ascontiguousarray(p2), [bool(v) for v in is_moved]


def first_seed(limit=64, **kw):
    """the first seed of scene() for which no moved pair is within THRESHOLD of its partner at the true pose"""
    for seed in range(limit):
        truth, p1, p2, mv = scene(seed=seed, **kw)
        d = AR.dist_many(truth, p1, p2)
        if not any(d[i] < THRESHOLD for i, v in enumerate(mv) if v):
            return seed
    raise AssertionError("no seed")


def pose_error(pose, truth):
    """(max |dR_ij|, |dt| in m)"""
    return SC.pose_error(pose, truth)


def solver_of(mc):
    """the `solve` argument of the restatement: mcorb_align_solve -> (R rows, t) or None"""
    def solve(p1, p2, member):
        got = mc.align_solve(p1, p2, member)
        return None if got is None else SC.lists(got)
    return solve


def run(mc, lm, p1, p2, mode=AR.SAC, lids1=None, **kw):
    kw.setdefault("threshold", THRESHOLD)
    kw.setdefault("inlier_dist", INLIER_DIST)
    if lids1 is not None:
        return lm.align_pose(p2, lids1=lids1, mode=mode, **kw)
    return lm.align_pose(p2, pts1=np.asarray(p1, np.float64).reshape(-1, 3), mode=mode, **kw)


def ref(mc, p1, p2, mode=AR.SAC, **kw):
    kw.setdefault("threshold", THRESHOLD)
    kw.setdefault("inlier_dist", INLIER_DIST)
    return AR.run(p1, p2, solver_of(mc), mode=mode, **kw)


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or AR.bits(float(a)) == AR.bits(float(b))


def same(got, want, what=""):
    """an AlignResult against align_ref.run's dict"""
    assert got.status == want["status"], (what, "status", NAMES[got.status], NAMES[want["status"]])
    assert got.used == want["used"], (what, "used", got.used, want["used"])
    assert P.same_bits(got.R.tolist(), want["R"]) and P.same_bits(got.t.tolist(), want["t"]), (what, "answer", got.R, want["R"])
    assert P.same_bits(got.sac_R.tolist(), want["sac_R"]) and P.same_bits(got.sac_t.tolist(), want["sac_t"]), (what, "winner")
    assert same_float(got.mean_error, want["mean_error"]), (what, "mean_error", got.mean_error, want["mean_error"])
    assert got.best_hypothesis == want["best"], (what, "best", got.best_hypothesis, want["best"])
    assert list(got.sample) == list(want["sample"]), (what, "sample", got.sample, want["sample"])
    assert got.n_inliers == want["n_inliers"], (what, "n_inliers", got.n_inliers, want["n_inliers"])
    assert got.sac_n_inliers == want["sac_n_inliers"], (what, "sac_n_inliers", got.sac_n_inliers, want["sac_n_inliers"])
    assert got.n_models == want["n_models"], (what, "n_models", got.n_models, want["n_models"])
    assert got.n_matches == len(want["inliers"]), (what, "n_matches")
    assert got.inliers.tolist() == [bool(v) for v in want["inliers"]], (what, "inliers")


def same_counts(lm, want, what=""):
    """the counts of all hypotheses through the read-back"""
    count, valid = lm.last_align_counts()
    assert valid.tolist() == [m is not None for m in want["models"]], (what, "models")
    assert count.tolist() == [c or 0 for c in want["counts"]], (what, "counts")


def same_results(a, b, what=""):
    """two AlignResults on the bytes"""
    for f in ("R", "t", "sac_R", "sac_t"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (what, f)
    assert same_float(a.mean_error, b.mean_error), (what, "mean_error")
    for f in ("status", "used", "n_inliers", "n_matches", "sac_n_inliers", "best_hypothesis", "sample", "n_models"):
        assert getattr(a, f) == getattr(b, f), (what, f)
    assert a.inliers.tolist() == b.inliers.tolist(), (what, "inliers")


# ---- rows written out by hand ----
def collinear(as_float=False):
    """three pairs on a line, frame 1 = frame 2 moved by TRUTH; as_float: every coordinate rounded to float afterwards"""
    R, t = np.asarray(TRUTH[0]), np.asarray(TRUTH[1])
    p2 = np.array([[0.5, -1.0, 3.0], [1.25, -0.25, 4.5], [2.75, 1.25, 7.5]])
    p1 = p2 @ R.T + t
    if as_float:
        p1, p2 = p1.astype(np.float32).astype(np.float64), p2.astype(np.float32).astype(np.float64)
    return p1, p2


def coincident():
    p2 = np.array([[1.0, 2.0, 3.0]] * 3)
    return p2 + 0.5, p2


def half_turn(n=40, seed=4):
    """-> (truth, p1, p2): a rotation by 180 degrees about a seeded axis -- the quaternion's scalar part is 0"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    R, t = 2.0 * np.outer(a, a) - np.eye(3), np.array([0.3, -0.2, 0.1])
    p2 = cloud(rng, n)
    return (R, t), p2 @ R.T + t, p2
