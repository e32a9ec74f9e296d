"""Chosen minimal problems for the five solver hooks and their device twins (test_solver_hook_cases_cpu.py,
test_gpu_solver_hooks.py): one table of named problems per solver -- sac (Grunert's quartic, one camera), rig (its generalized
continuation, with the fourth, disambiguating observation), rel (17 points), ess (five points), align (three points / least
squares) -- built from the families' *_cases.py helpers and restatements, so nothing is stated twice:

  the CPU suite's own solver inputs   the seeded cases test_sac_cpu.py, test_sac_rig_cpu.py, test_rel_cpu.py, test_align_cpu.py and
                                      test_ess_cpu.py hand their hooks, and their rows written out by hand
  the hostile tables' samples         for every row of hostile_cases.py, the sample of every hypothesis h < H by the restatement's
                                      draws, cut out of the scene: what the estimators reach on those rows by luck, as direct rows
  rows no scene can hold              coincident and collinear points, everything at the origin, points and keypoints scaled to
                                      where squares overflow or are subnormal, a NaN and an inf in each operand position in turn,
                                      one-camera and origin rigs, member masks and pair counts around one fold workgroup
  rig rows by the root that wins      seeded problems found on the host hook: the winner is root k, and only root k has a pose

A row is (name, hostile, problem ...): `hostile` is False for the noise-free seeded cases and True for everything else.  The
tables are built once and never changed by a test.  host_* runs a table through the host hook, one call a problem, and dev_*
through the device twin, one launch a table; both give the same tuple of arrays -- the count, every model slot, zero behind the
count -- so whole buffers compare."""
import functools
import math

import numpy as np

import align_cases as AC
import align_ref as AR
import ess_cases as EC
import ess_ref as ER
import hostile_cases as HC
import pose_cases as PC
import rel_cases as RC
import rel_ref as RR
import sac_cases as SC
import sac_ref as S
import sac_rig_cases as SRC
import sac_rig_ref as SR
import track_cases as T

NAN, INF = math.nan, math.inf
CUTS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257)     # around an EssGroup workgroup (4), a wave of quads (16), a wave of lanes (64)
f32 = HC.f32


def names(rows):
    return [r[0] for r in rows]


def mixed(rows):
    """the hostile rows interleaved one for one with the others, what is left of the longer list behind them -> row indices"""
    bad = [i for i, r in enumerate(rows) if r[1]]
    good = [i for i, r in enumerate(rows) if not r[1]]
    k = min(len(bad), len(good))
    return [i for pair in zip(bad[:k], good[:k]) for i in pair] + bad[k:] + good[k:]


def poke(values, at, v):
    """a nested list of numbers with the at-th number (row-major) replaced by v"""
    a = np.array(values, np.float64)
    a.reshape(-1)[at] = v
    return a.tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# ess: (name, hostile, five matches (u1, v1, u2, v2) as doubles), the camera EC.CAM
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ess_table():
    rows = []
    for kind in ("general", "coplanar"):
        rows += [("%s %d" % (kind, i), False, five) for i, (_, five) in enumerate(EC.solver_cases(kind))]
    base = EC.solver_cases("general")[0][1]
    for name, matches, kw in HC.ess_rows():
        for h in range(HC.H):
            smp, ok = ER.sample(0, h, len(matches))
            assert ok
            rows.append(("%s, h %d" % (name, h), True, [tuple(float(w) for w in matches[i]) for i in smp]))
    pp = (EC.CAM["u0"], EC.CAM["v0"])
    rows.append(("two coincident", True, [base[0], base[0]] + base[2:]))
    rows.append(("three coincident", True, [base[0]] * 3 + base[3:]))
    rows.append(("five coincident", True, [base[0]] * 5))
    rows.append(("collinear in both images", True, [(100.0 + 40 * i, 200.0 + 10 * i, 130.0 + 40 * i, 190.0 + 10 * i) for i in range(5)]))
    rows.append(("all at the principal point", True, [pp + pp] * 5))
    rows.append(("all at the origin", True, [(0.0, 0.0, 0.0, 0.0)] * 5))
    for k in (1e30, 1e36, 1e155, 1e200, 1e-30, 1e-200):
        rows.append(("keypoints times %g, as doubles" % k, True, [tuple(w * k for w in m) for m in base]))
    for at in range(20):
        for what, v in (("NaN", NAN), ("inf", INF), ("-inf", -INF)):
            rows.append(("%s at number %d" % (what, at), True, [tuple(m) for m in poke(base, at, v)]))
    assert len(set(names(rows))) == len(rows)
    return rows


# the rows of the table whose hypothesis has a rejected root between two kept ones, with tests/cpp/ess_roots.cpp's print of
# its real roots in ascending order (1 kept, 0 rejected): test_solver_hook_cases_cpu.py holds the list to that program
ESS_BETWEEN = (
    ("zero motion, h 31", "1011"), ("pure rotation, h 20", "100111"), ("pure rotation, h 26", "100001"), ("pure rotation, h 54", "1010"),
    ("keypoints times 1e30, h 1", "10010000"), ("keypoints times 1e30, h 2", "10100000"), ("keypoints times 1e30, h 5", "001001"),
    ("keypoints times 1e30, h 9", "0101"), ("keypoints times 1e30, h 10", "010100"), ("keypoints times 1e30, h 11", "010100"),
    ("keypoints times 1e30, h 21", "00100010"), ("keypoints times 1e30, h 25", "010100"), ("keypoints times 1e30, h 39", "100100"),
    ("keypoints times 1e30, h 43", "010010"), ("keypoints times 1e30, h 45", "001010"), ("keypoints times 1e30, h 48", "100100"),
    ("keypoints times 1e30, h 50", "100100"), ("keypoints times 1e30, h 51", "010100"), ("keypoints times 1e30, h 52", "1010"),
    ("keypoints times 1e30, h 54", "101000"), ("keypoints times 1e30, h 57", "10100000"), ("keypoints times 1e30, h 58", "100100"),
    ("keypoints times 1e30, h 61", "001001"), ("a shift of the image, h 4", "1101"), ("a shift of the image, h 5", "101111"),
    ("a shift of the image, h 9", "111101"), ("a shift of the image, h 29", "1101"), ("a shift of the image, h 31", "101111"),
    ("a shift of the image, h 32", "111011"), ("a shift of the image, h 33", "111011"), ("a shift of the image, h 36", "110111"),
    ("a shift of the image, h 37", "111011"), ("a shift of the image, h 48", "111011"), ("a shift of the image, h 57", "1101"),
    ("a shift of the image, h 58", "1011"), ("a shift of the image, h 62", "1101"), ("a lattice around the principal point, h 20", "101110"))


def ess_arrays(rows):
    a = np.array([r[2] for r in rows], np.float64).reshape(len(rows), 5, 4)
    return np.ascontiguousarray(a[:, :, 0:2]), np.ascontiguousarray(a[:, :, 2:4])


def host_ess(mc, rows):
    cc = EC.to_cam(mc)
    uv1, uv2 = ess_arrays(rows)
    count, E, z = np.zeros(len(rows), np.int32), np.zeros((len(rows), 10, 9)), np.zeros((len(rows), 10))
    for i in range(len(rows)):
        models, roots = mc.ess_solve(cc, uv1[i], uv2[i], with_roots=True)
        count[i] = len(models)
        for k, (M, r) in enumerate(zip(models, roots)):
            E[i, k], z[i, k] = M.reshape(9), r
    return count, E, z


def dev_ess(mc, rows, device=0):
    cc = EC.to_cam(mc)
    return mc.dev_ess_solve([cc] * len(rows), *ess_arrays(rows), device=device)


# ---------------------------------------------------------------------------------------------------------------------------
# views of the rigs: one track_view per list of camera dicts, kept
# ---------------------------------------------------------------------------------------------------------------------------
_VIEWS = {}


def view_of(mc, cams):
    if id(cams) not in _VIEWS:
        _VIEWS[id(cams)] = (cams, PC.to_cams(mc, cams))
    return _VIEWS[id(cams)][1]


def scaled_points(X, k):
    return (np.asarray(X, np.float64) * k).tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# sac: (name, hostile, cams, camera index, uv 3 x 2 floats, X 3 x 3)
# ---------------------------------------------------------------------------------------------------------------------------
FLAT = PC.flat_rig()
HAND_UV = ([[0.0, 0.0], [0.1, 0.0], [0.2, 0.0]], [[0.0, 0.0], [0.0, 0.0], [0.2, 0.1]])
HAND_X = ([[0.0, 0.0, 4.0], [0.4, 0.0, 4.0], [0.8, 0.0, 4.0]], [[0.0, 0.0, 4.0], [0.0, 0.0, 4.0], [0.8, 0.4, 4.0]])


def no_scene_three(cams, c, uv, X):
    """the rows no scene can hold around one well-posed problem -> [(name, uv, X)]"""
    uv, X = [list(p) for p in uv], np.asarray(X, np.float64).tolist()
    out = [("two coincident", [uv[0], uv[0], uv[2]], [X[0], X[0], X[2]]),
           ("three coincident", [uv[0]] * 3, [X[0]] * 3),
           ("collinear points", uv, [(np.asarray(X[0]) + i * np.array([0.5, 0.25, -0.125])).tolist() for i in range(3)]),
           ("points at the origin", uv, [[0.0] * 3] * 3)]
    for e in (155, 160, 165):
        for sign in (1, -1):
            out.append(("points times 1e%+d" % (sign * e), uv, scaled_points(X, 10.0 ** (sign * e))))
    for k in (1e30, 1e36):
        out.append(("keypoints times %g" % k, [[f32(w * k) for w in p] for p in uv], X))
    for what, v in (("NaN", NAN), ("inf", INF)):
        out += [("%s at keypoint number %d" % (what, at), poke(uv, at, v), X) for at in range(6)]
        out += [("%s at point number %d" % (what, at), uv, poke(X, at, v)) for at in range(9)]
    return out


@functools.lru_cache(None)
def sac_table():
    rows = []
    cases = SC.solver_cases()
    one = [cases[0][0]]
    for i, (cam, truth, uv, X) in enumerate(cases):
        rows.append(("seeded %d" % i, False, one, 0, uv, X.tolist()))
    for k in range(2):
        rows.append(("by hand %d" % k, True, FLAT, 0, HAND_UV[k], HAND_X[k]))
    for name, cams, obs, match, kw in HC.sac_rows():
        cons = S.consensus(obs, match)[0]
        for h in range(HC.H):
            s, ok = S.sample(0, h, obs, cons)
            if ok:
                three = [obs[i] for i in s[:3]]
                rows.append(("%s, h %d" % (name, h), True, cams, three[0][0], [[o[1], o[2]] for o in three], [list(o[4]) for o in three]))
    cam, truth, uv, X = cases[1]
    rows += [(name, True, one, 0, u, x) for name, u, x in no_scene_three(one, 0, uv, X)]
    assert len(set(names(rows))) == len(rows)
    return rows


def host_sac(mc, rows):
    count, R, t = np.zeros(len(rows), np.int32), np.zeros((len(rows), 4, 9)), np.zeros((len(rows), 4, 3))
    for i, (name, hostile, cams, c, uv, X) in enumerate(rows):
        poses = mc.sac_solve(view_of(mc, cams), c, uv, X)
        count[i] = len(poses)
        for k, (Rk, tk) in enumerate(poses):
            R[i, k], t[i, k] = Rk.reshape(9), tk
    return count, R, t


def dev_sac(mc, rows, device=0):
    return mc.dev_sac_solve([view_of(mc, r[2]) for r in rows], [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows], device=device)


# ---------------------------------------------------------------------------------------------------------------------------
# rig: (name, hostile, cams, camera indices 4, uv 4 x 2 floats, X 4 x 3): the fourth observation disambiguates
# ---------------------------------------------------------------------------------------------------------------------------
RIG_NCAMS = (1, 4, 8)
# (seed, index) into rig_chunk(seed): what rig_search found on mcorb_host_sac_rig_roots, every class within its first 128
# problems -- the winner is root k among at least two roots with a pose; only root k has a pose
RIG_BEST = {0: [(1000, 6), (1000, 7)], 1: [(1000, 22), (1000, 25)], 2: [(1000, 9), (1000, 16)], 3: [(1000, 36), (1001, 39)]}
RIG_ONLY = {0: [(1000, 0), (1000, 1)], 1: [(1000, 5), (1000, 10)], 2: [(1000, 2), (1000, 4)], 3: [(1000, 13), (1000, 17)]}
RIG_CHUNK = 64


def fourth(cams, truth, c, x=0.11, y=-0.07, z=5.0):
    """a noise-free fourth observation in camera c at the pose truth = (Rwb, twb), as SRC.solver_cases places its three"""
    cam = cams[c]
    u, v = PC.f32(cam["fx"] * x + cam["s"] * y + cam["u0"]), PC.f32(cam["fy"] * y + cam["v0"])
    f = np.asarray(S.bearing(cam, u, v))
    pb = np.asarray(cam["R"]) @ (f / f[2] * z) + np.asarray(cam["t"])
    return c, (u, v), (truth[0] @ pb + truth[1]).tolist()


def with_fourth(cams, case, i):
    truth, ci, uv, X = case
    c, q, X4 = fourth(cams, truth, i % len(cams), 0.11 + 0.001 * (i % 7), -0.07 + 0.002 * (i % 5))
    return list(ci) + [c], [list(p) for p in uv] + [list(q)], np.asarray(X).tolist() + [X4]


@functools.lru_cache(None)
def rig_chunk(seed):
    """RIG_CHUNK seeded four-observation problems on the outward rig of 4 cameras"""
    cases = SRC.solver_cases(4, n=RIG_CHUNK, seed=seed)[1]
    return RIG_CAMS[4], [with_fourth(RIG_CAMS[4], case, i) for i, case in enumerate(cases)]


RIG_CAMS = {n: SC.outward_rig(n) for n in RIG_NCAMS}
RIG_CENTRAL = [dict(c, t=[0.0, 0.0, 0.0]) for c in RIG_CAMS[4]]


def rig_search(mc, limit=100000, keep=2):
    """the search behind RIG_BEST and RIG_ONLY: the chunks of seeds 1000, 1001, .. on the host hook, at most `limit` problems ->
    ({k: [(seed, index)]} where root k wins among at least two roots with a pose, the same where only root k has one, problems
    looked at, how often each mask came up)"""
    best, only, masks, seen = {k: [] for k in range(4)}, {k: [] for k in range(4)}, {}, 0
    seed = 1000
    while seen < limit and any(len(v) < keep for v in list(best.values()) + list(only.values())):
        cams, probs = rig_chunk(seed)
        for i, (ci, uv, X) in enumerate(probs):
            poses, mask, b, _ = mc.sac_rig_roots(view_of(mc, cams), ci, uv, X)
            masks[mask] = masks.get(mask, 0) + 1
            if b >= 0 and len(poses) >= 2 and len(best[b]) < keep:
                best[b].append((seed, i))
            if mask in (1, 2, 4, 8) and len(only[mask.bit_length() - 1]) < keep:
                only[mask.bit_length() - 1].append((seed, i))
        seen += len(probs)
        seed += 1
    return best, only, seen, masks


@functools.lru_cache(None)
def rig_table():
    rows = []
    for ncams in RIG_NCAMS:
        cams = RIG_CAMS[ncams]
        for i, case in enumerate(SRC.solver_cases(ncams)[1]):
            rows.append(("seeded, %d cameras, %d" % (ncams, i), False, cams, *with_fourth(cams, case, i)))
    flat2 = PC.flat_rig(2)
    for k, ci in ((0, [0, 1, 0]), (1, [0, 0, 1])):
        rows.append(("by hand %d" % k, True, flat2, ci + [0], HAND_UV[k] + [[0.05, 0.05]], HAND_X[k] + [[0.2, 0.2, 4.0]]))
    for name, cams, obs, match, kw in HC.sac_rows():
        cons = S.consensus(obs, match)[0]
        for h in range(HC.H):
            s, ok = SR.sample(0, h, obs, cons)
            if ok:
                four = [obs[i] for i in s]
                rows.append(("%s, h %d" % (name, h), True, cams, [o[0] for o in four], [[o[1], o[2]] for o in four], [list(o[4]) for o in four]))
    cams = RIG_CAMS[4]
    case = SRC.solver_cases(4)[1][1]
    ci, uv, X = with_fourth(cams, case, 1)
    for name, u, x in no_scene_three(cams, ci[:3], uv[:3], X[:3]):
        rows.append((name, True, cams, ci, u + [uv[3]], x + [X[3]]))
    for what, v in (("NaN", NAN), ("inf", INF)):
        rows += [("%s at the fourth keypoint, number %d" % (what, at), True, cams, ci, uv[:3] + poke([uv[3]], at, v), X) for at in range(2)]
        rows += [("%s at the fourth point, number %d" % (what, at), True, cams, ci, uv, X[:3] + poke([X[3]], at, v)) for at in range(3)]
    rows.append(("the fourth is the first again", True, cams, ci[:3] + [ci[0]], uv[:3] + [uv[0]], X[:3] + [X[0]]))
    # the three observations in one camera, in three cameras, and in a rig whose cameras sit at the body's origin
    truth = case[0]
    for name, rig, cs in (("three observations in one camera", cams, (2, 2, 2)), ("three observations in three cameras", cams, (0, 1, 3)),
                          ("every camera at the body's origin", RIG_CENTRAL, (0, 1, 3)),
                          ("every camera at the body's origin, one camera", RIG_CENTRAL, (1, 1, 1))):
        obs = [fourth(rig, truth, c, x, y, z) for c, (x, y, z) in zip(cs + (cs[0],), ((0.3, 0.2, 4.0), (-0.4, 0.1, 7.0), (0.1, -0.3, 3.0), (0.0, 0.05, 6.0)))]
        rows.append((name, True, rig, [o[0] for o in obs], [list(o[1]) for o in obs], [o[2] for o in obs]))
        for e in (-155, -160, -165, 155, 160, 165):
            if rig is RIG_CENTRAL:
                rows.append(("%s, points times 1e%+d" % (name, e), True, rig, [o[0] for o in obs], [list(o[1]) for o in obs],
                             scaled_points([o[2] for o in obs], 10.0 ** e)))
    for kind, table in (("the winner is root", RIG_BEST), ("the only pose is root", RIG_ONLY)):
        for k, where in sorted(table.items()):
            for seed, i in where:
                rows.append(("%s %d (seed %d, %d)" % (kind, k, seed, i), True, cams, *rig_chunk(seed)[1][i]))
    assert len(set(names(rows))) == len(rows)
    return rows


def host_rig(mc, rows):
    n = len(rows)
    count, mask, best = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    R, t, Rb, tb = np.zeros((n, 4, 9)), np.zeros((n, 4, 3)), np.zeros((n, 9)), np.zeros((n, 3))
    for i, (name, hostile, cams, ci, uv, X) in enumerate(rows):
        poses, mask[i], best[i], (Rw, tw) = mc.sac_rig_roots(view_of(mc, cams), ci, uv, X)
        count[i] = len(poses)
        for k, (Rk, tk) in enumerate(poses):
            R[i, k], t[i, k] = Rk.reshape(9), tk
        Rb[i], tb[i] = Rw.reshape(9), tw
    return count, R, t, mask, best, Rb, tb


def dev_rig(mc, rows, device=0):
    return mc.dev_sac_solve_rig([view_of(mc, r[2]) for r in rows], [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows], device=device)


# ---------------------------------------------------------------------------------------------------------------------------
# rel: (name, hostile, cams, 17 matches (cam1, u1, v1, cam2, u2, v2), keypoints as doubles)
# ---------------------------------------------------------------------------------------------------------------------------
REL_NCAMS = (4, 8, 16)


@functools.lru_cache(None)
def rel_table():
    rows = []
    for ncams in REL_NCAMS:
        cams, cases = RC.solver_cases(ncams)
        rows += [("seeded, %d cameras, %d" % (ncams, i), False, cams, seventeen) for i, (_, seventeen) in enumerate(cases)]
    for rig, cams in (("outward", RC.outward_rig(1)), ("flat", [T.cam(fx=500.0, fy=500.0, u0=640.0, v0=360.0)])):
        rng = np.random.default_rng(5)
        arr = RC.rig_arrays(cams)
        R, t = RC.random_pose(rng)
        matches = [RC.exact_match(rng, cams, arr, R, t) for _ in range(40)]
        rows += [("a rig of one camera, %s, %d" % (rig, k), True, cams, matches[k:k + 17]) for k in range(24)]
    for name, cams, matches, kw in HC.rel_rows():
        for h in range(HC.H):
            smp, ok = RR.sample(0, h, len(matches))
            assert ok
            rows.append(("%s, h %d" % (name, h), True, cams, [matches[i] for i in smp]))
    cams, cases = RC.solver_cases(8)
    base = cases[0][1]
    arr = RC.rig_arrays(cams)
    rng = np.random.default_rng(23)
    zero = []
    while len(zero) < 17:
        m = RC.exact_match(rng, cams, arr, np.eye(3), np.array([0.25, -0.1, 0.3]))
        if m[0] == 0 and m[3] == 0:
            zero.append(m)
    rows.append(("all 17 in camera 0, pure translation", True, cams, zero))
    rows.append(("pure translation", True, cams, [RC.exact_match(rng, cams, arr, np.eye(3), np.array([0.25, -0.1, 0.3])) for _ in range(17)]))
    rows.append(("every keypoint at its principal point", True, cams, [(m[0], 640.0, 360.0, m[3], 640.0, 360.0) for m in base]))
    rows.append(("two coincident", True, cams, [base[0]] * 2 + base[2:]))
    rows.append(("three coincident", True, cams, [base[0]] * 3 + base[3:]))
    rows.append(("seventeen coincident", True, cams, [base[0]] * 17))
    # the keypoints of each image on one line of the image, in the matches' own cameras and in camera 0 alone
    line = [(m[0], 200.0 + 50.0 * i, 150.0 + 25.0 * i, m[3], 230.0 + 50.0 * i, 140.0 + 25.0 * i) for i, m in enumerate(base)]
    rows.append(("collinear in both images", True, cams, line))
    rows.append(("collinear in both images, all in camera 0", True, cams, [(0,) + m[1:3] + (0,) + m[4:6] for m in line]))
    rows.append(("all at the image's origin", True, cams, [(m[0], 0.0, 0.0, m[3], 0.0, 0.0) for m in base]))
    rows.append(("all at the image's origin, all in camera 0", True, cams, [(0, 0.0, 0.0, 0, 0.0, 0.0)] * 17))
    for k in (1e30, 1e36, 1e155, 1e200):
        rows.append(("keypoints times %g, as doubles" % k, True, cams, [(m[0], m[1] * k, m[2] * k, m[3], m[4] * k, m[5] * k) for m in base]))
    for j in range(17):
        for col in (1, 2, 4, 5):
            for what, v in (("NaN", NAN), ("inf", INF)):
                rows.append(("%s in match %d, column %d" % (what, j, col), True, cams,
                             [tuple(v if (i == j and k == col) else w for k, w in enumerate(m)) for i, m in enumerate(base)]))
    assert len(set(names(rows))) == len(rows)
    return rows


def rel_arrays(seventeen):
    """RC.arrays64 without its detour through float: these rows hold doubles no float holds"""
    a = np.array(seventeen, np.float64).reshape(17, 6)
    return a[:, 0].astype(np.int32), np.ascontiguousarray(a[:, 1:3]), a[:, 3].astype(np.int32), np.ascontiguousarray(a[:, 4:6])


def host_rel(mc, rows):
    count, R, t = np.zeros(len(rows), np.int32), np.zeros((len(rows), 9)), np.zeros((len(rows), 3))
    for i, (name, hostile, cams, seventeen) in enumerate(rows):
        got = mc.rel_solve(view_of(mc, cams), *rel_arrays(seventeen))
        if got is not None:
            count[i], R[i], t[i] = 1, got[0].reshape(9), got[1]
    return count, R, t


def dev_rel(mc, rows, device=0):
    a = [rel_arrays(r[3]) for r in rows]
    return mc.dev_rel_solve([view_of(mc, r[2]) for r in rows], [x[0] for x in a], [x[1] for x in a], [x[2] for x in a], [x[3] for x in a],
                            device=device)


# ---------------------------------------------------------------------------------------------------------------------------
# align: (name, hostile, p1 k x 3, p2 k x 3, member k or None)
# ---------------------------------------------------------------------------------------------------------------------------
ALIGN_COUNTS = (3, 255, 256, 257, 1025)     # around one fold workgroup of 256 lanes and one trip of it


@functools.lru_cache(None)
def align_table():
    rows = []
    for npts, count in ((3, 4000), (4, 400), (64, 400), (1000, 400)):
        for i, (truth, p1, p2) in enumerate(AC.solver_cases(npts, count, 100 + npts)):
            rows.append(("seeded, %d pairs, %d" % (npts, i), False, p1, p2, None))
    for npts in (3, 4, 64, 1000):
        for i, (truth, p1, p2) in enumerate(AC.solver_cases(npts, 400, 200 + npts, noise=0.02)[:40]):
            rows.append(("seeded with noise, %d pairs, %d" % (npts, i), False, p1, p2, None))
    truth, p1, p2 = AC.solver_cases(600, 1, 7, noise=0.02)[0]
    member = (np.arange(600) % 3 != 1)
    junk = p1.copy()
    junk[~member] = NAN
    rows.append(("a member set of 600", True, p1, p2, member))
    rows.append(("a member set of 600, NaN outside it", True, junk, p2, member))
    for name, (a, b) in (("collinear", AC.collinear()), ("collinear as float", AC.collinear(True)), ("coincident", AC.coincident())):
        rows.append((name + " triple", True, a, b, None))
    for name, p1, p2, kw in HC.align_rows():
        for h in range(HC.H):
            smp, ok = AR.sample(0, h, len(p1))
            assert ok
            rows.append(("%s, h %d" % (name, h), True, p1[smp], p2[smp], None))
        rows.append(("%s, all pairs" % name, True, p1, p2, None))
    truth, q1, q2 = AC.solver_cases(1025, 1, 31, noise=0.02)[0]
    R, t = truth
    for k in ALIGN_COUNTS:
        rows.append(("%d pairs" % k, True, q1[:k], q2[:k], None))
        rows.append(("%d pairs, every third a member" % k, True, q1[:k], q2[:k], np.arange(k) % 3 == 0))
        rows.append(("%d pairs, the last three members" % k, True, q1[:k], q2[:k], np.arange(k) >= k - 3))
    for m in (0, 1, 2, 3):
        rows.append(("a member mask of %d of 300" % m, True, q1[:300], q2[:300], np.isin(np.arange(300), (7, 256, 299)[:m])))
    for k in (0, 1, 2):
        rows.append(("%d pairs, all members" % k, True, q1[:k], q2[:k], None))
    rows.append(("two coincident of three", True, q1[[0, 0, 2]], q2[[0, 0, 2]], None))
    rows.append(("all at the origin", True, np.zeros((3, 3)), np.zeros((3, 3)), None))
    rows.append(("a reflection", True, (q2[:64] * np.array([1.0, 1.0, -1.0])) @ R.T + t, q2[:64], None))
    for e in (158, -158, 200, -200):
        rows.append(("times 1e%+d" % e, True, q1[:64] * 10.0 ** e, q2[:64] * 10.0 ** e, None))
    for at in range(9):
        for what, v in (("NaN", NAN), ("inf", INF)):
            rows.append(("%s in frame 1, number %d" % (what, at), True, np.array(poke(q1[:3], at, v)), q2[:3], None))
            rows.append(("%s in frame 2, number %d" % (what, at), True, q1[:3], np.array(poke(q2[:3], at, v)), None))
    assert len(set(names(rows))) == len(rows)
    return rows


def host_align(mc, rows):
    valid, R, t, gap = np.zeros(len(rows), np.int32), np.zeros((len(rows), 9)), np.zeros((len(rows), 3)), np.zeros(len(rows))
    for i, (name, hostile, p1, p2, member) in enumerate(rows):
        pose, gap[i] = mc.align_solve(p1, p2, member, with_gap=True)
        if pose is not None:
            valid[i], R[i], t[i] = 1, pose[0].reshape(9), pose[1]
    return valid, R, t, gap


def dev_align(mc, rows, device=0):
    return mc.dev_align_solve([(r[2], r[3], r[4]) for r in rows], device=device)


SOLVERS = {"sac": (sac_table, host_sac, dev_sac), "rig": (rig_table, host_rig, dev_rig), "rel": (rel_table, host_rel, dev_rel),
           "ess": (ess_table, host_ess, dev_ess), "align": (align_table, host_align, dev_align)}


def take(result, index):
    """the rows `index` of a host_* / dev_* result"""
    return tuple(a[index] for a in result)


def same(a, b):
    """two results, every array as raw bytes -> the indices of the problems that differ"""
    bad = set()
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, (x.shape, y.shape, x.dtype, y.dtype)
        n = len(x)
        if n == 0:
            continue
        bx, by = np.ascontiguousarray(x).view(np.uint8).reshape(n, -1), np.ascontiguousarray(y).view(np.uint8).reshape(n, -1)
        bad |= set(np.nonzero((bx != by).any(axis=1))[0].tolist())
    return sorted(bad)
