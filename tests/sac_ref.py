"""The absolute rig pose by RANSAC restated in plain Python, independently of csrc/mcorb_sac.h: Python floats (IEEE doubles, one
operation per operator, math.sqrt correctly rounded), Python integers for the draws, lists, no numpy in the arithmetic.

Restated: the draws (the splitmix64 finaliser), the walk that turns them into a sample, the bearing, the score (OpenGV's
reprojection distance of a non-central adapter, recalled: OpenGV is not in the reference tree), the counting over the consensus
set, the pick, the fold of observations to matches and the rule of FrontEnd.cpp:4786 between the RANSAC and the refinement
(pose_ref.refine).  NOT restated: the minimal solver -- a hypothesis's candidate poses come from the library's mcorb_sac_solve hook
through the `solve` argument (as mapping_new_ref.py takes X0 from the triangulate hook), so everything behind the solver compares
on the bits.  The disambiguation by the fourth point IS restated, on the hook's poses.

Also here, and used only to judge mcorb_sac_solve: an independent P3P -- the same Grunert quartic, its coefficients by numpy
polynomial products, its roots by numpy.polynomial.polyroots (companion-matrix eigenvalues), the alignment by Kabsch through
numpy.linalg.svd.

A rig, a pose and an observation are pose_ref.py's: cams as dicts, (R rows, t) = w_T_b, (cam, kx, ky, octave, X)."""
import math
import struct

import numpy as np

import pose_ref as P

OK, NO_OBS, NO_MODEL = 0, 1, 2
MASK = (1 << 64) - 1
DRAWS = 16
IDENT = ([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [0.0, 0.0, 0.0])


def draw(seed, h, j):
    """the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (1 + 16 h + j)"""
    z = (seed + 0x9E3779B97F4A7C15 * (1 + 16 * h + j)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def consensus(obs, match):
    """-> (the consensus observations: the first of each match, in input order; per match its first observation, and n)"""
    cons = [i for i in range(len(obs)) if match is None or i == 0 or match[i] != match[i - 1]]
    return cons, cons + [len(obs)]


def sample(seed, h, obs, cons):
    """-> ([s0, s1, s2, s3] with -1 for members not drawn, complete?)"""
    s = [cons[draw(seed, h, 0) % len(cons)], -1, -1, -1]
    own = [i for i in cons if obs[i][0] == obs[s[0]][0]]
    if len(own) < 4:
        return s, False
    have = 1
    for j in range(1, DRAWS):
        i = own[draw(seed, h, j) % len(own)]
        if i in s[:have]:
            continue
        s[have] = i
        have += 1
        if have == 4:
            return s, True
    return s, False


def bearing(cam, kx, ky):
    y = (ky - cam["v0"]) / cam["fy"]
    x = ((kx - cam["u0"]) - cam["s"] * y) / cam["fx"]
    n = math.sqrt((x * x + y * y) + 1.0)
    return [x / n, y / n, 1.0 / n]


def score(cam, pose, X, f):
    """1 - f . q / |q|; a zero q gives NaN (0.0 / 0.0 in IEEE; Python raises, so it is written out)"""
    pb = P.transform_to(pose[0], pose[1], X)
    q = P.transform_to(cam["R"], cam["t"], pb)
    dot = (f[0] * q[0] + f[1] * q[1]) + f[2] * q[2]
    nn = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
    if nn != nn or dot != dot:
        return float("nan")
    nq = math.sqrt(nn)
    if nq == 0.0:
        return float("nan") if dot == 0.0 or dot != dot else 1.0 - math.copysign(float("inf"), dot)
    if math.isinf(nq) and math.isinf(dot):
        return float("nan")
    return 1.0 - dot / nq


def obs_score(cams, pose, o):
    return score(cams[o[0]], pose, o[4], bearing(cams[o[0]], o[1], o[2]))


def model(cams, obs, s, solve):
    """the disambiguation: of the solver's poses on s[0 .. 2] the one with the smallest score at s[3]; a tie goes to the lowest
    index, a NaN never wins -> pose or None"""
    c = obs[s[0]][0]
    best, best_score = None, None
    for pose in solve(c, [obs[i] for i in s[:3]]):
        sc = obs_score(cams, pose, obs[s[3]])
        if sc != sc:
            continue
        if best is None or sc < best_score:
            best, best_score = pose, sc
    return best


def ransac(cams, obs, threshold, solve, match=None, max_iterations=100, seed=0):
    """-> dict(status, R, t, n_inliers, best, sample, n_models, n_consensus, counts (None without a model), models, samples,
    flags: per observation, inliers: per match)"""
    cons, first = consensus(obs, match)
    out = dict(status=NO_OBS, R=IDENT[0], t=IDENT[1], n_inliers=0, best=-1, sample=[-1] * 4, n_models=0, n_consensus=len(cons),
               counts=[], models=[], samples=[], flags=[False] * len(obs), inliers=[False] * len(cons), first=first)
    if not cons:
        return out
    best, best_count = -1, -1
    for h in range(max_iterations):
        s, complete = sample(seed, h, obs, cons)
        pose = model(cams, obs, s, solve) if complete else None
        count = None
        if pose is not None:
            count = sum(1 for i in cons if obs_score(cams, pose, obs[i]) < threshold)
            if count > best_count:
                best, best_count = h, count
        out["counts"].append(count)
        out["models"].append(pose)
        out["samples"].append(s)
    out["n_models"] = sum(1 for m in out["models"] if m is not None)
    out["status"] = NO_MODEL
    if best >= 0:
        pose = out["models"][best]
        flags = [False] * len(obs)
        for i in cons:
            flags[i] = obs_score(cams, pose, obs[i]) < threshold
        out.update(status=OK, R=pose[0], t=pose[1], n_inliers=best_count, best=best, sample=out["samples"][best], flags=flags,
                   inliers=[flags[i] for i in cons])
    return out


def ransac_refine(cams, obs, threshold, solve, inv_sigma2, match=None, max_iterations=100, seed=0, refine_iterations=25):
    """the RANSAC, the refinement over all observations from its pose, and the rule of :4786 -> (the ransac dict, the
    pose_ref.refine dict, dict(used, R, t, n_inliers, inliers))"""
    sac = ransac(cams, obs, threshold, solve, match, max_iterations, seed)
    ref = P.refine(cams, (sac["R"], sac["t"]), obs, inv_sigma2, refine_iterations)
    first = sac["first"]
    ref_match = [all(ref["inliers"][i] for i in range(first[k], first[k + 1])) for k in range(len(first) - 1)]
    use = sac["status"] == OK and not sac["n_inliers"] > sum(ref_match)
    final = dict(used=1, R=ref["R"], t=ref["t"], n_inliers=sum(ref_match), inliers=ref_match) if use else \
        dict(used=0, R=sac["R"], t=sac["t"], n_inliers=sac["n_inliers"], inliers=sac["inliers"])
    return sac, ref, final


def next_up(x):
    return math.nextafter(x, math.inf)


# ---------------------------------------------------------------------------------------------------------------------------
# the independent solver: judges mcorb_sac_solve, is never compared on the bits
# ---------------------------------------------------------------------------------------------------------------------------
def numpy_p3p(f, X):
    """the camera poses w_T_c (R 3 x 3, t) of a central P3P: bearings f (3 x 3, unit rows, camera frame), points X (3 x 3, world)"""
    f, X = np.asarray(f, np.float64), np.asarray(X, np.float64)
    a2, b2, c2 = np.sum((X[1] - X[2]) ** 2), np.sum((X[0] - X[2]) ** 2), np.sum((X[0] - X[1]) ** 2)
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    K, Cq = (a2 - c2) / b2, c2 / b2
    # ascending powers of v
    N = np.array([1 + K, -2 * K * cb, K - 1])
    D = np.array([2 * cg, -2 * ca])
    Q = np.array([1.0, -2 * cb, 1.0])
    pm = np.polynomial.polynomial.polymul
    D2 = pm(D, D)
    E = np.polynomial.polynomial.polyadd(np.polynomial.polynomial.polyadd(D2, pm(N, N)),
                                         -np.polynomial.polynomial.polyadd(2 * cg * pm(N, D), Cq * pm(Q, D2)))
    poses = []
    for v in np.polynomial.polynomial.polyroots(E):
        if abs(v.imag) > 1e-7 * max(1.0, abs(v)) or v.real <= 0:
            continue
        v = v.real
        u = np.polynomial.polynomial.polyval(v, N) / np.polynomial.polynomial.polyval(v, D)
        if not u > 0:
            continue
        s1 = math.sqrt(b2 / np.polynomial.polynomial.polyval(v, Q))
        Cc = np.array([s1 * f[0], u * s1 * f[1], v * s1 * f[2]])
        # Kabsch: R minimising |X - (R C + t)|
        mc_, mx = Cc.mean(axis=0), X.mean(axis=0)
        U, _, Vt = np.linalg.svd((X - mx).T @ (Cc - mc_))
        Dg = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        R = U @ Dg @ Vt
        poses.append((R, mx - R @ mc_))
    return poses


def rig_pose(cam, Rwc, twc):
    """w_T_b = w_T_c * (b_T_c)^-1 (numpy)"""
    Rc, tc = np.asarray(cam["R"]), np.asarray(cam["t"])
    R = Rwc @ Rc.T
    return R, twc - R @ tc


def pose_distance(pose, truth):
    """max |dR_ij| and |dt| / max(1, |t|)"""
    dR = float(np.max(np.abs(np.asarray(pose[0]) - np.asarray(truth[0]))))
    tt = np.asarray(truth[1], np.float64)
    return max(dR, float(np.linalg.norm(np.asarray(pose[1]) - tt)) / max(1.0, float(np.linalg.norm(tt))))


def same_bits(a, b):
    return P.same_bits(a, b)


def bits(x):
    return struct.pack("<d", x)
