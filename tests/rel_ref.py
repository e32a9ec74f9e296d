"""The relative rig pose between two frames by RANSAC restated in plain Python, independently of csrc/mcorb_rel.h: Python floats
(IEEE doubles, one operation per operator, math.sqrt correctly rounded), Python integers for the draws, lists.  The counting
over many matches runs the same operators as numpy elementwise operations on float64 columns (score_many), which test_rel_cpu.py
holds to the scalar form on the bits.

Restated: the draws (the splitmix64 finaliser), the partial Fisher-Yates walk that turns them into 17 distinct members, the rays,
the score (OpenGV's distance of the non-central relative problem, recalled: OpenGV is not in the reference tree), the counting
over all matches and the pick.  NOT restated: the 17-point solver -- a hypothesis's pose comes from the library's mcorb_rel_solve
hook through the `solve` argument (as sac_ref.py takes its poses from mcorb_sac_solve), so everything behind the solver compares
on the bits.

Also here, and used only to judge mcorb_rel_solve: an independent numpy solver of the same linear problem -- the null space by
numpy.linalg.svd, the rotation by an SVD polar decomposition, the translation by numpy.linalg.lstsq.

A rig is pose_ref.py's: cams as dicts.  A match is (cam1, u1, v1, cam2, u2, v2); a pose is (R rows, t) = b1_T_b2."""
import math

import numpy as np

import sac_ref as S

OK, NO_OBS, NO_MODEL = 0, 1, 2
MASK = (1 << 64) - 1
SAMPLE = 17
STRIDE = 32
IDENT = S.IDENT
NAN = float("nan")


def draw(seed, h, j):
    """the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (1 + 32 h + j)"""
    z = (seed + 0x9E3779B97F4A7C15 * (1 + STRIDE * h + j)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def walk(raw):
    """raw[j] in 0 .. S - j - 1: an index into the members not yet picked -> the members, in draw order"""
    picks = []
    for idx in raw:
        for p in sorted(picks):
            if p <= idx:
                idx += 1
        picks.append(idx)
    return picks


def sample(seed, h, n):
    """-> (the 17 members in draw order, or 17 x -1; complete?)"""
    if n < SAMPLE:
        return [-1] * SAMPLE, False
    return walk([draw(seed, h, j) % (n - j) for j in range(SAMPLE)]), True


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def rot(R, v):
    return [(R[i][0] * v[0] + R[i][1] * v[1]) + R[i][2] * v[2] for i in range(3)]


def ray(cam, u, v):
    """-> (d, c): the body-frame direction and centre of a keypoint's ray"""
    return rot(cam["R"], S.bearing(cam, u, v)), list(cam["t"])


def div(a, b):
    """IEEE a / b where Python raises"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def sqrt(x):
    return NAN if x != x or x < 0.0 else math.sqrt(x)


def rays_of(cams, m):
    """-> (a, c1, d2, c2) of a match"""
    a, c1 = ray(cams[m[0]], m[1], m[2])
    d2, c2 = ray(cams[m[3]], m[4], m[5])
    return a, c1, d2, c2


def score_rays(pose, rays):
    """the midpoint of the two rays' closest points in frame 1's body frame, then 1 - cos in both views, summed"""
    a, c1, d2, c2 = rays
    R, t = pose
    b = rot(R, d2)
    Rc = rot(R, c2)
    w = [(Rc[i] + t[i]) - c1[i] for i in range(3)]
    aa, ab, bb, aw, bw = dot(a, a), dot(a, b), dot(b, b), dot(a, w), dot(b, w)
    det = ab * ab - aa * bb
    lam = div(ab * bw - bb * aw, det)
    mu = div(aa * bw - ab * aw, det)
    P1 = [0.5 * ((lam * a[i]) + (w[i] + mu * b[i])) for i in range(3)]
    P2 = [P1[i] - w[i] for i in range(3)]
    return (1.0 - div(dot(a, P1), sqrt(dot(P1, P1)))) + (1.0 - div(dot(b, P2), sqrt(dot(P2, P2) * bb)))


def score(cams, pose, m):
    return score_rays(pose, rays_of(cams, m))


def columns(rays):
    """the rays of n matches as four (3, n) float64 arrays, for score_many"""
    return tuple(np.array([r[k] for r in rays], np.float64).reshape(-1, 3).T.copy() for k in range(4))


def score_many(pose, cols):
    """score_rays for all matches at once: the same operators in the same order, each a numpy elementwise operation on float64
    columns -- one IEEE operation per element, nothing fused -- so the same bits (test_rel_cpu.py checks it against score_rays).
    It is what lets the restatement count 16 384 hypotheses in seconds"""
    a, c1, d2, c2 = cols
    R, t = pose

    def dotc(x, y):
        return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]

    def rotc(v):
        return [(R[i][0] * v[0] + R[i][1] * v[1]) + R[i][2] * v[2] for i in range(3)]

    with np.errstate(all="ignore"):
        b = rotc(d2)
        Rc = rotc(c2)
        w = [(Rc[i] + t[i]) - c1[i] for i in range(3)]
        aa, ab, bb, aw, bw = dotc(a, a), dotc(a, b), dotc(b, b), dotc(a, w), dotc(b, w)
        det = ab * ab - aa * bb
        lam = (ab * bw - bb * aw) / det
        mu = (aa * bw - ab * aw) / det
        P1 = [0.5 * ((lam * a[i]) + (w[i] + mu * b[i])) for i in range(3)]
        P2 = [P1[i] - w[i] for i in range(3)]
        return (1.0 - dotc(a, P1) / np.sqrt(dotc(P1, P1))) + (1.0 - dotc(b, P2) / np.sqrt(dotc(P2, P2) * bb))


def ransac(cams, matches, threshold, solve, max_iterations=100, seed=0):
    """-> dict(status, R, t, n_inliers, best, sample, n_models, counts (None without a model), models, samples, inliers)"""
    n = len(matches)
    out = dict(status=NO_OBS, R=IDENT[0], t=IDENT[1], n_inliers=0, best=-1, sample=[-1] * SAMPLE, n_models=0, counts=[], models=[],
               samples=[], inliers=[False] * n)
    if not n:
        return out
    cols = columns([rays_of(cams, m) for m in matches])
    best, best_count = -1, -1
    for h in range(max_iterations):
        s, complete = sample(seed, h, n)
        pose = solve([matches[i] for i in s]) if complete else None
        count = None
        if pose is not None:
            count = int(np.count_nonzero(score_many(pose, cols) < threshold))
            if count > best_count:
                best, best_count = h, count
        out["counts"].append(count)
        out["models"].append(pose)
        out["samples"].append(s)
    out["n_models"] = sum(1 for m in out["models"] if m is not None)
    out["status"] = NO_MODEL
    if best >= 0:
        pose = out["models"][best]
        out.update(status=OK, R=pose[0], t=pose[1], n_inliers=best_count, best=best, sample=out["samples"][best],
                   inliers=[bool(v) for v in score_many(pose, cols) < threshold])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the independent solver: judges mcorb_rel_solve, is never compared on the bits
# ---------------------------------------------------------------------------------------------------------------------------
def np_rays(cams, matches):
    d1, c1, d2, c2 = [], [], [], []
    for m in matches:
        for (cam, u, v), dd, cc in (((m[0], m[1], m[2]), d1, c1), ((m[3], m[4], m[5]), d2, c2)):
            c = cams[cam]
            y = (v - c["v0"]) / c["fy"]
            x = ((u - c["u0"]) - c["s"] * y) / c["fx"]
            f = np.array([x, y, 1.0])
            dd.append(np.asarray(c["R"]) @ (f / np.linalg.norm(f)))
            cc.append(np.asarray(c["t"], np.float64))
    return np.array(d1), np.array(c1), np.array(d2), np.array(c2)


def numpy_solve17(cams, matches):
    """-> (R, t) or None: [A_E | A_R] (e, r) = 0 with E found first -- the null space of the projection of A_E onto the
    complement of A_R's column space (SVD both times) -- then the two rotations of E by the SVD of E (U W V^T, U W^T V^T), the
    nearest rotation by an SVD polar decomposition, t by lstsq, the smaller residual wins"""
    d1, c1, d2, c2 = np_rays(cams, matches)
    m1, m2 = np.cross(c1, d1), np.cross(c2, d2)
    AE = np.einsum("ia,ib->iab", d1, d2).reshape(-1, 9)
    AR = (np.einsum("ia,ib->iab", d1, m2) + np.einsum("ia,ib->iab", m1, d2)).reshape(-1, 9)
    U, s, _ = np.linalg.svd(AR, full_matrices=False)
    Q = U[:, s > 1e-10 * s[0]]
    B = AE - Q @ (Q.T @ AE)
    E = np.linalg.svd(B)[2][-1].reshape(3, 3)
    Ue, _, Vte = np.linalg.svd(E)
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    best = None
    for Wk in (W, W.T):
        R = Ue @ Wk @ Vte
        R = R * np.sign(np.linalg.det(R))
        Up, _, Vtp = np.linalg.svd(R)
        R = Up @ Vtp
        b = d2 @ R.T
        g = np.cross(b, d1)
        hh = -(np.einsum("ia,ia->i", d1, m2 @ R.T) + np.einsum("ia,ia->i", m1, b))
        t, _, rank, _ = np.linalg.lstsq(g, hh, rcond=None)
        res = float(np.sum((g @ t - hh) ** 2))
        if rank == 3 and (best is None or res < best[0]):
            best = (res, R, t)
    return None if best is None else (best[1], best[2])


def pose_distance(pose, truth):
    """max |dR_ij| and |dt| / max(1, |t|)"""
    return S.pose_distance(pose, truth)


def same_bits(a, b):
    return S.same_bits(a, b)


def bits(x):
    return S.bits(x)


def next_up(x):
    return math.nextafter(x, math.inf)
