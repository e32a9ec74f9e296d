"""mcorb_lmap_retriangulate restated in plain Python, independently of csrc/mcorb_retri.h: Python floats (IEEE doubles, one operation
per operator, math.sqrt correctly rounded), lists, no numpy in the arithmetic.  DESIGN.md section 9p.

From the reference (MCSlam/src/Backend.cpp:3577-3663): the landmarks seen in a moved keyframe are triangulated again from all of
their observations (triangulateSafe, then triangulatePoint3: the same DLT), updated through GlobalMap::updateLandmark or deleted.
Recalled, gtsam not being in the tree: the DLT rows on K [R | t], the rank test, the order of triangulateSafe's checks.  Stated:
the Gram matrix, the fold of its sums over 16 lanes, six cyclic Jacobi sweeps for the null vector and the third eigenvalue.

A rig and a pose are pose_ref.py's; an observation is (kf, cam, lm, kx, ky) with kx, ky the floats of a KeyPoint::pt."""
import math
import struct

LANES, SWEEPS = 16, 6
NOT_SELECTED, FEW_VIEWS, VALID_UPDATED, VALID_REJECTED, DEGENERATE, BEHIND, FAR, OUTLIER = range(8)
FAILED = (DEGENERATE, BEHIND, FAR, OUTLIER)
NAMES = ["NOT_SELECTED", "FEW_VIEWS", "VALID_UPDATED", "VALID_REJECTED", "DEGENERATE", "BEHIND", "FAR", "OUTLIER"]
INF = float("inf")
NAN = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000000))[0]


def div(a, b):
    """IEEE division: Python raises where the machine returns an infinity or a NaN"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def sqrt(x):
    return NAN if x < 0.0 else math.sqrt(x)


def default_nan(x):
    return NAN if x != x else x


def view(cam, pose):
    """-> 15 floats: P = K [R_cw | t_cw] row by row, then the camera centre"""
    R, t = pose
    Rc, tc = cam["R"], cam["t"]
    M = [[(Rc[0][k] * R[c][0] + Rc[1][k] * R[c][1]) + Rc[2][k] * R[c][2] for c in range(3)] for k in range(3)]
    d = [0.0 - t[0], 0.0 - t[1], 0.0 - t[2]]
    pb = [R[0][r] * d[0] + R[1][r] * d[1] + R[2][r] * d[2] for r in range(3)]
    e = [pb[0] - tc[0], pb[1] - tc[1], pb[2] - tc[2]]
    q = [Rc[0][r] * e[0] + Rc[1][r] * e[1] + Rc[2][r] * e[2] for r in range(3)]
    for k in range(3):
        M[k].append(q[k])
    K = [[cam["fx"], cam["s"], cam["u0"]], [0.0, cam["fy"], cam["v0"]], [0.0, 0.0, 1.0]]
    out = []
    for r in range(3):
        for c in range(4):
            out.append((K[r][0] * M[0][c] + K[r][1] * M[1][c]) + K[r][2] * M[2][c])
    for r in range(3):
        out.append(((R[r][0] * tc[0] + R[r][1] * tc[1]) + R[r][2] * tc[2]) + t[r])
    return out


def rows(V, kx, ky):
    """the DLT's two rows of an observation"""
    return [kx * V[8 + c] - V[c] for c in range(4)], [ky * V[8 + c] - V[4 + c] for c in range(4)]


def gram(items):
    """items: (view, kx, ky) in order -> the 10 upper entries of G row by row, folded as 16 lanes fold them"""
    s = [[0.0] * 10 for _ in range(LANES)]
    for l in range(LANES):
        for V, kx, ky in items[l::LANES]:
            a, b = rows(V, kx, ky)
            at = 0
            for i in range(4):
                for j in range(i, 4):
                    s[l][at] = s[l][at] + (a[i] * a[j] + b[i] * b[j])
                    at += 1
    stride = LANES // 2
    while stride >= 1:
        for l in range(stride):
            for k in range(10):
                s[l][k] = s[l][k] + s[l + stride][k]
        stride //= 2
    return s[0]


def rotate(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    tau = (A[q][q] - A[p][p]) / (2.0 * apq)
    at = -tau if tau < 0.0 else tau
    tt = 1.0 / (at + sqrt(tau * tau + 1.0))
    t = -tt if tau < 0.0 else tt
    c = 1.0 / sqrt(t * t + 1.0)
    s = t * c
    A[p][p] = A[p][p] - t * apq
    A[q][q] = A[q][q] + t * apq
    A[p][q] = A[q][p] = 0.0
    for r in range(4):
        if r != p and r != q:
            arp, arq = A[r][p], A[r][q]
            A[r][p] = c * arp - s * arq
            A[r][q] = s * arp + c * arq
            A[p][r] = A[r][p]
            A[q][r] = A[r][q]
        vrp, vrq = V[r][p], V[r][q]
        V[r][p] = c * vrp - s * vrq
        V[r][q] = s * vrp + c * vrq


def solve(G, rank_tol, sweeps=SWEEPS):
    """-> (degenerate, X, sqrt(max(lambda_3, 0)))"""
    A = [[0.0] * 4 for _ in range(4)]
    at = 0
    for i in range(4):
        for j in range(i, 4):
            A[i][j] = A[j][i] = G[at]
            at += 1
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            rotate(A, V, p, q)
    d = [A[i][i] for i in range(4)]
    k = 0
    for i in (1, 2, 3):
        if d[i] < d[k]:
            k = i
    rest = [d[i] for i in range(4) if i != k]
    l3 = rest[0]
    for x in rest[1:]:
        if x < l3:
            l3 = x
    inv = div(1.0, V[3][k])
    X = [V[c][k] * inv for c in range(3)]
    finite = all(not (x != x or x in (INF, -INF)) for x in X)
    s3 = sqrt(l3 if l3 > 0.0 else 0.0)
    return (not s3 > rank_tol) or not finite, [default_nan(x) for x in X], s3


def check(items, X, far_threshold):
    """-> (code of the first observation in order that fails: 0, FAR or BEHIND; the largest reprojection error)"""
    first, emax = 0, 0.0
    for V, kx, ky in items:
        d = [X[0] - V[12], X[1] - V[13], X[2] - V[14]]
        dist = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        x = ((V[0] * X[0] + V[1] * X[1]) + V[2] * X[2]) + V[3]
        y = ((V[4] * X[0] + V[5] * X[1]) + V[6] * X[2]) + V[7]
        z = ((V[8] * X[0] + V[9] * X[1]) + V[10] * X[2]) + V[11]
        if not first:
            if far_threshold > 0.0 and dist > far_threshold:
                first = FAR
            elif z <= 0.0:
                first = BEHIND
        eu, ev = div(x, z) - kx, div(y, z) - ky
        e = sqrt(eu * eu + ev * ev)
        if e != e:
            e = INF
        if e > emax:
            emax = e
    return first, emax


def update(pt, X, max_diff):
    """GlobalMap::updateLandmark -> (updated, diff_norm)"""
    d = [pt[k] - X[k] for k in range(3)]
    sq = 0.0
    for k in range(3):
        sq = sq + d[k] * d[k]
    diff = default_nan(sqrt(sq))
    return diff < max_diff, diff


def sort_obs(obs):
    return sorted(range(len(obs)), key=lambda i: (obs[i][2], obs[i][0], obs[i][1]))      # (sorted is stable)


def retriangulate(cams, poses, moved, pts, obs, rank_tol=1.0, far_threshold=-1.0, outlier_threshold=-1.0, max_diff=5.0, sweeps=SWEEPS,
                  detail=False):
    """pts: the landmarks' current points -> dict(pts, diff_norm, n_views, verdict, counts); with detail also s3 and emax per
    landmark (None where not computed)"""
    nlm = len(pts)
    per_lm = [[] for _ in range(nlm)]
    for i in sort_obs(obs):
        per_lm[obs[i][2]].append(i)
    table = {}
    out = dict(pts=[], diff_norm=[], n_views=[], verdict=[], counts=[0] * 8, s3=[], emax=[])
    for j in range(nlm):
        idx = per_lm[j]
        X, diff, s3, emax = [0.0, 0.0, 0.0], 0.0, None, None
        if not any(moved[obs[i][0]] for i in idx):
            verdict = NOT_SELECTED
        elif len(idx) < 2:
            verdict = FEW_VIEWS
        else:
            items = []
            for i in idx:
                kf, cam = obs[i][0], obs[i][1]
                if (kf, cam) not in table:
                    table[(kf, cam)] = view(cams[cam], poses[kf])
                items.append((table[(kf, cam)], obs[i][3], obs[i][4]))
            degenerate, X, s3 = solve(gram(items), rank_tol, sweeps)
            first, emax = check(items, X, far_threshold)
            if degenerate:
                verdict = DEGENERATE
            elif first:
                verdict = first
            elif outlier_threshold > 0.0 and not emax <= outlier_threshold:
                verdict = OUTLIER
            else:
                updated, diff = update(pts[j], X, max_diff)
                verdict = VALID_UPDATED if updated else VALID_REJECTED
        out["pts"].append(X)
        out["diff_norm"].append(diff)
        out["n_views"].append(len(idx))
        out["verdict"].append(verdict)
        out["counts"][verdict] += 1
        out["s3"].append(s3)
        out["emax"].append(emax)
    if not detail:
        del out["s3"], out["emax"]
    return out
