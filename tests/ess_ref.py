"""LocalMap.essential_pose restated in plain Python and numpy, independently of csrc/mcorb_ess.h.

Two kinds of code live here.  What the library must equal on the bits -- the draws, the normalised points, the Sampson distance,
the consensus key, the four candidates of E, the depths of the vote, the flags -- is written out in Python floats (or numpy
elementwise operations on float64 columns, one IEEE operation per element) in the order the header documents; the minimal
solver's models come from the library's hook, as rel_ref.py takes its own.  What only has to agree to a tolerance is written
with other means on purpose: numpy_solve5 (SVD null space, numpy.linalg.det, numpy.roots, lstsq) and numpy_decompose (SVD)."""
import math

import numpy as np

import rel_ref as RR

SAMPLE, ROOTS = 5, 10
OK, NO_OBS, NO_MODEL = 0, 1, 2
NAN = float("nan")
IDENT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
div, sqrt, dot, rot, bits = RR.div, RR.sqrt, RR.dot, RR.rot, RR.bits


def sample(seed, h, n):
    """-> (the 5 members in draw order, or 5 x -1; complete?): mcorb_lmap_relative_pose's walk on the draws j = 0 .. 4"""
    if n < SAMPLE:
        return [-1] * SAMPLE, False
    return RR.walk([RR.draw(seed, h, j) % (n - j) for j in range(SAMPLE)]), True


def normalise(cam, u, v):
    y = div(v - cam["v0"], cam["fy"])
    x = div((u - cam["u0"]) - cam["s"] * y, cam["fx"])
    return x, y


def point(cam, m):
    """a match (u1, v1, u2, v2) -> (x1, y1, x2, y2)"""
    return normalise(cam, m[0], m[1]) + normalise(cam, m[2], m[3])


def bearing(x, y):
    n = sqrt((x * x + y * y) + 1.0)
    return [div(x, n), div(y, n), div(1.0, n)]


def threshold2(cam, threshold_px):
    thr = threshold_px / ((cam["fx"] + cam["fy"]) / 2.0)
    return thr * thr


def sampson(E, p):
    """E: 9 floats, row-major"""
    x1, y1, x2, y2 = p
    a0, a1, a2 = (E[0] * x2 + E[1] * y2) + E[2], (E[3] * x2 + E[4] * y2) + E[5], (E[6] * x2 + E[7] * y2) + E[8]
    b0, b1 = (E[0] * x1 + E[3] * y1) + E[6], (E[1] * x1 + E[4] * y1) + E[7]
    r = (x1 * a0 + y1 * a1) + a2
    return div(r * r, ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1)


def sampson_many(E, cols):
    """sampson for all matches at once, the same operators in the same order on float64 columns (x1, y1, x2, y2)"""
    x1, y1, x2, y2 = cols
    with np.errstate(all="ignore"):
        a0, a1, a2 = (E[0] * x2 + E[1] * y2) + E[2], (E[3] * x2 + E[4] * y2) + E[5], (E[6] * x2 + E[7] * y2) + E[8]
        b0, b1 = (E[0] * x1 + E[3] * y1) + E[6], (E[1] * x1 + E[4] * y1) + E[7]
        r = (x1 * a0 + y1 * a1) + a2
        return (r * r) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1)


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def cof(A):
    return cross(A[3:6], A[6:9]) + cross(A[6:9], A[0:3]) + cross(A[0:3], A[3:6])


def decompose(E_in):
    """-> (R+ as 9, R- as 9, t^): E scaled to |E|_F^2 = 2, t^ the longest cross product of its columns (the first of equals),
    R+- = cof(E) -+ [t^]x E, three steps of R <- (R + R^-T) / 2 each"""
    nn = 0.0
    for v in E_in:
        nn += v * v
    scale = sqrt(div(2.0, nn))
    E = [v * scale for v in E_in]
    e0, e1, e2 = [E[0], E[3], E[6]], [E[1], E[4], E[7]], [E[2], E[5], E[8]]
    th, tn = None, None
    for x in (cross(e0, e1), cross(e1, e2), cross(e2, e0)):
        n = dot(x, x)
        if th is None or n > tn:
            th, tn = x, n
    tn = sqrt(tn)
    th = [div(v, tn) for v in th]
    C = cof(E)
    TE = [0.0] * 9
    for j in range(3):
        TE[j] = th[1] * E[6 + j] - th[2] * E[3 + j]
        TE[3 + j] = th[2] * E[j] - th[0] * E[6 + j]
        TE[6 + j] = th[0] * E[3 + j] - th[1] * E[j]
    out = []
    for s in range(2):
        R = [C[j] - TE[j] if s == 0 else C[j] + TE[j] for j in range(9)]
        for _ in range(3):
            K = cof(R)
            dR = (R[0] * K[0] + R[1] * K[1]) + R[2] * K[2]
            R = [0.5 * (R[j] + div(K[j], dR)) for j in range(9)]
        out.append(R)
    return out[0], out[1], th


def rows(R):
    return [list(R[0:3]), list(R[3:6]), list(R[6:9])]


def depths(R, t, p):
    """(z in camera 1, z in camera 2) of the midpoint of mcorb_lmap_relative_pose's score with a = d1, b = R d2, w = t"""
    a, d2 = bearing(p[0], p[1]), bearing(p[2], p[3])
    b = rot(rows(R), d2)
    aa, ab, bb, aw, bw = dot(a, a), dot(a, b), dot(b, b), dot(a, t), dot(b, t)
    det = ab * ab - aa * bb
    lam, mu = div(ab * bw - bb * aw, det), div(aa * bw - ab * aw, det)
    P1 = [0.5 * ((lam * a[i]) + (t[i] + mu * b[i])) for i in range(3)]
    P2 = [P1[i] - t[i] for i in range(3)]
    return P1[2], (R[2] * P2[0] + R[5] * P2[1]) + R[8] * P2[2]


def in_front(z, distance):
    return z[0] > 0.0 and z[0] < distance and z[1] > 0.0 and z[1] < distance


def candidate(cands, c):
    Rp, Rm, th = cands
    return (Rm if c & 1 else Rp), ([v for v in th] if c < 2 else [-v for v in th])


def key(count, h, c):
    return ((count + 1) << 18) | ((16383 - h) << 4) | (15 - c)


def ransac(cam, matches, solve, threshold_px=1.0, distance=50.0, max_iterations=100, seed=0):
    """solve(five matches) -> [E as 9 floats], the library's models.  -> dict(status, R, t (lists), E, n_ransac_inliers, n_inliers,
    best, root, sample, n_models, cheirality, inliers, ransac_inliers, counts / valid / models per slot, samples per hypothesis,
    roots: the models of each hypothesis)"""
    n, H = len(matches), max_iterations
    out = dict(status=NO_OBS, R=[v for r in IDENT for v in r], t=[0.0] * 3, E=[0.0] * 9, n_ransac_inliers=0, n_inliers=0, best=-1, root=-1,
               sample=[-1] * SAMPLE, n_models=0, cheirality=[0] * 4, inliers=[False] * n, ransac_inliers=[False] * n, counts=[], valid=[],
               models=[], samples=[], roots=[])
    if n == 0:
        return out
    thr2 = threshold2(cam, threshold_px)
    pts = [point(cam, m) for m in matches]
    cols = tuple(np.array([p[k] for p in pts], np.float64) for k in range(4))
    best_key, best = 0, None
    for h in range(H):
        smp, ok = sample(seed, h, n)
        models = solve([matches[i] for i in smp]) if ok else []
        assert len(models) <= ROOTS
        out["samples"].append(smp)
        out["roots"].append(len(models))
        for c in range(ROOTS):
            E = [float(v) for v in models[c]] if c < len(models) else None
            cnt = int((sampson_many(E, cols) < thr2).sum()) if E else 0
            out["counts"].append(cnt)
            out["valid"].append(E is not None)
            out["models"].append(E if E else [0.0] * 9)
            if E and key(cnt, h, c) > best_key:
                best_key, best = key(cnt, h, c), (h, c, E, cnt)
    out["n_models"] = sum(out["valid"])
    if best is None:
        out["status"] = NO_MODEL
        return out
    h, c, E, cnt = best
    cands = decompose(E)
    inl = [sampson(E, p) < thr2 for p in pts]
    assert sum(inl) == cnt
    passes = [[inl[i] and in_front(depths(*candidate(cands, k), pts[i]), distance) for k in range(4)] for i in range(n)]
    cheir = [sum(p[k] for p in passes) for k in range(4)]
    w = max(range(4), key=lambda k: (cheir[k], -k))
    R, t = candidate(cands, w)
    out.update(status=OK, R=R, t=t, E=E, n_ransac_inliers=cnt, n_inliers=cheir[w], best=h, root=c, sample=out["samples"][h], cheirality=cheir,
               inliers=[p[w] for p in passes], ransac_inliers=inl, winner=w, cands=cands)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the solver and the decomposition by other means: tolerances only
# ---------------------------------------------------------------------------------------------------------------------------
NODES = [2.0 * math.cos((2 * k + 1) * math.pi / 22.0) for k in range(11)]
XY = [(3, 0), (2, 1), (1, 2), (0, 3), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]   # x^3, x^2 y, x y^2, y^3, x^2, x y, y^2, x, y, 1


def pmul(a, b):
    """polynomials in (x, y, z) as 4 x 4 x 4 arrays of coefficients"""
    out = np.zeros((4, 4, 4))
    for ia in zip(*np.nonzero(a)):
        for ib in zip(*np.nonzero(b)):
            out[ia[0] + ib[0], ia[1] + ib[1], ia[2] + ib[2]] += a[ia] * b[ib]
    return out


def cubics(basis):
    """the ten cubics of E = x X + y Y + z Z + W: the entries of 2 E E^T E - tr(E E^T) E and det E"""
    E = np.empty((3, 3), object)
    for i in range(3):
        for j in range(3):
            p = np.zeros((4, 4, 4))
            p[1, 0, 0], p[0, 1, 0], p[0, 0, 1], p[0, 0, 0] = basis[0][i, j], basis[1][i, j], basis[2][i, j], basis[3][i, j]
            E[i, j] = p
    G = [[sum(pmul(E[i, l], E[m, l]) for l in range(3)) for m in range(3)] for i in range(3)]
    tr = G[0][0] + G[1][1] + G[2][2]
    out = [2.0 * sum(pmul(G[i][m], E[m, j]) for m in range(3)) - pmul(tr, E[i, j]) for i in range(3) for j in range(3)]
    det = (pmul(pmul(E[1, 1], E[2, 2]) - pmul(E[1, 2], E[2, 1]), E[0, 0]) + pmul(pmul(E[1, 2], E[2, 0]) - pmul(E[1, 0], E[2, 2]), E[0, 1])
           + pmul(pmul(E[1, 0], E[2, 1]) - pmul(E[1, 1], E[2, 0]), E[0, 2]))
    return out + [det]


def C_of(cub, z):
    zp = np.array([1.0, z, z * z, z * z * z])
    return np.array([[float(c[a, b, :] @ zp) for a, b in XY] for c in cub])


def numpy_solve5(cam, five, polish=3):
    """-> [E 3 x 3 with |E|_F^2 = 2]: the hidden-variable route with numpy's SVD, det, roots and lstsq"""
    d1 = np.array([bearing(*normalise(cam, m[0], m[1])) for m in five])
    d2 = np.array([bearing(*normalise(cam, m[2], m[3])) for m in five])
    A = np.array([np.outer(a, b).reshape(9) for a, b in zip(d1, d2)])
    if not np.isfinite(A).all():
        return []
    basis = [v.reshape(3, 3) for v in np.linalg.svd(A)[2][5:9]]
    cub = cubics(basis)
    dets = [np.linalg.det(C_of(cub, z)) for z in NODES]
    coef = np.linalg.solve(np.vander(NODES, 11, increasing=True), dets)
    flat = np.array([c.reshape(64) for c in cub])
    out = []
    for z in sorted(float(r.real) for r in np.roots(coef[::-1]) if abs(r.imag) < 1e-6 * max(1.0, abs(r))):
        v = np.linalg.svd(C_of(cub, z))[2][-1]
        if v[9] == 0.0:
            continue
        q = np.array([v[7] / v[9], v[8] / v[9], z])
        for _ in range(polish):
            pw = [np.array([1.0, w, w * w, w * w * w]) for w in q]
            dw = [np.array([0.0, 1.0, 2.0 * w, 3.0 * w * w]) for w in q]
            mon = lambda a, b, c: np.einsum("i,j,k->ijk", a, b, c).reshape(64)
            r = flat @ mon(pw[0], pw[1], pw[2])
            J = np.stack([flat @ mon(dw[0], pw[1], pw[2]), flat @ mon(pw[0], dw[1], pw[2]), flat @ mon(pw[0], pw[1], dw[2])], 1)
            q = q - np.linalg.lstsq(J, r, rcond=None)[0]
        E = q[0] * basis[0] + q[1] * basis[1] + q[2] * basis[2] + basis[3]
        out.append(E * math.sqrt(2.0 / (E * E).sum()))
    return out


def true_E(R, t):
    t = np.asarray(t, float)
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ np.asarray(R, float)
    return E * math.sqrt(2.0 / (E * E).sum())


def E_distance(models, E):
    """the smallest max |dE_ij| over the models and both signs"""
    return min([min(np.abs(np.asarray(m).reshape(3, 3) - E).max(), np.abs(np.asarray(m).reshape(3, 3) + E).max()) for m in models], default=math.inf)


def numpy_decompose(E):
    """-> the four (R, t) of E by its SVD"""
    U, _, Vt = np.linalg.svd(np.asarray(E, float).reshape(3, 3))
    U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return [(U @ Wk @ Vt, s * U[:, 2]) for Wk in (W, W.T) for s in (1.0, -1.0)]


def pose_error(pose, truth):
    """(max |dR_ij|, |t / |t| - t_true / |t_true||)"""
    R, t = np.asarray(pose[0], float).reshape(3, 3), np.asarray(pose[1], float)
    Rt, tt = np.asarray(truth[0], float), np.asarray(truth[1], float)
    return float(np.abs(R - Rt).max()), float(np.linalg.norm(t / np.linalg.norm(t) - tt / np.linalg.norm(tt)))
