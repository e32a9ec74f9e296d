"""FrontEnd::TriangulateNewLandmarks (MCSlam/src/FrontEnd.cpp:6465-6700) restated in plain Python, independently of
csrc/mcorb_mapping_new.h: Python floats, numpy.float32 where the reference has `float`, in the stated operation order.  The
initial point comes from the library's DLT hook (mcorb_host_triangulate, held to 1e-9 against an SVD by test_mapping_cpu.py), so
everything after it compares bit for bit.  A NaN that is returned is the default quiet NaN, as the library states."""
import math
import struct

import numpy as np

from mapping_ref import div, rays, views_of

f32 = np.float32
CHI2 = 5.991
COS_MAX = 0.99998


def canon(x):
    """the default quiet NaN for any NaN"""
    return float("nan") if x != x else x


def dbits(x):
    """a double as raw bytes, every NaN the default one"""
    x = float(x)
    return struct.pack("<Q", 0x7ff8000000000000) if x != x else struct.pack("<d", x)


def fbits(x):
    x = f32(x)
    return struct.pack("<I", 0x7fc00000) if x != x else x.tobytes()


def mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def point_in_camera(P, X):
    p = []
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += mul(P[r][k], X[k])
        p.append(s + P[r][3])
    return p


def residual(view, X):
    """-> (rx, ry, J as 2 x 3) of TriangulationFactor with unit noise; behind a camera: (2 fx, 2 fx) and J = 0"""
    P, K = view["P"], view["K"]
    fx, fy, u0, v0 = K[0][0], K[1][1], K[0][2], K[1][2]
    p = point_in_camera(P, X)
    if p[2] <= 0:
        return 2.0 * fx, 2.0 * fx, [[0.0] * 3, [0.0] * 3]
    d = div(1.0, p[2])
    u, v = mul(p[0], d), mul(p[1], d)
    rx = (mul(fx, u) + u0) - float(view["kx"])
    ry = (mul(fy, v) + v0) - float(view["ky"])
    D = [[mul(fx, d), 0.0, -mul(mul(fx, u), d)], [0.0, mul(fy, d), -mul(mul(fy, v), d)]]
    J = [[(mul(D[r][0], P[0][c]) + mul(D[r][1], P[1][c])) + mul(D[r][2], P[2][c]) for c in range(3)] for r in range(2)]
    return rx, ry, J


def normal_equations(views, X):
    H = {(i, j): 0.0 for i in range(3) for j in range(i, 3)}
    g = [0.0] * 3
    sq = 0.0
    for view in views:
        rx, ry, J = residual(view, X)
        for i in range(3):
            for j in range(i, 3):
                H[i, j] = H[i, j] + (mul(J[0][i], J[0][j]) + mul(J[1][i], J[1][j]))
        for i in range(3):
            g[i] = g[i] + (mul(J[0][i], rx) + mul(J[1][i], ry))
        sq = sq + (mul(rx, rx) + mul(ry, ry))
    return H, g, mul(0.5, sq)


def solve(H, g, lam):
    """(H + lam I) delta = -g by LDL^T; None when a pivot is not > 0"""
    a00, a01, a02, a11, a12, a22 = H[0, 0] + lam, H[0, 1], H[0, 2], H[1, 1] + lam, H[1, 2], H[2, 2] + lam
    d0 = a00
    l10, l20 = div(a01, d0), div(a02, d0)
    d1 = a11 - mul(mul(l10, l10), d0)
    l21 = div(a12 - mul(mul(l20, l10), d0), d1)
    d2 = (a22 - mul(mul(l20, l20), d0)) - mul(mul(l21, l21), d1)
    if not (d0 > 0 and d1 > 0 and d2 > 0):
        return None
    y0 = -g[0]
    y1 = -g[1] - mul(l10, y0)
    y2 = (-g[2] - mul(l20, y0)) - mul(l21, y1)
    x2 = div(y2, d2)
    x1 = div(y1, d1) - mul(l21, x2)
    x0 = (div(y0, d0) - mul(l10, x1)) - mul(l20, x2)
    return [x0, x1, x2]


def optimize(views, X0):
    """-> (X, solves, cost_initial, cost_final, accepted steps)"""
    X = list(X0)
    H, g, cost = normal_equations(views, X)
    cost_initial, lam, solves, accepted = cost, 1.0, 0, 0
    for it in range(50):
        solves = it + 1
        delta = solve(H, g, lam)
        accept = False
        if delta is not None:
            Xt = [X[k] + delta[k] for k in range(3)]
            Ht, gt, ct = normal_equations(views, Xt)
            accept = ct < cost
        if accept:
            dec = cost - ct
            stop = dec <= 1.0 or dec <= mul(1e-5, cost)
            X, H, g, cost = Xt, Ht, gt, ct
            accepted += 1
            lam = lam / 10.0
            if stop:
                break
        else:
            lam = lam * 10.0
            if lam > 1e5:
                break
    return X, solves, cost_initial, cost, accepted


def blank(verdict):
    return dict(verdict=verdict, X=[0.0] * 3, normal=[0.0] * 3, n_rays=0, dist=0.0, cos=f32(0.0), solves=0, cost_initial=0.0,
                cost_final=0.0, accepted=0)


def refine(views, nv1, X0, twc_cur, twc_prev, inv_sigma2):
    """everything after the DLT -> dict(verdict, X, normal, n_rays, dist, cos (float32), solves, cost_initial, cost_final)"""
    X0 = [float(x) for x in X0]
    if not all(math.isfinite(x) for x in X0):
        return blank(8)
    r = blank(0)
    r["X"] = X0
    for view in views:
        if point_in_camera(view["P"], X0)[2] <= 0:
            r["verdict"] = 3
            return r
    X, r["solves"], r["cost_initial"], r["cost_final"], r["accepted"] = optimize(views, X0)
    r["X"] = X
    for view in views:
        rx, ry, _ = residual(view, X)
        err = mul(mul(rx, rx) + mul(ry, ry), float(f32(inv_sigma2[view["octave"]])))
        if err > CHI2:
            r["verdict"] = 4
            return r
    ray = [X[k] - float(twc_cur[k]) for k in range(3)]
    ray1 = [X[k] - float(twc_prev[k]) for k in range(3)]
    s = s1 = dot = 0.0
    for k in range(3):
        s += mul(ray[k], ray[k])
    for k in range(3):
        s1 += mul(ray1[k], ray1[k])
    for k in range(3):
        dot += mul(ray1[k], ray[k])
    dist = math.sqrt(s)
    with np.errstate(all="ignore"):
        dist1 = f32(math.sqrt(s1))
        cos = f32(div(dot, mul(float(dist1), dist)))
    r["dist"], r["cos"] = dist, cos
    if float(cos) >= COS_MAX:
        r["verdict"] = 5
        return r
    acc = rays(views[:nv1], X)
    n_rays = nv1
    inv = 1.0 / n_rays
    normal = [mul(a, inv) for a in acc]
    acc = rays(views[nv1:], X)
    normal = [mul(normal[k], float(n_rays)) + acc[k] for k in range(3)]
    n_rays += len(views) - nv1
    inv = 1.0 / n_rays
    r["normal"], r["n_rays"] = [mul(c, inv) for c in normal], n_rays
    return r


def initial_point(mc, views):
    """X0 of the library's DLT on x = ((kx - K02) / K00, (ky - K12) / K11)"""
    x = np.array([[v["x"], v["y"]] for v in views], np.float64)
    P = np.ascontiguousarray([np.asarray(v["P"], np.float64).reshape(12) for v in views])
    X = np.zeros(3)
    assert mc._lib.load().mcorb_host_triangulate(x.ctypes.data, P.ctypes.data, len(views), X.ctypes.data) == 0
    return [float(v) for v in X]


def triangulate_new(mc, cur, lids_cur, prev, lids_prev, matches, K, inv_sigma2, next_lid):
    """the serial walk -> dict of per-match lists and the rest"""
    lc, lp = [int(l) for l in lids_cur], [int(l) for l in lids_prev]
    out = dict(records=[], verdict=[], inliers=[], new_lid=[], depth_vec=[], avg_depth=0.0, n_rays_hist=[0] * 16, n_by_verdict=[0] * 9)
    for q, t in np.asarray(matches).reshape(-1, 2).tolist():
        if lc[t] != -1:
            r = blank(6)
        else:
            v1, v2 = views_of(prev, q, K), views_of(cur, t, K)
            r = refine(v1 + v2, len(v1), initial_point(mc, v1 + v2), cur["twc"], prev["twc"], inv_sigma2)
        out["n_by_verdict"][r["verdict"]] += 1
        if r["verdict"] == 0:
            lp[q] = lc[t] = next_lid
            out["new_lid"].append(next_lid)
            out["depth_vec"].append(r["dist"])
            out["avg_depth"] += r["dist"]
            out["n_rays_hist"][len(v2) - 1] += 1
            next_lid += 1
        else:
            out["new_lid"].append(-1)
        out["records"].append(r)
        out["verdict"].append(r["verdict"])
        out["inliers"].append(r["verdict"] == 0)
    out["lids_cur"], out["lids_prev"], out["next_lid"] = lc, lp, next_lid
    return out
