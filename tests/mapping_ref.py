"""FrontEnd::triangulateNeighbors / triangulateMatches / getSceneDepthStats and Landmark::updateNormal restated in plain Python,
independently of csrc/mcorb_mapping.h: numpy.float32 scalars where the reference has `float`, Python floats elsewhere, in the
reference's operation order; the triangulation is numpy.linalg.svd on the DLT design (cv::sfm::triangulatePoints)."""
import math

import numpy as np

f32 = np.float32
NAN = float("nan")


def div(a, b):
    """IEEE double division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def views_of(frame, feat, K):
    """get3D_2DCorrs: cameras ascending with matchIndex != -1"""
    out = []
    for c, ind in enumerate(frame["match_index"][feat]):
        if ind == -1:
            continue
        kp = frame["kps"][c][ind]
        Kc = K[c]
        x = (float(kp["x"]) - float(Kc[0][2])) / float(Kc[0][0])
        y = (float(kp["y"]) - float(Kc[1][2])) / float(Kc[1][1])
        out.append(dict(cam=c, x=x, y=y, kx=f32(kp["x"]), ky=f32(kp["y"]), octave=int(kp["octave"]),
                        P=[[float(v) for v in row] for row in np.asarray(frame["proj"][c]).reshape(-1, 4)[:3]],
                        K=[[float(v) for v in row] for row in np.asarray(Kc).reshape(3, 3)],
                        centre=[float(v) for v in frame["centre_w"][c]]))
    return out


def centre_of(P):
    """-1 * R^T * t"""
    o = []
    for i in range(3):
        s = 0.0
        for k in range(3):
            s += P[k][i] * P[k][3]
        o.append(-s)
    return o


def epipolar(v1, v2, F):
    """-> (verdict 0 / 1 / 2, num * num / den as a float or None)"""
    F = [[float(v) for v in row] for row in np.asarray(F).reshape(3, 3)]
    x1, y1 = float(v1["kx"]), float(v1["ky"])
    with np.errstate(all="ignore"):
        a = f32(x1 * F[0][0] + y1 * F[0][1] + F[0][2])
        b = f32(x1 * F[1][0] + y1 * F[1][1] + F[1][2])
        c = f32(x1 * F[2][0] + y1 * F[2][1] + F[2][2])
        num = a * v2["kx"] + b * v2["ky"] + c
        den = a * a + b * b
        assert num.dtype == np.float32 and den.dtype == np.float32
        if den == 0:
            return 1, None
        d = num * num / den
        assert d.dtype == np.float32
    return (2 if float(d) >= 4.0 else 0), float(d)


def triangulate(views):
    """cv::sfm::triangulatePoints: triangulateDLT for two views, triangulateNViews otherwise; the null vector by SVD"""
    n = len(views)
    if n == 2:
        D = np.zeros((4, 4))
        for i, v in enumerate(views):
            P = np.array(v["P"])
            D[2 * i] = v["x"] * P[2] - P[0]
            D[2 * i + 1] = v["y"] * P[2] - P[1]
    else:
        D = np.zeros((3 * n, 4 + n))
        for i, v in enumerate(views):
            D[3 * i:3 * i + 3, :4] = -np.array(v["P"])
            D[3 * i:3 * i + 3, 4 + i] = [v["x"], v["y"], 1.0]
    h = np.linalg.svd(D)[2][-1]
    return [float(h[0] / h[3]), float(h[1] / h[3]), float(h[2] / h[3])]


def rays(views, X):
    acc = [0.0, 0.0, 0.0]
    for v in views:
        d = [X[k] - v["centre"][k] for k in range(3)]
        sq = 0.0
        for k in range(3):
            sq += d[k] * d[k]
        inv = div(1.0, math.sqrt(sq))
        acc = [acc[k] + d[k] * inv for k in range(3)]
    return acc


def after(views, nv1, X, inv_sigma2):
    """the per-view gates, the parallax window and the normal for a given X -> dict(verdict, dist2, cos, normal, n_rays, near)"""
    r = dict(verdict=0, dist2=0.0, cos=0.0, normal=[0.0] * 3, n_rays=0, near=False, X=list(X))
    for v in views:
        P, K = v["P"], v["K"]
        p = []
        for row in range(3):
            s = 0.0
            for k in range(3):
                s += P[row][k] * X[k]
            p.append(s + P[row][3])
        if abs(p[2]) <= 1e-6 * math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]):
            r["near"] = True
        if p[2] < 0:
            r["verdict"] = 3
            return r
        q = []
        for row in range(3):
            s = 0.0
            for k in range(3):
                s += K[row][k] * p[k]
            q.append(s)
        ex, ey = div(q[0], q[2]), div(q[1], q[2])
        kx, ky = float(v["kx"]), float(v["ky"])
        err = (ex - kx) * (ex - kx) + (ey - ky) * (ey - ky)
        err = err * float(inv_sigma2[v["octave"]])
        if abs(err - 5.991) <= 1e-6 * 5.991:
            r["near"] = True
        if err > 5.991:
            r["verdict"] = 4
            return r
    o1, o2 = centre_of(views[0]["P"]), centre_of(views[nv1]["P"])
    n1 = [X[k] - o1[k] for k in range(3)]
    n2 = [X[k] - o2[k] for k in range(3)]
    s1 = s2 = dot = 0.0
    for k in range(3):
        s1 += n1[k] * n1[k]
    for k in range(3):
        s2 += n2[k] * n2[k]
    for k in range(3):
        dot += n1[k] * n2[k]
    dist1, dist2 = math.sqrt(s1), math.sqrt(s2)
    cos = div(dot, dist1 * dist2)
    r["dist2"], r["cos"] = dist2, cos
    if abs(cos - 0.99998) <= 1e-6 * 0.99998 or abs(cos - 0.5) <= 1e-6 * 0.5:
        r["near"] = True
    if not (cos < 0.99998 and cos > 0.5):
        r["verdict"] = 5
        return r
    acc = rays(views[:nv1], X)
    n_rays = nv1
    inv = 1.0 / n_rays
    normal = [a * inv for a in acc]
    acc = rays(views[nv1:], X)
    normal = [normal[k] * float(n_rays) + acc[k] for k in range(3)]
    n_rays += len(views) - nv1
    inv = 1.0 / n_rays
    r["normal"], r["n_rays"] = [c * inv for c in normal], n_rays
    return r


def match(neigh, q, cur, t, F_table, K, inv_sigma2, triangulate=triangulate):
    """one match from :5826 to :5937; F_table[c_cur][c_neigh]"""
    v1, v2 = views_of(neigh, q, K), views_of(cur, t, K)
    F = np.asarray(F_table).reshape(len(K), len(K), 3, 3)[v2[0]["cam"]][v1[0]["cam"]]
    verdict, d = epipolar(v1[0], v2[0], F)
    near = d is not None and abs(d - 4.0) <= 1e-6 * 4.0
    if verdict:
        return dict(verdict=verdict, dist2=0.0, cos=0.0, normal=[0.0] * 3, n_rays=0, near=near, X=[0.0] * 3)
    r = after(v1 + v2, len(v1), triangulate(v1 + v2), inv_sigma2)
    r["near"] = r["near"] or near
    return r


def depth_z(Rcw, tcw, pt):
    s = 0.0
    for k in range(3):
        s += float(Rcw[2][k]) * float(pt[k])
    return s + float(tcw[2])


def triangulate_neighbours(store, cur, lids_cur, neigh, lids_neigh, F21, matches, K, inv_sigma2, Rcw, tcw, next_lid, triangulate=triangulate):
    """store: lid -> pt3D of the landmarks that exist.  -> dict of per-match lists (neighbours back to back) and the rest.
    triangulate(views) -> X: by default the SVD above; with the library's DLT in its place (mapping_new_ref.initial_point)
    everything behind the point compares bit for bit"""
    lc = [int(l) for l in lids_cur]
    out = dict(verdict=[], inliers=[], new_lid=[], pt3d=[], normal=[], near=[], skipped=[], depth_vec=[], lids_neigh=[], new={}, dist2=[],
               cos=[])
    twc = [float(v) for v in cur["twc"]]
    for s, kf in enumerate(neigh):
        ln = [int(l) for l in lids_neigh[s]]
        zs = sorted(depth_z(Rcw, tcw, store[l]) for l in ln if l != -1)
        skip = 0
        if not zs:
            skip = 2
        else:
            median = zs[(len(zs) - 1) // 2]
            d = [twc[k] - float(kf["twc"][k]) for k in range(3)]
            sq = 0.0
            for k in range(3):
                sq += d[k] * d[k]
            if div(math.sqrt(sq), median) < 0.01:
                skip = 1
        out["skipped"].append(skip)
        for q, t in np.asarray(matches[s]).reshape(-1, 2).tolist():
            r = None
            if skip:
                v = 7
            elif ln[q] != -1 or lc[t] != -1:
                v = 6
            else:
                r = match(kf, q, cur, t, F21[s], K, inv_sigma2, triangulate)
                v = r["verdict"]
            out["verdict"].append(v)
            out["inliers"].append(v in (0, 5))
            out["near"].append(bool(r and r["near"]))
            out["dist2"].append(r["dist2"] if r else 0.0)      # (0.0 where the match did not come to the parallax window)
            out["cos"].append(r["cos"] if r else 0.0)
            if v == 0:
                ln[q] = lc[t] = next_lid
                out["new"][next_lid] = (r["X"], r["normal"])
                out["new_lid"].append(next_lid)
                out["pt3d"].append(r["X"])
                out["normal"].append(r["normal"])
                out["depth_vec"].append(r["dist2"])
                next_lid += 1
            else:
                out["new_lid"].append(-1)
                out["pt3d"].append([0.0] * 3)
                out["normal"].append([0.0] * 3)
        out["lids_neigh"].append(ln)
    out["lids_cur"], out["next_lid"] = lc, next_lid
    return out
