"""FrontEnd::initialization (MCSlam/src/FrontEnd.cpp:2633-2839) restated in plain Python, independently of csrc/mcorb_init.h:
numpy.float32 scalars where the reference has `float`, Python floats elsewhere, in the reference's operation order; the
triangulation is numpy.linalg.svd on the DLT design (mapping_ref.triangulate) and the medians come from sorted().

A view is mapping_ref.views_of's dict.  For a view of the current frame `centre` holds the camera's cam_centre_body (the
translation column of cur_T_ref.inv()): the world centre is formed here from [R | t'], as the reference's updateNormal does."""
import math
import struct

import numpy as np

import mapping_ref as MR

DONE, BASELINE, PARALLAX, FEW = 0, 1, 2, 3
NAN = float("nan")


def sort_key(x):
    """the stated order where std::sort is undefined: the monotone key of the double's bits, any NaN after +inf"""
    if x != x:
        return 1 << 64
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | (1 << 63))


def baseline_ok(t, min_baseline):
    s = 0.0
    for k in range(3):
        s += float(t[k]) * float(t[k])
    return math.sqrt(s) > min_baseline


def gates(views, nv1, X, inv_sigma2):
    """:2702-2753 for a given X -> dict(verdict 0 / 3 / 4 / 5, dist2, cos, near)"""
    r = dict(verdict=0, dist2=0.0, cos=0.0, near=False, X=[float(v) for v in X])
    X = r["X"]
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
        ex, ey = MR.div(q[0], q[2]), MR.div(q[1], q[2])
        kx, ky = float(v["kx"]), float(v["ky"])
        err = (ex - kx) * (ex - kx) + (ey - ky) * (ey - ky)
        err = err * float(inv_sigma2[v["octave"]])
        if abs(err - 5.991) <= 1e-6 * 5.991:
            r["near"] = True
        if err > 5.991:
            r["verdict"] = 4
            return r
    o1, o2 = MR.centre_of(views[0]["P"]), MR.centre_of(views[nv1]["P"])
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
    cos = MR.div(dot, dist1 * dist2)
    r["dist2"], r["cos"] = dist2, cos
    if abs(cos - 0.99998) <= 1e-6 * 0.99998:
        r["near"] = True
    if not cos < 0.99998:
        r["verdict"] = 5
    return r


def normal_of(views, nv1, X, R, t_out):
    """Landmark(pt, lf_prev, ..) then addLfFrame(currentFrame, ..) on the stored point -> (normal, n_rays)"""
    acc = MR.rays(views[:nv1], X)
    n_rays = nv1
    inv = 1.0 / n_rays
    normal = [a * inv for a in acc]
    cur = []
    for v in views[nv1:]:
        c = v["centre"]
        w = [((R[i][0] * c[0] + R[i][1] * c[1]) + R[i][2] * c[2]) + t_out[i] for i in range(3)]
        cur.append(dict(centre=w))
    acc = MR.rays(cur, X)
    normal = [normal[k] * float(n_rays) + acc[k] for k in range(3)]
    n_rays += len(cur)
    inv = 1.0 / n_rays
    return [c * inv for c in normal], n_rays


def finish(recs, flags, views, nv1s, R, t, ncams, next_lid):
    """:2761-2839 over the loop's records (recs[i] is None where flags[i] is clear; views[i] / nv1s[i] are read for accepted
    matches only) -> the call's dict"""
    n = len(recs)
    R = [[float(v) for v in row] for row in np.asarray(R, np.float64).reshape(3, 3)]
    t = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
    par = [r["cos"] for r, f in zip(recs, flags) if f and r["verdict"] in (0, 5)]
    dep = [r["dist2"] for r, f in zip(recs, flags) if f and r["verdict"] == 0]
    parallax = depth = 0.0
    if par and dep:
        parallax = sorted(par, key=sort_key)[len(par) // 2]
        depth = sorted(dep, key=sort_key)[len(dep) // 2]
    out = dict(status=DONE, parallax=parallax, median_scene_depth=depth, n_matches=n, n_initial_inliers=sum(1 for f in flags if f),
               n_parallax=len(par), n_triangulated=len(dep), scaled=False, t_out=list(t), next_lid=next_lid,
               verdict=[r["verdict"] if f else 9 for r, f in zip(recs, flags)],
               inliers=[bool(f and r["verdict"] == 0) for r, f in zip(recs, flags)],
               near=[bool(f and r["near"]) for r, f in zip(recs, flags)],
               dist2=[r["dist2"] if f and r["verdict"] in (0, 5) else 0.0 for r, f in zip(recs, flags)],
               cos=[r["cos"] if f and r["verdict"] in (0, 5) else 0.0 for r, f in zip(recs, flags)],
               new_lid=[-1] * n, pt3d=[[0.0] * 3 for _ in range(n)], normal=[[0.0] * 3 for _ in range(n)], n_rays=[0] * n, new={})
    for i in range(n):
        if out["verdict"][i] == 0:
            out["pt3d"][i] = list(recs[i]["X"])
    if not (len(par) > 0 and parallax < 0.99998):
        out["status"] = PARALLAX
        return out
    if not len(dep) > 50:
        out["status"] = FEW
        return out
    s = 1.0
    if ncams == 1 or n < 50:
        out["scaled"] = True
        s = MR.div(1.0, depth)
        out["t_out"] = [v * s for v in t]
    for i in range(n):
        if out["verdict"][i] != 0:
            continue
        X = [v * s for v in recs[i]["X"]] if out["scaled"] else list(recs[i]["X"])
        normal, n_rays = normal_of(views[i], nv1s[i], X, R, out["t_out"])
        out["new_lid"][i], out["pt3d"][i], out["normal"][i], out["n_rays"][i] = next_lid, X, normal, n_rays
        out["new"][next_lid] = (X, normal, n_rays)
        next_lid += 1
    out["next_lid"] = next_lid
    return out


def run_cases(cases, flags, R, t, ncams, min_baseline):
    """the hook's restatement: cases[i] = dict(X, nv1, views) with caller-given X"""
    if not baseline_ok(t, min_baseline):
        return dict(status=BASELINE)
    sig = cases[0]["inv_sigma2"]
    recs = [gates(c["views"], c["nv1"], c["X"], sig) if f else None for c, f in zip(cases, flags)]
    return finish(recs, flags, [c["views"] for c in cases], [c["nv1"] for c in cases], R, t, ncams, 0)


def initialize(prev, lids_prev, cur, lids_cur, R, t, cam_centre_body, matches, inliers, K, inv_sigma2, next_lid, min_baseline,
               triangulate=MR.triangulate):
    """the whole call; prev / cur: mapping_cases frames (cur's centre_w is not read) -> finish's dict with lids_prev / lids_cur.
    triangulate(views) -> X: by default mapping_ref's SVD; with the library's DLT in its place (mapping_new_ref.initial_point)
    everything behind the point compares bit for bit"""
    lp, lc = [int(l) for l in lids_prev], [int(l) for l in lids_cur]
    if not baseline_ok(t, min_baseline):
        return dict(status=BASELINE, lids_prev=lp, lids_cur=lc)
    cur_body = dict(cur, centre_w=[[float(v) for v in c] for c in cam_centre_body])
    recs, views, nv1s = [], [], []
    for (q, tr), f in zip(np.asarray(matches).reshape(-1, 2).tolist(), inliers):
        v1, v2 = MR.views_of(prev, q, K), MR.views_of(cur_body, tr, K)
        views.append(v1 + v2)
        nv1s.append(len(v1))
        recs.append(gates(v1 + v2, len(v1), triangulate(v1 + v2), inv_sigma2) if f else None)
    out = finish(recs, [bool(f) for f in inliers], views, nv1s, R, t, len(K), next_lid)
    if out["status"] == DONE:
        for (q, tr), lid in zip(np.asarray(matches).reshape(-1, 2).tolist(), out["new_lid"]):
            if lid != -1:
                lp[q] = lc[tr] = lid
    out["lids_prev"], out["lids_cur"] = lp, lc
    return out
