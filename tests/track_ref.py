"""Fast tracking restated in plain Python from MCSlam/src/Tracking.cpp -- project_ (:208-260) and queryCurrentFrame /
querryEachFrame (:319-449) -- independently of csrc/mcorb_track.h: Python floats (IEEE doubles, one operation per operator),
numpy.float32 for the two casts and the bounds test, a sort on (d2, k) for the neighbours, lists with del / append for the
de-duplication.  gtsam's Pose3::transformFrom / transformTo, PinholePose::project2 and Cal3_S2::uncalibrate are written out as
recalled (gtsam 4.x); the kd-tree search is replaced by the exact neighbours, and a camera with fewer than 10 keypoints offers
only those it has.

A view is a dict: R0 (3 x 3 rows), t0, cols, rows, cams = [dict(R=3 x 3 rows, t, fx, fy, s, u0, v0)].  A store is a dict
lid -> (point, descriptor bytes)."""
import math

import numpy as np

KNN = 10


def default_nan32(v):
    """a NaN that is returned is the default quiet NaN (the C side pins it: host and device differ in an invalid operation's sign)"""
    return np.float32(np.nan) if np.isnan(v) else v


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def transform_from(R, t, X):
    """Pose3::transformFrom: R * X + t"""
    return [dot3(R[r], X) + t[r] for r in range(3)]


def transform_to(R, t, p):
    """Pose3::transformTo: R^T * (p - t)"""
    d = [p[0] - t[0], p[1] - t[1], p[2] - t[2]]
    return [R[0][r] * d[0] + R[1][r] * d[1] + R[2][r] * d[2] for r in range(3)]


class Cheirality(Exception):
    pass


def project2(view, p0):
    """CameraSet::project2 over the rig: one measurement per camera, or the exception of the first camera behind which p0 lies"""
    out = []
    for cam in view["cams"]:
        q = transform_to(cam["R"], cam["t"], p0)
        if q[2] <= 0:
            raise Cheirality()
        d = 1.0 / q[2]
        u, v = q[0] * d, q[1] * d
        out.append((cam["fx"] * u + cam["s"] * v + cam["u0"], cam["fy"] * v + cam["v0"]))
    return out


def project(view, store, lids):
    """project_: per camera the projected (lid, x, y) in candidate order, x and y numpy.float32; also per (lid, camera) why a
    pair did not make it: 'z', 'bounds' or None"""
    ncams = len(view["cams"])
    proj = [[] for _ in range(ncams)]
    why = {}
    seen = set()
    for lid in lids:
        if lid == -1 or lid in seen:
            continue
        seen.add(lid)
        p0 = transform_from(view["R0"], view["t0"], [float(v) for v in store[lid][0]])
        try:
            meas = project2(view, p0)
        except Cheirality:
            for c in range(ncams):
                why[(lid, c)] = "z"
            continue
        for c, (px, py) in enumerate(meas):
            with np.errstate(over="ignore", invalid="ignore"):
                x, y = default_nan32(np.float32(px)), default_nan32(np.float32(py))
            if x < np.float32(0) or x > np.float32(view["cols"]) or y < np.float32(0) or y > np.float32(view["rows"]):
                why[(lid, c)] = "bounds"
                continue
            why[(lid, c)] = None
            proj[c].append((lid, x, y))
    return proj, why


def hamming(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(bytes(a), bytes(b)))


def neighbours(x, y, kps, max_d2):
    """(d2, k) of the keypoints inside the radius, all of them, in order"""
    near = []
    for k, (kx, ky) in enumerate(kps):
        dx, dy = float(x) - float(kx), float(y) - float(ky)
        d2 = dx * dx + dy * dy
        if math.isnan(d2) or d2 > max_d2:
            continue
        near.append((d2, k))
    near.sort()
    return near


def query(x, y, desc, kps, kp_descs, max_d2, max_hamming):
    """one query of querryEachFrame before the mutex -> (bestMatchIndex, best, keypoints in radius, least distance among the 10)"""
    near = neighbours(x, y, kps, max_d2)
    best_kp, best, least = -1, 10000, None
    for d2, k in near[:KNN]:
        dist = hamming(desc, kp_descs[k])
        least = dist if least is None else min(least, dist)
        if dist < best and dist < max_hamming:
            best_kp, best = k, dist
    return best_kp, best, len(near), least


def dedup(queries, kps):
    """the serial part, :380-415, over (lid, best_kp, best) in query order -> the list of (kp, lid, dist), replacements, rejections"""
    entries, replaced, rejected = [], 0, 0
    for lid, k, dist in queries:
        if k == -1:
            continue
        pix = (int(kps[k][0]), int(kps[k][1]))
        found = None
        for i, e in enumerate(entries):
            if (int(kps[e[0]][0]), int(kps[e[0]][1])) == pix:
                found = i
                break
        if found is None:
            entries.append((k, lid, dist))
        elif entries[found][2] > dist:
            del entries[found]
            entries.append((k, lid, dist))
            replaced += 1
        else:
            rejected += 1
    return entries, replaced, rejected


def track(view, store, kps, kp_descs, lids, max_d2=10000.0, max_hamming=20):
    """-> dict with, per camera, proj = [(lid, x, y)], best = [(best_kp, best_dist)], matches = [(kp, lid, dist)], and the
    statistics a scene is judged by"""
    proj, why = project(view, store, lids)
    best, matches = [], []
    stats = dict(pairs=len(why), z=sum(w == "z" for w in why.values()), bounds=sum(w == "bounds" for w in why.values()),
                 projected=sum(w is None for w in why.values()), queries=0, matched=0, gated=0, empty=0, crowded=0, replaced=0,
                 rejected=0)
    for c, plist in enumerate(proj):
        rows = []
        for lid, x, y in plist:
            k, d, nnear, least = query(x, y, store[lid][1], kps[c], kp_descs[c], max_d2, max_hamming)
            rows.append((k, d))
            stats["queries"] += 1
            stats["matched"] += k != -1
            stats["gated"] += k == -1 and nnear > 0
            stats["empty"] += nnear == 0
            stats["crowded"] += nnear > KNN
        best.append(rows)
        entries, rep, rej = dedup([(lid, k, d) for (lid, _, _), (k, d) in zip(plist, rows)], kps[c])
        matches.append(entries)
        stats["replaced"] += rep
        stats["rejected"] += rej
    return dict(proj=proj, best=best, matches=matches, stats=stats)
