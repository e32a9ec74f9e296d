"""What one frame of fast tracking costs (mcorb_lmap_track: Tracking::project_ and Tracking::queryCurrentFrame), on the same
machine and inputs: 5 map entries of 3000 l_ids that name about 10 000 distinct landmarks, a rig of 4 cameras at 1280 x 720 and
2000 keypoints per camera, made from the true projections plus noise and clutter.
  device     the whole call on a device store, and k_track_project / k_track_match between HIP events; k_track_match against
             its algorithmic work -- queries x keypoints distance evaluations (5 fp64 operations each), and the bytes of the
             keypoints (8 per keypoint), of the descriptors the ten neighbours of a query need (10 x 32, and 32 of the landmark's),
             of the queries (8 + 1) and of the results (8);
  host only  the same call on the host-only store, on one thread.  (The reference runs one thread per camera.)
The two are timed in alternating runs, `reps` each after a warm-up; medians are reported.  bench.py times none of this.
    python scripts/track_rate.py [--reps 5] [--out profiles/track_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAMS, COLS, ROWS, KEYPOINTS, LANDMARKS, ENTRIES, LIDS_PER_ENTRY = 4, 1280, 720, 2000, 10000, 5, 3000


def workload():
    import track_cases as T
    rng = np.random.default_rng(31)
    cams = []
    for c in range(CAMS):
        Rc = T.rot(1, rng.uniform(-0.05, 0.05)) @ T.rot(0, rng.uniform(-0.03, 0.03))
        cams.append(T.cam(Rc, (0.25 * c - 0.4, rng.uniform(-0.02, 0.02), 0.0), fx=700.0, fy=700.0, s=0.0, u0=COLS / 2, v0=ROWS / 2))
    v = T.view(cams, COLS, ROWS, T.rot(1, 0.04), (0.2, -0.1, 0.3))
    pts = np.stack([rng.uniform(-8, 8, LANDMARKS), rng.uniform(-4.5, 4.5, LANDMARKS), rng.uniform(-1, 9, LANDMARKS)], axis=1)
    desc = rng.integers(0, 256, (LANDMARKS, 32), dtype=np.uint8)
    # the map entries' l_ids: windows of the landmark range that overlap, with -1 for features without a landmark
    lids = []
    for e in range(ENTRIES):
        w = (np.arange(LIDS_PER_ENTRY) * 3 + e * (LANDMARKS - LIDS_PER_ENTRY) // (ENTRIES - 1) + rng.integers(0, 3, LIDS_PER_ENTRY)) % LANDMARKS
        w[rng.random(LIDS_PER_ENTRY) < 0.05] = -1
        lids.append(w)
    lids = np.concatenate(lids).astype(np.int32)
    # keypoints: the landmarks' own projections (vectorised: a workload, not a reference), moved by a pixel, plus clutter
    R0, t0 = np.array(v["R0"]), np.array(v["t0"])
    p0 = pts @ R0.T + t0
    kps, descs = [], []
    for c in cams:
        q = (p0 - np.array(c["t"])) @ np.array(c["R"])
        ok = q[:, 2] > 0.1
        u = q[:, 0] / np.where(ok, q[:, 2], 1.0) * c["fx"] + c["u0"]
        w_ = q[:, 1] / np.where(ok, q[:, 2], 1.0) * c["fy"] + c["v0"]
        ok &= (u > 0) & (u < COLS) & (w_ > 0) & (w_ < ROWS)
        idx = rng.permutation(np.flatnonzero(ok))[:KEYPOINTS * 3 // 4]
        xy = np.stack([u[idx], w_[idx]], axis=1) + rng.normal(0, 1.0, (len(idx), 2))
        d = desc[idx].copy()
        flips = rng.integers(0, 256, (len(idx), 24))                   # up to 24 bits flipped
        for j in range(24):
            on = rng.random(len(idx)) < 0.5
            d[on, flips[on, j] // 8] ^= (1 << (flips[on, j] % 8)).astype(np.uint8)
        nclutter = KEYPOINTS - len(idx)
        xy = np.concatenate([xy, np.stack([rng.uniform(0, COLS, nclutter), rng.uniform(0, ROWS, nclutter)], axis=1)])
        d = np.concatenate([d, rng.integers(0, 256, (nclutter, 32), dtype=np.uint8)])
        order = rng.permutation(KEYPOINTS)
        kps.append(np.ascontiguousarray(xy[order], np.float32))
        descs.append(np.ascontiguousarray(d[order]))
    return dict(view=v, pts=pts, desc=desc, lids=lids, kps=kps, descs=descs)


def side(mcorb, device, w):
    import kfdb_cases
    lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=LANDMARKS,
                        max_candidates=LANDMARKS)
    lm.set(np.arange(LANDMARKS, dtype=np.int32), w["pts"], np.zeros_like(w["pts"]), w["desc"])
    return lm


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mcorb
    import track_cases as T
    w = workload()
    view = T.to_view(mcorb, w["view"])
    sides = {"device": side(mcorb, 0, w), "host_only": side(mcorb, -1, w)}
    t = {k: [] for k in sides}
    kus, same, res_d = [], True, None
    for rep in range(a.reps + 1):                                      # alternating; the first round is the warm-up
        out = {}
        for k, lm in sides.items():
            t0 = time.perf_counter()
            out[k] = lm.track(view, w["kps"], w["descs"], w["lids"])
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "device":
                kus.append(lm.last_track_timing())
        same = same and T.as_lists(out["device"]) == T.as_lists(out["host_only"])
        res_d = out["device"]
    kus = kus[1:]
    proj_us, match_us = float(np.median([u[0] for u in kus])), float(np.median([u[1] for u in kus]))
    queries = [len(p) for p in res_d.proj_lid]
    evals = sum(q * KEYPOINTS for q in queries)
    nq = sum(queries)
    match_bytes = CAMS * KEYPOINTS * 8 + nq * (10 * 32 + 32 + 8 + 8) + res_d.n_candidates * CAMS
    proj_bytes = res_d.n_candidates * (4 + 24 + CAMS * 9)
    res = {"cores": len(os.sched_getaffinity(0)), "cameras": CAMS, "image": [COLS, ROWS], "keypoints_per_camera": KEYPOINTS,
           "lids": int(len(w["lids"])), "candidates": int(res_d.n_candidates), "queries_per_camera": queries,
           "matched_per_camera": [int((b >= 0).sum()) for b in res_d.best_kp], "matches_per_camera": [len(m) for m in res_d.match_kp],
           "device_equals_host_only": bool(same),
           "k_track_project_us": round(proj_us, 1), "k_track_project_bytes": proj_bytes,
           "k_track_match_us": round(match_us, 1), "k_track_match_distance_evaluations": evals,
           "k_track_match_Gevals_per_s": round(evals / match_us / 1e3, 2), "k_track_match_fp64_GFLOPs": round(5 * evals / match_us / 1e3, 1),
           "k_track_match_bytes": match_bytes, "k_track_match_GBps": round(match_bytes / match_us / 1e3, 2)}
    for k in sides:
        v = t[k][1:]
        res["%s_track_ms" % k] = round(float(np.median(v)), 3)
        res["%s_track_ms_min_max" % k] = [round(min(v), 3), round(max(v), 3)]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
