"""What keeping the local map up to date costs at one keyframe insertion (mcorb_lmap_observe, mcorb_lmap_update_points,
mcorb_lmap_delete: Landmark::addLfFrame, GlobalMap::updateLandmark, GlobalMap::deleteLandmark), on the same machine and inputs: a
4-camera rig, 3000 observe items (half with one view, the rest with 2 to 4; a few landmarks twice), update_points over 30 000
landmarks (a tenth of the corrections beyond the gate) and 300 deletes.
  device     the whole calls on a device store, and k_lmap_observe / k_lmap_update between HIP events, against their algorithmic
             bytes: 8 (item) + 48 (point, normal) + 24 + 4 (normal, n_rays) -- with the 4 bytes of n_rays read for a later
             observation 76 to 88 -- per observe item; 32 (item) + 24 (point) + 16 (result) [+ 24 for a stored point] per update item;
  host only  the same calls on the host-only store.
The two are timed in alternating runs, `reps` each after a warm-up; medians are reported.  Every run does the same work: the
corrections are offsets from the points a store holds, and the deleted landmarks are set and observed again outside the timed
part (an observed landmark's list grows by one entry per run).  bench.py times none of this.
    python scripts/landmark_rate.py [--reps 5] [--out profiles/landmark_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAMS, LANDMARKS, OBSERVE, DELETE, FEATS = 4, 30000, 3000, 300, 4000


def workload():
    rng = np.random.default_rng(21)
    pts = np.stack([rng.uniform(-20, 20, LANDMARKS), rng.uniform(-5, 5, LANDMARKS), rng.uniform(3, 40, LANDMARKS)], axis=1)
    mi = np.full((FEATS, CAMS), -1, np.int32)
    for i in range(FEATS):
        nv = 1 if i % 2 == 0 else int(rng.integers(2, CAMS + 1))
        mi[i, rng.choice(CAMS, nv, replace=False)] = i
    centres = rng.uniform(-0.3, 0.3, (CAMS, 3))
    old = rng.uniform(-2, 2, (CAMS, 3))
    lids = rng.permutation(LANDMARKS)[:OBSERVE].astype(np.int32)
    lids[rng.permutation(OBSERVE)[:60]] = lids[:60]                  # two features of the frame on one landmark
    feats = rng.permutation(FEATS)[:OBSERVE].astype(np.int32)
    d = rng.normal(size=(LANDMARKS, 3))
    d *= (np.where(rng.random(LANDMARKS) < 0.1, rng.uniform(5.5, 9, LANDMARKS), rng.uniform(0, 0.5, LANDMARKS)) / np.linalg.norm(d, axis=1))[:, None]
    return dict(pts=pts, mi=mi, centres=centres, old=old, lids=lids, feats=feats, delta=d,
                dele=rng.permutation(LANDMARKS)[:DELETE].astype(np.int32))


def side(mcorb, device, w):
    import kfdb_cases
    lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=LANDMARKS,
                        max_candidates=16)
    all_lids = np.arange(LANDMARKS, dtype=np.int32)
    lm.set(all_lids, w["pts"], np.zeros_like(w["pts"]))
    prev = mcorb.obs_frame(1, w["mi"], w["old"])
    lm.observe(prev, all_lids, all_lids % FEATS)                     # every landmark has an observation: the frame adds a later one
    cur = mcorb.obs_frame(2, w["mi"], w["centres"])
    return lm, cur, prev, all_lids


def run(lm, cur, prev, all_lids, w, t):
    """one keyframe insertion; appends the three calls' milliseconds to t and restores the store"""
    t0 = time.perf_counter()
    rays = lm.observe(cur, w["lids"], w["feats"])
    t1 = time.perf_counter()
    new = w["cur_pts"] + w["delta"]
    t2 = time.perf_counter()
    upd, diff = lm.update_points(all_lids, new)
    t3 = time.perf_counter()
    pairs = lm.delete(w["dele"], cap=8 * DELETE)
    t4 = time.perf_counter()
    t["observe"].append((t1 - t0) * 1e3), t["update_points"].append((t3 - t2) * 1e3), t["delete"].append((t4 - t3) * 1e3)
    w["cur_pts"] = np.where(upd[:, None], new, w["cur_pts"])
    # the deleted landmarks come back as they were
    lm.set(w["dele"], w["cur_pts"][w["dele"]], np.zeros((DELETE, 3)))
    lm.observe(prev, w["dele"], w["dele"] % FEATS)
    return rays, upd, diff, pairs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mcorb
    w = workload()
    sides = {"device": side(mcorb, 0, w), "host_only": side(mcorb, -1, w)}
    ws = {k: dict(w, cur_pts=w["pts"].copy()) for k in sides}
    t = {k: {"observe": [], "update_points": [], "delete": []} for k in sides}
    kus, same = [], True
    for rep in range(a.reps + 1):                                    # alternating; the first round is the warm-up
        out = {}
        for k, s in sides.items():
            out[k] = run(*s, ws[k], t[k])
            if k == "device":
                kus.append(s[0].last_landmark_timing())
        d, h = out["device"], out["host_only"]
        same = same and d[0].tolist() == h[0].tolist() and d[1].tolist() == h[1].tolist() and d[2].tobytes() == h[2].tobytes() and d[3] == h[3]
    lm_d, lm_h = sides["device"][0], sides["host_only"][0]
    for l in np.concatenate([w["lids"][:200], w["dele"][:50]]).tolist():
        a_, b_ = lm_d.get(l), lm_h.get(l)
        same = same and a_[0].tobytes() == b_[0].tobytes() and a_[1].tobytes() == b_[1].tobytes() and lm_d.observations(l) == lm_h.observations(l)
    views = (w["mi"][w["feats"]] != -1).sum(axis=1)
    kus = kus[1:]
    obs_us, upd_us = float(np.median([u[0] for u in kus])), float(np.median([u[1] for u in kus]))
    stored = int(out["device"][1].sum())
    obs_bytes, upd_bytes = OBSERVE * (8 + 48 + 4 + 24 + 4), LANDMARKS * (32 + 24 + 16) + stored * 24
    res = {"cores": len(os.sched_getaffinity(0)), "cameras": CAMS, "landmarks": LANDMARKS, "observe_items": OBSERVE,
           "observe_items_1_view": int((views == 1).sum()), "observe_items_2_to_4_views": int((views > 1).sum()),
           "observe_rounds": 2, "update_items": LANDMARKS, "update_items_stored": stored, "deletes": DELETE,
           "device_equals_host_only": bool(same),
           "k_lmap_observe_us": round(obs_us, 1), "k_lmap_observe_bytes": obs_bytes, "k_lmap_observe_GBps": round(obs_bytes / obs_us / 1e3, 2),
           "k_lmap_update_us": round(upd_us, 1), "k_lmap_update_bytes": upd_bytes, "k_lmap_update_GBps": round(upd_bytes / upd_us / 1e3, 2)}
    for k in sides:
        for call, v in t[k].items():
            v = v[1:]
            res["%s_%s_ms" % (k, call)] = round(float(np.median(v)), 3)
            res["%s_%s_ms_min_max" % (k, call)] = [round(min(v), 3), round(max(v), 3)]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
