"""What one local-map search costs (mcorb_lmap_search: FrontEnd::searchLocalMap2 up to the camera-filtered matches), on the same
machine and inputs: 10 neighbouring keyframes of 3000 lIds each (a fifth of them -1, drawn from a map of 20000 landmarks, so the
keyframes overlap), a rig of 4 cameras at 1280 x 720 and a probe of 3000 LF features whose descriptors the landmarks' are near
copies of; a synthetic vocabulary (k = 10, L = 3, FeatureVector nodes one level above the words).
  device     the whole search call on a device store, and k_lmap_cull / k_kfdb_best2 between HIP events; k_lmap_cull against its
             algorithmic bytes: 48 B of point and normal, the 4-byte candidate id and the 4-byte mask per candidate;
  host only  the same call on the host-only store, vocabulary and database.
The two are timed in alternating runs, `reps` each; medians are reported.  bench.py times none of this.
    python scripts/lmap_rate.py [--reps 5] [--out profiles/lmap_rate.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KFS, LIDS, MAP, NPROBE, CAMS, W, H, LEVELSUP = 10, 3000, 20000, 3000, 4, 1280, 720, 1


def vocabulary(mcorb, device, k=10, L=3, seed=0):
    """a full k-ary tree of random descriptors in loadFromTextFile order (breadth first), every word with a weight"""
    rng = np.random.default_rng(seed)
    parent, leaf, frontier, nid = [], [], [(0, 0)], 0
    while frontier:
        pid, depth = frontier.pop(0)
        for _ in range(k):
            nid += 1
            parent.append(pid)
            leaf.append(1 if depth + 1 == L else 0)
            if depth + 1 < L:
                frontier.append((nid, depth + 1))
    n = len(parent)
    weight = np.where(np.array(leaf) == 1, rng.uniform(0.1, 9.0, n), 0.0)
    return mcorb.ORBVocabulary(device=device).create(k, L, 0, 0, parent, leaf, rng.integers(0, 256, (n, 32), dtype=np.uint8), weight)


def rot_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def workload(mcorb):
    rng = np.random.default_rng(2)
    twb = np.array([1.0, 0.5, -2.0])
    Rs = [rot_y(2 * math.pi * c / CAMS) for c in range(CAMS)]
    Kc = [[400.0, 0, 640.0], [0, 400.0, 360.0], [0, 0, 1.0]]
    view = mcorb.lmap_view(np.eye(3), -twb, Rs, [np.zeros(3)] * CAMS, [Kc] * CAMS, [twb] * CAMS, W, H)
    pts = np.stack([rng.uniform(-10, 10, MAP), rng.uniform(-2.5, 2.5, MAP), rng.uniform(-10, 10, MAP)], axis=1) + twb
    nrm = pts - twb + rng.normal(0, 4.0, (MAP, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    probe = rng.integers(0, 256, (NPROBE, 32), dtype=np.uint8)
    bits = np.unpackbits(probe[rng.integers(0, NPROBE, MAP)], axis=1)
    for r in bits:
        r[rng.integers(0, 256, int(rng.integers(0, 30)))] ^= 1
    desc = np.packbits(bits, axis=1)
    neigh = np.concatenate([np.where(rng.random(LIDS) < 0.2, -1, rng.integers(0, MAP, LIDS)) for _ in range(KFS)]).astype(np.int32)
    matched = rng.choice(MAP, 300, replace=False).astype(np.int32)
    cur = ((rng.random(NPROBE) < 0.1).astype(np.uint8), (rng.random(NPROBE) < 0.7).astype(np.uint8), rng.integers(0, CAMS, NPROBE).astype(np.int32))
    return view, (np.arange(MAP, dtype=np.int32), pts, nrm, desc, (rng.random(MAP) < 0.7).astype(np.uint8)), probe, neigh, matched, cur


def side(mcorb, device, land, probe):
    voc = vocabulary(mcorb, device)
    db = mcorb.ORBDatabase(voc, device=device, max_entries=1, max_words=4096, max_feats=NPROBE)
    db.reserve_probes(1)
    if device >= 0:
        bow, fv = voc.transform(probe, LEVELSUP)
    else:                                                       # (a host-only vocabulary has no transform: the device side's vectors)
        bow, fv = side.vectors
    side.vectors = (bow, fv)
    db.set_probe(0, bow, fv, probe)
    lm = mcorb.LocalMap(voc, device=device, max_landmarks=MAP, max_candidates=KFS * LIDS)
    lm.set(*land)
    return lm, db


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mcorb
    view, land, probe, neigh, matched, cur = workload(mcorb)
    sides = {"device": side(mcorb, 0, land, probe), "host_only": side(mcorb, -1, land, probe)}
    calls = {k: (lambda lm=lm, db=db: lm.search(view, neigh, matched, db, 0, *cur, levelsup=LEVELSUP)) for k, (lm, db) in sides.items()}
    got = {k: f() for k, f in calls.items()}                       # (also the warm-up)
    fields = ("new_lids", "cam_masks", "ind1", "ind2", "matches")
    same = all(np.array_equal(getattr(got["device"], f), getattr(got["host_only"], f)) for f in fields)
    t, kus = {k: [] for k in calls}, []
    for _ in range(a.reps):                                         # alternating
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "device":
                kus.append(sides["device"][0].last_timing())
    ncand = kus[0][2]
    cull_us, best2_us = float(np.median([u[0] for u in kus])), float(np.median([u[1] for u in kus]))
    alg = ncand * (48 + 4 + 4)
    res = {"cores": len(os.sched_getaffinity(0)), "keyframes": KFS, "lids_per_keyframe": LIDS, "cameras": CAMS, "probe_features": NPROBE,
           "candidates": ncand, "accepted": int(len(got["device"].new_lids)), "ind": int(len(got["device"].ind1)),
           "matches": int(len(got["device"].matches)), "device_equals_host_only": bool(same),
           "k_lmap_cull_us": round(cull_us, 1), "k_lmap_cull_algorithmic_KB": round(alg / 1e3, 1),
           "k_lmap_cull_GBps": round(alg / (cull_us * 1e-6) / 1e9, 2), "k_kfdb_best2_us": round(best2_us, 1)}
    for k in calls:
        res[k + "_call_ms"] = round(float(np.median(t[k])), 3)
        res[k + "_call_ms_min_max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
