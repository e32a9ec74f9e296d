"""What one mapping step costs (mcorb_lmap_triangulate_neighbours: FrontEnd::triangulateNeighbors with triangulateMatches and
getSceneDepthStats), on the same machine and inputs: 10 neighbouring keyframes of 500 unassigned inter-frame matches each on a rig
of 4 cameras, half of the matches with 2 views in total, the rest with 3 to 6; every neighbour also has 300 landmarks of the store
(the baseline gate's depths).  The scene is the tests' generator (tests/mapping_cases.py) with consistent observations, so most
matches run the whole path and become landmarks.
  device     the whole call on a device store, and k_map_triangulate (both instances) / k_map_depth between HIP events;
  host only  the same call on the host-only store.
The two are timed in alternating runs, `reps` each; medians are reported.  bench.py times none of this.
    python scripts/mapping_rate.py [--reps 5] [--out profiles/mapping_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KFS, MATCHES, CAMS, OLD, MAXLM = 10, 500, 4, 300, 1 << 15


def workload():
    import mapping_cases as Mc
    rng = np.random.default_rng(6)
    Ks, rigT = Mc.make_rig(CAMS, rng)
    cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(0.01, 0.02, -0.01), np.zeros(3)), rigT), Ks)
    shapes = [(1, 1)] * 5 + [(2, 1), (2, 2), (3, 2), (3, 3), (1, 3)]     # half 2 views, the rest 3 .. 6
    neigh, matches, F21, store = [], [], [], {}
    for s in range(KFS):
        g = Mc.frame_geometry(Mc.T4(Mc.rot(*rng.uniform(-0.05, 0.05, 3)), np.array([(-1.0) ** s * (0.8 + 0.1 * s), 0.05 * s, 0.0])), rigT)
        fb = Mc.FrameBuilder(g, Ks)
        mid = 0.5 * g["twc"]
        ms = []
        for i in range(MATCHES):
            a, b = shapes[i % len(shapes)]
            X = mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 15)])
            ms.append((fb.add(X, sorted(rng.choice(CAMS, a, replace=False).tolist()), rng),
                       cur.add(X, sorted(rng.choice(CAMS, b, replace=False).tolist()), rng)))
        for i in range(OLD):
            lid = 20000 + s * OLD + i
            store[lid] = g["twc"] + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 8)])
            fb.add(store[lid], [int(rng.integers(0, CAMS))], rng, lid=lid)
        neigh.append(fb.done())
        matches.append(np.array(ms, np.int32))
        F21.append(np.array([[Mc.fundamental(cur.g["full"][cc], g["full"][cn], Ks[cc], Ks[cn]) for cn in range(CAMS)] for cc in range(CAMS)]))
    Tcw = np.linalg.inv(cur.g["pose"])
    return dict(K=np.array(Ks), inv_sigma2=Mc.INV_SIGMA2, cur=cur.done(), neigh=neigh, matches=matches, F21=F21, store=store,
                Rcw=Tcw[:3, :3].copy(), tcw=Tcw[:3, 3].copy(), next_lid=0)


def side(mcorb, device, sc):
    import kfdb_cases
    import mapping_cases as Mc
    lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=MAXLM, max_candidates=16)
    Mc.fill_store(lm, sc["store"])
    args = (Mc.to_frame(mcorb, sc["cur"]), sc["cur"]["lids"], [Mc.to_frame(mcorb, f) for f in sc["neigh"]], [f["lids"] for f in sc["neigh"]],
            sc["F21"], sc["matches"], sc["K"], sc["inv_sigma2"], sc["Rcw"], sc["tcw"], sc["next_lid"])
    return lm, (lambda: lm.triangulate_neighbours(*args))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mcorb
    sc = workload()
    sides = {"device": side(mcorb, 0, sc), "host_only": side(mcorb, -1, sc)}
    got = {k: f() for k, (_, f) in sides.items()}                   # (also the warm-up)
    fields = ("verdict", "new_lid", "pt3d", "normal", "depth_vec", "lids_cur")
    same = all(np.asarray(getattr(got["device"], f)).tobytes() == np.asarray(getattr(got["host_only"], f)).tobytes() for f in fields)
    t, kus = {k: [] for k in sides}, []
    for _ in range(a.reps):                                         # alternating
        for k, (lm, f) in sides.items():
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "device":
                kus.append(lm.last_triangulate_timing())
    nviews = [int((sc["neigh"][s]["match_index"][q] != -1).sum() + (sc["cur"]["match_index"][tt] != -1).sum())
              for s in range(KFS) for q, tt in sc["matches"][s]]
    res = {"cores": len(os.sched_getaffinity(0)), "keyframes": KFS, "matches_per_keyframe": MATCHES, "cameras": CAMS,
           "matches_2_views": int(sum(v == 2 for v in nviews)), "matches_3_to_6_views": int(sum(v > 2 for v in nviews)),
           "launched": kus[0][2], "depths": kus[0][3], "landmarks_made": int(got["device"].n_triangulated),
           "device_equals_host_only": bool(same),
           "k_map_triangulate_us": round(float(np.median([u[0] for u in kus])), 1),
           "k_map_depth_us": round(float(np.median([u[1] for u in kus])), 1)}
    for k in sides:
        res[k + "_call_ms"] = round(float(np.median(t[k])), 3)
        res[k + "_call_ms_min_max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
