"""Rate of the local bundle adjustment (mcorb_lmap_bundle_adjust): a window of 8 keyframes, 2 of them
fixed, of section 9f's rig (4 cameras at 1280 x 720), about 2 000 landmarks, the free poses off by 0.02 rad and 0.1 m and the
points by 0.1 m (tests/ba_cases.py's seeded scene at this size).  bench.py times none of this.

--leg one: one process.  Medians of --reps (5) alternating runs after a warm-up:
  device   LocalMap.bundle_adjust on a device store, the whole call; the spans between its HIP events (last_ba_timing), the
           solves taken and the launches queued behind the loop's end
  host     the same on a host-only store, one thread
and whether every result of every run equals the restatement (tests/ba_ref.py) bit for bit -- asserted.

--leg all (the default): --leg one in --procs (3) fresh processes.

    python scripts/ba_rate.py [--out profiles/ba_rate.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPANS = ["begin_linearize_cost", "k_ba_schur", "k_ba_solve", "k_ba_update", "k_ba_accept", "later_iterations", "final_pass"]


def one_leg(a):
    import mcorb
    import ba_cases as BC
    import kfdb_cases
    sc = BC.scene(nkf=8, ncams=4, nlm=a.landmarks, nfixed=2, seed=7, fx=640.0, cols=1280, rows=720)
    stores = {}
    for name, device in (("device", 0), ("host", -1)):
        stores[name] = mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device,
                                      max_landmarks=len(sc["pts"]), max_candidates=1024)
    t0 = time.perf_counter()
    ref = BC.ref(sc)
    ref_s = time.perf_counter() - t0
    t = {k: [] for k in stores}
    spans, idle = [], 0
    import pose_cases as PC
    kf, cam, olm, uv, octave = BC.arrays(sc["obs"])                    # (the arrays are built once: the call is what is timed)
    args = (PC.to_cams(mcorb, sc["cams"]), np.array([p[0] for p in sc["poses"]]), np.array([p[1] for p in sc["poses"]]),
            np.array(sc["fixed"]), kf, cam, olm, uv, octave, sc["sigma"])
    pts = np.array(sc["pts"], np.float64)
    for rep in range(a.reps + 1):                                      # alternating; the first round is the warm-up
        for k, lm in stores.items():
            t0 = time.perf_counter()
            got = lm.bundle_adjust(*args, pts=pts)
            t[k].append((time.perf_counter() - t0) * 1e3)
            BC.same(BC.as_ref(got), ref, "%s, run %d" % (k, rep))      # asserted: bit for bit
            if k == "device":
                us, idle = lm.last_ba_timing()
                spans.append(us)
    views = len(set((o[2], o[0]) for o in sc["obs"] if not sc["fixed"][o[0]]))
    out = {"cores": len(os.sched_getaffinity(0)), "keyframes": 8, "fixed": 2, "cameras": 4, "image": [1280, 720],
           "landmarks": len(sc["pts"]), "observations": len(sc["obs"]), "views": views, "status": BC.NAMES[ref["status"]],
           "solves": ref["iterations"], "max_iterations": 25, "cost_initial": ref["cost_initial"], "cost_final": ref["cost_final"],
           "launches_queued_behind_done": idle, "all_results_equal_restatement": True, "restatement_s": round(ref_s, 2)}
    for k in stores:
        out["%s_ms" % k] = round(float(np.median(t[k][1:])), 3)
        out["%s_ms_runs" % k] = [round(x, 3) for x in t[k][1:]]
    med = np.median(np.array(spans[1:]), axis=0)
    out["spans_us"] = {n: round(float(v), 1) for n, v in zip(SPANS, med)}
    out["spans_us_total"] = round(float(med.sum()), 1)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--landmarks", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default="all", choices=["one", "all"])
    a = ap.parse_args()
    if a.leg == "one":
        one_leg(a)
        sys.exit(0)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "one", "--reps", str(a.reps), "--landmarks", str(a.landmarks)]
    runs = [json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=400).stdout.strip().splitlines()[-1])
            for _ in range(a.procs)]
    out = {"processes": runs, "device_ms_medians": [r["device_ms"] for r in runs], "host_ms_medians": [r["host_ms"] for r in runs]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
