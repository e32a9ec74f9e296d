"""Rate of the re-triangulation after the back end moved keyframes (mcorb_lmap_retriangulate), on two
cases: section 9o's measured window (8 keyframes of the 4-camera rig at 1280 x 720, 2 000 landmarks, 15 443 observations, every
keyframe moved) and a map-sized case (64 keyframes, 30 000 landmarks at 4 .. 16 views each, 10 on average).  bench.py times
none of this.

--leg one: one process.  Per case, medians of --reps (5) alternating runs after a warm-up:
  device   LocalMap.retriangulate in report mode on a device store, the whole call; the two kernels between its HIP events
           (last_retri_timing) and the bandwidth k_retri_solve's algorithmic bytes make of its span: 16 B per observation plus
           the 15 doubles of its view, read in both passes
  host     the same on a host-only store, one thread
and whether every result of every run equals the restatement (tests/retri_ref.py) bit for bit -- asserted.

--leg all (the default): the scenes and their restatements are made once, then --leg one runs in --procs (3) fresh processes.

    python scripts/retri_rate.py [--out profiles/retri_rate.json]"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cases(small):
    import ba_cases as BC
    import retri_cases as RC
    rng = np.random.default_rng(3)
    window = RC.from_ba(BC.scene(nkf=8, ncams=4, nlm=200 if small else 2000, nfixed=2, seed=7, fx=640.0, cols=1280, rows=720), moved=[True] * 8)
    views = [int(v) for v in rng.integers(4, 17, 300 if small else 30000)]
    out = {"window": window, "map": RC.synth(64, 4, views, seed=4)}
    made = {}
    for name, sc in out.items():
        t0 = time.perf_counter()
        made[name] = (sc, RC.ref(sc, max_diff=float("inf")), time.perf_counter() - t0)
    return made


def one_leg(a):
    import mcorb
    import kfdb_cases
    import pose_cases as PC
    import retri_cases as RC
    with open(a.cases, "rb") as f:
        made = pickle.load(f)
    out = {"cores": len(os.sched_getaffinity(0))}
    for name, (sc, ref, ref_s) in made.items():
        stores = {}
        for k, device in (("device", 0), ("host", -1)):
            stores[k] = mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device,
                                       max_landmarks=len(sc["pts"]), max_candidates=64)
            lids = RC.fill(stores[k], sc)
        kf, cam, olm, uv = RC.arrays(sc["obs"])                       # (the arrays are built once: the call is what is timed)
        args = (PC.to_cams(mcorb, sc["cams"]), np.array([p[0] for p in sc["poses"]]), np.array([p[1] for p in sc["poses"]]),
                np.array(sc["moved"]), lids, kf, cam, olm, uv)
        t = {k: [] for k in stores}
        spans = []
        for rep in range(a.reps + 1):                                 # alternating; the first round is the warm-up
            for k, lm in stores.items():
                t0 = time.perf_counter()
                got = lm.retriangulate(*args, max_diff=float("inf"))
                t[k].append((time.perf_counter() - t0) * 1e3)
                RC.same(got, ref, "%s, %s, run %d" % (name, k, rep))  # asserted: bit for bit
                if k == "device":
                    spans.append(lm.last_retri_timing())
        med = np.median(np.array(spans[1:]), axis=0)
        nobs = len(sc["obs"])
        solve_bytes = nobs * (16 + 2 * 15 * 8)
        r = {"keyframes": len(sc["poses"]), "cameras": len(sc["cams"]), "landmarks": len(sc["pts"]), "observations": nobs,
             "verdict_counts": ref["counts"], "all_results_equal_restatement": True, "restatement_s": round(ref_s, 2),
             "k_retri_views_us": round(float(med[0]), 1), "k_retri_solve_us": round(float(med[1]), 1),
             "k_retri_solve_algorithmic_bytes": solve_bytes, "k_retri_solve_GBps": round(solve_bytes / float(med[1]) / 1e3, 1)}
        for k in stores:
            r["%s_ms" % k] = round(float(np.median(t[k][1:])), 3)
            r["%s_ms_runs" % k] = [round(x, 3) for x in t[k][1:]]
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a tenth of the sizes: a quick check of the script itself")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default="all", choices=["one", "all"])
    ap.add_argument("--cases", default=None, help="(--leg one) the pickled scenes and restatements")
    a = ap.parse_args()
    if a.leg == "one":
        one_leg(a)
        sys.exit(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.pkl")
        with open(path, "wb") as f:
            pickle.dump(cases(a.small), f)
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", "one", "--reps", str(a.reps), "--cases", path]
        runs = [json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=400).stdout.strip().splitlines()[-1])
                for _ in range(a.procs)]
    out = {"processes": runs}
    for name in ("window", "map"):
        out[name] = {k: [r[name][k] for r in runs] for k in ("device_ms", "host_ms", "k_retri_views_us", "k_retri_solve_us", "k_retri_solve_GBps")}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
