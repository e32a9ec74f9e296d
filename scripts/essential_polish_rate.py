"""Rate of the polished essential pose (mcorb_lmap_essential_pose_polished) on section 9m's frame: the camera
of the tests, 2 000 matches with N(0, 0.1 px) between two frames, 30 % of them moved by 50 px in frame 2.  bench.py times none of
this.

--leg one: one process, the device store.  For max_iterations 1 000 and 10 000, medians of --reps (5) alternating runs after a
warm-up:
  ess_ms        LocalMap.essential_pose: the whole call
  polished_ms   LocalMap.essential_pose_polished (rounds 2, polish_iterations 10): the whole call
the five kernels between HIP events (k_ess_fit among them), the solves, statuses, members and counts per round, the distance to
the true pose before and after, and whether a host-only store gives the polished call's bytes (asserted; --no-host leaves it out).
A tree without the polished call (--tree PARENT) is timed on essential_pose alone.

--leg resources: the compiler's figures for the kernels of mcorb_ess_gpu.hip (hipcc -Rpass-analysis=kernel-resource-usage).
--leg all: --leg one in --procs (3) fresh processes; with --parent DIR (the parent commit's tree with its library built) the
  processes alternate with the parent's and section 9i's guard is worked out for essential_pose's whole call: this commit's medians
  against the parent's slowest run plus the parent's spread of medians.  --resources FILE: a record of --leg resources, copied in.

    python scripts/essential_polish_rate.py --leg resources > resources.json
    python scripts/essential_polish_rate.py --leg all --parent PARENT --resources resources.json --out profiles/essential_polish_rate.json"""
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


def one_leg(mcorb, a):
    import ess_cases as EC
    import ess_ref as ER
    import kfdb_cases
    truth, matches, moved = EC.scene("general", n=2000, seed=0, moved=0.3, noise=0.1)
    cc = EC.to_cam(mcorb)
    uv1, uv2 = EC.arrays(matches)
    polished = hasattr(mcorb.LocalMap, "essential_pose_polished")

    def store(device):
        return mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=64,
                              max_candidates=64)

    def dist(r):
        return list(ER.pose_error((r.R, r.t), truth))

    lm = store(0)
    host = store(-1) if polished and not a.no_host else None
    out = {"cores": len(os.sched_getaffinity(0)), "matches": len(matches), "polished": polished, "runs": {}}
    for H in (1000, 10000):
        t = {"ess": [], "polished": []}
        kus, fit_us = [], []
        for rep in range(a.reps + 1):                                  # alternating; the first round is the warm-up
            t0 = time.perf_counter()
            plain = lm.essential_pose(cc, uv1, uv2, 1.0, 50.0, H, 0)
            t["ess"].append((time.perf_counter() - t0) * 1e3)
            kus.append(lm.last_essential_timing()[0])
            if polished:
                t0 = time.perf_counter()
                got, pol = lm.essential_pose_polished(cc, uv1, uv2, 1.0, 50.0, H, 0, rounds=2, polish_iterations=10)
                t["polished"].append((time.perf_counter() - t0) * 1e3)
                fit_us.append(lm.last_essential_timing5()[0][4])
        ku = np.median(np.array(kus[1:]), axis=0)
        rec = {"hypotheses": H, "ransac_inliers": int(plain.n_ransac_inliers), "inliers": int(plain.n_inliers), "distance": dist(plain),
               "R_bytes": plain.R.tobytes().hex(), "k_ess_hypotheses_us": round(float(ku[0]), 1), "k_ess_score_us": round(float(ku[1]), 1),
               "k_ess_pick_us": round(float(ku[2]), 1), "k_ess_finish_us": round(float(ku[3]), 1),
               "ess_ms": round(float(np.median(t["ess"][1:])), 3), "ess_ms_runs": [round(x, 3) for x in t["ess"][1:]]}
        if polished:
            assert pol.R.tobytes() == plain.R.tobytes() and pol.t.tobytes() == plain.t.tobytes() and pol.n_inliers == plain.n_inliers
            rec.update(polished_ms=round(float(np.median(t["polished"][1:])), 3), polished_ms_runs=[round(x, 3) for x in t["polished"][1:]],
                       k_ess_fit_us=round(float(np.median(fit_us[1:])), 1), k_ess_fit_us_runs=[round(float(x), 1) for x in fit_us[1:]],
                       polished_ransac_inliers=int(got.n_ransac_inliers), polished_inliers=int(got.n_inliers), polished_distance=dist(got),
                       polished_R_bytes=got.R.tobytes().hex(), rounds=pol.rounds, stores_equal=host is not None)
            if host is not None:
                g2, p2 = host.essential_pose_polished(cc, uv1, uv2, 1.0, 50.0, H, 0, rounds=2, polish_iterations=10)
                assert g2.R.tobytes() == got.R.tobytes() and g2.t.tobytes() == got.t.tobytes() and g2.E.tobytes() == got.E.tobytes()
                assert g2.inliers.tolist() == got.inliers.tolist() and p2.rounds == pol.rounds
                assert (g2.n_inliers, g2.n_ransac_inliers) == (got.n_inliers, got.n_ransac_inliers)
        out["runs"][str(H)] = rec
    print(json.dumps(out))


def resources():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ess_rate
    return ess_rate.resources()


def child(a, tree=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "one", "--reps", str(a.reps)]
    cmd += (["--tree", tree] if tree else []) + (["--no-host"] if a.no_host else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=400).stdout.strip().splitlines()[-1])


def guard(pairs):
    """section 9i's rule on essential_pose's whole call, per hypothesis count"""
    out = {}
    for H in pairs[0]["this"]["runs"]:
        mine = [p["this"]["runs"][H]["ess_ms"] for p in pairs]
        theirs = [p["parent"]["runs"][H]["ess_ms"] for p in pairs]
        slowest = max(x for p in pairs for x in p["parent"]["runs"][H]["ess_ms_runs"])
        limit = slowest + (max(theirs) - min(theirs))
        out[H] = {"this_medians_ms": mine, "parent_medians_ms": theirs, "parent_slowest_run_ms": slowest, "limit_ms": round(limit, 3),
                  "met": max(mine) <= limit}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--leg", default="one", choices=["one", "all", "resources"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="leave the host-only store out")
    ap.add_argument("--tree", default=None, help="--leg one: a directory whose package and library are timed instead of this checkout's")
    ap.add_argument("--parent", default=None, help="--leg all: the parent commit's tree, its library built")
    ap.add_argument("--resources", default=None, help="--leg all: a record of --leg resources")
    a = ap.parse_args()
    if a.leg == "resources":
        print(json.dumps(resources(), indent=1))
        sys.exit(0)
    if a.leg == "one":
        if a.tree:
            sys.path.insert(0, os.path.abspath(a.tree))
        import mcorb
        one_leg(mcorb, a)
        sys.exit(0)
    if a.parent:
        pairs = [{"parent": child(a, a.parent), "this": child(a)} for _ in range(a.procs)]
        out = {"pairs": pairs, "guard": guard(pairs)}
        procs = [p["this"] for p in pairs]
        for p in pairs:      # the unpolished call computes what the parent's does
            for H in p["this"]["runs"]:
                assert p["this"]["runs"][H]["R_bytes"] == p["parent"]["runs"][H]["R_bytes"], H
    else:
        procs = [child(a) for _ in range(a.procs)]
        out = {"processes": procs}
    for p in procs:          # every process computes the same
        for H in procs[0]["runs"]:
            assert all(p["runs"][H][f] == procs[0]["runs"][H][f] for f in ("R_bytes", "polished_R_bytes", "rounds")), H
    if a.resources:
        with open(a.resources) as f:
            out["compiler_resource_usage"] = json.load(f)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
