"""Rate of the rig pose between two frames from 3D-3D pairs (mcorb_lmap_align_pose): 2 000 pairs with N(0,
0.02 m) per axis, 30 % of them moved by 1 m, at the reference's thresholds (0.2 and 0.1).  bench.py times none of this.

--leg one: one process.  For mode 1 at 100 hypotheses (the reference's value) and at 10 000, and for mode 0, medians of --reps (5)
alternating runs after a warm-up:
  align_device   LocalMap.align_pose, the device store: the whole call
  align_host     the same on a host-only store, one thread (--no-host leaves it out)
and the four kernels between HIP events, k_align_score's time per distance (models x n of them) and its grid, the part of the
device call that k_align_fit's single workgroup is, and whether the stores agree bit for bit -- which is asserted, as is that
every process gives the same result.

--leg resources: the compiler's figures for the four kernels (hipcc -Rpass-analysis=kernel-resource-usage), as JSON.
--leg all: --leg one in --procs (3) fresh processes -> profiles/align_rate.json.  --resources FILE: a record of --leg resources,
copied into the output.

    python scripts/align_rate.py --leg resources > resources.json
    python scripts/align_rate.py --leg all --resources resources.json --out profiles/align_rate.json"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE, HYP_BLOCK = 256, 32      # k_align_score's grid: (tiles of pairs, blocks of hypotheses)
CASES = (("sac_100", dict(mode="sac", max_iterations=100)), ("sac_10000", dict(mode="sac", max_iterations=10000)), ("all", dict(mode="all")))


def one_leg(mcorb, a):
    import align_cases as AC
    import kfdb_cases
    truth, p1, p2, moved = AC.scene(n=2000, seed=0, moved=600)
    moved = np.array(moved)

    def store(device):
        return mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=64,
                              max_candidates=64)

    stores = {"align_device": store(0)}
    if not a.no_host:
        stores["align_host"] = store(-1)
    n = len(p1)
    out = {"cores": len(os.sched_getaffinity(0)), "pairs": n, "moved": int(moved.sum()), "threshold": AC.THRESHOLD,
           "inlier_dist": AC.INLIER_DIST, "grid": {"tile": TILE, "hypothesis_block": HYP_BLOCK}, "runs": {}}
    for name, kw in CASES:
        t = {k: [] for k in stores}
        kus, res = [], {}
        for rep in range(a.reps + 1):                                  # alternating; the first round is the warm-up
            for k, lm in stores.items():
                t0 = time.perf_counter()
                res[k] = lm.align_pose(p2, pts1=p1, threshold=AC.THRESHOLD, inlier_dist=AC.INLIER_DIST, **kw)
                t[k].append((time.perf_counter() - t0) * 1e3)
                if k == "align_device":
                    kus.append(lm.last_align_timing()[0])
            d = res["align_device"]
            for r in res.values():
                AC.same_results(r, d, name)
        sac = kw["mode"] == "sac"
        if sac and len(stores) == 2:
            counts = [lm.last_align_counts() for lm in stores.values()]
            assert counts[0][0].tolist() == counts[1][0].tolist() and counts[0][1].tolist() == counts[1][1].tolist()
        ku = np.median(np.array(kus[1:]), axis=0)
        if not sac:
            ku[:3] = 0.0                                               # (mode 0 launches k_align_fit alone; the others are the last case's)
        err = AC.pose_error((d.R.tolist(), d.t.tolist()), truth)
        dev_ms = float(np.median(t["align_device"][1:]))
        rec = {"mode": kw["mode"], "hypotheses": kw.get("max_iterations", 0), "pairs": n, "n_models": int(d.n_models), "used": int(d.used),
               "inliers": int(d.n_inliers), "sac_inliers": int(d.sac_n_inliers), "unmoved": int((~moved).sum()),
               "unmoved_inliers": int((d.inliers & ~moved).sum()), "moved_inliers": int((d.inliers & moved).sum()),
               "best_hypothesis": int(d.best_hypothesis), "mean_error": d.mean_error, "error_R": err[0], "error_t_m": err[1],
               "R_bytes": d.R.tobytes().hex(), "stores_equal": len(stores) == 2,
               "k_align_hypotheses_us": round(float(ku[0]), 1), "k_align_score_us": round(float(ku[1]), 1),
               "k_align_pick_us": round(float(ku[2]), 1), "k_align_fit_us": round(float(ku[3]), 1),
               "k_align_fit_part_of_device_call": round(float(ku[3]) * 1e-3 / dev_ms, 4)}
        if sac:
            H = kw["max_iterations"]
            rec["k_align_score_grid"] = [(n + TILE - 1) // TILE, (H + HYP_BLOCK - 1) // HYP_BLOCK]
            rec["distances"] = int(d.n_models) * n
            rec["k_align_score_ns_per_distance"] = round(float(ku[1]) * 1e3 / max(1, int(d.n_models) * n), 5)
        for k in stores:
            rec["%s_ms" % k] = round(float(np.median(t[k][1:])), 3)
            rec["%s_ms_runs" % k] = [round(x, 3) for x in t[k][1:]]
        out["runs"][name] = rec
    print(json.dumps(out))


def resources():
    """the compiler's figures per kernel of mcorb_align_gpu.hip"""
    csrc = os.path.join(ROOT, "mc-slam_amd", "csrc")
    said = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "mcorb_align_gpu.hip"), "-o", os.devnull],
                          capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in said.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"k_align_[a-z]+", m.group(2)).group(0)
            out[name] = {}
        else:
            out[name][m.group(1)] = int(m.group(2))
    return out


def child(a):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "one", "--reps", str(a.reps)] + (["--no-host"] if a.no_host else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=400).stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--leg", default="one", choices=["one", "all", "resources"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="leave the host-only store out")
    ap.add_argument("--resources", default=None, help="--leg all: a record of --leg resources")
    a = ap.parse_args()
    if a.leg == "resources":
        print(json.dumps(resources(), indent=1))
        sys.exit(0)
    if a.leg == "one":
        import mcorb
        one_leg(mcorb, a)
        sys.exit(0)
    out = {"processes": [child(a) for _ in range(a.procs)]}
    first = out["processes"][0]
    for p in out["processes"]:      # every process computes the same
        for name in first["runs"]:
            assert all(p["runs"][name][f] == first["runs"][name][f] for f in ("R_bytes", "inliers", "best_hypothesis", "n_models")), name
    if a.resources:
        with open(a.resources) as f:
            out["compiler_resource_usage"] = json.load(f)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
