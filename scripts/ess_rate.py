"""Rate of the pose of one camera between two frames by five-point RANSAC (mcorb_lmap_essential_pose): the
camera of the tests, 2 000 matches with N(0, 0.1 px) between two frames, 30 % of them moved by 50 px in frame 2.  bench.py times
none of this.

--leg one: one process.  For max_iterations 1 000 (OpenCV's cap, the reference's effective count) and 10 000, medians of --reps
(5) alternating runs after a warm-up:
  ess_device   LocalMap.essential_pose, the device store: the whole call
  ess_host     the same on a host-only store, one thread (--no-host leaves it out)
and the four kernels between HIP events, k_ess_hypotheses' time per hypothesis, k_ess_score's time per Sampson distance (models x
S of them), and whether the stores agree on the bytes -- which is asserted, as is that every process gives the same result.

--leg resources: the compiler's figures for the four kernels (hipcc -Rpass-analysis=kernel-resource-usage), as JSON.
--leg all: --leg one in --procs (3) fresh processes -> profiles/ess_rate.json.
  --resources FILE  a record of --leg resources, copied into the output

    python scripts/ess_rate.py --leg resources > resources.json
    python scripts/ess_rate.py --leg all --resources resources.json --out profiles/ess_rate.json"""
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

FIELDS = ("status", "n_ransac_inliers", "n_inliers", "best_hypothesis", "best_root", "sample", "n_models", "cheirality")


def one_leg(mcorb, a):
    import ess_cases as EC
    import ess_ref as ER
    import kfdb_cases
    truth, matches, moved = EC.scene("general", n=2000, seed=0, moved=0.3, noise=0.1)
    moved = np.array(moved)
    cc = EC.to_cam(mcorb)
    uv1, uv2 = EC.arrays(matches)

    def store(device):
        return mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=64,
                              max_candidates=64)

    stores = {"ess_device": store(0)}
    if not a.no_host:
        stores["ess_host"] = store(-1)
    out = {"cores": len(os.sched_getaffinity(0)), "matches": len(matches), "moved": int(moved.sum()), "threshold_px": 1.0, "runs": {}}
    for H in (1000, 10000):
        t = {k: [] for k in stores}
        kus, res = [], {}
        for rep in range(a.reps + 1):                                  # alternating; the first round is the warm-up
            for k, lm in stores.items():
                t0 = time.perf_counter()
                res[k] = lm.essential_pose(cc, uv1, uv2, 1.0, 50.0, H, 0)
                t[k].append((time.perf_counter() - t0) * 1e3)
                if k == "ess_device":
                    kus.append(lm.last_essential_timing()[0])
            d = res["ess_device"]
            for r in res.values():
                assert r.R.tobytes() == d.R.tobytes() and r.t.tobytes() == d.t.tobytes() and r.E.tobytes() == d.E.tobytes()
                assert r.inliers.tolist() == d.inliers.tolist() and all(getattr(r, f) == getattr(d, f) for f in FIELDS)
        if len(stores) == 2:
            counts = [lm.last_essential_counts() for lm in stores.values()]
            assert all(x.tobytes() == y.tobytes() for x, y in zip(*counts))
        ku = np.median(np.array(kus[1:]), axis=0)
        S = len(matches)
        err = ER.pose_error((d.R, d.t), truth)
        rec = {"hypotheses": H, "matches": S, "n_models": int(d.n_models), "ransac_inliers": int(d.n_ransac_inliers), "inliers": int(d.n_inliers),
               "unmoved": int((~moved).sum()), "unmoved_inliers": int((d.inliers & ~moved).sum()), "moved_inliers": int((d.inliers & moved).sum()),
               "best_hypothesis": int(d.best_hypothesis), "best_root": int(d.best_root), "cheirality": list(d.cheirality),
               "error_R": err[0], "error_t_direction": err[1], "R_bytes": d.R.tobytes().hex(), "stores_equal": len(stores) == 2,
               "k_ess_hypotheses_us": round(float(ku[0]), 1), "k_ess_score_us": round(float(ku[1]), 1), "k_ess_pick_us": round(float(ku[2]), 1),
               "k_ess_finish_us": round(float(ku[3]), 1), "k_ess_hypotheses_ns_per_hypothesis": round(float(ku[0]) * 1e3 / H, 1),
               "sampson_distances": int(d.n_models) * S, "k_ess_score_ns_per_distance": round(float(ku[1]) * 1e3 / (int(d.n_models) * S), 5)}
        for k in stores:
            rec["%s_ms" % k] = round(float(np.median(t[k][1:])), 3)
            rec["%s_ms_runs" % k] = [round(x, 3) for x in t[k][1:]]
        out["runs"][str(H)] = rec
    print(json.dumps(out))


def resources():
    """the compiler's figures per kernel of mcorb_ess_gpu.hip"""
    csrc = os.path.join(ROOT, "mc-slam_amd", "csrc")
    said = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "mcorb_ess_gpu.hip"), "-o", os.devnull],
                          capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in said.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"k_ess_[a-z]+", m.group(2)).group(0)
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
        for H in first["runs"]:
            assert all(p["runs"][H][f] == first["runs"][H][f] for f in ("R_bytes", "inliers", "best_hypothesis", "best_root", "n_models")), H
    if a.resources:
        with open(a.resources) as f:
            out["compiler_resource_usage"] = json.load(f)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
