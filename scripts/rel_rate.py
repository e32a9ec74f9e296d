"""Rate of the relative rig pose between two frames by RANSAC (mcorb_lmap_relative_pose): the 8-camera
outward-facing rig of the tests, 2 000 matches with N(0, 0.1 px) between two frames, 30 % of them moved by 50 px in frame 2.
bench.py times none of this.

--leg one: one process.  For max_iterations 2 000 (LoopCloser::checkEssentialMatrix) and 10 000 (poseFromSeventeenPt), medians of
--reps (5) alternating runs after a warm-up:
  rel_device   LocalMap.relative_pose, the device store: the whole call
  rel_host     the same on a host-only store, one thread (--no-host leaves it out)
and the three kernels between HIP events, k_rel_score's time per two-view triangulation (models x S of them) and its grid, and
whether the stores agree bit for bit -- which is asserted, as is that every process gives the same result.

--leg resources: the compiler's figures for the three kernels (hipcc -Rpass-analysis=kernel-resource-usage), as JSON.
--leg all: --leg one in --procs (3) fresh processes -> profiles/rel_rate.json.
  --alt NAME=DIR    (repeatable) a copy of the package beside a library built with another k_rel_score block size
                    (make EXTRA=-DMCORB_REL_HYP_BLOCK=..), alternating with this one's, --procs processes each, device store only:
                    the block-size table
  --resources FILE  a record of --leg resources, copied into the output
--tree DIR (--leg one): DIR's package and library are timed instead of this checkout's.

    python scripts/rel_rate.py --leg resources > resources.json
    python scripts/rel_rate.py --leg all --alt block8=DIR8 --alt block128=DIR128 --resources resources.json --out profiles/rel_rate.json"""
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

TILE = 256      # k_rel_score's tile of matches


def one_leg(mcorb, a):
    import kfdb_cases
    import pose_cases as PC
    import rel_cases as RC
    cams, truth, matches, moved = RC.scene(8, 2000, 0, moved=0.3)
    moved = np.array(moved)
    cc = PC.to_cams(mcorb, cams)
    cam1, uv1, cam2, uv2 = RC.arrays(matches)
    thr = mcorb.rel_threshold(RC.K02)

    def store(device):
        return mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=64,
                              max_candidates=64)

    stores = {"rel_device": store(0)}
    if not a.no_host:
        stores["rel_host"] = store(-1)
    out = {"cores": len(os.sched_getaffinity(0)), "matches": len(matches), "moved": int(moved.sum()), "threshold": thr,
           "grid": {"tile": TILE, "hypothesis_block": a.hyp_block}, "runs": {}}
    for H in (2000, 10000):
        t = {k: [] for k in stores}
        kus, res = [], {}
        for rep in range(a.reps + 1):                                  # alternating; the first round is the warm-up
            for k, lm in stores.items():
                t0 = time.perf_counter()
                res[k] = lm.relative_pose(cc, cam1, uv1, cam2, uv2, thr, max_iterations=H)
                t[k].append((time.perf_counter() - t0) * 1e3)
                if k == "rel_device":
                    kus.append(lm.last_relative_timing()[0])
            d = res["rel_device"]
            for r in res.values():
                assert r.R.tobytes() == d.R.tobytes() and r.t.tobytes() == d.t.tobytes() and r.inliers.tolist() == d.inliers.tolist()
                assert (r.status, r.best_hypothesis, r.sample, r.n_inliers, r.n_models) == (d.status, d.best_hypothesis, d.sample, d.n_inliers,
                                                                                        d.n_models)
        if len(stores) == 2:
            counts = [lm.last_relative_counts() for lm in stores.values()]
            assert counts[0][0].tolist() == counts[1][0].tolist() and counts[0][1].tolist() == counts[1][1].tolist()
        ku = np.median(np.array(kus[1:]), axis=0)
        S = len(matches)
        err = RC.pose_error((d.R.tolist(), d.t.tolist()), truth)
        rec = {"hypotheses": H, "matches": S, "n_models": int(d.n_models), "inliers": int(d.n_inliers), "unmoved": int((~moved).sum()),
               "unmoved_inliers": int((d.inliers & ~moved).sum()), "moved_inliers": int((d.inliers & moved).sum()),
               "best_hypothesis": int(d.best_hypothesis), "error_R": err[0], "error_t_m": err[1], "R_bytes": d.R.tobytes().hex(),
               "stores_equal": len(stores) == 2,
               "k_rel_hypotheses_us": round(float(ku[0]), 1), "k_rel_score_us": round(float(ku[1]), 1), "k_rel_pick_us": round(float(ku[2]), 1),
               "k_rel_score_grid": [(S + TILE - 1) // TILE, (H + a.hyp_block - 1) // a.hyp_block],
               "triangulations": int(d.n_models) * S, "k_rel_score_ns_per_triangulation": round(float(ku[1]) * 1e3 / (int(d.n_models) * S), 5)}
        for k in stores:
            rec["%s_ms" % k] = round(float(np.median(t[k][1:])), 3)
            rec["%s_ms_runs" % k] = [round(x, 3) for x in t[k][1:]]
        out["runs"][str(H)] = rec
    print(json.dumps(out))


def resources():
    """the compiler's figures per kernel of mcorb_rel_gpu.hip"""
    csrc = os.path.join(ROOT, "mc-slam_amd", "csrc")
    said = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "mcorb_rel_gpu.hip"), "-o", os.devnull],
                          capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in said.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"k_rel_[a-z]+", m.group(2)).group(0)
            out[name] = {}
        else:
            out[name][m.group(1)] = int(m.group(2))
    return out


def child(a, tree=None, hyp_block=None, no_host=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "one", "--reps", str(a.reps), "--hyp-block", str(hyp_block or a.hyp_block)]
    cmd += (["--tree", tree] if tree else []) + (["--no-host"] if no_host or a.no_host else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=400).stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--leg", default="one", choices=["one", "all", "resources"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="leave the host-only store out")
    ap.add_argument("--tree", default=None, help="--leg one: a directory whose package and library are timed instead of this checkout's")
    ap.add_argument("--alt", action="append", default=[], help="--leg all: NAME=DIR or NAME=DIR:BLOCK, a library built with another block size")
    ap.add_argument("--hyp-block", type=int, default=32, help="the library's MCORB_REL_HYP_BLOCK, when it was built with another")
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
    out = {"processes": [child(a) for _ in range(a.procs)]}
    first = out["processes"][0]
    for p in out["processes"]:      # every process computes the same
        for H in first["runs"]:
            assert all(p["runs"][H][f] == first["runs"][H][f] for f in ("R_bytes", "inliers", "best_hypothesis", "n_models")), H
    for alt in a.alt:
        name, tree = alt.split("=", 1)
        tree, _, block = tree.partition(":")
        pairs = [{"alternate": child(a, tree, int(block or a.hyp_block), True), "this": child(a, None, None, True)} for _ in range(a.procs)]
        for p in pairs:
            for H in first["runs"]:
                assert p["alternate"]["runs"][H]["R_bytes"] == p["this"]["runs"][H]["R_bytes"] == first["runs"][H]["R_bytes"], (name, H)
        out.setdefault("alternates", {})[name] = pairs
    if a.resources:
        with open(a.resources) as f:
            out["compiler_resource_usage"] = json.load(f)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
