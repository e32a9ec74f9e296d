"""Rate of the absolute rig pose by RANSAC (mcorb_lmap_ransac_pose) on section 9g's frame: 4 cameras at
1280 x 720, an extraction job on the synthetic rig frame, landmarks back-projected from the keypoints, about 5 000 de-duplicated
matches -- with 30 % of the observations moved by 50 px in a random direction.  No predicted pose is given to the call.  bench.py
times none of this.

--leg one: one process.  For max_iterations 100 and 1 024, medians of --reps (5) alternating runs after a warm-up:
  sac_device         LocalMap.ransac_pose, the device store: the whole call
  sac_host           the same on a host-only store, one thread
  sac_refine_device  the call with refine= (k_pose_refine behind k_sac_pick in the same submission)
  sac_then_refine    ransac_pose followed by an explicit refine_pose from its pose, the device store
and the three kernels between HIP events, k_sac_score's time per reprojection (H x S of them) and its grid, and whether the
stores agree bit for bit.

--leg all: --leg one in --procs (3) fresh processes -> profiles/sac_rate.json.  --guard FILE: a record of
`pose_rate.py --leg ab --tree PARENT`, from which the one guard is computed: refine_pose's whole call (refine_device) on this
commit's library must not exceed the parent's slowest run by more than the parent's spread of medians.

--solver rig: every leg with solver="rig" (k_sac_hypotheses_rig in k_sac_hypotheses' place) -> profiles/sac_rate_rig.json.
--tree DIR (--leg one): DIR's package and library are timed instead of this checkout's -- a checkout of another commit, or a copy
of the package beside a library built with other switches.  With --leg all:
  --parent DIR      the parent commit's checkout: its library and this one's alternate, --procs processes each, with the
                    central solver; the guard is that ransac_pose's whole call on the device store (sac_device) on this commit's
                    library must not exceed the parent's slowest run by more than the parent's spread of medians
  --alt NAME=DIR    (repeatable) a library built with other switches -- MCORB_SAC_RIG_ONE_LANE, MCORB_SAC_RIG_NEWTON=8 --
                    alternating with this one's, --procs processes each, with --solver

    python scripts/sac_rate.py --leg all [--guard profiles/pose_rate_ab.json] [--out profiles/sac_rate.json]
    python scripts/sac_rate.py --leg all --solver rig --parent PARENT [--alt one_lane=DIR] --out profiles/sac_rate_rig.json"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

INV_SIGMA2 = [1.0 / 1.2 ** (2 * l) for l in range(8)]
TILE, HYP_BLOCK = 256, 8      # k_sac_score's grid: (tiles of consensus observations, blocks of hypotheses)


def frame(mcorb):
    """-> (view, stores, cam, uv, octave, lids): section 9g's matches, 30 % of them moved"""
    import kfdb_cases
    import track_cases as T
    import track_rate as TR
    rig = mcorb.Rig(TR.CAMS, TR.COLS, TR.ROWS, 1, 1, nfeatures=TR.KEYPOINTS)
    rig.upload([mcorb.synth_rig_frame(0, TR.CAMS, c, TR.COLS, TR.ROWS) for c in range(TR.CAMS)])
    rig.extract(TR.CAMS)
    v, pts, desc, lids = TR.slot_workload(mcorb, rig)
    view = T.to_view(mcorb, v)

    def store(device):
        lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=len(pts),
                            max_candidates=len(pts))
        lm.set(np.arange(len(pts), dtype=np.int32), pts, np.zeros_like(pts), desc)
        return lm

    lm, lm_host = store(0), store(-1)
    xy, ds = TR.readback(rig)
    r = lm.track_rig_frame(view, rig, 0, lids)
    cam = np.concatenate([np.full(len(r.match_kp[c]), c, np.int32) for c in range(TR.CAMS)])
    uv = np.concatenate([xy[c][r.match_kp[c]].reshape(-1, 2) for c in range(TR.CAMS)]).astype(np.float32)
    mlids = np.concatenate(r.match_lid).astype(np.int32)
    rng = np.random.default_rng(1)
    moved = rng.random(len(cam)) < 0.3
    ang = rng.uniform(0, 2 * math.pi, len(cam))
    uv[moved] += (50 * np.stack([np.cos(ang), np.sin(ang)], 1)[moved]).astype(np.float32)
    K02 = float(v["cams"][0]["u0"])
    return view, lm, lm_host, cam, uv, np.zeros(len(cam), np.int32), mlids, moved, mcorb.sac_threshold(K02)


def one_leg(mcorb, a):
    view, lm, lm_host, cam, uv, octave, lids, moved, thr = frame(mcorb)
    refine = mcorb.pose_params(INV_SIGMA2)
    kw = {} if a.solver == "central" else {"solver": a.solver}      # (a checkout from before the solvers has no such argument)
    out = {"solver": a.solver, "cores": len(os.sched_getaffinity(0)), "matches": int(len(cam)), "moved": int(moved.sum()), "threshold": thr,
           "grid": {"tile": TILE, "hypothesis_block": HYP_BLOCK}, "runs": {}}
    for H in (100, 1024):
        legs = ["sac_device", "sac_host", "sac_refine_device", "sac_then_refine"]
        t = {k: [] for k in legs}
        kus, res, same = [], {}, True
        for rep in range(a.reps + 1):                                  # alternating; the first round is the warm-up
            for k in legs:
                t0 = time.perf_counter()
                if k == "sac_device":
                    res[k] = lm.ransac_pose(view, cam, uv, octave, thr, lids=lids, max_iterations=H, **kw)
                elif k == "sac_host":
                    res[k] = lm_host.ransac_pose(view, cam, uv, octave, thr, lids=lids, max_iterations=H, **kw)
                elif k == "sac_refine_device":
                    res[k] = lm.ransac_pose(view, cam, uv, octave, thr, lids=lids, max_iterations=H, refine=refine, **kw)
                else:
                    s = lm.ransac_pose(view, cam, uv, octave, thr, lids=lids, max_iterations=H, **kw)
                    res[k] = lm.refine_pose(view, s.sac_R, s.sac_t, cam, uv, octave, INV_SIGMA2, lids=lids)
                t[k].append((time.perf_counter() - t0) * 1e3)
                if k == "sac_device":
                    kus.append(lm.last_ransac_timing()[0])
            d, h, r, e = (res[k] for k in legs)
            same = same and all(getattr(d, f).tobytes() == getattr(h, f).tobytes() == getattr(r, f).tobytes() for f in ("sac_R", "sac_t"))
            same = same and d.inliers.tolist() == h.inliers.tolist() and (d.best_hypothesis, d.sample) == (h.best_hypothesis, h.sample)
            same = same and r.refine.R.tobytes() == e.R.tobytes() and r.refine.t.tobytes() == e.t.tobytes()
        d = res["sac_device"]
        ku = np.median(np.array(kus[1:]), axis=0)
        S = int(d.n_consensus)
        rec = {"hypotheses": H, "consensus": S, "n_models": int(d.n_models), "sac_inliers": int(d.sac_n_inliers),
               "unmoved": int((~moved).sum()), "inliers_are_the_unmoved": bool((d.inliers == ~moved).all()),
               "used_with_refine": int(res["sac_refine_device"].used), "all_results_equal": bool(same),
               "k_sac_hypotheses_us": round(float(ku[0]), 1), "k_sac_score_us": round(float(ku[1]), 1), "k_sac_pick_us": round(float(ku[2]), 1),
               "k_sac_score_grid": [(S + TILE - 1) // TILE, (H + HYP_BLOCK - 1) // HYP_BLOCK],
               "reprojections": H * S, "k_sac_score_ns_per_reprojection": round(float(ku[1]) * 1e3 / (int(d.n_models) * S), 4)}
        for k in legs:
            rec["%s_ms" % k] = round(float(np.median(t[k][1:])), 3)
            rec["%s_ms_runs" % k] = [round(x, 3) for x in t[k][1:]]
        out["runs"][str(H)] = rec
    print(json.dumps(out))


def child(a, tree=None, solver=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "one", "--reps", str(a.reps), "--hyp-block", str(a.hyp_block), "--solver",
           solver or a.solver] + (["--tree", tree] if tree else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=400).stdout.strip().splitlines()[-1])


def guard_of(path):
    """the one guard, from a record of pose_rate.py --leg ab: refine_pose's whole call on the device store"""
    with open(path) as f:
        pairs = json.load(f)["pairs"]
    pm = [p["parent"]["refine_device_ms"] for p in pairs]
    slowest = max(x for p in pairs for x in p["parent"]["refine_device_ms_runs"])
    spread = max(pm) - min(pm)
    tm = [p["this"]["refine_device_ms"] for p in pairs]
    return {"leg": "refine_pose, the whole call on the device store", "parent_medians_ms": pm, "parent_slowest_run_ms": slowest,
            "parent_spread_of_medians_ms": round(spread, 3), "this_medians_ms": tm, "limit_ms": round(slowest + spread, 3),
            "met": bool(max(tm) <= slowest + spread)}


def parent_guard(a):
    """the parent's library and this one's alternating with the central solver -> the guard on ransac_pose's whole call"""
    pairs = [{"parent": child(a, a.parent, "central"), "this": child(a, None, "central")} for _ in range(a.procs)]
    out = {"leg": "ransac_pose with the central solver, the whole call on the device store", "met": True}
    for H in ("100", "1024"):
        pm = [p["parent"]["runs"][H]["sac_device_ms"] for p in pairs]
        slowest = max(x for p in pairs for x in p["parent"]["runs"][H]["sac_device_ms_runs"])
        spread = max(pm) - min(pm)
        tm = [p["this"]["runs"][H]["sac_device_ms"] for p in pairs]
        out[H] = {"parent_medians_ms": pm, "parent_slowest_run_ms": slowest, "parent_spread_of_medians_ms": round(spread, 3),
                  "this_medians_ms": tm, "limit_ms": round(slowest + spread, 3), "met": bool(max(tm) <= slowest + spread),
                  "parent_k_sac_hypotheses_us": [p["parent"]["runs"][H]["k_sac_hypotheses_us"] for p in pairs],
                  "this_k_sac_hypotheses_us": [p["this"]["runs"][H]["k_sac_hypotheses_us"] for p in pairs]}
        out["met"] = out["met"] and out[H]["met"]
    out["pairs"] = pairs
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--leg", default="one", choices=["one", "all"])
    ap.add_argument("--guard", default=None, help="a record of pose_rate.py --leg ab --tree PARENT")
    ap.add_argument("--out", default=None)
    ap.add_argument("--solver", default="central", choices=["central", "rig"])
    ap.add_argument("--tree", default=None, help="--leg one: a checkout whose package and library are timed instead of this one's")
    ap.add_argument("--parent", default=None, help="--leg all: the parent commit's checkout, for the guard on the central solver")
    ap.add_argument("--alt", action="append", default=[], help="--leg all: NAME=DIR, a library built with other switches")
    ap.add_argument("--hyp-block", type=int, default=HYP_BLOCK, help="the library's MCORB_SAC_HYP_BLOCK, when it was built with another")
    a = ap.parse_args()
    HYP_BLOCK = a.hyp_block
    if a.leg == "one":
        if a.tree:
            sys.path.insert(0, os.path.abspath(a.tree))
        import mcorb
        one_leg(mcorb, a)
        sys.exit(0)
    out = {"processes": [child(a) for _ in range(a.procs)]}
    if a.guard:
        out["regression_guard"] = guard_of(a.guard)
    if a.parent:
        out["central_solver_guard"] = parent_guard(a)
    for alt in a.alt:
        name, tree = alt.split("=", 1)
        out.setdefault("alternates", {})[name] = [{"alternate": child(a, tree), "this": child(a)} for _ in range(a.procs)]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
