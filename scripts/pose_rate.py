"""Rate of the rig pose refinement (mcorb_lmap_refine_pose, mcorb_lmap_set_track_refine) on section 9f's
frame: 4 cameras at 1280 x 720, an extraction job on the synthetic rig frame (about 2 000 keypoints per camera), landmarks
back-projected from those keypoints, 5 x 3 000 l_ids, about 5 000 de-duplicated matches.  The predicted pose is moved a little
from the one the landmarks were made with, so the refinement has something to do.  bench.py times none of this.

--leg one [--tree DIR]: one process on the imported library (DIR's, a checkout built from another commit, or this one's).
Medians of --reps (5) alternating runs after a warm-up:
  guard_track_off  LocalMap.track_rig_frame with the option off, alone and back to back, before any other leg: the one leg
                   that runs identically on a library without the feature, and the regression guard's
  track_off        the same call inside the alternation (every library has it; on this commit's library it follows a
                   millisecond of host-only refinement, during which the GPU idles)
  track_on         the same with set_track_refine on, then last_track_pose        (this commit's library only)
  refine_device    LocalMap.refine_pose on the frame's matches, the device store  (")
  refine_host      the same on a host-only store, one thread                      (")
and k_pose_refine between HIP events, the solves and passes per round, and whether all results are equal bit for bit.

--leg ab --tree PARENT: --leg one in fresh processes, PARENT's library and this one's alternating, --procs (3) each, and the
regression guard: with the option off this commit's track_rig_frame median must not exceed the parent's slowest run by more
than the parent's own spread (of medians) across its processes.

    python scripts/pose_rate.py --leg ab --tree PARENT [--out profiles/pose_rate.json]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

INV_SIGMA2 = [1.0 / 1.2 ** (2 * l) for l in range(8)]


def one_leg(mcorb, a):
    import kfdb_cases
    import track_cases as T
    import track_rate as TR
    rig = mcorb.Rig(TR.CAMS, TR.COLS, TR.ROWS, 1, 1, nfeatures=TR.KEYPOINTS)
    rig.upload([mcorb.synth_rig_frame(0, TR.CAMS, c, TR.COLS, TR.ROWS) for c in range(TR.CAMS)])
    rig.extract(TR.CAMS)
    v, pts, desc, lids = TR.slot_workload(mcorb, rig)
    # the predicted pose: 2 mrad and a few centimetres from the one the landmarks were made with
    v = T.view(v["cams"], v["cols"], v["rows"], R0=(T.rot(1, 0.002) @ T.rot(0, -0.001)).tolist(), t0=(0.03, -0.02, 0.04))
    view = T.to_view(mcorb, v)

    def store(device):
        lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=len(pts),
                            max_candidates=len(pts))
        lm.set(np.arange(len(pts), dtype=np.int32), pts, np.zeros_like(pts), desc)
        return lm

    lm = store(0)
    has = hasattr(lm, "refine_pose")
    legs = ["track_off"] + (["track_on", "refine_device", "refine_host"] if has else [])
    t = {k: [] for k in legs}
    kus, same = [], True
    if has:
        lm_host = store(-1)
        xy, ds = TR.readback(rig)
        r = lm.track_rig_frame(view, rig, 0, lids)
        cam = np.concatenate([np.full(len(r.match_kp[c]), c, np.int32) for c in range(TR.CAMS)])
        uv = np.concatenate([xy[c][r.match_kp[c]].reshape(-1, 2) for c in range(TR.CAMS)]).astype(np.float32)
        mlids = np.concatenate(r.match_lid).astype(np.int32)
        octave = np.zeros(len(cam), np.int32)
        R0, t0 = mcorb.pose_of_view(view)
    # the regression guard's leg, the same on every library: the call alone, back to back, before anything else runs
    guard = []
    for rep in range(a.reps + 1):
        t0_ = time.perf_counter()
        lm.track_rig_frame(view, rig, 0, lids)
        guard.append((time.perf_counter() - t0_) * 1e3)
    res = {}
    for rep in range(a.reps + 1):                                      # alternating; the first round is the warm-up
        for k in legs:
            if k == "track_off" and has:
                lm.set_track_refine(None)
            if k == "track_on":
                lm.set_track_refine(INV_SIGMA2)
            t0_ = time.perf_counter()
            if k == "track_off":
                res[k] = lm.track_rig_frame(view, rig, 0, lids)
            elif k == "track_on":
                res[k] = lm.track_rig_frame(view, rig, 0, lids)
                res["pose_on"] = lm.last_track_pose()
            elif k == "refine_device":
                res[k] = lm.refine_pose(view, R0, t0, cam, uv, octave, INV_SIGMA2, lids=mlids)
            else:
                res[k] = lm_host.refine_pose(view, R0, t0, cam, uv, octave, INV_SIGMA2, lids=mlids)
            t[k].append((time.perf_counter() - t0_) * 1e3)
            if k == "refine_device":
                kus.append(lm.last_pose_timing())
        if has:
            import pose_cases as PC
            same = same and T.as_lists(res["track_on"]) == T.as_lists(res["track_off"])
            for k in ("refine_host", "pose_on"):
                try:
                    PC.same(PC.as_ref(res[k]), PC.as_ref(res["refine_device"]), k)
                except AssertionError:
                    same = False
    r = res["track_off"]
    out = {"tree": os.path.abspath(a.tree or ROOT), "cores": len(os.sched_getaffinity(0)), "cameras": TR.CAMS, "image": [TR.COLS, TR.ROWS],
           "candidates": int(r.n_candidates), "matches_per_camera": [len(m) for m in r.match_kp], "has_refine_pose": bool(has)}
    out["guard_track_off_ms"] = round(float(np.median(guard[1:])), 3)
    out["guard_track_off_ms_runs"] = [round(x, 3) for x in guard[1:]]
    for k in legs:
        vals = t[k][1:]
        out["%s_ms" % k] = round(float(np.median(vals)), 3)
        out["%s_ms_runs" % k] = [round(x, 3) for x in vals]
    if has:
        p = res["refine_device"]
        import pose_cases as PC
        import pose_ref as P
        obs = [(int(cam[i]), float(uv[i][0]), float(uv[i][1]), 0, [float(x) for x in pts[mlids[i]]]) for i in range(len(cam))]
        t0_ = time.perf_counter()
        ref = P.refine(v["cams"], P.pose_of_view(v["R0"], v["t0"]), obs, INV_SIGMA2)
        try:
            PC.same(PC.as_ref(p), ref, "restatement")
            same_ref = True
        except AssertionError:
            same_ref = False
        out.update({"observations": int(p.n_obs), "inliers": int(p.n_inliers), "status": int(p.status), "solves_per_round": list(p.iterations),
                    "passes_per_round": ref["passes"], "cost_initial": p.cost_initial, "cost_final": p.cost_final,
                    "k_pose_refine_us": round(float(np.median(kus[1:])), 1), "k_pose_refine_us_runs": [round(float(u), 1) for u in kus[1:]],
                    "k_pose_refine_us_per_pass": round(float(np.median(kus[1:])) / max(1, sum(ref["passes"])), 2),
                    "all_results_equal": bool(same), "equals_restatement": bool(same_ref),
                    "restatement_s": round(time.perf_counter() - t0_, 2)})
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def child(a, tree):
    """one fresh process of this script on `tree`'s library -> its record"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "one", "--reps", str(a.reps)] + (["--tree", tree] if tree else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=240).stdout.strip().splitlines()[-1])


def ab_leg(a):
    pairs = []
    for _ in range(a.procs):
        pairs.append({"parent": child(a, a.tree), "this": child(a, None)})
    pm = [p["parent"]["guard_track_off_ms"] for p in pairs]
    slowest = max(x for p in pairs for x in p["parent"]["guard_track_off_ms_runs"])
    spread = max(pm) - min(pm)
    tm = [p["this"]["guard_track_off_ms"] for p in pairs]
    out = {"regression_guard": {"parent_medians_ms": pm, "parent_slowest_run_ms": slowest, "parent_spread_of_medians_ms": round(spread, 3),
                                "this_medians_ms": tm, "limit_ms": round(slowest + spread, 3), "met": max(tm) <= slowest + spread},
           "pairs": pairs}
    for p in pairs:
        p["parent"]["tree"] = "parent"
        p["this"]["tree"] = "this commit"
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default="one", choices=["one", "ab"])
    ap.add_argument("--tree", default=None, help="a checkout whose package is timed instead of this one's (--leg one); the parent "
                                                 "commit's checkout (--leg ab)")
    ap.add_argument("--procs", type=int, default=3, help="--leg ab: processes per tree")
    a = ap.parse_args()
    if a.leg == "ab":
        if not a.tree:
            ap.error("--leg ab needs --tree PARENT")
        ab_leg(a)
        sys.exit(0)
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    import mcorb
    one_leg(mcorb, a)
