"""What one frame of fast tracking costs (mcorb_lmap_track: Tracking::project_ and Tracking::queryCurrentFrame), on the same
machine and inputs: 5 map entries of 3000 l_ids that name about 10 000 distinct landmarks, a rig of 4 cameras at 1280 x 720 and
2000 keypoints per camera, made from the true projections plus noise and clutter.
  device     the whole call on a device store, and k_track_project / k_track_match between HIP events; k_track_match against
             its algorithmic work -- queries x keypoints distance evaluations (5 fp64 operations each), and the bytes of the
             keypoints (8 per keypoint), of the descriptors the ten neighbours of a query need (10 x 32, and 32 of the landmark's),
             of the queries (8 + 1) and of the results (8);
  host only  the same call on the host-only store, on one thread.  (The reference runs one thread per camera.)
The two are timed in alternating runs, `reps` each after a warm-up; medians are reported.  bench.py times none of this.
    python scripts/track_rate.py [--reps 5] [--out profiles/track_rate.json]

--leg slot: the frame comes from a rig slot (mcorb_lmap_track_rig_frame).  The same rig and counts; the keypoints are those of an
extraction job on the synthetic rig frame, the landmarks are back-projected from those keypoints through the camera that saw them
(a quarter behind the rig), their descriptors the keypoints' with up to 24 bits flipped.  Timed in alternating runs:
  readback_track   Rig.features of the four images, the reshape to n x 2 arrays, LocalMap.track: what a caller does without the
                   slot entry;
  track            LocalMap.track on those arrays;
  track_rig_frame  LocalMap.track_rig_frame (only where the library has it: --tree names a checkout built from another commit,
                   whose package is imported instead of this one, to time the first two there).
  submit_wait      LocalMap.track_rig_frame_submit and LocalMap.track_wait (where the library has them), the two timed apart: what
                   the submission costs the caller's thread and what is left to wait for when nothing is overlapped.
With a library built with -DMCORB_TRACK_PROF the host phases of the last three are recorded as well.
    python scripts/track_rate.py --leg slot [--tree DIR] [--reps 5] [--out FILE]

--leg slot_ab --tree PARENT: the slot leg in fresh processes, PARENT's library and this one's alternating, --procs (3) each; the
pass marks -- in every pair of processes the median of track_rig_frame, and of track, on this tree is below the parent's fastest
run of the same leg in that pair -- and every process's record go to --out.  --prof-tree DIR adds one process on a checkout of
this commit built with -DMCORB_TRACK_PROF, for the phases.
    python scripts/track_rate.py --leg slot_ab --tree PARENT [--prof-tree DIR] [--out profiles/track_dedup_rate.json]

--leg batch --tree PARENT: a 32-frame job of the slot leg's frame, 32 distinct views (the predicted pose moved a little per frame),
the slot leg's 5 x 3000 ids for every frame.  Fresh processes, PARENT's library and this one's alternating, --procs (3) each; in a
process, alternating runs after a warm-up, in ms per 32 frames: `single` 32 x track_rig_frame, `pair` 32 x (track_rig_frame_submit,
track_wait), and where the library has them `batch` one track_rig_frames and `batch_submit`, the return time of
track_rig_frames_submit (its wait follows, untimed); the five kernel intervals of `batch` divided by 32 beside the single call's.
Pass mark: in every pair of processes the median of `batch` on this tree is below the parent's fastest run of `single` and of
`pair`.  --prof-tree DIR adds one process on a checkout of this commit built with -DMCORB_TRACK_PROF, for the host phases.
    python scripts/track_rate.py --leg batch --tree PARENT [--prof-tree DIR] [--out profiles/track_batch_rate.json]

--leg stress: two frames on host arrays that load the de-duplication in opposite ways, the whole call and (where the library has
last_track_timing5) the kernels: `one_keypoint`, 8000 landmarks whose queries all match the single keypoint of their camera, so
every atomic of the arg-min lands on one address; `no_radius`, the frame of the default leg with max_d2 = inf, so every query has
ten neighbours.
    python scripts/track_rate.py --leg stress [--tree DIR] [--out FILE]"""
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

CAMS, COLS, ROWS, KEYPOINTS, LANDMARKS, ENTRIES, LIDS_PER_ENTRY = 4, 1280, 720, 2000, 10000, 5, 3000


def workload():
    import track_cases as T
    rng = np.random.default_rng(31)
    cams = []
    for c in range(CAMS):
        Rc = T.rot(1, rng.uniform(-0.05, 0.05)) @ T.rot(0, rng.uniform(-0.03, 0.03))
        cams.append(T.cam(Rc, (0.25 * c - 0.4, rng.uniform(-0.02, 0.02), 0.0), fx=700.0, fy=700.0, s=0.0, u0=COLS / 2, v0=ROWS / 2))
    v = T.view(cams, COLS, ROWS, T.rot(1, 0.04), (0.2, -0.1, 0.3))
    pts = np.stack([rng.uniform(-8, 8, LANDMARKS), rng.uniform(-4.5, 4.5, LANDMARKS), rng.uniform(-1, 9, LANDMARKS)], axis=1)
    desc = rng.integers(0, 256, (LANDMARKS, 32), dtype=np.uint8)
    # the map entries' l_ids: windows of the landmark range that overlap, with -1 for features without a landmark
    lids = []
    for e in range(ENTRIES):
        w = (np.arange(LIDS_PER_ENTRY) * 3 + e * (LANDMARKS - LIDS_PER_ENTRY) // (ENTRIES - 1) + rng.integers(0, 3, LIDS_PER_ENTRY)) % LANDMARKS
        w[rng.random(LIDS_PER_ENTRY) < 0.05] = -1
        lids.append(w)
    lids = np.concatenate(lids).astype(np.int32)
    # keypoints: the landmarks' own projections (vectorised: a workload, not a reference), moved by a pixel, plus clutter
    R0, t0 = np.array(v["R0"]), np.array(v["t0"])
    p0 = pts @ R0.T + t0
    kps, descs = [], []
    for c in cams:
        q = (p0 - np.array(c["t"])) @ np.array(c["R"])
        ok = q[:, 2] > 0.1
        u = q[:, 0] / np.where(ok, q[:, 2], 1.0) * c["fx"] + c["u0"]
        w_ = q[:, 1] / np.where(ok, q[:, 2], 1.0) * c["fy"] + c["v0"]
        ok &= (u > 0) & (u < COLS) & (w_ > 0) & (w_ < ROWS)
        idx = rng.permutation(np.flatnonzero(ok))[:KEYPOINTS * 3 // 4]
        xy = np.stack([u[idx], w_[idx]], axis=1) + rng.normal(0, 1.0, (len(idx), 2))
        d = desc[idx].copy()
        flips = rng.integers(0, 256, (len(idx), 24))                   # up to 24 bits flipped
        for j in range(24):
            on = rng.random(len(idx)) < 0.5
            d[on, flips[on, j] // 8] ^= (1 << (flips[on, j] % 8)).astype(np.uint8)
        nclutter = KEYPOINTS - len(idx)
        xy = np.concatenate([xy, np.stack([rng.uniform(0, COLS, nclutter), rng.uniform(0, ROWS, nclutter)], axis=1)])
        d = np.concatenate([d, rng.integers(0, 256, (nclutter, 32), dtype=np.uint8)])
        order = rng.permutation(KEYPOINTS)
        kps.append(np.ascontiguousarray(xy[order], np.float32))
        descs.append(np.ascontiguousarray(d[order]))
    return dict(view=v, pts=pts, desc=desc, lids=lids, kps=kps, descs=descs)


def side(mcorb, device, w):
    import kfdb_cases
    lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=LANDMARKS,
                        max_candidates=LANDMARKS)
    lm.set(np.arange(LANDMARKS, dtype=np.int32), w["pts"], np.zeros_like(w["pts"]), w["desc"])
    return lm


def slot_workload(mcorb, rig):
    """-> (view as a dict, points, descriptors, lids, the frame's arrays as Rig.features gives them)"""
    import track_cases as T
    rng = np.random.default_rng(37)
    cams = [T.cam(t=(1.5 * c, 0.0, 0.0), fx=700.0, fy=700.0, u0=COLS / 2, v0=ROWS / 2) for c in range(CAMS)]
    v = T.view(cams, COLS, ROWS)
    feats = [rig.features(c) for c in range(CAMS)]
    pts, desc = [], []
    for c in range(CAMS):
        _, k, d = feats[c]
        z = rng.uniform(2.0, 10.0, len(k))
        z[rng.random(len(k)) < 0.25] *= -1.0                            # behind the rig: dropped from every camera
        pts.append(np.stack([(k["x"] - COLS / 2) / 700.0 * z + 1.5 * c, (k["y"] - ROWS / 2) / 700.0 * z, z], axis=1))
        d = d.copy()
        flips = rng.integers(0, 256, (len(k), 24))
        for j in range(24):
            on = rng.random(len(k)) < 0.5
            d[on, flips[on, j] // 8] ^= (1 << (flips[on, j] % 8)).astype(np.uint8)
        desc.append(d)
    pts, desc = np.concatenate(pts), np.concatenate(desc)
    n = len(pts)
    lids = []
    for e in range(ENTRIES):
        w = (np.arange(LIDS_PER_ENTRY) * 3 + e * (n - LIDS_PER_ENTRY) // (ENTRIES - 1) + rng.integers(0, 3, LIDS_PER_ENTRY)) % n
        w[rng.random(LIDS_PER_ENTRY) < 0.05] = -1
        lids.append(w)
    return v, pts, desc, np.concatenate(lids).astype(np.int32)


def readback(rig):
    xy, ds = [], []
    for c in range(CAMS):
        _, k, d = rig.features(c)
        xy.append(np.ascontiguousarray(np.stack([k["x"], k["y"]], axis=1), np.float32))
        ds.append(d)
    return xy, ds


def slot_leg(mcorb, a):
    import ctypes
    import kfdb_cases
    import track_cases as T
    rig = mcorb.Rig(CAMS, COLS, ROWS, 1, 1, nfeatures=KEYPOINTS)
    rig.upload([mcorb.synth_rig_frame(0, CAMS, c, COLS, ROWS) for c in range(CAMS)])
    rig.extract(CAMS)
    v, pts, desc, lids = slot_workload(mcorb, rig)
    view = T.to_view(mcorb, v)
    lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=0).create(**kfdb_cases.vocabulary()), device=0, max_landmarks=len(pts), max_candidates=len(pts))
    lm.set(np.arange(len(pts), dtype=np.int32), pts, np.zeros_like(pts), desc)
    xy, ds = readback(rig)
    has_slot, has_pair = hasattr(lm, "track_rig_frame"), hasattr(lm, "track_rig_frame_submit")
    try:
        phases_fn = lm.L.mcorb_lmap_track_phases
    except AttributeError:
        phases_fn = None

    def phases():
        us = (ctypes.c_float * 5)()
        phases_fn(lm.h, us)
        return list(us)

    legs = ["readback_track", "track"] + (["track_rig_frame"] if has_slot else []) + (["submit_wait"] if has_pair else [])
    t = {k: [] for k in legs}
    t_submit = []
    kus = {k: [] for k in legs}
    ph = {k: [] for k in legs}
    res, same = {}, True
    for rep in range(a.reps + 1):                                      # alternating; the first round is the warm-up
        for k in legs:
            t0 = time.perf_counter()
            if k == "readback_track":
                xy_, ds_ = readback(rig)
                res[k] = lm.track(view, xy_, ds_, lids)
            elif k == "track":
                res[k] = lm.track(view, xy, ds, lids)
            elif k == "track_rig_frame":
                res[k] = lm.track_rig_frame(view, rig, 0, lids)
            else:
                lm.track_rig_frame_submit(view, rig, 0, lids)
                t_submit.append((time.perf_counter() - t0) * 1e3)
                res[k] = lm.track_wait()
            t[k].append((time.perf_counter() - t0) * 1e3)
            kus[k].append(lm.last_track_timing5() if has_pair else lm.last_track_timing4() if has_slot else lm.last_track_timing())
            if phases_fn is not None:
                ph[k].append(phases())
        same = same and all(T.as_lists(res[k]) == T.as_lists(res["track"]) for k in legs)
    r = res["track"]
    out = {"tree": os.path.abspath(a.tree or ROOT), "cores": len(os.sched_getaffinity(0)), "cameras": CAMS, "image": [COLS, ROWS],
           "keypoints_per_camera": [len(x) for x in xy], "landmarks": int(len(pts)), "lids": int(len(lids)),
           "candidates": int(r.n_candidates), "pairs": int(r.n_candidates) * CAMS, "queries_per_camera": [len(p) for p in r.proj_lid],
           "matched_per_camera": [int((b >= 0).sum()) for b in r.best_kp], "matches_per_camera": [len(m) for m in r.match_kp],
           "legs_equal": bool(same)}
    for k in legs:
        vals = t[k][1:]
        out["%s_ms" % k] = round(float(np.median(vals)), 3)
        out["%s_ms_runs" % k] = [round(x, 3) for x in vals]
        out["%s_kernel_us" % k] = [round(float(np.median([u[i] for u in kus[k][1:]])), 1) for i in range(len(kus[k][0]))]
        if phases_fn is not None:
            out["%s_host_phase_us" % k] = dict(zip(("candidate_walk", "submission", "wait", "deduplication", "output"),
                                                   [round(float(np.median([p[i] for p in ph[k][1:]])), 1) for i in range(5)]))
    if has_pair:
        out["submit_ms_runs"] = [round(x, 3) for x in t_submit[1:]]
        out["submit_ms"] = round(float(np.median(t_submit[1:])), 3)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def child(a, leg, tree):
    """one fresh process of this script on `tree`'s library -> its record"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(a.reps)] + (["--tree", tree] if tree else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=180).stdout.strip().splitlines()[-1])


def slot_ab_leg(a):
    pairs = []
    for _ in range(a.procs):
        pairs.append({"parent": child(a, "slot", a.tree), "this": child(a, "slot", None)})
    marks = {}
    for k in ("track_rig_frame", "track"):
        marks[k] = [{"this_median_ms": p["this"]["%s_ms" % k], "parent_fastest_ms": min(p["parent"]["%s_ms_runs" % k]),
                     "met": p["this"]["%s_ms" % k] < min(p["parent"]["%s_ms_runs" % k])} for p in pairs]
    out = {"pass_marks": marks, "pass_marks_met": all(m["met"] for v in marks.values() for m in v), "pairs": pairs}
    if a.prof_tree:
        out["phases"] = child(a, "slot", a.prof_tree)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


BATCH_FRAMES = 32


def batch_one_leg(mcorb, a):
    """one process of --leg batch on the imported library -> its record"""
    import ctypes
    import kfdb_cases
    import track_cases as T
    F = BATCH_FRAMES
    rig = mcorb.Rig(CAMS, COLS, ROWS, F, 1, nfeatures=KEYPOINTS)
    rig.upload([mcorb.synth_rig_frame(0, CAMS, c, COLS, ROWS) for c in range(CAMS)] * F)
    rig.extract(F * CAMS)
    v, pts, desc, lids = slot_workload(mcorb, rig)
    views = [T.to_view(mcorb, dict(v, t0=[0.002 * f, -0.001 * f, 0.0005 * f])) for f in range(F)]
    lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=0).create(**kfdb_cases.vocabulary()), device=0, max_landmarks=len(pts), max_candidates=len(pts))
    lm.set(np.arange(len(pts), dtype=np.int32), pts, np.zeros_like(pts), desc)
    has_batch = hasattr(lm, "track_rig_frames")
    try:
        phases_fn = lm.L.mcorb_lmap_track_phases
    except AttributeError:
        phases_fn = None

    def phases():
        us = (ctypes.c_float * 5)()
        phases_fn(lm.h, us)
        return list(us)

    legs = ["single", "pair"] + (["batch", "batch_submit"] if has_batch else [])
    t = {k: [] for k in legs}
    kus = {k: [] for k in ("single", "batch")}
    ph = {k: [] for k in ("single", "batch")}
    frames, lidss = list(range(F)), [lids] * F
    res = {}
    for rep in range(a.reps + 1):                                      # alternating; the first round is the warm-up
        for k in legs:
            t0 = time.perf_counter()
            if k == "single":
                res[k] = [lm.track_rig_frame(views[f], rig, f, lids) for f in range(F)]
            elif k == "pair":
                res[k] = []
                for f in range(F):
                    lm.track_rig_frame_submit(views[f], rig, f, lids)
                    res[k].append(lm.track_wait())
            elif k == "batch":
                res[k] = lm.track_rig_frames(views, rig, frames, lidss)
            else:
                lm.track_rig_frames_submit(views, rig, frames, lidss)
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "batch_submit":
                res[k] = lm.track_frames_wait()
            if k in kus:
                kus[k].append(lm.last_track_timing5())
                if phases_fn is not None:
                    ph[k].append(phases())
    same = all([T.as_lists(r) for r in res[k]] == [T.as_lists(r) for r in res["single"]] for k in legs)
    r0 = res["single"][0]
    out = {"tree": os.path.abspath(a.tree or ROOT), "cores": len(os.sched_getaffinity(0)), "cameras": CAMS, "image": [COLS, ROWS],
           "frames": F, "keypoints_per_camera": [len(rig.features(c)[1]) for c in range(CAMS)], "landmarks": int(len(pts)),
           "lids_per_frame": int(len(lids)), "candidates_per_frame": int(r0.n_candidates),
           "queries_per_camera_frame0": [len(p) for p in r0.proj_lid], "matches_per_camera_frame0": [len(m) for m in r0.match_kp],
           "frames_differ": bool(T.as_lists(res["single"][0])["proj"] != T.as_lists(res["single"][F - 1])["proj"]),
           "legs_equal": bool(same)}
    for k in legs:
        vals = t[k][1:]
        out["%s_ms_per_32" % k] = round(float(np.median(vals)), 3)
        out["%s_ms_per_32_runs" % k] = [round(x, 3) for x in vals]
    for k, div in (("single", 1), ("batch", F)):
        if kus[k]:                                                     # (single: the last of the 32 calls of a run)
            out["%s_kernel_us_per_frame" % k] = [round(float(np.median([u[i] for u in kus[k][1:]])) / div, 1) for i in range(5)]
        if ph[k]:
            out["%s_host_phase_us" % k] = dict(zip(("candidate_walk", "submission", "wait", "deduplication", "output"),
                                                   [round(float(np.median([p[i] for p in ph[k][1:]])), 1) for i in range(5)]))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def batch_leg(a):
    pairs = []
    for _ in range(a.procs):
        pairs.append({"parent": child(a, "batch_one", a.tree), "this": child(a, "batch_one", None)})
    marks = [{"this_batch_median_ms": p["this"]["batch_ms_per_32"], "parent_single_fastest_ms": min(p["parent"]["single_ms_per_32_runs"]),
              "parent_pair_fastest_ms": min(p["parent"]["pair_ms_per_32_runs"]),
              "met": p["this"]["batch_ms_per_32"] < min(p["parent"]["single_ms_per_32_runs"] + p["parent"]["pair_ms_per_32_runs"])}
             for p in pairs]
    out = {"pass_mark": marks, "pass_mark_met": all(m["met"] for m in marks), "pairs": pairs}
    if a.prof_tree:
        out["phases"] = child(a, "batch_one", a.prof_tree)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def stress_leg(mcorb, a):
    import kfdb_cases
    import track_cases as T
    rng = np.random.default_rng(41)
    n = 8000
    frames = {}
    # every query of a camera matches that camera's one keypoint: landmarks within 35 px of it, descriptors up to 12 bits off
    d0 = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.repeat(d0[None], n, axis=0)
    flips = rng.integers(0, 256, (n, 12))
    for j in range(12):
        on = rng.random(n) < 0.5
        desc[on, flips[on, j] // 8] ^= (1 << (flips[on, j] % 8)).astype(np.uint8)
    pts = np.stack([rng.uniform(600, 650, n), rng.uniform(350, 400, n), np.ones(n)], axis=1)
    frames["one_keypoint"] = dict(view=T.flat_view(COLS, ROWS, ncams=CAMS), pts=pts, desc=desc, lids=np.arange(n, dtype=np.int32),
                                  kps=[np.array([[625.0, 375.0]], np.float32)] * CAMS, descs=[d0[None].copy()] * CAMS, kw={})
    w = workload()
    w["kw"] = {"max_d2": float("inf")}
    frames["no_radius"] = w
    out = {"tree": os.path.abspath(a.tree or ROOT)}
    for name, w in frames.items():
        view = T.to_view(mcorb, w["view"])
        nl = len(w["pts"])
        lm = mcorb.LocalMap(mcorb.ORBVocabulary(device=0).create(**kfdb_cases.vocabulary()), device=0, max_landmarks=nl, max_candidates=nl)
        lm.set(np.arange(nl, dtype=np.int32), w["pts"], np.zeros_like(w["pts"]), w["desc"])
        ts, kus = [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            r = lm.track(view, w["kps"], w["descs"], w["lids"], **w["kw"])
            ts.append((time.perf_counter() - t0) * 1e3)
            kus.append(lm.last_track_timing5() if hasattr(lm, "last_track_timing5") else lm.last_track_timing())
        out[name] = {"candidates": int(r.n_candidates), "queries_per_camera": [len(p) for p in r.proj_lid],
                     "matched_per_camera": [int((b >= 0).sum()) for b in r.best_kp], "matches_per_camera": [len(m) for m in r.match_kp],
                     "track_ms": round(float(np.median(ts[1:])), 3), "track_ms_runs": [round(x, 3) for x in ts[1:]],
                     "kernel_us": [round(float(np.median([u[i] for u in kus[1:]])), 1) for i in range(len(kus[0]))]}
        lm.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default="stores", choices=["stores", "slot", "slot_ab", "stress", "batch", "batch_one"])
    ap.add_argument("--tree", default=None, help="a checkout whose package is timed instead of this one's (--leg slot, stress); "
                                                 "the parent commit's checkout (--leg slot_ab, batch)")
    ap.add_argument("--prof-tree", default=None, help="--leg slot_ab, batch: a checkout of this commit built with -DMCORB_TRACK_PROF")
    ap.add_argument("--procs", type=int, default=3, help="--leg slot_ab, batch: processes per tree")
    a = ap.parse_args()
    if a.leg == "slot_ab":
        if not a.tree:
            ap.error("--leg slot_ab needs --tree PARENT")
        slot_ab_leg(a)
        sys.exit(0)
    if a.leg == "batch":
        if not a.tree:
            ap.error("--leg batch needs --tree PARENT")
        batch_leg(a)
        sys.exit(0)
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    import mcorb
    if a.leg == "slot":
        slot_leg(mcorb, a)
        sys.exit(0)
    if a.leg == "stress":
        stress_leg(mcorb, a)
        sys.exit(0)
    if a.leg == "batch_one":
        batch_one_leg(mcorb, a)
        sys.exit(0)
    import track_cases as T
    w = workload()
    view = T.to_view(mcorb, w["view"])
    sides = {"device": side(mcorb, 0, w), "host_only": side(mcorb, -1, w)}
    t = {k: [] for k in sides}
    kus, same, res_d = [], True, None
    for rep in range(a.reps + 1):                                      # alternating; the first round is the warm-up
        out = {}
        for k, lm in sides.items():
            t0 = time.perf_counter()
            out[k] = lm.track(view, w["kps"], w["descs"], w["lids"])
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "device":
                kus.append(lm.last_track_timing())
        same = same and T.as_lists(out["device"]) == T.as_lists(out["host_only"])
        res_d = out["device"]
    kus = kus[1:]
    proj_us, match_us = float(np.median([u[0] for u in kus])), float(np.median([u[1] for u in kus]))
    queries = [len(p) for p in res_d.proj_lid]
    evals = sum(q * KEYPOINTS for q in queries)
    nq = sum(queries)
    match_bytes = CAMS * KEYPOINTS * 8 + nq * (10 * 32 + 32 + 8 + 8) + res_d.n_candidates * CAMS
    proj_bytes = res_d.n_candidates * (4 + 24 + CAMS * 9)
    res = {"cores": len(os.sched_getaffinity(0)), "cameras": CAMS, "image": [COLS, ROWS], "keypoints_per_camera": KEYPOINTS,
           "lids": int(len(w["lids"])), "candidates": int(res_d.n_candidates), "queries_per_camera": queries,
           "matched_per_camera": [int((b >= 0).sum()) for b in res_d.best_kp], "matches_per_camera": [len(m) for m in res_d.match_kp],
           "device_equals_host_only": bool(same),
           "k_track_project_us": round(proj_us, 1), "k_track_project_bytes": proj_bytes,
           "k_track_match_us": round(match_us, 1), "k_track_match_distance_evaluations": evals,
           "k_track_match_Gevals_per_s": round(evals / match_us / 1e3, 2), "k_track_match_fp64_GFLOPs": round(5 * evals / match_us / 1e3, 1),
           "k_track_match_bytes": match_bytes, "k_track_match_GBps": round(match_bytes / match_us / 1e3, 2)}
    for k in sides:
        v = t[k][1:]
        res["%s_track_ms" % k] = round(float(np.median(v)), 3)
        res["%s_track_ms_min_max" % k] = [round(min(v), 3), round(max(v), 3)]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
