"""What mcorb_lmap_triangulate_new costs (FrontEnd::TriangulateNewLandmarks), on the same machine and inputs: one frame of 3000
unassigned matches against the previous keyframe on the 4-camera rig of scripts/mapping_rate.py, half of the matches with 2 views in
total, the rest with 3 to 6; the keypoints are the exact projections rounded to float plus sub-pixel noise, so the refinement
takes steps.  With --scale 1 (noise of 0.8 px at level 0, ORB's table) every match ends after its first solve; --scale 16
multiplies the noise and divides the table, as the tests' scene does, so that a share of the matches takes two or three.
  --leg one (default)
    device     the whole call on a device store, and k_map_refine_new (both instances) between HIP events;
    host only  the same call on the host-only store, one thread;
    solves     the distribution of solves per launched match, and a model of what the lanes of a wave wait for its slowest one:
               a lane's work is views * (1 + solves) residual passes, a wave costs its count times its largest lane, and the
               share reported is 1 - sum(work) / sum(wave cost) over the call's blocks as the host cuts them.
    The two sides are timed in alternating runs, `reps` each after a warm-up; medians are reported.
  --leg guard [--tree T]
    the whole call on a device store of the three triangulation entries, `reps` runs after a warm-up each, on this tree's library
    or on the one of checkout T: mcorb_lmap_triangulate_neighbours on mapping_rate.py's frame, mcorb_lmap_triangulate_new on this
    script's frame at --scale 1 and 16, mcorb_lmap_initialize on init_rate.py's rig at 300 and 3 000 matches.  Next to the times
    of a call: the digest of everything it returns and of the landmarks it stored.
  --leg ab --tree PARENT
    the regression guard: --procs pairs of fresh processes of --leg guard, the parent's alternating with this commit's.  Per call
    this commit's medians must not exceed the parent's slowest run plus the parent's own spread of medians across its processes,
    and every digest must be the same in all processes of both trees: the script fails otherwise.
bench.py times none of this.
    python scripts/mapping_new_rate.py [--reps 5] [--out profiles/mapping_new_rate.json]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MATCHES, CAMS, MAXLM, NOISE = 3000, 4, 1 << 15, 0.8


def workload(scale=1.0):
    import mapping_cases as Mc
    import mapping_new_cases as Nc
    rng = np.random.default_rng(6)
    Ks, rigT = Mc.make_rig(CAMS, rng)
    cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(0.01, 0.02, -0.01), np.zeros(3)), rigT), Ks)
    prev = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(*rng.uniform(-0.05, 0.05, 3)), np.array([0.8, 0.05, 0.0])), rigT), Ks)
    shapes = [(1, 1)] * 5 + [(2, 1), (2, 2), (3, 2), (3, 3), (1, 3)]     # half 2 views, the rest 3 .. 6
    mid = 0.5 * prev.g["twc"]
    ms = []
    for i in range(MATCHES):
        a, b = shapes[i % len(shapes)]
        X = mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 15)])
        q = prev.add(X, sorted(rng.choice(CAMS, a, replace=False).tolist()), rng)
        t = cur.add(X, sorted(rng.choice(CAMS, b, replace=False).tolist()), rng)
        Nc.jitter(prev, q, rng, NOISE * scale), Nc.jitter(cur, t, rng, NOISE * scale)
        ms.append((q, t))
    return dict(K=np.array(Ks), inv_sigma2=Nc.inv_sigma2(scale), cur=cur.done(), prev=prev.done(), matches=np.array(ms, np.int32), next_lid=0)


def side(mcorb, device, sc):
    import mapping_cases as Mc
    lm = new_store(mcorb, device)
    args = (Mc.to_frame(mcorb, sc["cur"]), sc["cur"]["lids"], Mc.to_frame(mcorb, sc["prev"]), sc["prev"]["lids"], sc["matches"], sc["K"],
            sc["inv_sigma2"], sc["next_lid"])
    return lm, (lambda: lm.triangulate_new(*args))


def waiting_share(sc, solves):
    """the model of the docstring, over the blocks of the call: <= 4 views first, each part ordered by view count, 64 per block"""
    nv = np.array([int((sc["prev"]["match_index"][q] != -1).sum() + (sc["cur"]["match_index"][t] != -1).sum()) for q, t in sc["matches"]])
    work = nv * (1 + solves)
    done = cost = 0
    for part in (np.nonzero(nv <= 4)[0], np.nonzero(nv > 4)[0]):
        part = part[np.argsort(nv[part], kind="stable")]
        for k in range(0, len(part), 64):
            w = work[part[k:k + 64]]
            done += int(w.sum())
            cost += int(len(w) * w.max())
    return 1.0 - done / max(cost, 1)


def one_leg(mcorb, a):
    import mapping_new_cases as Nc
    sc = workload(a.scale)
    sides = {"device": side(mcorb, 0, sc), "host_only": side(mcorb, -1, sc)}
    got = {k: f() for k, (_, f) in sides.items()}                   # (also the warm-up)
    try:
        Nc.same(got["device"], got["host_only"])
        same = True
    except AssertionError:
        same = False
    t, kus = {k: [] for k in sides}, []
    for _ in range(a.reps):                                         # alternating
        for k, (lm, f) in sides.items():
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "device":
                kus.append(lm.last_triangulate_new_timing())
    d = got["device"]
    nv = [int((sc["prev"]["match_index"][q] != -1).sum() + (sc["cur"]["match_index"][tt] != -1).sum()) for q, tt in sc["matches"]]
    res = {"cores": len(os.sched_getaffinity(0)), "matches": MATCHES, "cameras": CAMS, "noise_px_at_level_0": NOISE * a.scale, "scale": a.scale,
           "matches_2_views": int(sum(v == 2 for v in nv)), "matches_3_to_6_views": int(sum(v > 2 for v in nv)),
           "launched": kus[0][1], "landmarks_made": int(d.n_triangulated), "by_verdict": d.n_by_verdict.tolist(),
           "device_equals_host_only": bool(same),
           "solves_histogram": np.bincount(d.iterations, minlength=8).tolist(),
           "accepted_matches_mean_solves": round(float(d.iterations[d.verdict == 0].mean()), 3),
           "wave_waiting_share_model": round(float(waiting_share(sc, d.iterations)), 3),
           "k_map_refine_new_us": round(float(np.median([u[0] for u in kus])), 1),
           "k_map_refine_new_us_runs": [round(float(u[0]), 1) for u in kus]}
    for k in sides:
        res[k + "_call_ms"] = round(float(np.median(t[k])), 3)
        res[k + "_call_ms_runs"] = [round(x, 3) for x in t[k]]
    return res


def new_store(mcorb, device):
    import kfdb_cases
    return mcorb.LocalMap(mcorb.ORBVocabulary(device=device).create(**kfdb_cases.vocabulary()), device=device, max_landmarks=MAXLM, max_candidates=16)


def digest(lm, res):
    """everything a call returned (none of it is a time) and the landmarks it stored"""
    h = hashlib.sha256()
    for k, v in sorted(vars(res).items()):
        for x in (v if isinstance(v, list) else [v]):
            h.update(k.encode() + np.ascontiguousarray(x).tobytes())
    for lid in res.new_lid[res.new_lid >= 0]:
        pt, normal, _, _ = lm.get(int(lid))
        h.update(pt.tobytes() + normal.tobytes() + np.array([lm.observations(int(lid))[0]], np.int64).tobytes())
    return h.hexdigest()


def guard_calls(mcorb):
    """name -> (store, call) of the five guarded calls, each on a device store of its own"""
    import init_cases as Ic
    import init_rate
    import mapping_rate
    calls = {"triangulate_neighbours": mapping_rate.side(mcorb, 0, mapping_rate.workload())}
    for scale in (1, 16):
        calls["triangulate_new_scale_%d" % scale] = side(mcorb, 0, workload(float(scale)))
    for n in (300, 3000):
        lm, sc = new_store(mcorb, 0), Ic.scene(init_rate.CAMS, n=n, seed=17)
        calls["initialize_%d" % n] = (lm, (lambda lm=lm, sc=sc: Ic.run_scene(mcorb, lm, sc)))
    return calls


def guard_leg(mcorb, a):
    out = {}
    for name, (lm, f) in guard_calls(mcorb).items():
        first = f()                                                 # (also the warm-up)
        runs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            f()
            runs.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"call_ms": round(float(np.median(runs)), 3), "call_ms_runs": [round(x, 3) for x in runs], "digest": digest(lm, first)}
    return out


def child(a, tree):
    """one fresh process of --leg guard on `tree`'s library -> its record"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "guard", "--reps", str(a.reps)] + (["--tree", tree] if tree else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1])


def ab_leg(a):
    pairs = [{"parent": child(a, a.tree), "this": child(a, None)} for _ in range(a.procs)]
    guard = {}
    for name in pairs[0]["parent"]:
        assert len({p[t][name]["digest"] for p in pairs for t in p}) == 1, "the results of %s differ between the trees or the processes" % name
        pm = [p["parent"][name]["call_ms"] for p in pairs]
        slowest = max(x for p in pairs for x in p["parent"][name]["call_ms_runs"])
        spread = max(pm) - min(pm)
        tm = [p["this"][name]["call_ms"] for p in pairs]
        guard[name] = {"parent_medians_ms": pm, "parent_slowest_run_ms": slowest, "parent_spread_of_medians_ms": round(spread, 3),
                       "this_medians_ms": tm, "limit_ms": round(slowest + spread, 3), "met": bool(max(tm) <= slowest + spread)}
    return {"regression_guard": guard, "equal_bytes_across_trees_and_processes": True, "pairs": pairs}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default="one", choices=["one", "guard", "ab"])
    ap.add_argument("--tree", default=None, help="--leg guard: a checkout whose package is timed instead of this one's; --leg ab: the "
                                                 "parent commit's checkout")
    ap.add_argument("--scale", type=float, default=1.0, help="--leg one: keypoint noise and the sigma table's unit, in pixels at level 0 "
                                                               "over 0.8 and 1 (16: costs large enough for second steps)")
    ap.add_argument("--procs", type=int, default=3, help="--leg ab: processes per tree")
    a = ap.parse_args()
    if a.leg == "ab":
        if not a.tree:
            ap.error("--leg ab needs --tree PARENT")
        out = ab_leg(a)
    else:
        sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
        import mcorb
        out = one_leg(mcorb, a) if a.leg == "one" else guard_leg(mcorb, a)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if a.leg == "ab" and not all(g["met"] for g in out["regression_guard"].values()):
        sys.exit("a call is slower than the parent's limit")
