"""What the map initialization costs (mcorb_lmap_initialize: FrontEnd::initialization, FrontEnd.cpp:2633-2839), on the same machine
and inputs: two frames of a rig of 4 cameras with 300, 1 000 and 3 000 matches (the tests' generator, tests/init_cases.py: about
55 % of the matches become landmarks, the rest end at every other verdict).
  device     the whole call on a device store, and k_init_triangulate (both instances) / k_init_select / k_init_put between HIP
             events;
  host only  the same call on the host-only store, one thread.
Per size the two are timed in alternating runs after a warm-up, `reps` each, in `processes` fresh processes; medians are reported
per process.  Every output and the store read back must be equal bytes across the two stores and across the processes: the
script fails otherwise.  bench.py times none of this.
    python scripts/init_rate.py [--reps 5] [--processes 3] [--out profiles/init_rate.json]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES, CAMS, MAXLM = (300, 1000, 3000), 4, 1 << 15
FIELDS = ("inliers", "verdict", "new_lid", "pt3d", "normal", "dist2", "cos_parallax", "t_out", "lids_prev", "lids_cur")


def digest(lm, res):
    h = hashlib.sha256()
    for f in FIELDS:
        h.update(np.ascontiguousarray(getattr(res, f)).tobytes())
    h.update(np.array([res.parallax, res.median_scene_depth]).tobytes())
    h.update(np.array([res.status, res.n_initial_inliers, res.n_parallax, res.n_triangulated, int(res.scaled), res.next_lid], np.int64).tobytes())
    for lid in res.new_lid[res.new_lid >= 0]:
        p, q, _, _ = lm.get(int(lid))
        h.update(p.tobytes() + q.tobytes() + np.array([lm.observations(int(lid))[0]], np.int64).tobytes())
    return h.hexdigest()


def one_process(reps):
    import init_cases as Ic
    import kfdb_cases
    import mcorb
    out = {}
    for n in SIZES:
        sc = Ic.scene(CAMS, n=n, seed=17)
        lms = {k: mcorb.LocalMap(mcorb.ORBVocabulary(device=d).create(**kfdb_cases.vocabulary()), device=d, max_landmarks=MAXLM, max_candidates=16)
               for k, d in (("device", 0), ("host_only", -1))}
        first = {k: Ic.run_scene(mcorb, lm, sc) for k, lm in lms.items()}       # (also the warm-up)
        dg = {k: digest(lms[k], first[k]) for k in lms}
        assert dg["device"] == dg["host_only"], "the two stores differ at %d matches" % n
        t, kus = {k: [] for k in lms}, []
        for _ in range(reps):                                                   # alternating
            for k, lm in lms.items():
                t0 = time.perf_counter()
                Ic.run_scene(mcorb, lm, sc)
                t[k].append((time.perf_counter() - t0) * 1e3)
                if k == "device":
                    kus.append(lm.last_initialize_timing())
        r = {"matches": n, "flagged": int(sc["flags"].sum()), "landmarks_made": int(first["device"].n_triangulated),
             "status": int(first["device"].status), "digest": dg["device"]}
        for i, name in enumerate(("k_init_triangulate_us", "k_init_select_us", "k_init_put_us")):
            r[name] = round(float(np.median([u[i] for u in kus])), 1)
        for k in lms:
            r[k + "_call_ms"] = round(float(np.median(t[k])), 3)
            r[k + "_call_ms_min_max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
        out[str(n)] = r
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(one_process(a.reps)))
        sys.exit(0)
    runs = []
    for _ in range(a.processes):                                                # fresh processes, one after another
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.exit("a child failed:\n" + p.stderr[-2000:])
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    for n in SIZES:
        assert len({r[str(n)]["digest"] for r in runs}) == 1, "the processes differ at %d matches" % n
    res = {"cores": len(os.sched_getaffinity(0)), "cameras": CAMS, "reps": a.reps, "k_init_select_form": "radix select over the keys, one workgroup",
           "equal_bytes_across_stores_and_processes": True, "processes": runs}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
