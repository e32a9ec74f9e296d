"""What UndistortKeyPoints on the device (mcorb_rig_set_undistortion, k_undistort inside the job) costs, in one process, with
undistortion off and on in alternating blocks (4 cameras 1280x720, 2000 features, realistic radtan coefficients):
  (a) one rig frame at a time as MC-SLAM calls: upload -> extract + match -> keypoint records incl. features_undist on the host,
      median over >= 200 frames per setting;
  (b) batched throughput the way bench.py takes its value: 4 slots x 128 rig frames, inputs resident, frames/s.
    python scripts/undistort_rate.py [--frames 240] [--rounds 6] [--out profiles/undistort_rate.json] [--quick]
k_undistort's own kernel time comes from a separate rocprofv3 --kernel-trace --stats run of this script (--quick)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

C, W, H, N = 4, 1280, 720, 2000
# radtan (k1 k2 p1 p2 [k3]) of typical 720p machine-vision lenses; none passes the reference's zero test
DISTS = [[-0.2873, 0.0912, 0.00031, -0.00047], [-0.3012, 0.1040, -0.00022, 0.00051, -0.0147],
         [-0.2791, 0.0835, 0.00044, 0.00013], [-0.2950, 0.0978, -0.00035, -0.00029, -0.0102]]


def kmat(c):
    f = 0.85 * W + 7.0 * c
    return np.array([[f, 0.0, W / 2 + 2.5 - c], [0.0, f * 1.001, H / 2 - 1.5 + c], [0.0, 0.0, 1.0]])


def set_on(rig, on):
    for c in range(C):
        if on:
            rig.set_undistortion(c, kmat(c), DISTS[c])
        else:
            rig.set_undistortion(c)


def one_frame(mcorb, frames, blocks=4, distinct=8):
    rig = mcorb.Rig(C, W, H, max_frames=1, nslots=1, nfeatures=N)
    sets = [[mcorb.synth_rig_frame(f, C, c, W, H) for c in range(C)] for f in range(distinct)]
    per = max(1, frames // blocks)
    t = {False: [], True: []}
    k = 0
    for b in range(2 * blocks):
        on = b % 2 == 1
        set_on(rig, on)
        for i in range(per + 10):   # the first 10 of a block (graph re-capture, caches) are not counted
            imgs = sets[k % distinct]
            k += 1
            t0 = time.perf_counter()
            rig.upload(imgs)
            rig.process(1)
            feats = [rig.features(c) for c in range(C)]
            und = [rig.features_undist(c) for c in range(C)]
            tr, _ = rig.tracks(0)
            t1 = time.perf_counter()
            if i >= 10:
                t[on].append(t1 - t0)
    moved = sum(int(not np.array_equal(u["x"], f[1]["x"])) for u, f in zip(und, feats))
    rig.close()
    med = {on: float(np.median(v)) * 1e3 for on, v in t.items()}
    return {"frames_per_setting": len(t[False]), "off_ms": round(med[False], 4), "on_ms": round(med[True], 4),
            "delta_us": round((med[True] - med[False]) * 1e3, 1),
            "off_p95_ms": round(float(np.percentile(t[False], 95)) * 1e3, 4), "on_p95_ms": round(float(np.percentile(t[True], 95)) * 1e3, 4),
            "cameras_moved_last_frame": moved}


def batched(mcorb, rounds, steps=6, slots=4, F=128):
    rig = mcorb.Rig(C, W, H, max_frames=F, nslots=slots, nfeatures=N)
    for s in range(slots):
        rig.upload([mcorb.synth_rig_frame(f + 1000 * s, C, c, W, H) for f in range(F) for c in range(C)], slot=s)
    rate = {False: [], True: []}
    for r in range(2 * rounds):
        on = r % 2 == 1
        set_on(rig, on)
        for s in range(slots):   # warm-up step of the setting
            rig.process_submit(F, slot=s)
        for s in range(slots):
            rig.process_wait(slot=s)
        t0 = time.perf_counter()
        for _ in range(steps):
            for s in range(slots):
                rig.process_submit(F, slot=s)
            for s in range(slots):
                rig.process_wait(slot=s)
        rate[on].append(steps * slots * F / (time.perf_counter() - t0))
    rig.close()
    med = {on: float(np.median(v)) for on, v in rate.items()}
    return {"rounds_per_setting": rounds, "rig_frames_per_round": steps * slots * F, "off_fps": round(med[False], 1),
            "on_fps": round(med[True], 1), "ratio_on_off": round(med[True] / med[False], 4),
            "off_all": [round(v, 1) for v in rate[False]], "on_all": [round(v, 1) for v in rate[True]]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a short run (for the rocprofv3 kernel trace)")
    a = ap.parse_args()
    import mcorb
    if a.quick:
        a.frames, a.rounds = 40, 1
    res = {"config": {"cams": C, "width": W, "height": H, "nfeatures": N, "coefficients": DISTS},
           "one_frame": one_frame(mcorb, a.frames), "batched": batched(mcorb, a.rounds)}
    res["bars"] = {"one_frame_delta_le_10us": res["one_frame"]["delta_us"] <= 10.0,
                   "batched_ratio_ge_0.97": res["batched"]["ratio_on_off"] >= 0.97}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
