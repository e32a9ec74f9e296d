"""What cv::undistort at the hand-off (mcorb_rig_set_image_undistortion, k_remap_u8 behind every upload) costs, in one process,
with rectification off and on for all four cameras in alternating blocks (4 cameras 1280x720, 2000 features):
  (a) one rig frame at a time as MC-SLAM calls: upload -> extract + match -> records on the host, median per setting;
  (b) batched, with the hand-off in front of every batch (the remap belongs to the upload): `slots` slots x F rig frames,
      upload_staged + process per step, rig frames/s;
  (c) --kernel-only N: nothing but N-image uploads with rectification on (for a rocprofv3 --kernel-trace --stats or --pmc run
      of its own: k_remap_u8 alone).
    python scripts/undistort_image_rate.py [--frames 240] [--rounds 5] [--batch 128] [--out profiles/undistort_image_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

C, W, H, N = 4, 1280, 720, 2000
DISTS = [[-0.2873, 0.0912, 0.00031, -0.00047], [-0.3012, 0.1040, -0.00022, 0.00051, -0.0147],
         [-0.2791, 0.0835, 0.00044, 0.00013], [-0.2950, 0.0978, -0.00035, -0.00029, -0.0102]]


def kmat(c):
    f = 0.85 * W + 7.0 * c
    return np.array([[f, 0.0, W / 2 + 2.5 - c], [0.0, f * 1.001, H / 2 - 1.5 + c], [0.0, 0.0, 1.0]])


def set_on(rig, on):
    for c in range(C):
        if on:
            rig.set_image_undistortion(c, kmat(c), DISTS[c])
        else:
            rig.set_image_undistortion(c)


def one_frame(mcorb, frames, blocks=4, distinct=8):
    rig = mcorb.Rig(C, W, H, max_frames=1, nslots=1, nfeatures=N)
    sets = [[mcorb.synth_rig_frame(f, C, c, W, H) for c in range(C)] for f in range(distinct)]
    per = max(1, frames // blocks)
    t = {False: [], True: []}
    k = 0
    for b in range(2 * blocks):
        on = b % 2 == 1
        set_on(rig, on)
        for i in range(per + 10):   # the first 10 of a block are not counted
            imgs = sets[k % distinct]
            k += 1
            t0 = time.perf_counter()
            rig.upload(imgs)
            rig.process(1)
            [rig.features(c) for c in range(C)]
            rig.tracks(0)
            t1 = time.perf_counter()
            if i >= 10:
                t[on].append(t1 - t0)
    rig.close()
    med = {on: float(np.median(v)) * 1e3 for on, v in t.items()}
    return {"frames_per_setting": len(t[False]), "off_ms": round(med[False], 4), "on_ms": round(med[True], 4),
            "delta_us": round((med[True] - med[False]) * 1e3, 1)}


def fill_staging(mcorb, rig, slots, F):
    for s in range(slots):
        for m in range(F * C):
            rig.staging(m, slot=s)[:] = mcorb.synth_rig_frame((m // C) % 16 + 100 * s, C, m % C, W, H)


def batched(mcorb, rounds, steps=4, slots=4, F=128):
    rig = mcorb.Rig(C, W, H, max_frames=F, nslots=slots, nfeatures=N)
    fill_staging(mcorb, rig, slots, F)
    rate = {False: [], True: []}

    def step():
        for s in range(slots):
            rig.upload_staged(F * C, slot=s)
            rig.process_submit(F, slot=s)
        for s in range(slots):
            rig.process_wait(slot=s)

    for r in range(2 * rounds):
        on = r % 2 == 1
        set_on(rig, on)
        step()   # warm-up step of the setting
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        rate[on].append(steps * slots * F / (time.perf_counter() - t0))
    rig.close()
    med = {on: float(np.median(v)) for on, v in rate.items()}
    ms = {on: 1e3 * slots * F / med[on] for on in med}   # per step of `slots` batches
    return {"rounds_per_setting": rounds, "slots": slots, "frames_per_batch": F, "off_fps": round(med[False], 1), "on_fps": round(med[True], 1),
            "ratio_on_off": round(med[True] / med[False], 4), "added_ms_per_batch": round((ms[True] - ms[False]) / slots, 4),
            "off_all": [round(v, 1) for v in rate[False]], "on_all": [round(v, 1) for v in rate[True]]}


def kernel_only(mcorb, nimg, reps=12):
    F = nimg // C
    rig = mcorb.Rig(C, W, H, max_frames=F, nslots=1, nfeatures=N)
    fill_staging(mcorb, rig, 1, F)
    set_on(rig, True)
    for _ in range(reps):
        rig.upload_staged(nimg)
    rig.level(0, 0)   # drains the stream
    rig.close()
    return {"images_per_launch": nimg, "launches": reps, "algorithmic_bytes_per_launch": 2 * W * H * nimg + 6 * W * H * C}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128, help="rig frames per batch of the batched leg")
    ap.add_argument("--kernel-only", type=int, default=0, metavar="NIMG")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mcorb
    if a.kernel_only:
        res = {"kernel_only": kernel_only(mcorb, a.kernel_only)}
    else:
        res = {"config": {"cams": C, "width": W, "height": H, "nfeatures": N, "coefficients": DISTS},
               "one_frame": one_frame(mcorb, a.frames), "batched": batched(mcorb, a.rounds, F=a.batch)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
