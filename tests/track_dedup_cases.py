"""Inputs and helpers of the de-duplication and submit / wait tests of fast tracking (test_gpu_track_dedup.py,
test_gpu_track_async.py, test_track_async_cpu.py): flat scenes (track_cases.flat_view: landmark (x, y, 1) projects to exactly
(x, y)) in which every candidate is put on a chosen keypoint at a chosen Hamming distance, so that which entry of the
de-duplication survives is known by hand; and the comparison of one call on several stores.

A keypoint's descriptor is random (two of them differ in about 128 bits, far beyond any gate used here); a candidate on keypoint k
at distance d carries that descriptor with its first d bits flipped, so it matches k and nothing else."""
import numpy as np

import track_cases as T
import track_ref as R

FAR_XY = (1100.0, 650.0)     # inside the default view, more than 100 px from every keypoint of these scenes


def kp_descs(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def scene(kps, specs, seed=0):
    """kps: [(x, y)]; specs: per candidate None (a query that matches nothing: it sits at FAR_XY), (k, d) (on keypoint k, Hamming
    distance d) or (k, d, (x, y)) (the same from another position) -> (store, keypoint array, descriptors, lids); lid = the
    candidate's index"""
    xy = np.asarray(kps, np.float32).reshape(-1, 2)
    ds = kp_descs(len(xy), seed)
    nobody = T.desc_at(np.zeros(32, np.uint8), 128)
    store = {}
    for j, sp in enumerate(specs):
        if sp is None:
            store[j] = ((FAR_XY[0], FAR_XY[1], 1.0), nobody)
            continue
        k, d = sp[0], sp[1]
        x, y = sp[2] if len(sp) > 2 else (float(xy[k][0]), float(xy[k][1]))
        store[j] = ((float(x), float(y), 1.0), T.desc_at(ds[k], d))
    return store, xy, ds, list(range(len(specs)))


def ordinary(arrays):
    """every coordinate converts to int the way Python and C agree on: finite and inside int's range"""
    return all(bool(np.isfinite(a).all()) and bool((np.abs(a) < 2.0 ** 31).all()) for a in arrays)


def answers(mc, lms, v, store, kps, descs, lids, restate=True, **kw):
    """LocalMap.track of every store of lms (the first is the one under test) on one frame; all equal, bit for bit, and equal to the
    restatement unless restate is False -- the case of keypoint coordinates that are NaN or outside int's range, which
    track_ref cannot convert.  -> (the first store's result as lists, the restatement or None)"""
    xy, ds = T.kp_arrays(kps, descs)
    assert restate == ordinary(xy), "only a case with NaN or out-of-int coordinates goes without the restatement"
    view = T.to_view(mc, v)
    got = [T.as_lists(lm.track(view, xy, ds, lids, **kw)) for lm in lms]
    for g in got[1:]:
        T.same(got[0], g, "the first store against another")
        assert g["n_candidates"] == got[0]["n_candidates"]
    ref = None
    if restate:
        ref = R.track(v, store, [a.tolist() for a in xy], ds, [int(l) for l in lids], **kw)
        T.same(got[0], T.ref_lists(ref, store), "store against the restatement")
    return got[0], ref


def dedup_counts(ref, kps):
    """from the restatement alone: per camera (replacements, rejections) of the serial list"""
    out = []
    for c, (plist, rows) in enumerate(zip(ref["proj"], ref["best"])):
        _, rep, rej = R.dedup([(lid, k, d) for (lid, _, _), (k, d) in zip(plist, rows)], kps[c])
        out.append((rep, rej))
    return out


def shifted_rig(ncams, cols=1280, rows=720, step=25.0):
    """camera c stands step * c to the right of camera 0 and looks the same way: a landmark (X, Y, 1) projects to (X - step * c, Y),
    so the cameras keep unequal numbers of a row of landmarks"""
    return T.view([T.cam(t=(step * c, 0.0, 0.0)) for c in range(ncams)], cols, rows)


def rig_scene(ncams, seed, n_landmarks=60, step=25.0):
    """-> (view, store, kps, descs, lids) on shifted_rig: landmarks in a row from x = 5 on, 9 px apart, every third with a twin on
    the same point (the twin better, equal or worse in turn).  Camera c's keypoints: the projections of every other landmark it
    keeps, with the landmark's descriptor a few bits off -- except camera 1, whose keypoints carry descriptors nobody matches
    (queries, no match), and camera 2, which has no keypoints"""
    rng = np.random.default_rng(seed)
    v = shifted_rig(ncams, step=step)
    base = rng.integers(0, 256, (n_landmarks, 32), dtype=np.uint8)
    store, lids = {}, []
    for i in range(n_landmarks):
        pt = (5.0 + 9.0 * i, 40.0 + (i % 7) * 3.0, 1.0)
        store[len(store)] = (pt, T.desc_at(base[i], 6))
        lids.append(len(store) - 1)
        if i % 3 == 0:
            store[len(store)] = (pt, T.desc_at(base[i], (4, 6, 9)[(i // 3) % 3]))
            lids.append(len(store) - 1)
    kps, descs = [], []
    for c in range(ncams):
        xy, ds = [], []
        if c != 2:
            for i in range(c % 2, n_landmarks, 2):
                x = 5.0 + 9.0 * i - step * c
                if x < 0:
                    continue
                xy.append((x, 40.0 + (i % 7) * 3.0))
                ds.append(rng.integers(0, 256, 32, dtype=np.uint8) if c == 1 else base[i])
        kps.append(np.array(xy, np.float32).reshape(-1, 2))
        descs.append(np.array(ds, np.uint8).reshape(-1, 32))
    return v, store, kps, descs, [-1] + lids + [lids[3], -1]
