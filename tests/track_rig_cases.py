"""Inputs and helpers of the slot entry of fast tracking (test_gpu_track_rig.py): a rig slot's frame read back as host arrays --
the oracle every case is held against -- and landmarks built from the frame itself.  With the flat view of track_cases (fx = fy =
1, u0 = v0 = 0) a landmark (x, y, 1) made from a keypoint's pt projects to exactly that pt in every camera, so its query sits on
the keypoint it came from."""
import numpy as np

import track_cases as T
import track_ref as R

MARGIN = (400, 300)   # the view is this much larger than the image: room for queries more than 100 px from every keypoint


def slot_frame(rig, frame, slot=0):
    """Rig.features of the images of `frame` -> per camera (keypoint records, image_kps' pt as n x 2 float32, descriptors)"""
    recs, xy, ds = [], [], []
    for c in range(rig.ncams):
        _, k, d = rig.features(frame * rig.ncams + c, slot)
        assert len(k) < rig.kcap                                              # the padding of a row is never a keypoint
        recs.append(k)
        xy.append(np.ascontiguousarray(np.stack([k["x"], k["y"]], axis=1), np.float32).reshape(-1, 2))
        ds.append(np.ascontiguousarray(d, np.uint8).reshape(-1, 32))
    return recs, xy, ds


def view_of(rig):
    return T.flat_view(rig.w + MARGIN[0], rig.h + MARGIN[1], ncams=rig.ncams)


def same_pixel_pairs(rec):
    """pairs of keypoints of different pyramid levels on one level-0 pixel ((int)pt.x, (int)pt.y)"""
    at = {}
    for k in range(len(rec)):
        at.setdefault((int(rec["x"][k]), int(rec["y"][k])), []).append(k)
    return [(g[0], g[1]) for g in at.values() if len(g) > 1 and rec["octave"][g[0]] != rec["octave"][g[1]]]


def landmarks(rng, frames, cols, rows, per_cam=8, twins=4, levels=2):
    """frames: slot_frame results -> (store, lids).  Per frame and camera: per_cam keypoints become one landmark each, the
    keypoint's descriptor with 0 .. 12 bits flipped; `twins` keypoints become two landmarks each, the later with fewer flipped bits
    (a replacement), as many (a rejection) or more (a rejection); `levels` pairs of keypoints of different pyramid levels on one
    level-0 pixel become one landmark each, which the de-duplication treats as one keypoint.  Then landmarks behind the rig, outside
    the view, and inside the view more than 100 px from every keypoint.  lids: every landmark in that order, so a twin's second
    landmark is the later query, with -1 and repeats mixed in."""
    store = {}

    def add(pt, desc, z=1.0):
        store[len(store)] = ((float(pt[0]), float(pt[1]), z), np.asarray(desc, np.uint8))

    flips = [(9, 3), (4, 4), (2, 8), (12, 0), (0, 0), (6, 7)]
    for recs, xy, ds in frames:
        for c in range(len(xy)):
            n = len(xy[c])
            order = rng.permutation(n)
            for k in order[:per_cam]:
                add(xy[c][k], T.desc_at(ds[c][k], int(rng.integers(0, 13)), rng))
            for j, k in enumerate(order[per_cam:per_cam + twins]):
                a, b = flips[j % len(flips)]
                add(xy[c][k], T.desc_at(ds[c][k], a, rng))
                add(xy[c][k], T.desc_at(ds[c][k], b, rng))
            for j, (k1, k2) in enumerate(same_pixel_pairs(recs[c])[:levels]):
                a, b = flips[j % len(flips)]
                add(xy[c][k1], T.desc_at(ds[c][k1], a, rng))
                add(xy[c][k2], T.desc_at(ds[c][k2], b, rng))
    some = store[0][1] if store else np.zeros(32, np.uint8)
    for j in range(4):
        add((20.0 + 30 * j, 25.0), some, z=-1.0)                              # behind the rig
        add((-5.0 - j, 30.0) if j % 2 else (cols + MARGIN[0] + 1.0 + j, 30.0), some)   # outside the view
        add((cols + MARGIN[0] - 40.0 - j, rows + MARGIN[1] - 30.0), some)     # in the view, no keypoint within 100 px
    lids = list(range(len(store)))
    return store, [-1] + lids[:5] + lids + [lids[len(lids) // 2], -1, lids[0]]


def restated(v, store, xy, ds, lids, **kw):
    return R.track(v, store, [a.tolist() for a in xy], ds, [int(l) for l in lids], **kw)


def assert_not_vacuous(ref, xy):
    """from the restatement alone: every camera that has keypoints has a match; a replacement, a rejection, a query with more than
    10 keypoints in radius and a query with none"""
    for c, a in enumerate(xy):
        assert not len(a) or len(ref["matches"][c]) >= 1, "camera %d has keypoints and no match" % c
    s = ref["stats"]
    assert s["replaced"] >= 1 and s["rejected"] >= 1 and s["crowded"] >= 1 and s["empty"] >= 1, s
