"""A plain-Python restatement of what the local map computes (mcorb_lmap_search): FrontEnd::searchLocalMap2 from the candidate
landmarks to the camera-filtered matches (MCSlam/src/FrontEnd.cpp:4953-5171, without the fbow block), next to kfdb_probe_ref.py.

* candidates (:4990-4998): the neighbouring keyframes' lIds in order, without -1, without what was seen before in the walk
  (lmSet) and without the members of matchedlmset -- Python sets, where the library stamps slots;
* the frustum test (:5000-5027) in Python floats, which are fp64 and round every operation: a matrix product is, per element, the
  sum over k ascending from 0.0 of a[k] * b[k], then the addend; normal.dot and cv::norm add their three terms in order;
  `tmp / tmp_z` is tmp * (1.0 / tmp_z), as cv::MatExpr evaluates a division by a scalar; math.sqrt is correctly rounded.  The
  comparisons have the reference's form, so a NaN fails none of them;
* transform() of the accepted descriptors through the oracle's DBoW2 restatement (oracle_lib.bow_transform), FeatureVectors as dicts;
* InterMatchingBow (:3791-3845): oracle_lib.get_matches_dist_ratio per shared node in ascending node id, outputs appended;
* the filter by viewing camera (:5122-5171)."""
import math

import numpy as np

import oracle_lib as O

Z_GATE, NORMAL_GATE, BOUNDS_GATE, SEEN = "z", "normal", "bounds", "seen"


def _div(a, b):
    """IEEE division of Python floats (Python raises where C++ gives inf / NaN)"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _mul(a, b):
    return a * b       # (Python floats: one rounding; 0.0 * inf is NaN without an exception)


def mat_vec(A, b, c=None):
    out = []
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += _mul(A[r][k], b[k])
        out.append(s + c[r] if c is not None else s)
    return out


def camera_verdict(view, cam, pt, normal):
    """where one (landmark, camera) pair ends: the gate that drops it, or SEEN"""
    body = mat_vec(view["Rcw"], pt, view["tcw"])
    pc = mat_vec(cam["R"], body, cam["t"])
    if pc[2] < 0:
        return Z_GATE
    cur_dir = [pt[k] - cam["centre_w"][k] for k in range(3)]
    dot = 0.0
    for k in range(3):
        dot += normal[k] * cur_dir[k]
    sq = 0.0
    for k in range(3):
        sq += cur_dir[k] * cur_dir[k]
    if dot < 0.5 * math.sqrt(sq):
        return NORMAL_GATE
    tmp = mat_vec(cam["K"], pc)
    scale = _div(1.0, tmp[2])
    x, y = _mul(tmp[0], scale), _mul(tmp[1], scale)
    if x < 30 or x > (view["width"] - 30):
        return BOUNDS_GATE
    if y < 30 or y > (view["height"] - 30):
        return BOUNDS_GATE
    return SEEN


def cull(view, pt, normal):
    """-> the camera bit mask of one landmark (lm_projected_cam_ids)"""
    pt, normal = [float(v) for v in pt], [float(v) for v in normal]
    mask = 0
    for c, cam in enumerate(view["cams"]):
        if camera_verdict(view, cam, pt, normal) == SEEN:
            mask |= 1 << c
    return mask


def candidates(neighbour_lids, matched_lids):
    seen, matched, out = set(), set(int(l) for l in matched_lids), []
    for l in neighbour_lids:
        l = int(l)
        if l == -1 or l in seen or l in matched:
            continue
        seen.add(l)
        out.append(l)
    return out


def search(view, store, neighbour_lids, matched_lids, vocab, probe_fv, probe_desc, matched_cur, mono_cur, cam_cur, levelsup, ratio=0.85):
    """store: {lid: (pt3D, normal, descriptor, mono)} -> dict(new_lids, cam_masks, ind1, ind2, matches, fv)"""
    new_lids, masks = [], []
    for l in candidates(neighbour_lids, matched_lids):
        m = cull(view, store[l][0], store[l][1])
        if m:
            new_lids.append(l)
            masks.append(m)
    A = np.array([store[l][2] for l in new_lids], np.uint8).reshape(-1, 32)
    _, fa = O.bow_transform(vocab, A, levelsup)
    fb = {int(k): [int(i) for i in f] for k, f in probe_fv.items()}
    ind1, ind2 = [], []
    for node in sorted(set(fa) & set(fb)):
        mA, mB, _ = O.get_matches_dist_ratio(A, fa[node], probe_desc, fb[node], ratio)
        ind1 += mA.tolist()
        ind2 += mB.tolist()
    matches = []
    for a, b in zip(ind1, ind2):
        if matched_cur[b]:
            continue
        if store[new_lids[a]][3] and mono_cur[b]:
            for cid in [c for c in range(len(view["cams"])) if (masks[a] >> c) & 1]:
                if cid == cam_cur[b]:
                    matches.append((a, b))
    return dict(new_lids=np.array(new_lids, np.int32), cam_masks=np.array(masks, np.uint32), ind1=np.array(ind1, np.uint32),
                ind2=np.array(ind2, np.uint32), matches=np.array(matches, np.int32).reshape(-1, 2), fv=fa)
