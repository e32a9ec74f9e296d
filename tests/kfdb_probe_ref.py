"""A plain-Python restatement of what the keyframe database's probe slots compute (mcorb_kfdb_*probe*), next to kfdb_ref.py:

* a probe is a frame held beside the database: query / score are RefDatabase's on the probe's vectors, and nothing is added;
* FrontEnd::InterMatchingBow (FrontEnd.cpp:3676-3788) / Relocalization::featureMatchesBow (relocalization.cpp:327-371): for every
  FeatureVector node the entry (A) and the probe (B) share, in ascending node id, oracle_lib.get_matches_dist_ratio(A, B), outputs
  appended -- over dict FeatureVectors, so the lower_bound walk of the library has nothing to share with it;
* FrontEnd::findInterMatches (FrontEnd.cpp:3344-3499) line by line: knnMatch(k = 2) by brute force, the lowest train index first
  among equal distances, then the ratio gate, the depth gate and the uniqueness on trainIdx.

Python floats are fp64 and `a*a + b*b + c*c` adds left to right; DMatch::distance is a float holding an integer, so
float(d0) > 0.7 * float(d1) is the reference's comparison; cv::norm's result is narrowed to float before `<= 2.0`."""
import math

import numpy as np

import oracle_lib as O
from kfdb_ref import RefDatabase


class RefProbes:
    """probe slots beside a RefDatabase"""

    def __init__(self, ref):
        self.ref = ref
        self.slots = {}

    def set_probe(self, p, bow, fv, desc):
        self.slots[p] = ([int(w) for w in bow[0]], [float(v) for v in bow[1]], {int(k): [int(i) for i in f] for k, f in fv.items()},
                         np.ascontiguousarray(desc, np.uint8).reshape(-1, 32))

    def query_full(self, p, max_id=-1):
        return self.ref.query_full(self.slots[p][:2], max_id)

    def score(self, entry, p):
        """score(entry's vector, probe's): the sum runs over the second vector's words, ascending"""
        da = dict(zip(*self.ref.entries[entry][:2]))
        s = 0.0
        for w, v in zip(*self.slots[p][:2]):
            if w in da:
                s += abs(da[w] - v) - abs(da[w]) - abs(v)
        return -s / 2.0

    def feature_matches(self, entry, p, ratio=0.85):
        fa, A = self.ref.entries[entry][2:]
        fb, B = self.slots[p][2:]
        i1, i2 = [], []
        for node in sorted(set(fa) & set(fb)):
            mA, mB, _ = O.get_matches_dist_ratio(A, fa[node], B, fb[node], ratio)
            i1 += mA.tolist()
            i2 += mB.tolist()
        return np.array(i1, np.uint32), np.array(i2, np.uint32)


def knn_match2(descs1, descs2):
    """BFMatcher(NORM_HAMMING).knnMatch(descs1, descs2, 2): per query the up to two nearest (trainIdx, distance), nearest first,
    the lower train index first among equal distances"""
    a = np.unpackbits(np.ascontiguousarray(descs1, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    b = np.unpackbits(np.ascontiguousarray(descs2, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    out = []
    for row in a:
        d = np.abs(b - row).sum(axis=1) if len(b) else np.zeros(0, np.int32)
        order = np.argsort(d, kind="stable")[:2]
        out.append([(int(t), int(d[t])) for t in order])
    return out


def inter_matches_bf(descs_prev, descs_cur, lids_prev, mono_prev, p3d_prev, mono_cur, p3d_cur):
    """findInterMatches -> matches_z_filtered as (queryIdx, trainIdx, distance) arrays.  Where the reference would read m[1] (or
    m[0]) past the end of a short row -- a probe of fewer than two features -- the row is dropped unless it is a landmark's."""
    inds1, inds2, dist = [], [], []
    for q, m in enumerate(knn_match2(descs_prev, descs_cur)):
        if not m:
            continue
        if lids_prev[q] != -1:
            pass                                            # a landmark is used as it is
        else:
            if len(m) < 2:
                continue
            if float(m[0][1]) > 0.7 * float(m[1][1]):
                continue
        t = m[0][0]
        if not mono_prev[q] and not mono_cur[t]:
            dx, dy, dz = (float(p3d_prev[q][i]) - float(p3d_cur[t][i]) for i in range(3))
            distance = np.float32(math.sqrt(dx * dx + dy * dy + dz * dz))
            if not distance <= 2.0:
                continue
        if t not in inds2:
            inds2.append(t)
            inds1.append(q)
            dist.append(m[0][1])
        else:
            k = inds2.index(t)
            if m[0][1] < dist[k]:
                inds1[k] = q
                dist[k] = m[0][1]
    return np.array(inds1, np.int32), np.array(inds2, np.int32), np.array(dist, np.int32)


__all__ = ["RefDatabase", "RefProbes", "knn_match2", "inter_matches_bf"]
