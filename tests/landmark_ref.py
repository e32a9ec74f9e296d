"""A plain-Python restatement of the reference's landmark bookkeeping, written from MCSlam/src/GlobalMap.cpp and independently of
csrc/mcorb_landmark.h: the Landmark constructor (:6-14), Landmark::addLfFrame (:24-29), Landmark::updateNormal(frame, featInd)
(:37-74), GlobalMap::deleteLandmark (:151-160), GlobalMap::updateLandmark (:162-185) and the keys of searchLocalMap2's kfMap
(FrontEnd.cpp:4925-4933).  Python floats are IEEE doubles, math.sqrt is correctly rounded and nothing is fused, so with every
cv::Mat `/ scalar` written as a multiplication by the reciprocal (cv::MatExpr's rule) the results are the library's bit for bit.

A frame is dict(kf_id, match_index = [[..ncams..], ..nfeat..], centres = [[x, y, z], ..ncams..]): centres[ii] is the translation
column of W_T_cur = pose * cur_T_ref.inv() for camera ii, which the caller of the library computes too."""
import math


def cv_norm(d):
    return math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


class Landmark:
    def __init__(self, pt3D, normal=(0.0, 0.0, 0.0), n_rays=0, mono=False):
        self.pt3D, self.normal, self.n_rays, self.mono = [float(x) for x in pt3D], [float(x) for x in normal], int(n_rays), mono
        self.KFs, self.featInds = [], []

    def update_normal(self, lf_frame, featInd):
        """:37-74"""
        normal = [0.0, 0.0, 0.0]
        n_rays = 0
        ii = 0
        for ind in lf_frame["match_index"][featInd]:
            if ind != -1:
                c = lf_frame["centres"][ii]
                normal_cur = [self.pt3D[k] - c[k] for k in range(3)]
                inv = 1.0 / cv_norm(normal_cur)
                normal = [normal[k] + normal_cur[k] * inv for k in range(3)]
                n_rays += 1
            ii += 1
        assert len(self.KFs) != 0
        if len(self.KFs) == 1:
            inv = 1.0 / n_rays
            self.normal = [normal[k] * inv for k in range(3)]
            self.n_rays = n_rays
        else:
            self.normal = [self.normal[k] * float(self.n_rays) + normal[k] for k in range(3)]
            self.n_rays = self.n_rays + n_rays
            inv = 1.0 / self.n_rays
            self.normal = [self.normal[k] * inv for k in range(3)]

    def add_lf_frame(self, lf_frame, featInd):
        """:24-29; on a landmark without a frame this is the constructor's push and updateNormal (:9-13)"""
        self.KFs.append(lf_frame["kf_id"])
        self.featInds.append(featInd)
        self.update_normal(lf_frame, featInd)

    def record(self, lf_frame, featInd):
        """the push alone: the normal of a landmark fresh from triangulateMatches holds both of its frames already"""
        self.KFs.append(lf_frame["kf_id"])
        self.featInds.append(featInd)

    def observations(self):
        return list(zip(self.KFs, self.featInds))


class GlobalMap:
    def __init__(self):
        self.mapPoints = {}

    def insert(self, lid, pt3D, normal=(0.0, 0.0, 0.0), n_rays=0):
        self.mapPoints[lid] = Landmark(pt3D, normal, n_rays)

    def observe(self, lf_frame, lids, feats, record=False):
        """a batch of addLfFrame, serially; -> n_rays after every item"""
        out = []
        for lid, feat in zip(lids, feats):
            l = self.mapPoints[int(lid)]
            (l.record if record else l.add_lf_frame)(lf_frame, int(feat))
            out.append(l.n_rays)
        return out

    def update_landmark(self, lid, point_new, max_diff=5.0):
        """:162-185 -> (replaced, diff_norm)"""
        l = self.mapPoints[int(lid)]
        diff_lm = [l.pt3D[k] - float(point_new[k]) for k in range(3)]
        diff_norm = cv_norm(diff_lm)
        if diff_norm < max_diff:
            l.pt3D = [float(x) for x in point_new]
            return True, diff_norm
        return False, diff_norm

    def delete_landmark(self, lid):
        """:151-160 -> the (kf_id, feat) pairs whose lIds entry becomes -1"""
        l = self.mapPoints.pop(int(lid))
        return l.observations()

    def observers(self, lids):
        """kfMap's keys (FrontEnd.cpp:4925-4933): a std::map, so ascending and unique"""
        return sorted({kf for lid in lids for kf in self.mapPoints[int(lid)].KFs})
