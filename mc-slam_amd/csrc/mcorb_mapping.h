// mcorb_mapping.h -- the arithmetic of one inter-frame match of FrontEnd::triangulateMatches (MCSlam/src/FrontEnd.cpp:5826-5933)
// and of Landmark::updateNormal (GlobalMap.cpp:37-74) for the two addLfFrame steps of a fresh landmark (:5935-5937), written in
// the reference's operation order.  No HIP dependency: the host-only store (mcorb_mapping.cpp), k_map_triangulate
// (mcorb_mapping_gpu.hip) and a plain g++ program include the same code.  Compile with -ffp-contract=off (the library's flag):
// every product, sum, division and sqrt below is one IEEE operation in the order written, in the type written, so the device and
// the host agree bit for bit.
//
// Per match, in order:
//   views (get3D_2DCorrs, :2454-2479)   cameras ascending with matchIndex != -1, first the neighbour's, then the current frame's;
//                                       x = (pt.x - K02) / K00, y = (pt.y - K12) / K11 in double from the float pt, true divisions;
//                                       P = rows 0..2 of that camera's cur_T_W; kps (float) and octave kept
//   camera centres (:5835, :5838)       o = -1 * R^T * t of the first neighbour view (o1) and of the first current view (o2): per
//                                       element the sum over k ascending, from 0.0, of R[k][i] * t[k], then negated
//   epipolar gate (:5848-5870)          a, b, c in double from float * double products added left to right, then rounded to
//                                       float; num = a * x2 + b * y2 + c and den = a * a + b * b in float, each operation rounded
//                                       on its own; den == 0 rejects; num * num / den (float) >= 4.0 (after promotion) rejects
//   triangulation (:5881)               cv::sfm::triangulatePoints = mcorb::triangulate (mcorb_triangulate.h), unpinned, 1e-9
//   per view (:5885-5913)               p = P[:, :3] * X + P[:, 3] in cv::Mat's order (sum over k from 0.0, then the addend);
//                                       p.z < 0 rejects; q = K * p; ex = q0 / q2, ey = q1 / q2 (plain doubles: true divisions);
//                                       err = (ex - kx) * (ex - kx) + (ey - ky) * (ey - ky), then err * invSigma2[octave] (a
//                                       float promoted); err > 5.991 rejects
//   parallax (:5918-5926)               n1 = X - o1, n2 = X - o2; cv::norm and Mat::dot add three terms in order; cos = dot /
//                                       (dist1 * dist2); a landmark is made only when cos < 0.99998 && cos > 0.5
//   normal (GlobalMap.cpp:37-74)        updateNormal(neighbour) with KFs.size() == 1, then updateNormal(current) with size 2; each
//                                       normal_cur / cv::norm(normal_cur) and each / n_rays is a multiplication by the reciprocal
//                                       (cv::MatExpr's rule for a division by a scalar)
// The comparisons keep the reference's form, so that a NaN falls where it falls there: a NaN z is not "behind", a NaN err passes,
// a NaN cos makes no landmark.  A match that passes every reject gate but fails the parallax window (a NaN cos included) keeps
// inliers[i] == true in the reference although no landmark is made: verdict kMapParallax is an inlier.
#pragma once
#include "mcorb_landmark.h"
#include "mcorb_triangulate.h"

namespace mcorb {

// how a match ends; 0 .. 5 are decided by the arithmetic here, 6 and 7 by the serial walk (mcorb_mapping.cpp)
enum MapVerdict {
    kMapLandmark = 0,     // a new landmark
    kMapEpiZero = 1,      // epipolar line with den == 0
    kMapEpiDist = 2,      // epipolar distance
    kMapBehind = 3,       // behind a camera
    kMapChi2 = 4,         // reprojection error
    kMapParallax = 5,     // outside the parallax window: still an inlier
    kMapAssigned = 6,     // one of the two features has a landmark already
    kMapNeighbourSkipped = 7
};

// the views of one match: [0, nv1) the neighbour's, [nv1, nv) the current frame's
struct MapViews {
    int nv, nv1;
    const double *P[MCORB_MAX_CAMS];        // 3x4 row-major
    const double *K[MCORB_MAX_CAMS];        // 3x3 row-major, the view's camera
    const double *centre[MCORB_MAX_CAMS];   // W_T_cur's translation of the view's camera and frame
    float kx[MCORB_MAX_CAMS], ky[MCORB_MAX_CAMS];
    int octave[MCORB_MAX_CAMS];
};

// what a match leaves behind.  X from verdict 3 on; dist2 and cos for 0 and 5; normal and n_rays for 0; everything else is zero
struct MapOut {
    double X[3], normal[3], dist2, cos;
    int32_t verdict, n_rays;
};

MCORB_TRI_HD inline void map_clear(MapOut &o)
{
    for (int k = 0; k < 3; k++) o.X[k] = o.normal[k] = 0.0;
    o.dist2 = o.cos = 0.0;
    o.verdict = o.n_rays = 0;
}

// the epipolar gate; F = F21 of (camera of the first current view, camera of the first neighbour view)
MCORB_TRI_HD inline int map_epipolar(const MapViews &v, const double *F)
{
    const double x1 = (double)v.kx[0], y1 = (double)v.ky[0];
    const float a = (float)(x1 * F[0] + y1 * F[1] + F[2]);
    const float b = (float)(x1 * F[3] + y1 * F[4] + F[5]);
    const float c = (float)(x1 * F[6] + y1 * F[7] + F[8]);
    const float num = a * v.kx[v.nv1] + b * v.ky[v.nv1] + c;
    const float den = a * a + b * b;
    if (den == 0) return kMapEpiZero;
    const float d = num * num / den;
    if ((double)d >= 4.0) return kMapEpiDist;
    return kMapLandmark;
}

// o = -1 * P[:, :3]^T * P[:, 3]
MCORB_TRI_HD inline void map_centre(const double *P, double o[3])
{
    for (int i = 0; i < 3; i++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s += P[4 * k + i] * P[4 * k + 3];
        o[i] = -s;
    }
}

// the sum of normal_cur / cv::norm(normal_cur) over views [i0, i1) (mcorb_landmark.h has the ray)
MCORB_TRI_HD inline void map_rays(const MapViews &v, int i0, int i1, const double X[3], double acc[3])
{
    acc[0] = acc[1] = acc[2] = 0.0;
    for (int i = i0; i < i1; i++) lm_ray_add(X, v.centre[i], acc);
}

// the per-view gates (:5885-5913; FrontEnd::initialization has the same loop, :2702-2724): 0 when X passes every view, otherwise
// kMapBehind or kMapChi2 of the first view that rejects
MCORB_TRI_HD inline int map_view_gates(const MapViews &v, const double X[3], const float *inv_sigma2)
{
    for (int i = 0; i < v.nv; i++) {
        const double *P = v.P[i], *K = v.K[i];
        double p[3], q[3];
        for (int r = 0; r < 3; r++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += P[4 * r + k] * X[k];
            p[r] = s + P[4 * r + 3];
        }
        if (p[2] < 0) return kMapBehind;
        for (int r = 0; r < 3; r++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += K[3 * r + k] * p[k];
            q[r] = s;
        }
        const double ex = q[0] / q[2], ey = q[1] / q[2];
        const double kx = (double)v.kx[i], ky = (double)v.ky[i];
        double err = (ex - kx) * (ex - kx) + (ey - ky) * (ey - ky);
        err = err * (double)inv_sigma2[v.octave[i]];
        if (err > 5.991) return kMapChi2;
    }
    return kMapLandmark;
}

// the two rays of the parallax tests (:5918-5926; FrontEnd::initialization has the same lines, :2731-2745): n1 = X - o1 and
// n2 = X - o2 from the first view of each frame; dist2 = |n2| and cos = dot / (dist1 * dist2), as they come
MCORB_TRI_HD inline void map_parallax(const MapViews &v, const double X[3], double &dist2, double &cosp)
{
    double o1[3], o2[3], n1[3], n2[3];
    map_centre(v.P[0], o1);
    map_centre(v.P[v.nv1], o2);
    for (int k = 0; k < 3; k++) { n1[k] = X[k] - o1[k]; n2[k] = X[k] - o2[k]; }
    double s1 = 0.0, s2 = 0.0, dot = 0.0;
    for (int k = 0; k < 3; k++) s1 += n1[k] * n1[k];
    for (int k = 0; k < 3; k++) s2 += n2[k] * n2[k];
    for (int k = 0; k < 3; k++) dot += n1[k] * n2[k];
    const double dist1 = sqrt(s1);
    dist2 = sqrt(s2);
    cosp = dot / (dist1 * dist2);
}

// a new landmark's normal and ray count: Landmark(pt3d, prev_kf, ..) -- KFs.size() == 1, normal = rays / n_rays -- over views
// [0, nv1), then addLfFrame(currentFrame, ..) -- size 2, normal = (normal * n_rays + rays) / (n_rays + rays') -- over [nv1, nv)
MCORB_TRI_HD inline void map_new_normal(const MapViews &v, const double X[3], double normal[3], int32_t &n_rays)
{
    double acc[3];
    map_rays(v, 0, v.nv1, X, acc);
    lm_normal_first(acc, v.nv1, normal, n_rays);
    map_rays(v, v.nv1, v.nv, X, acc);
    lm_normal_add(acc, v.nv - v.nv1, normal, n_rays);
}

// everything after the triangulation: the per-view gates, the parallax window, the normal of the new landmark.  Doubles that
// leave the record go through lm_default_nan, as mcorb_mapping_new.h's and mcorb_init.h's do: the host and the device give a NaN
// different signs
MCORB_TRI_HD inline void map_after(const MapViews &v, const double X[3], const float *inv_sigma2, MapOut &o)
{
    for (int k = 0; k < 3; k++) o.X[k] = lm_default_nan(X[k]);
    const int gate = map_view_gates(v, X, inv_sigma2);
    if (gate != kMapLandmark) { o.verdict = gate; return; }
    double dist2, cosp;
    map_parallax(v, X, dist2, cosp);
    o.dist2 = lm_default_nan(dist2);
    o.cos = lm_default_nan(cosp);
    if (!(cosp < 0.99998 && cosp > 0.5)) { o.verdict = kMapParallax; return; }
    map_new_normal(v, X, o.normal, o.n_rays);
    for (int k = 0; k < 3; k++) o.normal[k] = lm_default_nan(o.normal[k]);
    o.verdict = kMapLandmark;
}

// the DLT of a match's views (:5881): x = (pt.x - K02) / K00, y = (pt.y - K12) / K11, then mcorb::triangulate.  kAnyViews = false:
// nv <= 4 only, as triangulate<false>
template <bool kAnyViews>
MCORB_TRI_HD inline void map_dlt(const MapViews &v, double X[3])
{
    double xx[2 * MCORB_MAX_CAMS];
    for (int i = 0; i < v.nv; i++) {
        const double *K = v.K[i];
        xx[2 * i] = ((double)v.kx[i] - K[2]) / K[0];
        xx[2 * i + 1] = ((double)v.ky[i] - K[5]) / K[4];
    }
    triangulate<kAnyViews>(xx, v.P, v.nv, X);
}

// one match from the epipolar gate to the normal
template <bool kAnyViews>
MCORB_TRI_HD inline void map_match(const MapViews &v, const double *F, const float *inv_sigma2, MapOut &o)
{
    map_clear(o);
    o.verdict = map_epipolar(v, F);
    if (o.verdict != kMapLandmark) return;
    double X[3];
    map_dlt<kAnyViews>(v, X);
    map_after(v, X, inv_sigma2, o);
}

// ---- the packed observations of a call: one block of memory, the same on the host and in HBM ----
struct MapKp { float x, y; int32_t octave; };
struct MapFrameDev {            // one keyframe
    double proj[MCORB_MAX_CAMS][12];
    double centre[MCORB_MAX_CAMS][3];
    int32_t kp_off[MCORB_MAX_CAMS];   // the camera's first keypoint in the MapKp pool
    int32_t mi_off, pad;              // the frame's match_index (nfeat x ncams) in the int pool
};
struct MapItem { int32_t q, t, rec; };           // neighbour feature, current feature, output record
constexpr int kMapBlock = 64;                    // the lanes of a workgroup of the block kernels: one wave
struct MapBlock { int32_t seg, first, count; };  // one wave: neighbour, first item, items (<= kMapBlock)

struct MapArgs {
    const MapFrameDev *frames;   // [0] the current frame, [1 + s] neighbour s
    const int32_t *mi;
    const MapKp *kp;
    const double *F;             // per neighbour ncams x ncams x 9, [c_cur][c_neigh]
    const double *K;             // ncams x 9
    const float *inv_sigma2;
    const MapBlock *blocks;
    const MapItem *items;
    MapOut *out;
    int32_t ncams;
};

// the views of feature `feat` of a frame appended to v (cameras ascending); returns the camera of the first one
MCORB_TRI_HD inline int map_gather(const MapArgs &a, const MapFrameDev &f, int feat, MapViews &v)
{
    int first = -1;
    const int32_t *row = a.mi + f.mi_off + (size_t)feat * a.ncams;
    for (int c = 0; c < a.ncams; c++) {
        const int ind = row[c];
        if (ind == -1) continue;
        const MapKp kp = a.kp[f.kp_off[c] + ind];
        const int i = v.nv++;
        v.P[i] = f.proj[c];
        v.K[i] = a.K + 9 * c;
        v.centre[i] = f.centre[c];
        v.kx[i] = kp.x; v.ky[i] = kp.y; v.octave[i] = kp.octave;
        if (first < 0) first = c;
    }
    return first;
}

// the views of a match of feature q of frames[1] (the previous keyframe, prev) with feature t of frames[0] (the current frame)
MCORB_TRI_HD inline void map_gather_pair(const MapArgs &a, int q, int t, MapViews &v)
{
    v.nv = 0;
    map_gather(a, a.frames[1], q, v);
    v.nv1 = v.nv;
    map_gather(a, a.frames[0], t, v);
}

template <bool kAnyViews>
MCORB_TRI_HD inline void map_item(const MapArgs &a, int seg, const MapItem &it)
{
    MapViews v;
    v.nv = 0;
    const int c_neigh = map_gather(a, a.frames[1 + seg], it.q, v);
    v.nv1 = v.nv;
    const int c_cur = map_gather(a, a.frames[0], it.t, v);
    const double *F = a.F + ((size_t)seg * a.ncams * a.ncams + (size_t)c_cur * a.ncams + c_neigh) * 9;
    MapOut o;
    map_match<kAnyViews>(v, F, a.inv_sigma2, o);
    a.out[it.rec] = o;
}

#ifdef __HIPCC__
// the block kernels (k_map_triangulate, k_map_refine_new, k_init_triangulate): the wave's block record; false for a lane without
// an item, whose item is otherwise a.items[b.first + threadIdx.x]
__device__ inline bool map_lane(const MapArgs &a, int block0, MapBlock &b)
{
    b = a.blocks[block0 + blockIdx.x];
    return (int)threadIdx.x < b.count;
}
#endif

// the cases of the test hooks (mcorb_host_* / mcorb_dev_*_selftest of the gates, of map_refine and of the initialization):
// everything but the triangulation for caller-given points, views and constants.  Case i has nv[i] views, the first nv1[i] the
// neighbour's (the previous keyframe's), starting at view voff[i]
struct MapCases {
    const double *X;            // 3 per case
    const int32_t *nv1, *nv, *voff;
    const double *P, *K, *centre;   // 12, 9, 3 per view
    const float *kps;           // 2 per view
    const int32_t *octave;      // per view
    const float *inv_sigma2;
};
struct MapGateCases : MapCases { const double *F; };   // 9 per case

MCORB_TRI_HD inline void map_case_views(const MapCases &c, int i, MapViews &v)
{
    v.nv = c.nv[i];
    v.nv1 = c.nv1[i];
    for (int j = 0; j < v.nv; j++) {
        const size_t w = (size_t)c.voff[i] + j;
        v.P[j] = c.P + 12 * w;
        v.K[j] = c.K + 9 * w;
        v.centre[j] = c.centre + 3 * w;
        v.kx[j] = c.kps[2 * w]; v.ky[j] = c.kps[2 * w + 1];
        v.octave[j] = c.octave[w];
    }
}

MCORB_TRI_HD inline void map_gate_case(const MapGateCases &c, int i, MapOut &o)
{
    MapViews v;
    map_case_views(c, i, v);
    map_clear(o);
    o.verdict = map_epipolar(v, c.F + 9 * (size_t)i);
    if (o.verdict == kMapLandmark) map_after(v, c.X + 3 * (size_t)i, c.inv_sigma2, o);
}

// getSceneDepthStats' z (:4846-4847): row 2 of Rcw * pt3D + tcw
MCORB_TRI_HD inline double map_depth(const double Rcw[9], const double tcw[3], const double *pt)
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += Rcw[6 + k] * pt[k];
    return s + tcw[2];
}

}  // namespace mcorb
