// mcorb_landmark.h -- the arithmetic of a landmark's life after it was made: Landmark::updateNormal(frame, featInd)
// (MCSlam/src/GlobalMap.cpp:37-74, through the constructor :6-14 and addLfFrame :24-29) and GlobalMap::updateLandmark (:162-185),
// written in the reference's operation order.  No HIP dependency: the host-only store (mcorb_landmark.cpp), k_lmap_observe and
// k_lmap_update (mcorb_landmark_gpu.hip) and the new landmark's two addLfFrame steps in mcorb_mapping.h run the same code.
// Compile with -ffp-contract=off (the library's flag): every product, sum, division and sqrt below is one IEEE operation in the
// order written, so the device and the host agree bit for bit.
//
//   rays (:42-55)          over the cameras ascending with matchIndex != -1, from 0.0: normal_cur = pt3D - c, then
//                          normal + normal_cur / cv::norm(normal_cur); cv::norm adds three squares in order and takes the sqrt, the
//                          division by a scalar is cv::MatExpr's multiplication by the reciprocal
//   KFs.size() == 1 (:58)  normal = rays / n (a multiplication by 1.0 / n), n_rays = n
//   otherwise (:62-67)     normal = normal * n_rays + rays, n_rays += n, normal = normal / n_rays (by the reciprocal again)
//   updateLandmark         diff = pt3D - point_new, diff_norm = cv::norm(diff); the point is replaced iff diff_norm < max_diff
//                          (5.0 in the reference), so that a NaN stores nothing
// A NaN that reaches a normal (a landmark at a camera centre: 0 * inf) keeps the sign and payload the machine gives it; only
// diff_norm, which is returned, is made the default quiet NaN.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MCORB_LM_HD __host__ __device__
#else
#define MCORB_LM_HD
#endif

#ifndef MCORB_MAX_CAMS
#define MCORB_MAX_CAMS 16   // (include/mcorb.h)
#endif

namespace mcorb {

// acc = acc + (pt - centre) * (1.0 / cv::norm(pt - centre))
MCORB_LM_HD inline void lm_ray_add(const double pt[3], const double centre[3], double acc[3])
{
    double d[3], sq = 0.0;
    for (int k = 0; k < 3; k++) d[k] = pt[k] - centre[k];
    for (int k = 0; k < 3; k++) sq += d[k] * d[k];
    const double inv = 1.0 / sqrt(sq);
    for (int k = 0; k < 3; k++) acc[k] = acc[k] + d[k] * inv;
}

// the constructor's updateNormal: KFs.size() == 1
MCORB_LM_HD inline void lm_normal_first(const double acc[3], int n, double normal[3], int32_t &n_rays)
{
    const double inv = 1.0 / (double)n;
    for (int k = 0; k < 3; k++) normal[k] = acc[k] * inv;
    n_rays = n;
}

// addLfFrame's updateNormal: KFs.size() > 1
MCORB_LM_HD inline void lm_normal_add(const double acc[3], int n, double normal[3], int32_t &n_rays)
{
    for (int k = 0; k < 3; k++) normal[k] = normal[k] * (double)n_rays + acc[k];
    n_rays += n;
    const double inv = 1.0 / (double)n_rays;
    for (int k = 0; k < 3; k++) normal[k] = normal[k] * inv;
}

// one item of mcorb_lmap_observe as a lane sees it: the slot, the cameras that see the feature (bits 0 .. MCORB_MAX_CAMS - 1) and
// kLmFirst when this is the landmark's first observation
constexpr uint32_t kLmFirst = 1u << 31;
struct LmObsItem { int32_t lid; uint32_t mask; };
// W_T_cur's translation per camera of the observing keyframe: uniform for a launch
struct LmCentres { double c[MCORB_MAX_CAMS][3]; };

MCORB_LM_HD inline void lm_observe(const LmCentres &cen, int ncams, uint32_t mask, const double pt[3], double normal[3], int32_t &n_rays)
{
    double acc[3] = {0.0, 0.0, 0.0};
    int n = 0;
    for (int c = 0; c < ncams; c++) {
        if (!((mask >> c) & 1u)) continue;
        lm_ray_add(pt, cen.c[c], acc);
        n++;
    }
    if (mask & kLmFirst) lm_normal_first(acc, n, normal, n_rays);
    else lm_normal_add(acc, n, normal, n_rays);
}

// IEEE 754 leaves the sign and payload of a NaN result to the implementation, and the host's sqrtsd and the device's sqrt
// expansion differ in the sign: a NaN that is returned to the caller becomes the default quiet NaN, 0x7ff8000000000000, on both.
// On the bits: a compiler may drop `x != x ? NaN : x` as a no-op
MCORB_LM_HD inline double lm_default_nan(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof(b));
    if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
    __builtin_memcpy(&x, &b, sizeof(b));
    return x;
}

// one item of mcorb_lmap_update_points: the slot, the item's place in the caller's arrays, the new point
struct LmUpdItem { int32_t lid, idx; double p[3]; };
struct LmUpdOut { double diff_norm; int32_t updated, pad; };

// updateLandmark: true (and pt replaced) iff cv::norm(pt - p) < max_diff
MCORB_LM_HD inline bool lm_update(double pt[3], const double p[3], double max_diff, double &diff_norm)
{
    double d[3], sq = 0.0;
    for (int k = 0; k < 3; k++) d[k] = pt[k] - p[k];
    for (int k = 0; k < 3; k++) sq += d[k] * d[k];
    diff_norm = sqrt(sq);
    diff_norm = lm_default_nan(diff_norm);
    if (diff_norm < max_diff) {
        for (int k = 0; k < 3; k++) pt[k] = p[k];
        return true;
    }
    return false;
}

}  // namespace mcorb
