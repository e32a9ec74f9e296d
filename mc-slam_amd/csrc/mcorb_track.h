// mcorb_track.h -- the arithmetic of fast tracking: Tracking::project_ (MCSlam/src/Tracking.cpp:208-260) and the per-query part of
// Tracking::querryEachFrame (:329-377), written in the reference's operation order.  No HIP dependency: the host-only store
// (mcorb_track.cpp), k_track_project and k_track_match (mcorb_track_gpu.hip) run the same code.  Compile with -ffp-contract=off
// (the library's flag): every product, sum, difference, 1.0 / z and conversion below is one IEEE operation in the order written,
// so the device and the host agree bit for bit.
//
//   project_ (:222-228)    point3 = c0_T_w.transformFrom(X): R0 * X + t0; project2 per camera: pose.transformTo(point3) =
//                          R^T * (point3 - t), CheiralityException for z <= 0 (the landmark leaves every camera), the intrinsic
//                          coordinates (x / z, y / z) through the reciprocal, Cal3_S2::uncalibrate: fx * u + s * v + u0,
//                          fy * v + v0.  gtsam is not vendored: this is its 4.x arithmetic as recalled
//   the bounds (:234-245)  the float casts, then x < 0 || x > imgCols || y < 0 || y > imgRows in float
//   the query (:331-352)   cvflann::L2<double> over the doubles of the float coordinates, the gate dists > 10000
//   the gate (:363-377)    best = 10000, dist < best && dist < 20 over the neighbours in order
#pragma once
#include <stdint.h>

#include "../../include/mcorb.h"

#if defined(__HIPCC__)
#define MCORB_TR_HD __host__ __device__
#else
#define MCORB_TR_HD
#endif

namespace mcorb {

// a float that is returned to the caller: IEEE 754 leaves the sign and payload of a NaN result to the implementation (host and
// device differ in the sign of an invalid operation's), so a NaN becomes the default quiet NaN on both.  On the bits: a compiler
// may drop `x != x ? NaN : x` as a no-op
MCORB_TR_HD inline float tr_default_nan(float x)
{
    uint32_t b;
    __builtin_memcpy(&b, &x, sizeof(b));
    if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;
    __builtin_memcpy(&x, &b, sizeof(b));
    return x;
}

// point3 = c0_T_w.transformFrom(X)
MCORB_TR_HD inline void tr_body(const double R0[9], const double t0[3], const double X[3], double p0[3])
{
    for (int r = 0; r < 3; r++) p0[r] = (R0[3 * r] * X[0] + R0[3 * r + 1] * X[1] + R0[3 * r + 2] * X[2]) + t0[r];
}

// q = pose.transformTo(point3) = R^T * (point3 - t)
MCORB_TR_HD inline void tr_cam(const mcorb_track_cam &cam, const double p0[3], double q[3])
{
    const double d[3] = {p0[0] - cam.t[0], p0[1] - cam.t[1], p0[2] - cam.t[2]};
    for (int r = 0; r < 3; r++) q[r] = cam.R[r] * d[0] + cam.R[3 + r] * d[1] + cam.R[6 + r] * d[2];
}

// false when a camera has the point at z <= 0: project2 throws and the landmark is skipped for the whole rig.  The comparison
// keeps the reference's form, so a NaN z throws nothing
MCORB_TR_HD inline bool tr_in_front(const mcorb_track_view &v, const double p0[3])
{
    for (int c = 0; c < v.ncams; c++) {
        double q[3];
        tr_cam(v.cams[c], p0, q);
        if (q[2] <= 0) return false;
    }
    return true;
}

// the projected keypoint of camera c; false when it is outside the image (both edges and a NaN are kept)
MCORB_TR_HD inline bool tr_pixel(const mcorb_track_view &v, int c, const double p0[3], float &x, float &y)
{
    const mcorb_track_cam &cam = v.cams[c];
    double q[3];
    tr_cam(cam, p0, q);
    const double d = 1.0 / q[2];
    const double pu = q[0] * d, pv = q[1] * d;
    const double px = (cam.fx * pu + cam.s * pv) + cam.u0, py = cam.fy * pv + cam.v0;
    x = tr_default_nan((float)px);
    y = tr_default_nan((float)py);
    return !(x < 0 || x > (float)v.cols || y < 0 || y > (float)v.rows);
}

// A neighbour's place in the total order (d2, k).  d2 is a sum of two squares: never negative, never -0.0, and a NaN is no
// candidate, so its bit pattern orders as the number does; `none` (all ones) is greater than every candidate's key
struct TrKey { uint64_t d2; uint32_t k; };
MCORB_TR_HD inline bool tr_less(uint64_t ad2, uint32_t ak, uint64_t bd2, uint32_t bk) { return ad2 < bd2 || (ad2 == bd2 && ak < bk); }
constexpr uint64_t kTrNoneD2 = ~0ull;
constexpr uint32_t kTrNoneK = ~0u;

// cvflann::L2<double> of the query (x, y) and the keypoint (kx, ky), and whether the keypoint is a candidate
MCORB_TR_HD inline bool tr_d2(float x, float y, float kx, float ky, double max_d2, uint64_t &bits)
{
    const double dx = (double)x - (double)kx, dy = (double)y - (double)ky;
    const double d2 = dx * dx + dy * dy;
    __builtin_memcpy(&bits, &d2, sizeof(bits));
    return !(d2 > max_d2) && d2 == d2;   // the reference's form; a NaN d2 has no place in the order
}

// the descriptor gate over neighbours in order: dist < best && dist < max_hamming, so the least distance and of equal ones the
// earliest rank -- the minimum of dist * 16 + rank over the ranks with dist < max_hamming
constexpr int kTrBest0 = 10000;          // `double best = 10000`: what best_dist holds when nothing was taken
constexpr uint32_t kTrNoGate = ~0u;
MCORB_TR_HD inline uint32_t tr_gate_key(int dist, int rank, int max_hamming)
{
    return dist < max_hamming ? (uint32_t)dist * 16u + (uint32_t)rank : kTrNoGate;
}

// The de-duplication (querryEachFrame:380-415) compares keypoints by their pixel ((int)pt.x, (int)pt.y).  The conversion, defined
// for every float: truncation toward zero for |v| < 2^31, INT32_MIN otherwise, a NaN included (what an x86-64 cvttss2si gives).
// The host tail and k_track_dedup_min share it.  Every 64-bit value is the key of some pixel -- (-1, -1) is all ones, (0, 0) is
// zero -- so no key can stand for "empty"
MCORB_TR_HD inline int32_t tr_pixel_coord(float v)
{
    return v > -2147483648.0f && v < 2147483648.0f ? (int32_t)v : INT32_MIN;
}
MCORB_TR_HD inline uint64_t pixel_key(int32_t px, int32_t py) { return ((uint64_t)(uint32_t)px << 32) | (uint32_t)py; }
MCORB_TR_HD inline uint64_t tr_pixel_key(float x, float y) { return pixel_key(tr_pixel_coord(x), tr_pixel_coord(y)); }
// What the serial list leaves, in closed form.  The list never holds two entries of one pixel; an entry is replaced only by a
// strictly smaller distance, and the replacement is appended.  So of the matched queries of one pixel the entry that survives is
// the one with the least (dist, candidate index) -- tr_dedup_value orders them -- and the final list holds the survivors in
// ascending candidate index: a segmented arg-min and an ordered stream compaction
MCORB_TR_HD inline uint64_t tr_dedup_value(int32_t dist, int32_t i) { return ((uint64_t)(uint32_t)dist << 32) | (uint32_t)i; }
// a device store's arg-min table of one camera has 1 << tr_dedup_log2(n) slots for n candidates: the next power of two >= 2 * n
inline int tr_dedup_log2(int n)
{
    int log2p = 1;
    while (((size_t)1 << log2p) < 2 * (size_t)n) log2p++;
    return log2p;
}

// what k_track_match is told about the frame: per camera the keypoint count and the first keypoint's place in the packed block
struct TrFrame { int32_t n_kp[MCORB_MAX_CAMS]; int32_t first[MCORB_MAX_CAMS]; };
// a query's result before the serial part
struct TrBest { int32_t kp, dist; };
// a kept (camera, candidate) pair as the host tail walks it: the candidate's place in the call's list, the projected keypoint, the
// query's result.  A camera's rows are its kept candidates in candidate order, n_proj of them from row c * n (k_track_compact on a
// device store, the serial path itself on a host-only one)
struct TrRow { int32_t i; float x, y; int32_t kp, dist; };
// an entry of a camera's de-duplicated list: the candidate's place in the call's list, its keypoint, the distance.  A camera's
// entries are n_match of them from entry c * n (k_track_dedup_emit on a device store, the serial list on a host-only one)
struct TrMatch { int32_t i, kp, dist; };
// One frame of a tracking call -- any entry, 1 .. MCORB_TRACK_MAX_FRAMES of them -- as the kernels read it from device memory,
// frame blockIdx.z: its view's place among the call's views; its n candidates, cand_first candidates into the call's list; rows:
// where its block of every per-pair array begins, ncams * cand_first -- inside the block the layout is [c * n + i]; tab: where
// its de-duplication tables begin, ncams << log2p slots; frame: camera c's n_kp[c] keypoints from kp0 + first[c] on in the
// kp_xy the kernels are given, their descriptors from keypoint desc0 + first[c] on in kp_desc.  A rig slot's frame: kp_xy is the
// store's keypoint buffer, first[c] = c * kcap and kp0 = (f * ncams) * kcap, k_track_points' rows of img0, its first image of
// the slot; kp_desc is the slot's descriptors, desc0 = img0 * kcap.  A host-array frame: kp_xy and kp_desc are the uploaded
// block's, first[c] is the running keypoint count, kp0 = desc0 = 0 and img0 is not read
struct TrItem {
    int32_t view, n, log2p, img0;
    uint64_t cand_first, rows, tab, kp0, desc0;
    TrFrame frame;
};

}  // namespace mcorb
