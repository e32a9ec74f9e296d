// mcorb_init.h -- the arithmetic of FrontEnd::initialization from the pose between the first two rig frames to the first
// landmarks (MCSlam/src/FrontEnd.cpp:2633-2839), written in the reference's operation order.  No HIP dependency: the host-only
// store (mcorb_init.cpp, init_run_serial), the kernels of mcorb_init_gpu.hip and a plain g++ program include the same code.
// Compile with -ffp-contract=off (the library's flag): every product, sum, division and sqrt below is one IEEE operation in the
// order written, in fp64, so the device and the host agree bit for bit.
//
//   baseline (:2633)        sqrt(t0 * t0 + t1 * t1 + t2 * t2) > min_baseline, the three squares added in order (cv::norm)
//   per flagged match       the views by get3D_2DCorrs (mcorb_mapping.h: prev's first, cameras ascending), the DLT exactly as
//   (:2665-2757)            map_match calls it -- no epipolar gate --, the per-view gates of triangulateMatches (map_view_gates: the
//                           same loop, :2702-2724), then cos = dot / (dist1 * dist2) from o1, o2 = -1 * R^T * t of the first prev
//                           and the first cur view.  cos < 0.99998 alone makes a landmark candidate; otherwise, a NaN included, the
//                           flag is cleared (verdict 5)
//   medians (:2761-2772)    element size / 2 of the sorted cos over the matches that passed the view gates (parllaxVec) and of the
//                           sorted dist2 over the candidates (depthVec), both 0.0 unless both are non-empty.  std::sort over a NaN
//                           is undefined in the reference; stated: the order is that of init_key, so a NaN sorts after +inf
//   verdict (:2776, :2783)  parllaxVec non-empty && parallax < 0.99998, then num_triangulated > 50
//   scale (:2785-2818)      ncams == 1 || n < 50 (the second arm cannot hold with num_triangulated > 50; restated as written):
//                           s = 1.0 / median_scene_depth, t' = t * s, X' = X * s -- cv::MatExpr's division by a scalar
//   normal (:2819-2821)     Landmark(pt, lf_prev) then addLfFrame(currentFrame) on the stored point: lm_normal_first over prev's
//                           views, lm_normal_add over cur's; cur's camera centres are the translation column of [R | t'] *
//                           cur_T_ref.inv(): per row ((R_i0 c0 + R_i1 c1) + R_i2 c2) + t'_i (recalled from cv::gemm's small-matrix
//                           path)
#pragma once
#include <algorithm>
#include <vector>

#include "mcorb_mapping.h"

#ifndef MCORB_INIT_MAX_MATCHES
#define MCORB_INIT_MAX_MATCHES 16384   // (include/mcorb.h)
#endif

namespace mcorb {

constexpr int kInitUnflagged = 9;   // a match whose flag is clear on entry
enum InitStatus { kInitDone = 0, kInitBaseline = 1, kInitParallax = 2, kInitFew = 3 };

// what is uniform for a call
struct InitJob {
    double R[9], t[3];
    int32_t n, ncams, next_lid, n_initial;   // n_initial: the flags set on entry
};

// what k_init_select leaves: the sizes of parllaxVec and depthVec and their medians as :2761-2772 take them
struct InitSel {
    double parallax, depth;
    int32_t n_parallax, n_depth;
};

// the call's record
struct InitCall {
    double parallax, depth, t_out[3];
    int32_t status, n_initial, n_parallax, n_triangulated, scaled, next_lid;
};

// the usual monotone 64-bit key of a double's bits, after lm_default_nan: -inf < .. < -0.0 < 0.0 < .. < +inf < NaN
MCORB_TRI_HD inline uint64_t init_key(double x)
{
    x = lm_default_nan(x);
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

MCORB_TRI_HD inline double init_unkey(uint64_t k)
{
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    __builtin_memcpy(&x, &b, sizeof(b));
    return x;
}

MCORB_TRI_HD inline bool init_baseline(const double t[3], double min_baseline)
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += t[k] * t[k];
    return sqrt(s) > min_baseline;
}

// everything of a flagged match after the triangulation (:2702-2753).  A record holds X from verdict 3 on, dist2 and cos for 0
// and 5 (a NaN as the default quiet NaN); the normal waits for the scale (init_store)
MCORB_TRI_HD inline void init_after(const MapViews &v, const double X[3], const float *inv_sigma2, MapOut &o)
{
    for (int k = 0; k < 3; k++) o.X[k] = X[k];
    const int gate = map_view_gates(v, X, inv_sigma2);
    if (gate != kMapLandmark) { o.verdict = gate; return; }
    double dist2, cosp;
    map_parallax(v, X, dist2, cosp);
    o.dist2 = lm_default_nan(dist2);
    o.cos = lm_default_nan(cosp);
    o.verdict = cosp < 0.99998 ? kMapLandmark : kMapParallax;
}

// one flagged match from the views to the parallax test
template <bool kAnyViews>
MCORB_TRI_HD inline void init_match(const MapViews &v, const float *inv_sigma2, MapOut &o)
{
    map_clear(o);
    double X[3];
    map_dlt<kAnyViews>(v, X);
    init_after(v, X, inv_sigma2, o);
}

// the views of a match are map_gather_pair's: frames[1] is prev, frames[0] is cur, whose `centre` holds cam_centre_body
template <bool kAnyViews>
MCORB_TRI_HD inline void init_item(const MapArgs &a, const MapItem &it)
{
    MapViews v;
    map_gather_pair(a, it.q, it.t, v);
    MapOut o;
    init_match<kAnyViews>(v, a.inv_sigma2, o);
    a.out[it.rec] = o;
}

// a record is a member of parllaxVec / of depthVec
MCORB_TRI_HD inline bool init_in_parallax(int flag, int verdict) { return flag && (verdict == kMapLandmark || verdict == kMapParallax); }
MCORB_TRI_HD inline bool init_in_depth(int flag, int verdict) { return flag && verdict == kMapLandmark; }

// the verdict and the scale (:2776-2790), formed alike by every workgroup of k_init_put and by the host
MCORB_TRI_HD inline void init_verdict(const InitJob &job, const InitSel &sel, InitCall &c, double &s)
{
    c.parallax = sel.parallax;
    c.depth = sel.depth;
    c.n_initial = job.n_initial;
    c.n_parallax = sel.n_parallax;
    c.n_triangulated = sel.n_depth;
    c.scaled = 0;
    s = 1.0;
    for (int k = 0; k < 3; k++) c.t_out[k] = job.t[k];
    if (!(sel.n_parallax > 0 && sel.parallax < 0.99998)) c.status = kInitParallax;
    else if (!(sel.n_depth > 50)) c.status = kInitFew;
    else {
        c.status = kInitDone;
        if (job.ncams == 1 || job.n < 50) {
            c.scaled = 1;
            s = 1.0 / sel.depth;
            for (int k = 0; k < 3; k++) c.t_out[k] = job.t[k] * s;
        }
    }
    c.next_lid = job.next_lid + (c.status == kInitDone ? sel.n_depth : 0);
}

// the stored point and the normal of an accepted match: views [0, nv1) are prev's, whose centre is centre_w; views [nv1, nv) are
// cur's, whose `centre` is the camera's cam_centre_body
MCORB_TRI_HD inline void init_store(const MapViews &v, const double R[9], const double t_out[3], int scaled, double s, MapOut &o)
{
    if (scaled)
        for (int k = 0; k < 3; k++) o.X[k] = o.X[k] * s;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < v.nv1; i++) lm_ray_add(o.X, v.centre[i], acc);
    lm_normal_first(acc, v.nv1, o.normal, o.n_rays);
    acc[0] = acc[1] = acc[2] = 0.0;
    for (int i = v.nv1; i < v.nv; i++) {
        const double *c = v.centre[i];
        double w[3];
        for (int r = 0; r < 3; r++) w[r] = ((R[3 * r] * c[0] + R[3 * r + 1] * c[1]) + R[3 * r + 2] * c[2]) + t_out[r];
        lm_ray_add(o.X, w, acc);
    }
    lm_normal_add(acc, v.nv - v.nv1, o.normal, o.n_rays);
    for (int k = 0; k < 3; k++) {   // (as dist2 and cos above: the host and the device give a NaN different signs)
        o.X[k] = lm_default_nan(o.X[k]);
        o.normal[k] = lm_default_nan(o.normal[k]);
    }
}

// what a match returns once the verdict is known: rec is k_init_triangulate's record (ignored for a clear flag).  Returns true
// when the record is a landmark to be stored (status DONE, verdict 0); its point and normal are then the stored ones
MCORB_TRI_HD inline bool init_finish(const MapViews &v, const InitJob &job, const InitCall &c, double s, int flag, MapOut &rec)
{
    if (!flag) {
        map_clear(rec);
        rec.verdict = kInitUnflagged;
        return false;
    }
    if (rec.verdict != kMapLandmark) {
        for (int k = 0; k < 3; k++) rec.X[k] = 0.0;
        return false;
    }
    if (c.status != kInitDone) return false;
    init_store(v, job.R, c.t_out, c.scaled, s, rec);
    return true;
}

// ---- host only from here to init_run_serial ----
// element size / 2 of the keys in init_key's order, 0.0 for none
inline double init_median(std::vector<uint64_t> &keys)
{
    if (keys.empty()) return 0.0;
    std::sort(keys.begin(), keys.end());
    return init_unkey(keys[keys.size() / 2]);
}

// :2761-2772 over the records of a call (flags: as on entry)
inline void init_select_serial(const MapOut *recs, const uint8_t *flags, int n, InitSel &sel)
{
    std::vector<uint64_t> kp, kd;
    for (int i = 0; i < n; i++) {
        if (init_in_parallax(flags[i], recs[i].verdict)) kp.push_back(init_key(recs[i].cos));
        if (init_in_depth(flags[i], recs[i].verdict)) kd.push_back(init_key(recs[i].dist2));
    }
    sel.n_parallax = (int32_t)kp.size();
    sel.n_depth = (int32_t)kd.size();
    sel.parallax = sel.depth = 0.0;
    if (!kp.empty() && !kd.empty()) {
        sel.parallax = init_median(kp);
        sel.depth = init_median(kd);
    }
}

// The host-only store's path from the packed block on: the records of all n matches (recs: n entries, in match order), the
// call's record, and -- status DONE -- the accepted points and normals into geom (6 doubles per slot) and the ray counts into
// n_rays from slot job.next_lid on, in match order.  views(i, v): the views of match i
template <class Views>
inline void init_finish_serial(const InitJob &job, const uint8_t *flags, MapOut *recs, Views views, InitCall &call, double *geom, int32_t *n_rays)
{
    InitSel sel;
    init_select_serial(recs, flags, job.n, sel);
    double s;
    init_verdict(job, sel, call, s);
    int32_t id = job.next_lid;
    for (int i = 0; i < job.n; i++) {
        MapViews v;
        v.nv = v.nv1 = 0;
        if (flags[i] && recs[i].verdict == kMapLandmark && call.status == kInitDone) views(i, v);
        if (!init_finish(v, job, call, s, flags[i], recs[i])) continue;
        double *g = geom + (size_t)id * 6;
        for (int k = 0; k < 3; k++) { g[k] = recs[i].X[k]; g[3 + k] = recs[i].normal[k]; }
        n_rays[id] = recs[i].n_rays;
        id++;
    }
}

// a: the packed block (MapLayout; frames[0] cur with cam_centre_body as its centres, frames[1] prev); query / train: the matches
inline void init_run_serial(const InitJob &job, const MapArgs &a, const int32_t *query, const int32_t *train, const uint8_t *flags,
                            MapOut *recs, InitCall &call, double *geom, int32_t *n_rays)
{
    for (int i = 0; i < job.n; i++) {
        map_clear(recs[i]);
        if (!flags[i]) continue;
        MapViews v;
        map_gather_pair(a, query[i], train[i], v);
        if (v.nv <= 4) init_match<false>(v, a.inv_sigma2, recs[i]); else init_match<true>(v, a.inv_sigma2, recs[i]);
    }
    init_finish_serial(job, flags, recs, [&](int i, MapViews &v) { map_gather_pair(a, query[i], train[i], v); }, call, geom, n_rays);
}

// the test hooks (mcorb_host_init_cases, mcorb_dev_init_cases_selftest): everything but the triangulation for caller-given X and
// views (MapCases); centre: centre_w for a view of prev, the camera's cam_centre_body for a view of cur
MCORB_TRI_HD inline void init_gate_case(const MapCases &c, int i, MapOut &o)
{
    MapViews v;
    map_case_views(c, i, v);
    map_clear(o);
    init_after(v, c.X + 3 * (size_t)i, c.inv_sigma2, o);
}

}  // namespace mcorb
