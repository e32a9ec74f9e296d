// mcorb_retri.h -- the arithmetic of mcorb_lmap_retriangulate: a landmark's point made again from all of its observations after
// the back end moved keyframes, the loop of Backend::UpdateVariables_SmartFactors (MCSlam/src/Backend.cpp:3594-3663: triangulateSafe,
// triangulatePoint3, GlobalMap::updateLandmark, Smartfactor_deleteLandmark), DESIGN.md section 9p.  gtsam is not in the tree: its
// DLT on CameraProjectionMatrix rows, its rank test and the order of triangulateSafe's checks are recalled; the Gram matrix, the
// fold of its sums and the Jacobi route to the null vector are stated instead of gtsam's SVD.  No HIP dependency: the host-only
// store (retri_run_serial below, mcorb_retri.cpp) and k_retri_views / k_retri_solve (mcorb_retri_gpu.hip) run the same functions.
// Compile with -ffp-contract=off: everything is fp64, one IEEE operation per operator in the order written; only + - * /,
// comparisons and sqrt occur, so the device, the host and tests/retri_ref.py agree bit for bit.
//
//   an observation   (landmark, keyframe, camera, uv); the host sorts them stably by (landmark, keyframe, camera): "in order"
//   a view           a (keyframe, camera) pair of a keyframe that has an observation: P = K [R_cw | t_cw] (12) and the camera
//                    centre (3)
//   G                the 10 upper entries of sum (a a^T + b b^T) row by row, a = u P[2] - P[0], b = v P[2] - P[1]; lane l of 16
//                    adds the landmark's observations l, l + 16, .. ascending into +0.0, the 16 sums fold with strides 8, 4, 2, 1
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mcorb_align.h"
#include "mcorb_landmark.h"

namespace mcorb {

constexpr int kRetriLanes = 16;    // the lanes of a landmark's group: part of the definition of G
constexpr int kRetriSweeps = 6;    // cyclic Jacobi sweeps over the six pairs of the 4 x 4 G, align_from_sums' order
constexpr int kRetriView = 15;     // doubles of a view: P row by row, then the centre
constexpr int kRetriG = 10;
constexpr int32_t kRetriNoKey = 0x7fffffff;
constexpr int kRetriFarCode = 1, kRetriBehindCode = 2;

// an observation as the kernels read it, in sorted order: the keypoint, its view and the slot of its keyframe among the
// keyframes that have an observation
struct RetriObs { float u, v; int32_t view, slot; };
static_assert(sizeof(RetriObs) == 16, "k_retri_solve reads 16 bytes per observation");

// one call as the kernels read it from device memory
struct RetriJob {
    mcorb_track_cam cams[MCORB_MAX_CAMS];
    double rank_tol, far_threshold, outlier_threshold, max_diff;
    int32_t ncams, nslots, nlm, nobs, apply, reserved;
};

// what the host reads per landmark (host-mapped)
struct RetriOut { double X[3], diff_norm; int32_t n_views, verdict; };
static_assert(sizeof(RetriOut) == 40, "five doubles");

// the kernels' arguments.  The input block (device memory): job, poses (the w_T_b of slot s), moved (a byte per slot), lids, the
// sorted observations, obs_first (nlm + 1).  views: 15 doubles per (slot, camera).  geom: the store's points; out: host-mapped
struct RetriArgs {
    const RetriJob *job;
    const PoseState *poses;
    const uint8_t *moved;
    const int32_t *lids;
    const RetriObs *obs;
    const int32_t *obs_first;
    double *views;
    double *geom;
    RetriOut *out;
    int32_t nviews, nlm;
};

MCORB_POSE_HD bool retri_finite(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof(b));
    return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// A view of the rig camera `cam` in the keyframe w_T_b = P.  c_T_w = (R_cw, t_cw): R_cw = Rc^T R^T entry by entry as
// ba_observation's M, t_cw = pose_cam(pose_body(origin)); the centre is w_T_c's translation R tc + t.  Then K [R_cw | t_cw] with
// K = (fx s u0; 0 fy v0; 0 0 1), every entry (k0 m0 + k1 m1) + k2 m2, the zeros and the one of K included
MCORB_POSE_HD void retri_view(const mcorb_track_cam &cam, const PoseState &P, double out[kRetriView])
{
    double M[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[k][c] = (cam.R[k] * P.R[3 * c] + cam.R[3 + k] * P.R[3 * c + 1]) + cam.R[6 + k] * P.R[3 * c + 2];
    const double origin[3] = {0.0, 0.0, 0.0};
    double pb[3], q[3];
    pose_body(P, origin, pb);
    pose_cam(cam, pb, q);
    M[0][3] = q[0];
    M[1][3] = q[1];
    M[2][3] = q[2];
    const double K[3][3] = {{cam.fx, cam.s, cam.u0}, {0.0, cam.fy, cam.v0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) out[4 * r + c] = (K[r][0] * M[0][c] + K[r][1] * M[1][c]) + K[r][2] * M[2][c];
#pragma unroll
    for (int r = 0; r < 3; r++) out[12 + r] = ((P.R[3 * r] * cam.t[0] + P.R[3 * r + 1] * cam.t[1]) + P.R[3 * r + 2] * cam.t[2]) + P.t[r];
}

// G = G + (a a^T + b b^T) of one observation: the DLT's two rows
MCORB_POSE_HD void retri_add(const double *view, float kx, float ky, double G[kRetriG])
{
    const double u = (double)kx, v = (double)ky;
    double a[4], b[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        a[c] = u * view[8 + c] - view[c];
        b[c] = v * view[8 + c] - view[4 + c];
    }
    int at = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i; j < 4; j++, at++) G[at] = G[at] + (a[i] * a[j] + b[i] * b[j]);
}

// The null vector and the rank of the folded G: kRetriSweeps cyclic Jacobi sweeps with align_rotate; the eigenvector of the
// smallest diagonal entry (the first of equals) is the homogeneous point, X = v[0..2] * (1.0 / v[3]); lambda_3, the third-largest
// eigenvalue, is the smallest of the other three (the first of equals).  true: the landmark is degenerate -- not sqrt(max(
// lambda_3, 0)) > rank_tol, or a component of X is not finite.  A NaN component of X is returned as the default quiet NaN
MCORB_POSE_HD bool retri_solve(const double G[kRetriG], double rank_tol, double X[3])
{
    double A[4][4], V[4][4];
    int at = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i; j < 4; j++, at++) A[i][j] = A[j][i] = G[at];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kRetriSweeps; sweep++) {
        align_rotate<0, 1>(A, V);
        align_rotate<0, 2>(A, V);
        align_rotate<0, 3>(A, V);
        align_rotate<1, 2>(A, V);
        align_rotate<1, 3>(A, V);
        align_rotate<2, 3>(A, V);
    }
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2], d3 = A[3][3];
    int k = 0;
    double lo = d0;
    k = d1 < lo ? 1 : k;
    lo = d1 < lo ? d1 : lo;
    k = d2 < lo ? 2 : k;
    lo = d2 < lo ? d2 : lo;
    k = d3 < lo ? 3 : k;
    // the smallest of the other three, by selects: e0, e1, e2 are they in index order
    const double e0 = k == 0 ? d1 : d0, e1 = k <= 1 ? d2 : d1, e2 = k == 3 ? d2 : d3;
    double l3 = e0;
    l3 = e1 < l3 ? e1 : l3;
    l3 = e2 < l3 ? e2 : l3;
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = k == 0 ? V[r][0] : k == 1 ? V[r][1] : k == 2 ? V[r][2] : V[r][3];
    const double inv = 1.0 / v[3];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double x = v[c] * inv;
        finite = finite && retri_finite(x);
        X[c] = lm_default_nan(x);
    }
    const double s3 = __builtin_sqrt(l3 > 0.0 ? l3 : 0.0);
    return !(s3 > rank_tol) || !finite;
}

// triangulateSafe's checks of one observation, the idx-th of its landmark in order, at the point X.  key: the smallest (idx << 2 |
// code) of the observations that fail, code 1 (far: the threshold is > 0 and |X - centre| > it) before code 2 (behind: the
// camera-frame z <= 0); emax: the largest reprojection error norm, a NaN counted as +inf.  Both folds are independent of the
// order of the observations
MCORB_POSE_HD void retri_check(const double *view, const double X[3], float kx, float ky, double far_threshold, int idx, int32_t &key,
                               double &emax)
{
    const double d0 = X[0] - view[12], d1 = X[1] - view[13], d2 = X[2] - view[14];
    const double dist = __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    const double x = ((view[0] * X[0] + view[1] * X[1]) + view[2] * X[2]) + view[3];
    const double y = ((view[4] * X[0] + view[5] * X[1]) + view[6] * X[2]) + view[7];
    const double z = ((view[8] * X[0] + view[9] * X[1]) + view[10] * X[2]) + view[11];
    const bool is_far = far_threshold > 0.0 && dist > far_threshold;
    const bool behind = z <= 0.0;
    const int code = is_far ? kRetriFarCode : behind ? kRetriBehindCode : 0;
    const int32_t mine = code ? (int32_t)((idx << 2) | code) : kRetriNoKey;
    key = mine < key ? mine : key;
    const double eu = x / z - (double)kx, ev = y / z - (double)ky;
    double e = __builtin_sqrt(eu * eu + ev * ev);
    e = e != e ? __builtin_inf() : e;
    emax = e > emax ? e : emax;
}

// the verdict of a selected landmark with at least two observations, before the update's gate
MCORB_POSE_HD int retri_verdict(bool degenerate, int32_t key, double emax, double outlier_threshold)
{
    if (degenerate) return MCORB_RETRI_DEGENERATE;
    if (key != kRetriNoKey) return (key & 3) == kRetriFarCode ? MCORB_RETRI_FAR : MCORB_RETRI_BEHIND;
    if (outlier_threshold > 0.0 && !(emax <= outlier_threshold)) return MCORB_RETRI_OUTLIER;
    return MCORB_RETRI_VALID_UPDATED;
}

// GlobalMap::updateLandmark on a valid point: the verdict, and the store's point pt replaced iff diff_norm < max_diff and apply
MCORB_POSE_HD int retri_update(double *pt, const double X[3], double max_diff, bool apply, double &diff_norm)
{
    double p[3] = {pt[0], pt[1], pt[2]};
    if (!lm_update(p, X, max_diff, diff_norm)) return MCORB_RETRI_VALID_REJECTED;
    if (apply) {
        pt[0] = p[0];
        pt[1] = p[1];
        pt[2] = p[2];
    }
    return MCORB_RETRI_VALID_UPDATED;
}

// ---- the host's side ------------------------------------------------------------------------------------------------------

// The plan of a call: the keyframes that have an observation ascending (kf_of_slot), the sorted observations and the landmarks'
// spans.  The arguments are checked by the caller
struct RetriPlan {
    std::vector<int32_t> kf_of_slot, obs_first;
    std::vector<RetriObs> obs;
};

inline void retri_plan(int nkf, int ncams, int nlm, int nobs, const int32_t *obs_lm, const int32_t *obs_kf, const int32_t *obs_cam,
                       const float *uv, RetriPlan &plan)
{
    std::vector<int32_t> slot_of_kf((size_t)nkf, -1);
    for (int i = 0; i < nobs; i++) slot_of_kf[obs_kf[i]] = 0;
    plan.kf_of_slot.clear();
    for (int k = 0; k < nkf; k++)
        if (slot_of_kf[k] == 0) {
            slot_of_kf[k] = (int32_t)plan.kf_of_slot.size();
            plan.kf_of_slot.push_back(k);
        }
    std::vector<int> order((size_t)nobs);
    for (int i = 0; i < nobs; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        if (obs_lm[x] != obs_lm[y]) return obs_lm[x] < obs_lm[y];
        if (obs_kf[x] != obs_kf[y]) return obs_kf[x] < obs_kf[y];
        return obs_cam[x] < obs_cam[y];
    });
    plan.obs.resize((size_t)nobs);
    plan.obs_first.assign((size_t)nlm + 1, 0);
    int at = 0;
    for (int j = 0; j < nlm; j++) {
        plan.obs_first[j] = at;
        for (; at < nobs && obs_lm[order[at]] == j; at++) {
            const int i = order[at], s = slot_of_kf[obs_kf[i]];
            plan.obs[at] = RetriObs{uv[2 * (size_t)i], uv[2 * (size_t)i + 1], s * ncams + obs_cam[i], s};
        }
    }
    plan.obs_first[nlm] = at;
}

// One landmark on the host as its group of 16 lanes computes it: the selection, the 16 partial sums of G and their stride tree,
// the solve, the checks, the gated update of pt (the store's point of the landmark)
inline void retri_landmark_serial(const RetriJob &job, const uint8_t *moved, const RetriObs *obs, int o0, int o1, const double *views,
                                  double *pt, RetriOut &out)
{
    const int n = o1 - o0;
    bool selected = false;
    for (int i = o0; i < o1; i++) selected = selected || moved[obs[i].slot] != 0;
    out.X[0] = out.X[1] = out.X[2] = out.diff_norm = 0.0;
    out.n_views = n;
    out.verdict = !selected ? MCORB_RETRI_NOT_SELECTED : MCORB_RETRI_FEW_VIEWS;
    if (!selected || n < 2) return;
    double s[kRetriLanes][kRetriG];
    for (int l = 0; l < kRetriLanes; l++) {
        for (int k = 0; k < kRetriG; k++) s[l][k] = 0.0;
        for (int i = o0 + l; i < o1; i += kRetriLanes) retri_add(views + (size_t)kRetriView * obs[i].view, obs[i].u, obs[i].v, s[l]);
    }
    for (int stride = kRetriLanes / 2; stride >= 1; stride >>= 1)
        for (int l = 0; l < stride; l++)
            for (int k = 0; k < kRetriG; k++) s[l][k] = s[l][k] + s[l + stride][k];
    const bool degenerate = retri_solve(s[0], job.rank_tol, out.X);
    int32_t key = kRetriNoKey;
    double emax = 0.0;
    for (int i = o0; i < o1; i++)
        retri_check(views + (size_t)kRetriView * obs[i].view, out.X, obs[i].u, obs[i].v, job.far_threshold, i - o0, key, emax);
    out.verdict = retri_verdict(degenerate, key, emax, job.outlier_threshold);
    if (out.verdict == MCORB_RETRI_VALID_UPDATED) out.verdict = retri_update(pt, out.X, job.max_diff, job.apply != 0, out.diff_norm);
}

// The whole call on the host, serially: the view table, then landmark by landmark.  poses, moved: per slot; geom: the store's
// [.][6] rows; out: nlm records
inline void retri_run_serial(const RetriJob &job, const RetriPlan &plan, const PoseState *poses, const uint8_t *moved,
                             const int32_t *lids, double *geom, RetriOut *out)
{
    std::vector<double> views((size_t)kRetriView * job.nslots * job.ncams + 1);
    for (int s = 0; s < job.nslots; s++)
        for (int c = 0; c < job.ncams; c++) retri_view(job.cams[c], poses[s], &views[(size_t)kRetriView * (s * job.ncams + c)]);
    for (int j = 0; j < job.nlm; j++)
        retri_landmark_serial(job, moved, plan.obs.data(), plan.obs_first[j], plan.obs_first[j + 1], views.data(),
                              geom + 6 * (size_t)lids[j], out[j]);
}

}  // namespace mcorb
