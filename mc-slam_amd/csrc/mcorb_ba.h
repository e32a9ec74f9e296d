// mcorb_ba.h -- the arithmetic of the local bundle adjustment over rig keyframes and landmarks: the projection factor of the
// reference's back end (MCSlam/src/Backend.cpp:1380-1393 and :1426-1440: GenericProjectionFactor<Pose3, Point3, Cal3_S2> on the
// body pose with body_P_sensor, Huber at sqrt(5.991) over an isotropic sigma per octave; the cheirality value of
// GtsamFactorHelpers.h:75-100) around the Levenberg-Marquardt that section 9g states, with the landmarks eliminated by the Schur
// complement.  No HIP dependency: the host-only store (ba_run_serial below, mcorb_ba.cpp) and the kernels
// of mcorb_ba_gpu.hip run the same functions.  Compile with -ffp-contract=off: everything is fp64, one IEEE operation per
// operator in the order written; only + - * /, comparisons and the Huber square root occur, so the device, the host and
// tests/ba_ref.py agree bit for bit.
//
//   an observation          (kf, cam, lm, uv, octave); the host sorts them stably by (lm, kf), so a landmark's observations are
//                           consecutive and, among them, a keyframe's
//   a view                  a (landmark, keyframe of the system) pair with at least one observation: 45 sums
//   the system              the free keyframes that have an observation, ascending; 6 unknowns each, at most 96
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mcorb_pose.h"

namespace mcorb {

// a view's 45 sums: the 21 upper entries of U = sum w J^T J row by row, the 6 of g = sum w J^T r, the 6 x 3 of W = sum w J^T JX
constexpr int kBaView = 45, kBaG = 21, kBaW = 27;
constexpr int kBaDiag = 27;                           // what a keyframe folds: U (21) and rhs = g - e (6)
constexpr int kBaPair = 36;                           // what a keyframe pair folds: E_ab, 6 x 6 row by row
constexpr int kBaMaxN = 6 * MCORB_BA_MAX_KF;          // unknowns of the reduced system
constexpr int kBaTri = kBaMaxN * (kBaMaxN + 1) / 2;   // its packed upper triangle
constexpr int kBaMaxPairs = MCORB_BA_MAX_KF * (MCORB_BA_MAX_KF + 1) / 2;

// an observation as the walks read it, in sorted order; orig: its place in the caller's arrays
struct BaObs { float u, v; int32_t kf, cam, lm, octave, orig, reserved; };

// One problem as the kernels read it from device memory.  sys_of_kf: a keyframe's place in the system, -1 for a fixed keyframe
// and for a free one nobody observes
struct BaJob {
    mcorb_track_cam cams[MCORB_MAX_CAMS];
    double inv_s[MCORB_MAX_LEVELS];   // 1.0 / sigma[level]
    double huber_k;
    int32_t nkf, ncams, nlm, nobs, nsys, nviews, max_iterations, reserved;
    int8_t sys_of_kf[MCORB_BA_MAX_KF];
};

// the loop's record: pose_round's locals.  cur: which half of the state buffers holds the current state (the other the trial);
// relin: the current state moved since it was linearized; step_ok: the solve of this iteration gave a step
struct BaRecord {
    double lambda, cost, cost_initial;
    int32_t solves, any, converged, done, cur, relin, step_ok, reserved;
};

// what the host reads after the chain (host-mapped): the result and the keyframes' poses
struct BaOut { mcorb_ba_result res; PoseState poses[MCORB_BA_MAX_KF]; };

// The kernels' arguments.  The input block (device memory): job, poses_in (nkf), lids or pts_in (nlm; the other NULL; geom: the
// store's points), the sorted observations and the per-landmark tables of BaPlan.  The chain's scratch: poses (2 x
// MCORB_BA_MAX_KF) and pts (2 x nlm x 3), half rec->cur the current state; V, gp, cost per landmark; views; diag (27 per
// keyframe of the system), pairs (36 per pair), delta.  out, out_pts, flags: host-mapped.  The counts are the job's, by value
struct BaArgs {
    const BaJob *job;
    const PoseState *poses_in;
    const int32_t *lids;
    const double *pts_in, *geom;
    const BaObs *obs;
    const int32_t *obs_first, *view_first;
    const int8_t *slot;
    PoseState *poses;
    double *pts, *V, *gp, *cost, *views, *diag, *pairs, *delta;
    BaRecord *rec;
    int32_t *count;   // the inliers of each workgroup of k_ba_flags
    BaOut *out;
    double *out_pts;
    uint8_t *flags;
    int32_t nkf, nlm, nobs, nsys, max_iterations;
};

// where entry (j, i), j <= i, of an n x n upper triangle packed row by row lies: the entries of S, and the keyframe pairs
MCORB_POSE_HD int ba_tri(int j, int i, int n) { return j * n - j * (j - 1) / 2 + (i - j); }

// The whitened residual of an observation and, with J, its whitened Jacobians: J by the pose (pose_residual's) and JX by the
// point, JX = Dpi(q) * M with M = Rc^T R^T; both zero behind the camera, by select.  Then Huber at k on the whitened residual
template <bool WithJ>
MCORB_POSE_HD void ba_observation(const mcorb_track_cam &cam, const PoseState &P, const double X[3], float kx, float ky, double inv_s,
                                  double k, double &rx, double &ry, double J[2][6], double JX[2][3], double &w, double &rho)
{
    pose_residual<WithJ>(cam, P, X, kx, ky, rx, ry, J);
    rx = rx * inv_s;
    ry = ry * inv_s;
    pose_huber(rx, ry, k, w, rho);
    if (!WithJ) return;
    // Dpi once more, as pose_residual has it
    double pb[3], q[3];
    pose_body(P, X, pb);
    pose_cam(cam, pb, q);
    const bool behind = q[2] <= 0;
    const double d = 1.0 / q[2];
    const double u = q[0] * d, v = q[1] * d;
    const double D00 = cam.fx * d, D01 = cam.s * d, D02 = -((cam.fx * u + cam.s * v) * d);
    const double D11 = cam.fy * d, D12 = -((cam.fy * v) * d);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // column c of M: M[k][c] = sum over m of Rc[m][k] * R[c][m]
        const double M0 = (cam.R[0] * P.R[3 * c] + cam.R[3] * P.R[3 * c + 1]) + cam.R[6] * P.R[3 * c + 2];
        const double M1 = (cam.R[1] * P.R[3 * c] + cam.R[4] * P.R[3 * c + 1]) + cam.R[7] * P.R[3 * c + 2];
        const double M2 = (cam.R[2] * P.R[3 * c] + cam.R[5] * P.R[3 * c + 1]) + cam.R[8] * P.R[3 * c + 2];
        JX[0][c] = (behind ? 0.0 : (D00 * M0 + D01 * M1) + D02 * M2) * inv_s;
        JX[1][c] = (behind ? 0.0 : D11 * M1 + D12 * M2) * inv_s;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) {
        J[0][c] = J[0][c] * inv_s;
        J[1][c] = J[1][c] * inv_s;
    }
}

// A landmark's observations obs[o0 .. o1) at the poses and the point X, in order into +0.0: V (6 upper entries of sum w JX^T
// JX), gp (sum w JX^T r), the cost (sum rho) and, per keyframe of the system that sees it, a view's 45 sums, written to views
// one after the other as each is finished
MCORB_POSE_HD void ba_linearize_lm(const BaJob &job, const PoseState *poses, const BaObs *obs, int o0, int o1, const double X[3],
                                   double V[6], double gp[3], double &cost, double *views)
{
    double acc[kBaView];
#pragma unroll
    for (int k = 0; k < 6; k++) V[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) gp[k] = 0.0;
    cost = 0.0;
    int cur_kf = -1;
    for (int i = o0; i < o1; i++) {
        const BaObs o = obs[i];
        double rx, ry, J[2][6], JX[2][3], w, rho;
        ba_observation<true>(job.cams[o.cam], poses[o.kf], X, o.u, o.v, job.inv_s[o.octave], job.huber_k, rx, ry, J, JX, w, rho);
        int at = 0;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a; b < 3; b++, at++) V[at] = V[at] + w * (JX[0][a] * JX[0][b] + JX[1][a] * JX[1][b]);
#pragma unroll
        for (int a = 0; a < 3; a++) gp[a] = gp[a] + w * (JX[0][a] * rx + JX[1][a] * ry);
        cost = cost + rho;
        if (job.sys_of_kf[o.kf] < 0) continue;
        if (o.kf != cur_kf) {
            if (cur_kf >= 0) {
#pragma unroll
                for (int k = 0; k < kBaView; k++) views[k] = acc[k];
                views += kBaView;
            }
#pragma unroll
            for (int k = 0; k < kBaView; k++) acc[k] = 0.0;
            cur_kf = o.kf;
        }
        at = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++, at++) acc[at] = acc[at] + w * (J[0][a] * J[0][b] + J[1][a] * J[1][b]);
#pragma unroll
        for (int a = 0; a < 6; a++) acc[kBaG + a] = acc[kBaG + a] + w * (J[0][a] * rx + J[1][a] * ry);
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = 0; c < 3; c++) acc[kBaW + 3 * a + c] = acc[kBaW + 3 * a + c] + w * (J[0][a] * JX[0][c] + J[1][a] * JX[1][c]);
    }
    if (cur_kf >= 0)
#pragma unroll
        for (int k = 0; k < kBaView; k++) views[k] = acc[k];
}

// the cost alone: the variant that serves a trial state
MCORB_POSE_HD double ba_cost_lm(const BaJob &job, const PoseState *poses, const BaObs *obs, int o0, int o1, const double X[3])
{
    double cost = 0.0;
    for (int i = o0; i < o1; i++) {
        const BaObs o = obs[i];
        double rx, ry, w, rho;
        ba_observation<false>(job.cams[o.cam], poses[o.kf], X, o.u, o.v, job.inv_s[o.octave], job.huber_k, rx, ry, nullptr, nullptr, w, rho);
        cost = cost + rho;
    }
    return cost;
}

// the flag of an observation at the returned state: 0 when the whitened r . r > 5.991 (a NaN is not greater)
MCORB_POSE_HD uint8_t ba_inlier(const BaJob &job, const PoseState *poses, const BaObs &o, const double X[3])
{
    double rx, ry, w, rho;
    ba_observation<false>(job.cams[o.cam], poses[o.kf], X, o.u, o.v, job.inv_s[o.octave], job.huber_k, rx, ry, nullptr, nullptr, w, rho);
    return (rx * rx + ry * ry) > 5.991 ? 0 : 1;
}

// V' = V with d + lambda * d on the diagonal, as an LDL^T written out (new_solve's, mcorb_mapping_new.h).  ok: every pivot > 0;
// otherwise the landmark is inactive for this solve
struct BaLdl { double l10, l20, l21, d0, d1, d2; bool ok; };
MCORB_POSE_HD BaLdl ba_ldl3(const double V[6], double lambda)
{
    BaLdl L;
    const double a00 = V[0] + lambda * V[0], a01 = V[1], a02 = V[2], a11 = V[3] + lambda * V[3], a12 = V[4], a22 = V[5] + lambda * V[5];
    L.d0 = a00;
    L.l10 = a01 / L.d0;
    L.l20 = a02 / L.d0;
    L.d1 = a11 - (L.l10 * L.l10) * L.d0;
    L.l21 = (a12 - (L.l20 * L.l10) * L.d0) / L.d1;
    L.d2 = (a22 - (L.l20 * L.l20) * L.d0) - (L.l21 * L.l21) * L.d1;
    L.ok = (L.d0 > 0) & (L.d1 > 0) & (L.d2 > 0);
    return L;
}
// x = V'^-1 b
MCORB_POSE_HD void ba_solve3(const BaLdl &L, double b0, double b1, double b2, double x[3])
{
    const double y0 = b0;
    const double y1 = b1 - L.l10 * y0;
    const double y2 = (b2 - L.l20 * y0) - L.l21 * y1;
    x[2] = y2 / L.d2;
    x[1] = y1 / L.d1 - L.l21 * x[2];
    x[0] = (y0 / L.d0 - L.l10 * x[1]) - L.l20 * x[2];
}

// what an active landmark adds for a keyframe of the system that sees it: U_aj and g_aj - e_aj, e_aj = W_aj (V'^-1 gp_j)
MCORB_POSE_HD void ba_diag_term(const BaLdl &L, const double *view, const double gp[3], double out[kBaDiag])
{
    double z[3];
    ba_solve3(L, gp[0], gp[1], gp[2], z);
#pragma unroll
    for (int k = 0; k < kBaG; k++) out[k] = view[k];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double *W = view + kBaW + 3 * i;
        out[kBaG + i] = view[kBaG + i] - ((W[0] * z[0] + W[1] * z[1]) + W[2] * z[2]);
    }
}

// what an active landmark adds for a pair of keyframes that both see it: E_abj = W_aj (V'^-1 W_bj^T), column by column
MCORB_POSE_HD void ba_pair_term(const BaLdl &L, const double *view_a, const double *view_b, double out[kBaPair])
{
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const double *Wb = view_b + kBaW + 3 * c;
        double y[3];
        ba_solve3(L, Wb[0], Wb[1], Wb[2], y);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double *Wa = view_a + kBaW + 3 * i;
            out[6 * i + c] = (Wa[0] * y[0] + Wa[1] * y[1]) + Wa[2] * y[2];
        }
    }
}

// entry (6 a + i, 6 b + k) of S, a <= b and, on the diagonal blocks, i <= k: S_aa = (U_a + lambda diag(U_a)) - E_aa, S_ab = -E_ab.
// diag: the keyframes' 27 folded sums; pairs: the pairs' 36
MCORB_POSE_HD double ba_system_entry(const double *diag, const double *pairs, int nsys, double lambda, int a, int b, int i, int k)
{
    const double e = pairs[(size_t)kBaPair * ba_tri(a, b, nsys) + 6 * i + k];
    if (a != b) return -e;
    const double u = diag[kBaDiag * a + (i * 6 - i * (i - 1) / 2 + (k - i))];
    return i == k ? (u + lambda * u) - e : u - e;
}

// the back-substitution of an active landmark: tt = gp + sum over the keyframes of the system that see it, ascending, of W^T
// delta_a; X' = X + V'^-1 (-tt).  slot: the landmark's 16 view slots (-1: none), views: its first view
MCORB_POSE_HD void ba_backsub_lm(const BaLdl &L, const double gp[3], const int8_t *slot, const double *views, int nsys,
                                 const double *delta, const double X[3], double Xn[3])
{
    double tt[3] = {gp[0], gp[1], gp[2]};
    for (int a = 0; a < nsys; a++) {
        const int s = slot[a];
        if (s < 0) continue;
        const double *W = views + (size_t)kBaView * s + kBaW, *d = delta + 6 * a;
#pragma unroll
        for (int c = 0; c < 3; c++)
            tt[c] = tt[c] + (((((W[c] * d[0] + W[3 + c] * d[1]) + W[6 + c] * d[2]) + W[9 + c] * d[3]) + W[12 + c] * d[4]) + W[15 + c] * d[5]);
    }
    double dX[3];
    ba_solve3(L, -tt[0], -tt[1], -tt[2], dX);
#pragma unroll
    for (int c = 0; c < 3; c++) Xn[c] = X[c] + dX[c];
}

// the acceptance rule of pose_round on the record, after the solve of an iteration; trial_cost is read only when step_ok
MCORB_POSE_HD void ba_decide(BaRecord &r, double trial_cost, int max_iterations)
{
    r.solves = r.solves + 1;
    const bool accept = r.step_ok && trial_cost < r.cost;
    if (accept) {
        const double dec = r.cost - trial_cost;
        const bool stop = dec < 1e-6 || dec < 1e-6 * r.cost;
        r.cur ^= 1;
        r.cost = trial_cost;
        r.any = 1;
        r.relin = 1;
        r.lambda = r.lambda * 0.5;
        if (stop) { r.converged = 1; r.done = 1; }
        else if (r.lambda < 1e-16) r.done = 1;
    } else {
        r.relin = 0;
        r.lambda = r.lambda * 2.0;
        if (r.lambda > 1e32) r.done = 1;
    }
    if (r.solves >= max_iterations) r.done = 1;
}

MCORB_POSE_HD int32_t ba_status(const BaRecord &r)
{
    return !r.any ? MCORB_BA_NO_STEP : r.converged ? MCORB_BA_CONVERGED : MCORB_BA_MAX_ITER;
}

// ---- host side: the plan of a call, the dense solve, the fold and the serial run ----

// the sorted observations and the per-landmark tables the walks read.  obs_first / view_first: nlm + 1 entries; slot: per
// landmark 16 bytes, slot[16 j + a] = which of landmark j's views is keyframe a's of the system, -1: none
struct BaPlan {
    std::vector<BaObs> obs;
    std::vector<int32_t> obs_first, view_first;
    std::vector<int8_t> slot;
};

// job: nkf, ncams, nlm, nobs set; fixed: per keyframe.  Fills job.sys_of_kf / nsys / nviews and the plan.  The
// indices have been checked
inline void ba_plan(BaJob &job, const uint8_t *fixed, const int32_t *obs_kf, const int32_t *obs_cam, const int32_t *obs_lm,
                    const float *uv, const int32_t *octave, BaPlan &plan)
{
    const int nobs = job.nobs, nlm = job.nlm;
    bool seen[MCORB_BA_MAX_KF] = {};
    for (int i = 0; i < nobs; i++) seen[obs_kf[i]] = true;
    job.nsys = 0;
    for (int k = 0; k < MCORB_BA_MAX_KF; k++) job.sys_of_kf[k] = -1;
    for (int k = 0; k < job.nkf; k++)
        if (!fixed[k] && seen[k]) job.sys_of_kf[k] = (int8_t)job.nsys++;
    std::vector<int32_t> order((size_t)nobs);
    for (int i = 0; i < nobs; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return obs_lm[x] != obs_lm[y] ? obs_lm[x] < obs_lm[y] : obs_kf[x] < obs_kf[y];
    });
    plan.obs.resize((size_t)nobs);
    plan.obs_first.assign((size_t)nlm + 1, 0);
    plan.view_first.assign((size_t)nlm + 1, 0);
    plan.slot.assign((size_t)nlm * MCORB_BA_MAX_KF, -1);
    int at = 0, nviews = 0;
    for (int j = 0; j < nlm; j++) {
        plan.obs_first[j] = at;
        plan.view_first[j] = nviews;
        int last_kf = -1, nv = 0;
        for (; at < nobs && obs_lm[order[at]] == j; at++) {
            const int i = order[at];
            plan.obs[at] = BaObs{uv[2 * (size_t)i], uv[2 * (size_t)i + 1], obs_kf[i], obs_cam[i], j, octave[i], i, 0};
            const int a = job.sys_of_kf[obs_kf[i]];
            if (a >= 0 && obs_kf[i] != last_kf) {
                plan.slot[(size_t)j * MCORB_BA_MAX_KF + a] = (int8_t)nv++;
                last_kf = obs_kf[i];
            }
        }
        nviews += nv;
    }
    plan.obs_first[nlm] = at;
    plan.view_first[nlm] = nviews;
    job.nviews = nviews;
}

// S delta = -rhs by pose_solve's LDL^T on n unknowns, in place on the packed upper triangle A (entry (j, i), j <= i, becomes
// L[i][j]; the pivots go to D); every dot product subtracts in ascending k.  false when a pivot is not > 0, a NaN included
inline bool ba_solve_dense(double *A, const double *rhs, int n, double *D, double *y, double *delta)
{
    bool ok = true;
    for (int j = 0; j < n; j++) {
        double dj = A[ba_tri(j, j, n)];
        for (int k = 0; k < j; k++) dj = dj - (A[ba_tri(k, j, n)] * A[ba_tri(k, j, n)]) * D[k];
        if (!(dj > 0)) ok = false;
        D[j] = dj;
        for (int i = j + 1; i < n; i++) {
            double v = A[ba_tri(j, i, n)];
            for (int k = 0; k < j; k++) v = v - (A[ba_tri(k, i, n)] * A[ba_tri(k, j, n)]) * D[k];
            A[ba_tri(j, i, n)] = v / dj;
        }
    }
    if (!ok) return false;
    for (int i = 0; i < n; i++) {
        double v = -rhs[i];
        for (int k = 0; k < i; k++) v = v - A[ba_tri(k, i, n)] * y[k];
        y[i] = v;
    }
    for (int i = n - 1; i >= 0; i--) {
        double v = y[i] / D[i];
        for (int k = i + 1; k < n; k++) v = v - A[ba_tri(i, k, n)] * delta[k];
        delta[i] = v;
    }
    return true;
}

// fold_j: lane l of 256 adds the terms of landmarks l, l + 256, .. ascending into +0.0 -- term(j, t) -> whether landmark j
// qualifies -- and the lanes fold as pose_fold states
template <int K, class Term>
inline void ba_fold(int nlm, Term &&term, double S[K])
{
    static thread_local double s[MCORB_POSE_LANES][K];
    for (int l = 0; l < MCORB_POSE_LANES; l++) {
        for (int k = 0; k < K; k++) s[l][k] = 0.0;
        for (int j = l; j < nlm; j += MCORB_POSE_LANES) {
            double t[K];
            if (!term(j, t)) continue;
            for (int k = 0; k < K; k++) s[l][k] = s[l][k] + t[k];
        }
    }
    pose_fold<K>(s, S);
}

// The whole call on the host, serially: what the kernel chain does, landmark by landmark and then the fold.  poses (nkf) and
// pts (nlm x 3): the initial state in, the returned state out; inlier: nobs flags in the caller's order.  nobs >= 1
inline void ba_run_serial(const BaJob &job, const BaPlan &plan, PoseState *poses, double *pts, mcorb_ba_result &res, uint8_t *inlier)
{
    const int nlm = job.nlm, nsys = job.nsys, n = 6 * nsys;
    std::vector<PoseState> P[2] = {std::vector<PoseState>(poses, poses + job.nkf), std::vector<PoseState>(poses, poses + job.nkf)};
    std::vector<double> X[2] = {std::vector<double>(pts, pts + 3 * (size_t)nlm), std::vector<double>(3 * (size_t)nlm)};
    std::vector<double> V(6 * (size_t)nlm), gp(3 * (size_t)nlm), cst((size_t)nlm), views((size_t)kBaView * job.nviews + 1);
    std::vector<double> diag((size_t)kBaDiag * MCORB_BA_MAX_KF), pairs((size_t)kBaPair * kBaMaxPairs), A(kBaTri), D(kBaMaxN), y(kBaMaxN),
        delta(kBaMaxN), rhs(kBaMaxN);
    const BaObs *obs = plan.obs.data();
    auto fold_cost = [&] {
        double S[1];
        ba_fold<1>(nlm, [&](int j, double t[1]) { t[0] = cst[j]; return true; }, S);
        return S[0];
    };
    BaRecord r = {};
    r.lambda = 1e-4;
    r.relin = 1;
    for (int it = -1; it < job.max_iterations && !r.done; it++) {
        const std::vector<PoseState> &Pc = P[r.cur];
        const std::vector<double> &Xc = X[r.cur];
        if (r.relin)
            for (int j = 0; j < nlm; j++)
                ba_linearize_lm(job, Pc.data(), obs, plan.obs_first[j], plan.obs_first[j + 1], &Xc[3 * (size_t)j], &V[6 * (size_t)j],
                                &gp[3 * (size_t)j], cst[j], &views[(size_t)kBaView * plan.view_first[j]]);
        if (it < 0) {   // the cost at the initial state
            r.cost = r.cost_initial = fold_cost();
            continue;
        }
        // the reduced system
        for (int a = 0; a < nsys; a++) {
            ba_fold<kBaDiag>(nlm, [&](int j, double t[kBaDiag]) {
                const int s = plan.slot[(size_t)j * MCORB_BA_MAX_KF + a];
                if (s < 0) return false;
                const BaLdl L = ba_ldl3(&V[6 * (size_t)j], r.lambda);
                if (!L.ok) return false;
                ba_diag_term(L, &views[(size_t)kBaView * (plan.view_first[j] + s)], &gp[3 * (size_t)j], t);
                return true;
            }, &diag[(size_t)kBaDiag * a]);
            for (int b = a; b < nsys; b++)
                ba_fold<kBaPair>(nlm, [&](int j, double t[kBaPair]) {
                    const int sa = plan.slot[(size_t)j * MCORB_BA_MAX_KF + a], sb = plan.slot[(size_t)j * MCORB_BA_MAX_KF + b];
                    if (sa < 0 || sb < 0) return false;
                    const BaLdl L = ba_ldl3(&V[6 * (size_t)j], r.lambda);
                    if (!L.ok) return false;
                    ba_pair_term(L, &views[(size_t)kBaView * (plan.view_first[j] + sa)], &views[(size_t)kBaView * (plan.view_first[j] + sb)], t);
                    return true;
                }, &pairs[(size_t)kBaPair * ba_tri(a, b, nsys)]);
        }
        for (int a = 0; a < nsys; a++)
            for (int b = a; b < nsys; b++)
                for (int i = 0; i < 6; i++)
                    for (int k = (a == b ? i : 0); k < 6; k++)
                        A[ba_tri(6 * a + i, 6 * b + k, n)] = ba_system_entry(diag.data(), pairs.data(), nsys, r.lambda, a, b, i, k);
        for (int a = 0; a < nsys; a++)
            for (int i = 0; i < 6; i++) rhs[6 * a + i] = diag[(size_t)kBaDiag * a + kBaG + i];
        r.step_ok = ba_solve_dense(A.data(), rhs.data(), n, D.data(), y.data(), delta.data()) ? 1 : 0;
        double trial_cost = 0.0;
        if (r.step_ok) {
            std::vector<PoseState> &Pt = P[r.cur ^ 1];
            std::vector<double> &Xt = X[r.cur ^ 1];
            for (int k = 0; k < job.nkf; k++) {
                if (job.sys_of_kf[k] < 0) Pt[k] = Pc[k];
                else pose_retract(Pc[k], &delta[6 * job.sys_of_kf[k]], Pt[k]);
            }
            for (int j = 0; j < nlm; j++) {
                const BaLdl L = ba_ldl3(&V[6 * (size_t)j], r.lambda);
                if (L.ok)
                    ba_backsub_lm(L, &gp[3 * (size_t)j], &plan.slot[(size_t)j * MCORB_BA_MAX_KF], &views[(size_t)kBaView * plan.view_first[j]],
                                  nsys, delta.data(), &Xc[3 * (size_t)j], &Xt[3 * (size_t)j]);
                else
                    for (int c = 0; c < 3; c++) Xt[3 * (size_t)j + c] = Xc[3 * (size_t)j + c];
                cst[j] = ba_cost_lm(job, Pt.data(), obs, plan.obs_first[j], plan.obs_first[j + 1], &Xt[3 * (size_t)j]);
            }
            trial_cost = fold_cost();
        }
        ba_decide(r, trial_cost, job.max_iterations);
    }
    const std::vector<PoseState> &Pf = P[r.cur];
    const std::vector<double> &Xf = X[r.cur];
    res.cost_initial = pose_default_nan(r.cost_initial);
    res.cost_final = pose_default_nan(r.cost);
    res.status = ba_status(r);
    res.iterations = r.solves;
    res.n_obs = job.nobs;
    res.n_inliers = 0;
    for (int j = 0; j < nlm; j++)
        for (int i = plan.obs_first[j]; i < plan.obs_first[j + 1]; i++) {
            const uint8_t in = ba_inlier(job, Pf.data(), obs[i], &Xf[3 * (size_t)j]);
            inlier[obs[i].orig] = in;
            res.n_inliers += in;
        }
    std::copy(Pf.begin(), Pf.end(), poses);
    std::copy(Xf.begin(), Xf.end(), pts);
}

}  // namespace mcorb
