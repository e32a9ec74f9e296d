// mcorb_ess_polish.h -- the opt-in polish of mcorb_lmap_essential_pose's winner over its inliers (mcorb_lmap_essential_pose_polished):
// a Levenberg-Marquardt on the Sampson residual over the five unknowns of (R, t), |t| = 1.  Stated, not recalled: OpenCV has no such
// step behind recoverPose and the reference calls none (deviation 6).  mcorb_ess.h's conventions: no HIP
// dependency -- the host-only store (ess_polish_serial, mcorb_ess.cpp) and k_ess_fit (mcorb_ess_gpu.hip) run the same code --
// compiled with -ffp-contract=off, fp64, one IEEE operation per operator in the order written, only + - * /, comparisons and sqrt,
// every loop bounded by a count whatever the data holds.  mcorb_pose.h's pose_round and pose_solve are written for six unknowns and
// pose_solve refuses a pivot that is not > 0; the Sampson value does not depend on |t|, so a sixth unknown along t would have a
// zero column and every solve would be refused.  ess_fit_solve and ess_fit_round are their five-unknown counterparts: the same
// form, schedule, constants and statuses.
//   the unknowns                   delta[5]: a rotation (delta[0 .. 2]) and a move of t in its tangent plane (delta[3], delta[4])
//   the retraction                 R' = R * C(delta[0 .. 2]) with pose_retract's Cayley matrix, operator for operator; t' = u / |u|,
//                                  u = (t + delta[3] b1) + delta[4] b2.  With k the index of the smallest |t_k|, the first of equals:
//                                  b1 = (t x e_k) / |t x e_k|, b2 = t x b1.  The basis is that of the pose that is retracted: the
//                                  pass's current pose, for a trial and for the five perturbations alike
//   the residual of a match        E = [t]x R (mcorb_ess_result's convention: x1^T E x2 = 0, X_c1 = R X_c2 + t); with ess_sampson's r,
//                                  a, b: res = (r / sqrt(((a0 a0 + a1 a1) + b0 b0) + b1 b1)) * (1 / thr), thr = threshold_px / ((fx +
//                                  fy) / 2).  res^2 = err / thr^2: a member that is an inlier adds less than 1 to the cost, so the
//                                  round's absolute stop at 1e-6 is on the scale of the inlier test.  A NaN residual makes the
//                                  cost NaN: the round rejects that as a trial and, at the start, answers NO_STEP
//   the Jacobian                   forward differences through the retraction, h = 2^-20: column k is (res(E_k) - res(E_0)) * 2^20
//                                  with E_0 of the pass's pose and E_k of retract(pose, h e_k); the six E are formed once per pass
//   the solve                      refused for fewer than five members (fewer residuals than unknowns), whatever the damping
//   the sums                       21: the 15 upper entries of J^T J row by row, the 5 of J^T res, the cost res^2.  Match i goes to
//                                  lane i mod 256 in ascending i; the lanes fold in pose_fold's tree
//   the rounds                     one or two: ess_fit_round over the members from the current pose; then all S matches are tested
//                                  at its result -- ess_sampson(E') < thr^2 and ess_in_front(ess_depths(R', t')) -- and the result
//                                  replaces the current pose, E, flags and both counts iff its number of flags is at least the
//                                  current n_inliers, otherwise polishing ends.  Round 1's members are the winner's flags, round
//                                  2's are round 1's.  The four-candidate vote is not run again.  A round without a step returns
//                                  the pose it began from bit for bit (its E is then [t]x R of that pose)
#pragma once
#include <stdint.h>

#include "mcorb_ess.h"
#include "mcorb_pose.h"

namespace mcorb {

constexpr int kEssFitUnknowns = 5;
constexpr int kEssFitSums = 21, kEssFitG = 15, kEssFitCost = 20;   // the 15 of J^T J, the 5 of J^T res, the cost
constexpr int kEssFitPoses = 6;                                    // the pass's pose and its five perturbations
constexpr double kEssFitH = 1.0 / 1048576.0, kEssFitInvH = 1048576.0;
constexpr int kEssFitRounds = MCORB_ESS_POLISH_ROUNDS, kEssFitMaxIterations = MCORB_ESS_POLISH_MAX_ITERATIONS;

// what k_ess_fit leaves for the host next to the EssOut: the layout of mcorb_ess_polish
typedef mcorb_ess_polish EssPolish;

// 1 / thr, the scale of the residual
MCORB_POSE_HD double ess_fit_scale(double threshold_px, double fx, double fy) { return 1.0 / (threshold_px / ((fx + fy) / 2.0)); }

// the basis of t's tangent plane
MCORB_POSE_HD void ess_fit_basis(const double t[3], double b1[3], double b2[3])
{
    const double a0 = sac_abs(t[0]), a1 = sac_abs(t[1]), a2 = sac_abs(t[2]);
    int k = 0;
    double least = a0;
    if (a1 < least) {
        k = 1;
        least = a1;
    }
    if (a2 < least) k = 2;
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double c[3];
    rel_cross(t, e, c);
    const double n = __builtin_sqrt(sac_dot(c, c));
    b1[0] = c[0] / n;
    b1[1] = c[1] / n;
    b1[2] = c[2] / n;
    rel_cross(t, b1, b2);
}

MCORB_POSE_HD void ess_fit_retract(const PoseState &P, const double delta[kEssFitUnknowns], PoseState &Q)
{
    const double rot[6] = {delta[0], delta[1], delta[2], 0.0, 0.0, 0.0};
    PoseState T;
    pose_retract(P, rot, T);   // (its R: P.R * C; its t is not used)
    double b1[3], b2[3], u[3];
    ess_fit_basis(P.t, b1, b2);
#pragma unroll
    for (int i = 0; i < 3; i++) u[i] = (P.t[i] + delta[3] * b1[i]) + delta[4] * b2[i];
    const double n = __builtin_sqrt(sac_dot(u, u));
#pragma unroll
    for (int j = 0; j < 9; j++) Q.R[j] = T.R[j];
#pragma unroll
    for (int i = 0; i < 3; i++) Q.t[i] = u[i] / n;
}

// pose k of a pass: P itself (k = 0) or retract(P, h e_(k - 1)).  k may be a run-time value: nothing is indexed by it
MCORB_POSE_HD void ess_fit_pose(const PoseState &P, int k, PoseState &Q)
{
    const double delta[kEssFitUnknowns] = {k == 1 ? kEssFitH : 0.0, k == 2 ? kEssFitH : 0.0, k == 3 ? kEssFitH : 0.0, k == 4 ? kEssFitH : 0.0,
                                           k == 5 ? kEssFitH : 0.0};
    PoseState T;
    ess_fit_retract(P, delta, T);
#pragma unroll
    for (int j = 0; j < 9; j++) Q.R[j] = k == 0 ? P.R[j] : T.R[j];
#pragma unroll
    for (int j = 0; j < 3; j++) Q.t[j] = k == 0 ? P.t[j] : T.t[j];
}

// E = [t]x R
MCORB_POSE_HD void ess_fit_E(const PoseState &P, double *E)
{
#pragma unroll
    for (int j = 0; j < 3; j++) {
        E[j] = P.t[1] * P.R[6 + j] - P.t[2] * P.R[3 + j];
        E[3 + j] = P.t[2] * P.R[j] - P.t[0] * P.R[6 + j];
        E[6 + j] = P.t[0] * P.R[3 + j] - P.t[1] * P.R[j];
    }
}

MCORB_POSE_HD double ess_fit_residual(const double *E, const EssPt &p, double inv_thr)
{
    const double a0 = (E[0] * p.x2 + E[1] * p.y2) + E[2], a1 = (E[3] * p.x2 + E[4] * p.y2) + E[5], a2 = (E[6] * p.x2 + E[7] * p.y2) + E[8];
    const double b0 = (E[0] * p.x1 + E[3] * p.y1) + E[6], b1 = (E[1] * p.x1 + E[4] * p.y1) + E[7];
    const double r = (p.x1 * a0 + p.y1 * a1) + a2;
    return (r / __builtin_sqrt(((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1)) * inv_thr;
}

// one member into a lane's 21 sums.  E: the kEssFitPoses matrices of the pass, read at constant indices
MCORB_POSE_HD void ess_fit_add(const double (*E)[9], const EssPt &p, double inv_thr, double s[kEssFitSums])
{
    const double r0 = ess_fit_residual(E[0], p, inv_thr);
    double J[kEssFitUnknowns];
#pragma unroll
    for (int k = 0; k < kEssFitUnknowns; k++) J[k] = (ess_fit_residual(E[1 + k], p, inv_thr) - r0) * kEssFitInvH;
    int at = 0;
#pragma unroll
    for (int i = 0; i < kEssFitUnknowns; i++)
#pragma unroll
        for (int j = i; j < kEssFitUnknowns; j++, at++) s[at] = s[at] + J[i] * J[j];
#pragma unroll
    for (int i = 0; i < kEssFitUnknowns; i++) s[kEssFitG + i] = s[kEssFitG + i] + J[i] * r0;
    s[kEssFitCost] = s[kEssFitCost] + r0 * r0;
}

// (H + lambda * diag(H)) * delta = -g by an LDL^T without square roots; false when a pivot is not > 0, a NaN included: pose_solve's
// form on five unknowns.  Refused as well, before any arithmetic, when the sums hold fewer than five members: a member is one
// residual, so H = J^T J then has rank below five, and the damping alone would make the matrix positive definite and the step fit
// those members exactly (with one member g, pivot 1 is g1^2 ((1 + lambda) - 1 / (1 + lambda)) > 0).  Five or more members whose
// rows are dependent are not told apart: there the damping and the rounds' acceptance rule stand
MCORB_POSE_HD bool ess_fit_solve(const double S[kEssFitSums], int members, double lambda, double delta[kEssFitUnknowns])
{
    constexpr int N = kEssFitUnknowns;
    if (members < N) return false;
    double A[N][N], L[N][N], D[N], y[N];
    int at = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++, at++) A[i][j] = S[at];
#pragma unroll
    for (int i = 0; i < N; i++) A[i][i] = A[i][i] + lambda * A[i][i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) dj = dj - (L[j][k] * L[j][k]) * D[k];
        if (!(dj > 0)) ok = false;
        D[j] = dj;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double v = A[j][i];
#pragma unroll
            for (int k = 0; k < j; k++) v = v - (L[i][k] * L[j][k]) * D[k];
            L[i][j] = v / dj;
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < N; i++) {
        double v = -S[kEssFitG + i];
#pragma unroll
        for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double v = y[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) v = v - L[k][i] * delta[k];
        delta[i] = v;
    }
    return true;
}

// One round from `init`: pose_round's schedule and constants on the 21 sums.  pass(P, S): the sums at P over the members (`members`
// of them, for ess_fit_solve), the same value in every lane of a device workgroup.  lambda0 = 1e-4, factor 2 both ways, bounds [1e-16, 1e32]; a trial is accepted iff its
// cost is less (a NaN rejects); the round ends on an accepted step whose decrease is < 1e-6 or < 1e-6 * cost, after max_iterations
// solves, or when lambda leaves its bounds
template <class Pass>
MCORB_POSE_HD void ess_fit_round(Pass &pass, const PoseState &init, int members, int max_iterations, PoseState &out, int32_t &iterations, int32_t &status,
                                 double &cost_initial, double &cost_final)
{
    PoseState cur = init;
    double S[kEssFitSums], T[kEssFitSums];
    pass(cur, S);
    double cost = S[kEssFitCost], lambda = 1e-4;
    cost_initial = cost;
    bool any = false, converged = false;
    iterations = 0;
    for (int it = 0; it < max_iterations; it++) {
        iterations = it + 1;
        double delta[kEssFitUnknowns];
        PoseState trial;
        bool accept = false;
        if (ess_fit_solve(S, members, lambda, delta)) {
            ess_fit_retract(cur, delta, trial);
            pass(trial, T);
            accept = T[kEssFitCost] < cost;
        }
        if (accept) {
            const double dec = cost - T[kEssFitCost];
            const bool stop = dec < 1e-6 || dec < 1e-6 * cost;
            cur = trial;
#pragma unroll
            for (int k = 0; k < kEssFitSums; k++) S[k] = T[k];
            cost = T[kEssFitCost];
            any = true;
            lambda = lambda * 0.5;
            if (stop) { converged = true; break; }
            if (lambda < 1e-16) break;
        } else {
            lambda = lambda * 2.0;
            if (lambda > 1e32) break;
        }
    }
    out = any ? cur : init;
    status = !any ? MCORB_POSE_NO_STEP : converged ? MCORB_POSE_CONVERGED : MCORB_POSE_MAX_ITER;
    cost_final = cost;
}

// a match at a round's result: whether it is within the threshold, and whether it is flagged (that and the depth test)
MCORB_POSE_HD void ess_fit_test(const PoseState &P, const double *E, const EssPt &p, double threshold2, double distance, bool &within, bool &flag)
{
    within = sac_is_inlier(ess_sampson(E, p), threshold2);
    flag = false;
    if (within) {
        double z1, z2;
        ess_depths(P.R, P.t, p, z1, z2);
        flag = ess_in_front(z1, z2, distance);
    }
}

// a polish record before any round: the winner's pose, E and counts, every round empty
MCORB_POSE_HD void ess_polish_begin(EssPolish &rec, const PoseState &win, const double *E, int32_t n_ransac, int32_t n_inliers)
{
    for (int j = 0; j < 9; j++) rec.R[j] = win.R[j];
    for (int j = 0; j < 3; j++) rec.t[j] = win.t[j];
    for (int j = 0; j < 9; j++) rec.E[j] = E[j];
    for (int k = 0; k < kEssFitRounds; k++) {
        mcorb_ess_polish_round &q = rec.round[k];
        q.cost_initial = q.cost_final = 0.0;
        q.n_members = q.iterations = q.status = q.n_ransac_inliers = q.n_inliers = q.accepted = 0;
    }
    rec.n_ransac_inliers = n_ransac;
    rec.n_inliers = n_inliers;
    rec.rounds_run = 0;
    rec.reserved = 0;
}

// a pass of the serial run: the fold-ordered sums at P over the members
struct EssFitSerialPass {
    const EssPt *pts;
    const uint8_t *member;
    int S;
    double inv_thr;
    double (*lanes)[kEssFitSums];   // [MCORB_POSE_LANES]
    void operator()(const PoseState &P, double sums[kEssFitSums])
    {
        double E[kEssFitPoses][9];
        for (int k = 0; k < kEssFitPoses; k++) {
            PoseState Q;
            ess_fit_pose(P, k, Q);
            ess_fit_E(Q, E[k]);
        }
        for (int l = 0; l < MCORB_POSE_LANES; l++) {
            for (int k = 0; k < kEssFitSums; k++) lanes[l][k] = 0.0;
            for (int i = l; i < S; i += MCORB_POSE_LANES)
                if (member[i]) ess_fit_add(E, pts[i], inv_thr, lanes[l]);
        }
        pose_fold(lanes, sums);
    }
};

// The rounds, serially: what a host-only store runs behind ess_run_serial, and the hook.  pose / E / n_ransac / n_inliers / flags:
// the current ones (the winner's) in, the accepted ones out; member: round 1's members, S bytes, overwritten; scratch (S bytes)
// and lanes are the caller's
inline void ess_polish_serial(const EssPt *pts, int S, double threshold2, double distance, double inv_thr, int rounds, int max_iterations,
                              PoseState &pose, double *E, int32_t &n_ransac, int32_t &n_inliers, uint8_t *flags, uint8_t *member,
                              uint8_t *scratch, double (*lanes)[kEssFitSums], EssPolish &rec)
{
    static_assert(MCORB_POSE_LANES == 256, "match i is lane i mod 256's");
    EssFitSerialPass pass{pts, member, S, inv_thr, lanes};
    ess_polish_begin(rec, pose, E, n_ransac, n_inliers);
    for (int round = 0; round < rounds; round++) {
        mcorb_ess_polish_round &q = rec.round[round];
        int32_t members = 0;
        for (int i = 0; i < S; i++) members += member[i] ? 1 : 0;
        PoseState cand;
        double c0, c1, Ec[9];
        ess_fit_round(pass, pose, members, max_iterations, cand, q.iterations, q.status, c0, c1);
        ess_fit_E(cand, Ec);
        int32_t nr = 0, n = 0;
        for (int i = 0; i < S; i++) {
            bool within, flag;
            ess_fit_test(cand, Ec, pts[i], threshold2, distance, within, flag);
            scratch[i] = flag ? 1 : 0;
            nr += within ? 1 : 0;
            n += flag ? 1 : 0;
        }
        q.cost_initial = pose_default_nan(c0);
        q.cost_final = pose_default_nan(c1);
        q.n_members = members;
        q.n_ransac_inliers = nr;
        q.n_inliers = n;
        q.accepted = n >= n_inliers ? 1 : 0;
        rec.rounds_run = round + 1;
        if (!q.accepted) break;
        pose = cand;
        for (int j = 0; j < 9; j++) E[j] = Ec[j];
        n_ransac = nr;
        n_inliers = n;
        for (int i = 0; i < S; i++) flags[i] = member[i] = scratch[i];
    }
}

}  // namespace mcorb
