// mcorb_pose.h -- the arithmetic of the rig pose refinement: the cost and the outlier rule of FrontEnd::OptimizePose
// (MCSlam/src/FrontEnd.cpp:4272-4409) with the RigResectioningFactor (MCSlam/include/MCSlam/GtsamFactorHelpers.h:48-100), around
// a Levenberg-Marquardt that is stated here because gtsam's is not in the tree.  No HIP dependency: the
// host-only store (mcorb_pose.cpp) and k_pose_refine (mcorb_pose_gpu.hip) run the same code.  Compile with -ffp-contract=off (the
// library's flag): everything below is fp64, one IEEE operation per operator in the order written; only + - * /, comparisons and
// one square root (the Huber norm) occur, so the device, the host and tests/pose_ref.py agree bit for bit.
//
//   the factor (GtsamFactorHelpers.h:75-100)   project(pose.compose(body_P_sensor), K) - p; a CheiralityException gives the value
//                                              (2 fx, 2 fx) and a zero Jacobian
//   the noise (FrontEnd.cpp:4276-4279)         Huber at sqrt(5.991) on a one-pixel sigma
//   the rounds (:4361-4400)                    two, each from the initial estimate; after each the factors with
//                                              dot(err, err * GetInverseScaleSigmaSquares()[octave]) > 5.991 leave for good
//   the optimizer                              stated: diagonal damping, an LDL^T, a Cayley retraction, a fixed schedule
#pragma once
#include <stdint.h>

#include "mcorb_track.h"

// everything below is inlined into k_pose_refine: an array whose address went to a call would live in scratch
#if defined(__HIPCC__)
#define MCORB_POSE_HD __host__ __device__ __forceinline__
#else
#define MCORB_POSE_HD inline
#endif

namespace mcorb {

// (R, t) = w_T_b, the body's pose in the world, R row-major
struct PoseState { double R[9], t[3]; };

// a model's R[9], t[3] into a PoseState, and the pose of a call without a model: copies of doubles, no arithmetic
MCORB_POSE_HD void pose_load(PoseState &P, const double *R, const double *t)
{
#pragma unroll
    for (int j = 0; j < 9; j++) P.R[j] = R[j];
#pragma unroll
    for (int j = 0; j < 3; j++) P.t[j] = t[j];
}
MCORB_POSE_HD void pose_identity(PoseState &P)
{
#pragma unroll
    for (int j = 0; j < 9; j++) P.R[j] = (j % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) P.t[j] = 0.0;
}

// the 28 sums of a pass: the 21 upper entries of H row by row, the 6 of g, the cost
constexpr int kPoseSums = 28, kPoseG = 21, kPoseCost = 27;
constexpr int kPoseBlock = 64, kPoseBlocks = MCORB_POSE_LANES / kPoseBlock;
static_assert(kPoseBlocks == 4, "the four block sums combine as (b0 + b1) + (b2 + b3)");

// an observation as the passes read it; its point is pts[i] or the store's point of lids[i]
struct PoseObs { float u, v; int32_t cam, octave; };

// One problem as k_pose_refine reads it from device memory.  obs0: where its observations begin in the obs / lids / pts / alive /
// flag arrays.  from_track: the observations are not given but built by the kernel's prologue from a tracking submission's
// frame -- its n_cand candidates from cand_first on, its block of the per-pair arrays at rows (the layout of TrItem), its
// keypoints from kp0 on with frame.first[c] -- and n is then the capacity, ncams * n_cand
struct PoseJob {
    PoseState init;
    double inv_sigma2[MCORB_MAX_LEVELS];
    double huber_k;
    mcorb_track_cam cams[MCORB_MAX_CAMS];
    int32_t ncams, nlevels, max_iterations, n;
    uint64_t obs0;
    int32_t from_track, n_cand;
    uint64_t cand_first, rows, kp0;
    TrFrame frame;
};

// a cost that is returned to the caller: a NaN becomes the default quiet NaN on the bits, for tr_default_nan's reason
MCORB_POSE_HD double pose_default_nan(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof(b));
    if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
    __builtin_memcpy(&x, &b, sizeof(b));
    return x;
}

// a mcorb_track_view read as a rig: the body is camera 0's frame and w_T_b = (R0^T, -(R0^T * t0))
MCORB_POSE_HD void pose_of_view(const double R0[9], const double t0[3], PoseState &P)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) P.R[3 * r + c] = R0[3 * c + r];
        P.t[r] = -((R0[r] * t0[0] + R0[3 + r] * t0[1]) + R0[6 + r] * t0[2]);
    }
}

// p_b = R^T * (X - t): tr_cam's form
MCORB_POSE_HD void pose_body(const PoseState &P, const double X[3], double pb[3])
{
    const double d0 = X[0] - P.t[0], d1 = X[1] - P.t[1], d2 = X[2] - P.t[2];
    pb[0] = P.R[0] * d0 + P.R[3] * d1 + P.R[6] * d2;
    pb[1] = P.R[1] * d0 + P.R[4] * d1 + P.R[7] * d2;
    pb[2] = P.R[2] * d0 + P.R[5] * d1 + P.R[8] * d2;
}

// q = Rc^T * (p_b - tc): tr_cam, written out (a loop the compiler leaves rolled would index q in scratch)
MCORB_POSE_HD void pose_cam(const mcorb_track_cam &cam, const double pb[3], double q[3])
{
    const double d0 = pb[0] - cam.t[0], d1 = pb[1] - cam.t[1], d2 = pb[2] - cam.t[2];
    q[0] = cam.R[0] * d0 + cam.R[3] * d1 + cam.R[6] * d2;
    q[1] = cam.R[1] * d0 + cam.R[4] * d1 + cam.R[7] * d2;
    q[2] = cam.R[2] * d0 + cam.R[5] * d1 + cam.R[8] * d2;
}

// The residual and, with J, its Jacobian w.r.t. the right perturbation xi = (omega, upsilon) of w_T_b, gtsam's order:
// J = Dpi(q) * Rc^T * [ [p_b]x | -I ].  q.z <= 0 (the reference's form: a NaN does not take it) is the CheiralityException
template <bool WithJ>
MCORB_POSE_HD void pose_residual(const mcorb_track_cam &cam, const PoseState &P, const double X[3], float kx, float ky, double &rx, double &ry,
                                      double J[2][6])
{
    double pb[3], q[3];
    pose_body(P, X, pb);
    pose_cam(cam, pb, q);
    // (no branch: both values of every output are computed and one is taken, which gives the kernel straight-line code)
    const bool behind = q[2] <= 0;
    const double d = 1.0 / q[2];
    const double u = q[0] * d, v = q[1] * d;
    const double behind_r = 2.0 * cam.fx;
    rx = behind ? behind_r : ((cam.fx * u + cam.s * v) + cam.u0) - (double)kx;
    ry = behind ? behind_r : (cam.fy * v + cam.v0) - (double)ky;
    if (!WithJ) return;
    // Dpi: the derivative of (fx u + s v + u0, fy v + v0) by q; its (1, 0) entry is zero
    const double D00 = cam.fx * d, D01 = cam.s * d, D02 = -((cam.fx * u + cam.s * v) * d);
    const double D11 = cam.fy * d, D12 = -((cam.fy * v) * d);
    // B = Rc^T * [ [p_b]x | -I ], row by row; M = Rc^T
    double B[3][6];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double M0 = cam.R[k], M1 = cam.R[3 + k], M2 = cam.R[6 + k];
        B[k][0] = M1 * pb[2] - M2 * pb[1];
        B[k][1] = M2 * pb[0] - M0 * pb[2];
        B[k][2] = M0 * pb[1] - M1 * pb[0];
        B[k][3] = -M0;
        B[k][4] = -M1;
        B[k][5] = -M2;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) {
        J[0][c] = behind ? 0.0 : (D00 * B[0][c] + D01 * B[1][c]) + D02 * B[2][c];
        J[1][c] = behind ? 0.0 : D11 * B[1][c] + D12 * B[2][c];
    }
}

// noiseModel::mEstimator::Huber at k on a unit sigma: the weight and the loss of a residual
MCORB_POSE_HD void pose_huber(double rx, double ry, double k, double &w, double &rho)
{
    const double e2 = rx * rx + ry * ry;
    const double e = __builtin_sqrt(e2);
    const bool in = e <= k;
    w = in ? 1.0 : k / e;
    rho = in ? 0.5 * e2 : k * (e - 0.5 * k);
}

// one observation into a lane's 28 sums
MCORB_POSE_HD void pose_add(const mcorb_track_cam &cam, const PoseState &P, const double X[3], float kx, float ky, double k,
                                 double s[kPoseSums])
{
    double rx, ry, J[2][6], w, rho;
    pose_residual<true>(cam, P, X, kx, ky, rx, ry, J);
    pose_huber(rx, ry, k, w, rho);
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++, at++) s[at] = s[at] + w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]);
#pragma unroll
    for (int i = 0; i < 6; i++) s[kPoseG + i] = s[kPoseG + i] + w * (J[0][i] * rx + J[1][i] * ry);
    s[kPoseCost] = s[kPoseCost] + rho;
}

// the cull of a round: dot(err, err * inv_sigma2[octave]) > 5.991 at the round's result
MCORB_POSE_HD bool pose_is_outlier(const mcorb_track_cam &cam, const PoseState &P, const double X[3], float kx, float ky,
                                        double inv_sigma2)
{
    double rx, ry;
    pose_residual<false>(cam, P, X, kx, ky, rx, ry, nullptr);
    return (rx * rx + ry * ry) * inv_sigma2 > 5.991;
}

// (H + lambda * diag(H)) * delta = -g by an LDL^T without square roots; false when a pivot is not > 0, a NaN included
MCORB_POSE_HD bool pose_solve(const double S[kPoseSums], double lambda, double delta[6])
{
    double A[6][6], L[6][6], D[6], y[6];
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++, at++) A[i][j] = S[at];
#pragma unroll
    for (int i = 0; i < 6; i++) A[i][i] = A[i][i] + lambda * A[i][i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) dj = dj - (L[j][k] * L[j][k]) * D[k];
        if (!(dj > 0)) ok = false;
        D[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = A[j][i];
#pragma unroll
            for (int k = 0; k < j; k++) v = v - (L[i][k] * L[j][k]) * D[k];
            L[i][j] = v / dj;
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = -S[kPoseG + i];
#pragma unroll
        for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double v = y[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v = v - L[k][i] * delta[k];
        delta[i] = v;
    }
    return true;
}

// the retraction without transcendentals: a = omega / 2, C = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a) (Cayley), R' = R * C,
// t' = t + R * upsilon
MCORB_POSE_HD void pose_retract(const PoseState &P, const double delta[6], PoseState &Q)
{
    const double a0 = delta[0] * 0.5, a1 = delta[1] * 0.5, a2 = delta[2] * 0.5;
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double den = 1.0 + aa, one = 1.0 - aa;
    const double a01 = 2.0 * (a0 * a1), a02 = 2.0 * (a0 * a2), a12 = 2.0 * (a1 * a2);
    const double C[9] = {(one + 2.0 * (a0 * a0)) / den, (a01 - 2.0 * a2) / den, (a02 + 2.0 * a1) / den,
                         (a01 + 2.0 * a2) / den, (one + 2.0 * (a1 * a1)) / den, (a12 - 2.0 * a0) / den,
                         (a02 - 2.0 * a1) / den, (a12 + 2.0 * a0) / den, (one + 2.0 * (a2 * a2)) / den};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double r0 = P.R[3 * i], r1 = P.R[3 * i + 1], r2 = P.R[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; j++) Q.R[3 * i + j] = (r0 * C[j] + r1 * C[3 + j]) + r2 * C[6 + j];
        Q.t[i] = P.t[i] + ((r0 * delta[3] + r1 * delta[4]) + r2 * delta[5]);
    }
}

// One round from `init`.  pass(P, S): the 28 sums at P over the observations that are still in, the same value in every lane of
// a device workgroup.  lambda0 = 1e-4, factor 2 both ways, bounds [1e-16, 1e32]; a trial is accepted iff its cost is less (a NaN
// rejects); the round ends on an accepted step whose decrease is < 1e-6 or < 1e-6 * cost, after max_iterations solves, or when
// lambda leaves its bounds: every loop is bounded by these counts whatever the data holds
template <class Pass>
MCORB_POSE_HD void pose_round(Pass &pass, const PoseState &init, int max_iterations, PoseState &out, int32_t &iterations,
                                   int32_t &status, double &cost_initial, double &cost_final)
{
    PoseState cur = init;
    double S[kPoseSums], T[kPoseSums];
    pass(cur, S);
    double cost = S[kPoseCost], lambda = 1e-4;
    cost_initial = cost;
    bool any = false, converged = false;
    iterations = 0;
    for (int it = 0; it < max_iterations; it++) {
        iterations = it + 1;
        double delta[6];
        PoseState trial;
        bool accept = false;
        if (pose_solve(S, lambda, delta)) {
            pose_retract(cur, delta, trial);
            pass(trial, T);
            accept = T[kPoseCost] < cost;
        }
        if (accept) {
            const double dec = cost - T[kPoseCost];
            const bool stop = dec < 1e-6 || dec < 1e-6 * cost;
            cur = trial;
#pragma unroll
            for (int k = 0; k < kPoseSums; k++) S[k] = T[k];
            cost = T[kPoseCost];
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

// the fold of the lanes' K sums, host side: s[lane][k].  Each block of 64 lanes folds with strides 32 .. 1, s[l] = s[l] + s[l +
// stride], and the four block sums combine as (b0 + b1) + (b2 + b3) -- what the wave shuffles and the LDS of k_pose_refine (28
// sums), k_rel_fit (28) and k_ess_fit (21) do
template <int K>
inline void pose_fold(double s[MCORB_POSE_LANES][K], double S[K])
{
    for (int b = 0; b < kPoseBlocks; b++)
        for (int stride = kPoseBlock / 2; stride >= 1; stride >>= 1)
            for (int l = 0; l < stride; l++)
                for (int k = 0; k < K; k++) s[b * kPoseBlock + l][k] = s[b * kPoseBlock + l][k] + s[b * kPoseBlock + l + stride][k];
    for (int k = 0; k < K; k++) S[k] = (s[0][k] + s[kPoseBlock][k]) + (s[2 * kPoseBlock][k] + s[3 * kPoseBlock][k]);
}

}  // namespace mcorb
