// mcorb_align.h -- the arithmetic of the rig pose between two frames from 3D-3D correspondences: the third estimator of
// FrontEnd::estimatePoseLF, PC_ALIGN (MCSlam/src/FrontEnd.cpp:4421-4440), FrontEnd::poseFromPCAlignment (:4441-4530).  Its live
// code is OpenGV's point_cloud::optimize_nonlinear over all correspondences (:4466-4468); what its SAC argument is for is commented
// out (:4476-4489): sac::Ransac<PointCloudSacProblem>, threshold_ = 0.2, max_iterations_ = 100; its own verdict follows (:4493-4514):
// delta = p1 - (R p2 + t), an inlier iff |delta| < 0.1.  OpenGV is not in the tree: the SAC problem's distance |p1 - (R p2 + t)|,
// its sample size 3 and that its minimal solver is the least-squares rigid fit are recalled, and three things are stated instead of
// OpenGV's: the draws, the solver (Horn's unit-quaternion absolute orientation, which serves the sample, the
// refit over a consensus set and the all-correspondence mode) and the absence of the adaptive stop.  Same conventions as
// mcorb_rel.h: no HIP dependency -- the host-only store (mcorb_align.cpp) and k_align_hypotheses / k_align_score / k_align_pick /
// k_align_fit (mcorb_align_gpu.hip) run the same code -- compiled with -ffp-contract=off, fp64, one IEEE operation per operator in
// the order written, only + - * /, comparisons and sqrt, every loop bounded by a count whatever the data holds.
//   The unknown is (R, t) = b1_T_b2: X_1 = R X_2 + t, section 9j's.  Pair i is the point p1[i] of frame 1 and p2[i] of frame 2.
#pragma once
#include <stdint.h>

#include "mcorb_rel.h"

namespace mcorb {

constexpr int kAlignSample = MCORB_ALIGN_SAMPLE;   // the pairs of a minimal sample
constexpr int kAlignSweeps = 6;                    // cyclic Jacobi sweeps over the six pairs of Horn's 4 x 4 matrix
constexpr double kAlignGap = 1e-12;                // a fit is kept iff l1 - l2 > kAlignGap (l1 - l4): the members are not collinear
constexpr int kAlignLanes = MCORB_POSE_LANES;   // the sums fold as mcorb_pose.h's pose_fold states
static_assert(kAlignSample == 3, "align_fit3 is written out for three pairs");
static_assert(MCORB_ALIGN_MAX_ITERATIONS == MCORB_REL_MAX_ITERATIONS, "kRelKeyBits holds every hypothesis index");

// a hypothesis's model: b1_T_b2, whether there is one, and the pairs it was drawn from in draw order (-1: not drawn)
struct AlignModel {
    double R[9], t[3];
    int32_t valid, sample[kAlignSample], pad[4];
};
static_assert(sizeof(AlignModel) == 128, "the kernels read models at 128-byte strides");

// one call as the kernels read it from device memory
struct AlignJob {
    double threshold, inlier_dist;
    uint64_t seed;
    int32_t n, H, mode, refit;
};

// what k_align_pick leaves for k_align_fit: the winner (best -1: none, the identity), its count, the hypotheses with a model
struct AlignPick {
    double R[9], t[3];
    int32_t best, count, n_models, sample[kAlignSample];
};

// what k_align_fit leaves for the host: the answer, the winner of the hypotheses (mode 1; the identity and -1s otherwise), the
// mean distance, status MCORB_ALIGN_*, which of the two the answer is (MCORB_ALIGN_USED_*), the counts
struct AlignOut {
    double R[9], t[3], sac_R[9], sac_t[3], mean_error;
    int32_t status, used, n_inliers, sac_n_inliers, best, n_models, sample[kAlignSample], pad;
};


// the SAC problem's distance (recalled) and the reference's delta.norm() (:4499-4503): |p1 - (R p2 + t)|
MCORB_POSE_HD double align_dist(const PoseState &P, const double p1[3], const double p2[3])
{
    double q[3];
    rel_rot(P.R, p2, q);
    const double dx = p1[0] - (q[0] + P.t[0]), dy = p1[1] - (q[1] + P.t[1]), dz = p1[2] - (q[2] + P.t[2]);
    return __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
}

// ---- the sums of a fit.  Member i of the pairs belongs to lane i mod 256; a lane starts at 0.0 and adds its members in ascending
// i; the lanes' sums fold as mcorb_pose.h's: each block of 64 with strides 32 .. 1, s[l] = s[l] + s[l + stride], then (b0 + b1) +
// (b2 + b3).  Pass 1: the six coordinate sums (p1, then p2), which the member count divides into the centroids.  Pass 2: the nine
// entries of M = sum (p2 - c2)(p1 - c1)^T, row-major
constexpr int kAlignSums1 = 6, kAlignSums2 = 9;

MCORB_POSE_HD void align_add1(const double p1[3], const double p2[3], double s[kAlignSums1])
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s[k] = s[k] + p1[k];
        s[3 + k] = s[3 + k] + p2[k];
    }
}

MCORB_POSE_HD void align_centroids(const double S[kAlignSums1], int cnt, double c1[3], double c2[3])
{
    const double m = (double)cnt;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c1[k] = S[k] / m;
        c2[k] = S[3 + k] / m;
    }
}

MCORB_POSE_HD void align_add2(const double p1[3], const double p2[3], const double c1[3], const double c2[3], double s[kAlignSums2])
{
    const double a0 = p2[0] - c2[0], a1 = p2[1] - c2[1], a2 = p2[2] - c2[2];
    const double b0 = p1[0] - c1[0], b1 = p1[1] - c1[1], b2 = p1[2] - c1[2];
    s[0] = s[0] + a0 * b0;
    s[1] = s[1] + a0 * b1;
    s[2] = s[2] + a0 * b2;
    s[3] = s[3] + a1 * b0;
    s[4] = s[4] + a1 * b1;
    s[5] = s[5] + a1 * b2;
    s[6] = s[6] + a2 * b0;
    s[7] = s[7] + a2 * b1;
    s[8] = s[8] + a2 * b2;
}

// the fold with lanes 0, 1 and 2 occupied by one member each, written out: a lane's sum is 0.0 + a, the empty lanes add + 0.0,
// which leaves a value that is not -0.0 as it is, and lane 0 receives lane 2 (stride 2) before lane 1 (stride 1)
MCORB_POSE_HD double align_fold3(double a0, double a1, double a2) { return ((0.0 + a0) + (0.0 + a2)) + (0.0 + a1); }

// One Jacobi rotation of the symmetric 4 x 4 matrix A in the plane (P, Q), accumulated into V (A = V diag V^T at the end): tau =
// (a_qq - a_pp) / (2 a_pq), t = sign(tau) / (|tau| + sqrt(tau^2 + 1)) (tau = 0: t = 1; an infinite tau: t = 0), c = 1 / sqrt(t^2 +
// 1), s = t c; a pair with a_pq == 0 is skipped.  P and Q are template arguments: every index is a constant, A and V are registers
template <int P, int Q>
MCORB_POSE_HD void align_rotate(double A[4][4], double V[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double tau = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double at = tau < 0.0 ? -tau : tau;
    const double tt = 1.0 / (at + __builtin_sqrt(tau * tau + 1.0));
    const double t = tau < 0.0 ? -tt : tt;
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = 0.0;
    A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = c * arp - s * arq;
            A[r][Q] = s * arp + c * arq;
            A[P][r] = A[r][P];
            A[Q][r] = A[r][Q];
        }
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// Horn's closed-form absolute orientation (stated) from the folded sums: M = sum (p2 - c2)(p1 - c1)^T with entries Sab, a of frame
// 2 and b of frame 1, gives the symmetric
//       | Sxx + Syy + Szz   Syz - Szy          Szx - Sxz          Sxy - Syx        |
//   N = |                   Sxx - Syy - Szz    Sxy + Syx          Szx + Sxz        |
//       |                                     -Sxx + Syy - Szz    Syz + Szy        |
//       |                                                        -Sxx - Syy + Szz  |
// whose eigenvector of the largest eigenvalue is the unit quaternion (w, x, y, z) of R.  The eigenvectors by cyclic Jacobi: the
// pairs (0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), kAlignSweeps sweeps.  The largest diagonal entry, the first of equals, names
// the column of V; R from the quaternion divided by its squared length -- a proper rotation whatever the data, so there is no
// reflection case -- and t = c1 - R c2.  With l1 >= l2 >= l3 >= l4 the diagonal in order, the fit is valid iff cnt >= 3, the 12
// numbers are finite and l1 - l2 > kAlignGap (l1 - l4): collinear members (three coincident ones among them) leave the rotation
// about their line free and l1 = l2.  gap (may be null): (l1 - l2) / (l1 - l4), for the record
MCORB_POSE_HD bool align_from_sums(const double M[kAlignSums2], const double c1[3], const double c2[3], int cnt, PoseState &out, double *gap)
{
    const double Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
    double A[4][4], V[4][4];
    A[0][0] = (Sxx + Syy) + Szz;
    A[1][1] = (Sxx - Syy) - Szz;
    A[2][2] = (Syy - Sxx) - Szz;
    A[3][3] = (Szz - Sxx) - Syy;
    A[0][1] = A[1][0] = Syz - Szy;
    A[0][2] = A[2][0] = Szx - Sxz;
    A[0][3] = A[3][0] = Sxy - Syx;
    A[1][2] = A[2][1] = Sxy + Syx;
    A[1][3] = A[3][1] = Szx + Sxz;
    A[2][3] = A[3][2] = Syz + Szy;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kAlignSweeps; sweep++) {
        align_rotate<0, 1>(A, V);
        align_rotate<0, 2>(A, V);
        align_rotate<0, 3>(A, V);
        align_rotate<1, 2>(A, V);
        align_rotate<1, 3>(A, V);
        align_rotate<2, 3>(A, V);
    }
    // the column of the largest eigenvalue, by selects
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2], d3 = A[3][3];
    int k = 0;
    double l1 = d0;
    k = d1 > l1 ? 1 : k;
    l1 = d1 > l1 ? d1 : l1;
    k = d2 > l1 ? 2 : k;
    l1 = d2 > l1 ? d2 : l1;
    k = d3 > l1 ? 3 : k;
    l1 = d3 > l1 ? d3 : l1;
    double q[4];
#pragma unroll
    for (int r = 0; r < 4; r++) q[r] = k == 0 ? V[r][0] : k == 1 ? V[r][1] : k == 2 ? V[r][2] : V[r][3];
    // the second largest and the smallest: the largest of the other three, the smallest of all
    const double e0 = k == 0 ? d1 : d0, e1 = k <= 1 ? d2 : d1, e2 = k <= 2 ? d3 : d2;
    double l2 = e0;
    l2 = e1 > l2 ? e1 : l2;
    l2 = e2 > l2 ? e2 : l2;
    double l4 = e0;
    l4 = e1 < l4 ? e1 : l4;
    l4 = e2 < l4 ? e2 : l4;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double nn = (ww + xx) + (yy + zz);
    const double xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    out.R[0] = ((ww + xx) - (yy + zz)) / nn;
    out.R[1] = (2.0 * (xy - wz)) / nn;
    out.R[2] = (2.0 * (xz + wy)) / nn;
    out.R[3] = (2.0 * (xy + wz)) / nn;
    out.R[4] = ((ww - xx) + (yy - zz)) / nn;
    out.R[5] = (2.0 * (yz - wx)) / nn;
    out.R[6] = (2.0 * (xz - wy)) / nn;
    out.R[7] = (2.0 * (yz + wx)) / nn;
    out.R[8] = ((ww - xx) - (yy - zz)) / nn;
    double Rc[3];
    rel_rot(out.R, c2, Rc);
    bool ok = cnt >= 3;
#pragma unroll
    for (int j = 0; j < 3; j++) out.t[j] = c1[j] - Rc[j];
#pragma unroll
    for (int j = 0; j < 9; j++) ok = ok && sac_finite(out.R[j]);
#pragma unroll
    for (int j = 0; j < 3; j++) ok = ok && sac_finite(out.t[j]);
    if (gap) *gap = (l1 - l2) / (l1 - l4);
    return ok && (l1 - l2) > kAlignGap * (l1 - l4);   // (false for a NaN too)
}

// align_fit on the three pairs of a sample, in draw order: lanes 0, 1 and 2 hold one member each
MCORB_POSE_HD bool align_fit3(const double p1[kAlignSample][3], const double p2[kAlignSample][3], PoseState &out)
{
    double S[kAlignSums1], M[kAlignSums2], c1[3], c2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        S[k] = align_fold3(p1[0][k], p1[1][k], p1[2][k]);
        S[3 + k] = align_fold3(p2[0][k], p2[1][k], p2[2][k]);
    }
    align_centroids(S, kAlignSample, c1, c2);
    double m[kAlignSample][kAlignSums2];
#pragma unroll
    for (int j = 0; j < kAlignSample; j++) {
#pragma unroll
        for (int k = 0; k < kAlignSums2; k++) m[j][k] = 0.0;
        align_add2(p1[j], p2[j], c1, c2, m[j]);
    }
#pragma unroll
    for (int k = 0; k < kAlignSums2; k++) M[k] = (m[0][k] + m[2][k]) + m[1][k];   // (align_fold3 with the lanes' 0.0 + a done)
    return align_from_sums(M, c1, c2, kAlignSample, out, nullptr);
}

// align_fit over the members of n pairs (member null: all of them), host side -> whether the fit is valid; cnt: the members
inline bool align_fit_host(int n, const double *p1, const double *p2, const uint8_t *member, PoseState &out, int &cnt, double *gap = nullptr)
{
    static_assert(kAlignSums2 >= kAlignSums1, "one lane array serves both passes");
    double lanes[kAlignLanes][kAlignSums2];
    double S[kAlignSums2], M[kAlignSums2], c1[3], c2[3];
    for (int l = 0; l < kAlignLanes; l++)
        for (int k = 0; k < kAlignSums2; k++) lanes[l][k] = 0.0;
    cnt = 0;
    for (int i = 0; i < n; i++) {
        if (member && !member[i]) continue;
        align_add1(p1 + 3 * (size_t)i, p2 + 3 * (size_t)i, lanes[i % kAlignLanes]);
        cnt++;
    }
    pose_fold<kAlignSums2>(lanes, S);
    align_centroids(S, cnt, c1, c2);
    for (int l = 0; l < kAlignLanes; l++)
        for (int k = 0; k < kAlignSums2; k++) lanes[l][k] = 0.0;
    for (int i = 0; i < n; i++) {
        if (member && !member[i]) continue;
        align_add2(p1 + 3 * (size_t)i, p2 + 3 * (size_t)i, c1, c2, lanes[i % kAlignLanes]);
    }
    pose_fold<kAlignSums2>(lanes, M);
    return align_from_sums(M, c1, c2, cnt, out, gap);
}

// a hypothesis's record, written member by member: M may be device memory
MCORB_POSE_HD void align_write_model(AlignModel &M, bool ok, const PoseState &P, const int32_t sample[kAlignSample])
{
#pragma unroll
    for (int k = 0; k < 9; k++) M.R[k] = ok ? P.R[k] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) M.t[k] = ok ? P.t[k] : 0.0;
    M.valid = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < kAlignSample; k++) M.sample[k] = sample[k];
#pragma unroll
    for (int k = 0; k < 4; k++) M.pad[k] = 0;
}

// hypothesis h of a call: its sample (section 9j's walk on three draws), its pairs through point(i, p1, p2), its model
template <class Point>
MCORB_POSE_HD void align_hypothesis(const AlignJob &job, int h, const Point &point, AlignModel &M)
{
    int32_t sample[kAlignSample];
    bool ok = rel_sample_k<kAlignSample>(job.seed, h, job.n, sample);
    PoseState P = PoseState{};
    if (ok) {
        double p1[kAlignSample][3], p2[kAlignSample][3];
        point(sample[0], p1[0], p2[0]);
        point(sample[1], p1[1], p2[1]);
        point(sample[2], p1[2], p2[2]);
        ok = align_fit3(p1, p2, P);
    }
    align_write_model(M, ok, P, sample);
}

// the pairs of a host-only store, gathered
struct AlignHostPoint {
    const double *p1, *p2;
    inline void operator()(int i, double a[3], double b[3]) const
    {
        for (int k = 0; k < 3; k++) {
            a[k] = p1[3 * (size_t)i + k];
            b[k] = p2[3 * (size_t)i + k];
        }
    }
};

// the reference's verdict with the answer P (have: there is one): flags, count and the fold-ordered sum of the distances over n
inline void align_verdict_host(const AlignJob &job, const double *p1, const double *p2, bool have, const PoseState &P, AlignOut &out,
                               uint8_t *flags)
{
    double lanes[kAlignLanes][1], S[1];
    for (int l = 0; l < kAlignLanes; l++) lanes[l][0] = 0.0;
    out.n_inliers = 0;
    for (int i = 0; i < job.n; i++) {
        flags[i] = 0;
        if (!have) continue;
        const double d = align_dist(P, p1 + 3 * (size_t)i, p2 + 3 * (size_t)i);
        flags[i] = sac_is_inlier(d, job.inlier_dist) ? 1 : 0;
        out.n_inliers += flags[i];
        lanes[i % kAlignLanes][0] = lanes[i % kAlignLanes][0] + d;
    }
    pose_fold<1>(lanes, S);
    out.mean_error = have ? pose_default_nan(S[0] / (double)job.n) : 0.0;
}

// The kernels, serially: what a host-only store runs (mcorb_align.cpp).  p1, p2: the n pairs, gathered; models[H], count[H] (mode
// 1) and member[n] are the caller's scratch; flags: n, written.  job.n >= 1
inline void align_run_serial(const AlignJob &job, const double *p1, const double *p2, AlignModel *models, int32_t *count, uint8_t *member,
                             AlignOut &out, uint8_t *flags)
{
    const int n = job.n;
    PoseState win, ans;
    pose_identity(win);
    pose_identity(ans);
    bool have = false;
    out.used = MCORB_ALIGN_USED_SAC;
    out.sac_n_inliers = 0;
    out.best = -1;
    out.n_models = 0;
    for (int j = 0; j < kAlignSample; j++) out.sample[j] = -1;
    out.pad = 0;
    if (job.mode == MCORB_ALIGN_MODE_ALL) {
        int cnt;
        PoseState P;
        have = align_fit_host(n, p1, p2, nullptr, P, cnt);
        if (have) ans = P;
        out.used = have ? MCORB_ALIGN_USED_FIT : MCORB_ALIGN_USED_SAC;
    } else {
        const AlignHostPoint point{p1, p2};
        for (int h = 0; h < job.H; h++) {
            AlignModel &M = models[h];
            align_hypothesis(job, h, point, M);
            count[h] = 0;
            if (!M.valid) continue;
            PoseState P;
            pose_load(P, M.R, M.t);
            for (int i = 0; i < n; i++)
                count[h] += sac_is_inlier(align_dist(P, p1 + 3 * (size_t)i, p2 + 3 * (size_t)i), job.threshold) ? 1 : 0;
        }
        const ConsensusBest won = consensus_best<kRelKeyBits>(job.H, [&](int h) { return models[h].valid; }, [&](int h) { return count[h]; });
        const int best = consensus_key_index<kRelKeyBits>(won.key);
        out.best = best;
        out.n_models = won.n_models;
        if (best >= 0) {
            have = true;
            pose_load(win, models[best].R, models[best].t);
            for (int j = 0; j < kAlignSample; j++) out.sample[j] = models[best].sample[j];
            out.sac_n_inliers = count[best];
            ans = win;
            if (job.refit) {
                for (int i = 0; i < n; i++)
                    member[i] = sac_is_inlier(align_dist(win, p1 + 3 * (size_t)i, p2 + 3 * (size_t)i), job.threshold) ? 1 : 0;
                int cnt;
                PoseState P;
                if (align_fit_host(n, p1, p2, member, P, cnt)) {
                    ans = P;
                    out.used = MCORB_ALIGN_USED_FIT;
                }
            }
        }
    }
    for (int j = 0; j < 9; j++) out.R[j] = ans.R[j], out.sac_R[j] = win.R[j];
    for (int j = 0; j < 3; j++) out.t[j] = ans.t[j], out.sac_t[j] = win.t[j];
    out.status = have ? MCORB_ALIGN_OK : MCORB_ALIGN_NO_MODEL;
    align_verdict_host(job, p1, p2, have, ans, out, flags);
}

}  // namespace mcorb
