// mcorb_rel.h -- the arithmetic of the relative rig pose between two frames by RANSAC: the estimator the reference's front end
// selects by default (MCSlam/include/MCSlam/FrontEnd.h:623, posestAlgo_ = SEVENTEEN_PT), FrontEnd::poseFromSeventeenPt
// (MCSlam/src/FrontEnd.cpp:4532-4657, max_iterations_ = 10000) and LoopCloser::checkEssentialMatrix (LoopCloser.cpp:353-446, 2000
// iterations): OpenGV's sac::Ransac<NoncentralRelativePoseSacProblem>(SEVENTEENPT) on 2D-2D matches.  OpenGV is not in the tree:
// its distance (midpoint triangulation, 1 - cos in both views) is recalled, and three things are stated instead of OpenGV's
// (DESIGN.md section 9j): the draws, the linear 17-point solver (Li, Hartley and Kim's generalized epipolar constraint, E found
// before R) and the absence of the adaptive stop.  Same conventions as mcorb_sac.h: no HIP dependency -- the host-only store
// (mcorb_rel.cpp) and k_rel_hypotheses / k_rel_score / k_rel_pick (mcorb_rel_gpu.hip) run the same code -- compiled with
// -ffp-contract=off, fp64, one IEEE operation per operator in the order written, only + - * /, comparisons and sqrt (and what
// null_vector uses), every loop bounded by a count whatever the data holds.  The second half of the file is the opt-in polish of
// the winner over its inliers (rel_polish_serial, k_rel_fit), a fourth stated thing.
//   The unknown is (R, t) = b1_T_b2: X_b1 = R X_b2 + t.  Observation i is a keypoint in camera cam1 of frame 1 and one in camera
//   cam2 of frame 2; each is the body-frame ray c + l d, c = cams[cam].t, d = cams[cam].R f with f the bearing of mcorb_sac.h, and
//   m = c x d its moment.
#pragma once
#include <stdint.h>

#include "mcorb_sac.h"
#include "mcorb_triangulate.h"

namespace mcorb {

constexpr int kRelSample = 17;          // the matches of a minimal sample
constexpr int kRelDrawStride = 32;      // draw j of hypothesis h is number 1 + 32 h + j
constexpr int kRelPolish = 3;           // steps of R <- (R + R^-T) / 2
constexpr double kRelDrop = 1e-20;      // a column of A_R is dropped when this fraction of its squared length is all that remains
constexpr double kRelScale = 1e-12;     // the model is kept iff det N > kRelScale (tr N / 3)^3: the scale of t is observable
constexpr int kRelKeyBits = 14;
static_assert((1 << kRelKeyBits) == MCORB_REL_MAX_ITERATIONS, "the key holds every hypothesis index");

// a match as the kernels read it: the keypoints and cameras of the two frames
struct RelObs { float u1, v1, u2, v2; int32_t cam1, cam2; };

// a hypothesis's model: b1_T_b2, whether there is one, and the matches it was drawn from in draw order (-1: not drawn)
struct RelModel {
    double R[9], t[3];
    int32_t valid, sample[kRelSample], pad[6];
};
static_assert(sizeof(RelModel) == 192, "the kernels read models at 192-byte strides");

// one call as the kernels read it from device memory
struct RelJob {
    mcorb_track_cam cams[MCORB_MAX_CAMS];
    double threshold;
    uint64_t seed;
    int32_t ncams, S, H, pad;
};

// what k_rel_pick leaves for the host: the winner's b1_T_b2 (the identity without one), status MCORB_REL_*, the winner's count,
// its index (-1: none) and sample, and the hypotheses that had a model
struct RelOut {
    double R[9], t[3];
    int32_t status, n_inliers, best, n_models, sample[kRelSample], pad[3];
};

// a match's two rays
struct RelRays { double d1[3], c1[3], d2[3], c2[3]; };

MCORB_POSE_HD uint64_t rel_draw(uint64_t seed, int h, int j)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(1 + kRelDrawStride * (int64_t)h + j);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The sample of hypothesis h: 17 distinct members of 0 .. S - 1 by a partial Fisher-Yates walk, without rejection.  Draw j mod
// (S - j) is an index into the members not yet picked: the earlier picks are walked in ascending order and the index steps over
// each that is <= it.  sample: in draw order.  false: S < 17 (every member -1).  rel_sample_k: the same walk on K draws, which
// mcorb_align.h takes three of
template <int K>
MCORB_POSE_HD bool rel_sample_k(uint64_t seed, int h, int S, int32_t sample[K])
{
    int32_t sorted[K];
    for (int j = 0; j < K; j++) sample[j] = -1;
    if (S < K) return false;
    for (int j = 0; j < K; j++) {
        int32_t idx = (int32_t)(rel_draw(seed, h, j) % (uint64_t)(S - j));
        for (int k = 0; k < j; k++) idx += sorted[k] <= idx ? 1 : 0;
        sample[j] = idx;
        int p = j;
        for (int k = j - 1; k >= 0 && sorted[k] > idx; k--) {
            sorted[k + 1] = sorted[k];
            p = k;
        }
        sorted[p] = idx;
    }
    return true;
}
MCORB_POSE_HD bool rel_sample(uint64_t seed, int h, int S, int32_t sample[kRelSample])
{
    return rel_sample_k<kRelSample>(seed, h, S, sample);
}

MCORB_POSE_HD void rel_cross(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// R v, R row-major
MCORB_POSE_HD void rel_rot(const double R[9], const double v[3], double out[3])
{
    out[0] = (R[0] * v[0] + R[1] * v[1]) + R[2] * v[2];
    out[1] = (R[3] * v[0] + R[4] * v[1]) + R[5] * v[2];
    out[2] = (R[6] * v[0] + R[7] * v[1]) + R[8] * v[2];
}

MCORB_POSE_HD void rel_rays(const mcorb_track_cam *cams, const RelObs &o, RelRays &r)
{
    double f[3];
    sac_bearing(cams[o.cam1], o.u1, o.v1, f);
    sac_ray(cams[o.cam1], f, r.c1, r.d1);
    sac_bearing(cams[o.cam2], o.u2, o.v2, f);
    sac_ray(cams[o.cam2], f, r.c2, r.d2);
}

// the rays of a match whose keypoints are given in double, for the host hooks: sac_bearing's arithmetic operator by operator, so a
// float's value gives rel_rays' bits; a keypoint that no float holds lets a test state a noise-free problem in both frames
MCORB_POSE_HD void rel_bearing_d(const mcorb_track_cam &cam, double u, double v, double f[3])
{
    const double y = (v - cam.v0) / cam.fy;
    const double x = ((u - cam.u0) - cam.s * y) / cam.fx;
    const double n = __builtin_sqrt((x * x + y * y) + 1.0);
    f[0] = x / n;
    f[1] = y / n;
    f[2] = 1.0 / n;
}
MCORB_POSE_HD void rel_rays_d(const mcorb_track_cam *cams, int cam1, const double uv1[2], int cam2, const double uv2[2], RelRays &r)
{
    double f[3];
    rel_bearing_d(cams[cam1], uv1[0], uv1[1], f);
    sac_ray(cams[cam1], f, r.c1, r.d1);
    rel_bearing_d(cams[cam2], uv2[0], uv2[1], f);
    sac_ray(cams[cam2], f, r.c2, r.d2);
}

// the cofactor matrix (not its transpose) of a 3 x 3 matrix, row-major: its rows are the cross products of the other two rows
MCORB_POSE_HD void rel_cof(const double A[9], double C[9])
{
    rel_cross(A + 3, A + 6, C);
    rel_cross(A + 6, A, C + 3);
    rel_cross(A, A + 3, C + 6);
}

// t of the 17 equations g_i . t = h_i at the rotation R, g_i = (R d2) x d1, h_i = -(d1 . R m2 + m1 . R d2), by the 3 x 3 normal
// equations N t = r solved by cofactors -> the sum of squared residuals; det and tr are N's
MCORB_POSE_HD double rel_translation(const double R[9], const RelRays *rays, const double (*m1)[3], const double (*m2)[3], double t[3],
                                     double &det, double &tr)
{
    double N00 = 0.0, N01 = 0.0, N02 = 0.0, N11 = 0.0, N12 = 0.0, N22 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int i = 0; i < kRelSample; i++) {
        double b[3], Rm[3], g[3];
        rel_rot(R, rays[i].d2, b);
        rel_rot(R, m2[i], Rm);
        rel_cross(b, rays[i].d1, g);
        const double h = -(sac_dot(rays[i].d1, Rm) + sac_dot(m1[i], b));
        N00 += g[0] * g[0];
        N01 += g[0] * g[1];
        N02 += g[0] * g[2];
        N11 += g[1] * g[1];
        N12 += g[1] * g[2];
        N22 += g[2] * g[2];
        r0 += g[0] * h;
        r1 += g[1] * h;
        r2 += g[2] * h;
    }
    const double c00 = N11 * N22 - N12 * N12, c01 = N12 * N02 - N01 * N22, c02 = N01 * N12 - N11 * N02;
    const double c11 = N00 * N22 - N02 * N02, c12 = N01 * N02 - N00 * N12, c22 = N00 * N11 - N01 * N01;
    det = (N00 * c00 + N01 * c01) + N02 * c02;
    tr = (N00 + N11) + N22;
    t[0] = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
    t[1] = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
    t[2] = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
    double res = 0.0;
    for (int i = 0; i < kRelSample; i++) {
        double b[3], Rm[3], g[3];
        rel_rot(R, rays[i].d2, b);
        rel_rot(R, m2[i], Rm);
        rel_cross(b, rays[i].d1, g);
        const double h = -(sac_dot(rays[i].d1, Rm) + sac_dot(m1[i], b));
        const double e = sac_dot(g, t) - h;
        res += e * e;
    }
    return res;
}

// Two steps of refinement of B's null vector e (unit length) against B itself: e <- normalise(e - M^-1 B^T (B e)) with M = B^T B +
// (tr / 9) e e^T factored once as L D L^T.  null_vector works on the Gram matrix, whose rounding moves the vector by eps (s_max /
// s_2)^2 with s_2 the smallest singular value but one of B -- 1e-4 on the worst of 12 000 noise-free samples, where s_2 / s_max
// is 1e-6; the residual B e is taken from B, so a step leaves eps s_max / s_2.  A pivot that is not > 0: e stays as it is
MCORB_POSE_HD void rel_refine_null(const double *B, double e[9])
{
    double M[81], L[81], D[9];
    double tr = 0.0;
    for (int p = 0; p < 9; p++)
        for (int q = p; q < 9; q++) {
            double acc = 0.0;
            for (int i = 0; i < kRelSample; i++) acc += B[9 * i + p] * B[9 * i + q];
            M[9 * p + q] = M[9 * q + p] = acc;
            if (p == q) tr += acc;
        }
    const double mu = tr / 9.0;
    for (int p = 0; p < 9; p++)
        for (int q = 0; q < 9; q++) M[9 * p + q] += mu * (e[p] * e[q]);
    bool ok = true;
    for (int j = 0; j < 9; j++) {
        double d = M[9 * j + j];
        for (int k = 0; k < j; k++) d -= (L[9 * j + k] * L[9 * j + k]) * D[k];
        ok = ok && d > 0.0;
        D[j] = d;
        for (int i = j + 1; i < 9; i++) {
            double a = M[9 * i + j];
            for (int k = 0; k < j; k++) a -= (L[9 * i + k] * L[9 * j + k]) * D[k];
            L[9 * i + j] = a / d;
        }
    }
    if (!ok) return;
    for (int step = 0; step < 2; step++) {
        double g[9];
        for (int p = 0; p < 9; p++) g[p] = 0.0;
        for (int i = 0; i < kRelSample; i++) {
            double r = 0.0;
            for (int p = 0; p < 9; p++) r += B[9 * i + p] * e[p];
            for (int p = 0; p < 9; p++) g[p] += B[9 * i + p] * r;
        }
        for (int i = 0; i < 9; i++)
            for (int k = 0; k < i; k++) g[i] -= L[9 * i + k] * g[k];
        for (int i = 0; i < 9; i++) g[i] = g[i] / D[i];
        for (int i = 8; i >= 0; i--)
            for (int k = i + 1; k < 9; k++) g[i] -= L[9 * k + i] * g[k];
        double nn = 0.0;
        for (int p = 0; p < 9; p++) {
            e[p] -= g[p];
            nn += e[p] * e[p];
        }
        nn = __builtin_sqrt(nn);
        for (int p = 0; p < 9; p++) e[p] = e[p] / nn;
    }
}

// The linear 17-point solver (stated; Li, Hartley and Kim's method, which OpenGV's seventeenpt cites) on the rays of 17 matches.
// The generalized epipolar constraint is d1^T E d2 + d1^T R m2 + m1^T R d2 = 0 with E = [t]x R; per row A_E = vec(d1 d2^T) and
// A_R = vec(d1 m2^T + m1 d2^T), row-major.  When a match has the same camera in both frames (E, R) = (0, I) is always in the
// null space of [A_E | A_R], so E is found first:
//   0. The origin is moved to o, the centre of the first match's frame-1 camera, for the solve: m = (c - o) x d, and t = t' - R o
//      + o at the end.  A sample whose rays all leave one centre then has m = 0 exactly -- every column of A_R is dropped, E is
//      the eight-point essential matrix and step 7 refuses it; about the body's origin such a sample's A_R lies in A_E's column
//      space and E would be any vector of an eight-dimensional null space.
//   1. A_R's 9 columns (length 17) are orthonormalised by modified Gram-Schmidt, two passes; a column whose remainder has v.v <=
//      kRelDrop x its original v.v is dropped.
//   2. B = A_E - Q (Q^T A_E), column by column, each projection taken off the running remainder.
//   3. e = null_vector(B, 17, 9), refined against B (rel_refine_null), scaled so that |E|_F^2 = 2.
//   4. t^ is the longest of the three cross products of E's columns (the first of equals), normalised.
//   5. R+- = cof(E) -+ [t^]x E: exact for a true essential matrix, [t]x E = (t t^T - I) R and cof([t]x R) = t t^T R.  Each takes
//      kRelPolish steps of R <- (R + R^-T) / 2, the inverse by cofactors.
//   6. For each, t by rel_translation; the candidate with the smaller sum of squared residuals wins, a tie goes to +, a NaN
//      never wins.
//   7. The model is kept iff its 12 numbers are finite, det N > kRelScale (tr N / 3)^3 and step 1 kept a column: a central rig,
//      whose scale is not observable, gets no model and never a pose with an invented scale.  (The determinant alone refuses a
//      central sample only while it is noise-free: the rounding of its keypoints to float already lifts N's smallest eigenvalue
//      to 1e-13 of the others, and every h_i is exactly zero there, so t' would be 0 -- a camera that did not move.)
MCORB_POSE_HD bool rel_solve17(const RelRays *rays, PoseState &out)
{
    // 0. the moments about o, the centre of the first match's frame-1 camera
    const double o[3] = {rays[0].c1[0], rays[0].c1[1], rays[0].c1[2]};
    double m1[kRelSample][3], m2[kRelSample][3];
    for (int i = 0; i < kRelSample; i++) {
        const double a1[3] = {rays[i].c1[0] - o[0], rays[i].c1[1] - o[1], rays[i].c1[2] - o[2]};
        const double a2[3] = {rays[i].c2[0] - o[0], rays[i].c2[1] - o[1], rays[i].c2[2] - o[2]};
        rel_cross(a1, rays[i].d1, m1[i]);
        rel_cross(a2, rays[i].d2, m2[i]);
    }
    // 1. Q: the kept columns, column k at Q + 17 k
    double Q[9 * kRelSample];
    int nq = 0;
    for (int col = 0; col < 9; col++) {
        const int a = col / 3, b = col % 3;
        double *v = Q + kRelSample * nq;
        double orig = 0.0;
        for (int i = 0; i < kRelSample; i++) {
            v[i] = rays[i].d1[a] * m2[i][b] + m1[i][a] * rays[i].d2[b];
            orig += v[i] * v[i];
        }
        for (int pass = 0; pass < 2; pass++)
            for (int k = 0; k < nq; k++) {
                const double *q = Q + kRelSample * k;
                double dot = 0.0;
                for (int i = 0; i < kRelSample; i++) dot += q[i] * v[i];
                for (int i = 0; i < kRelSample; i++) v[i] -= dot * q[i];
            }
        double rem = 0.0;
        for (int i = 0; i < kRelSample; i++) rem += v[i] * v[i];
        if (rem > kRelDrop * orig) {   // (false for a NaN too)
            const double inv = 1.0 / __builtin_sqrt(rem);
            for (int i = 0; i < kRelSample; i++) v[i] *= inv;
            nq++;
        }
    }
    // 2. B, row-major 17 x 9
    double B[kRelSample * 9];
    for (int col = 0; col < 9; col++) {
        const int a = col / 3, b = col % 3;
        for (int i = 0; i < kRelSample; i++) B[9 * i + col] = rays[i].d1[a] * rays[i].d2[b];
        for (int k = 0; k < nq; k++) {
            const double *q = Q + kRelSample * k;
            double dot = 0.0;
            for (int i = 0; i < kRelSample; i++) dot += q[i] * B[9 * i + col];
            for (int i = 0; i < kRelSample; i++) B[9 * i + col] -= dot * q[i];
        }
    }
    // 3.
    double E[9];
    null_vector_t<kRelSample, 9>(B, kRelSample, 9, E);   // (null_vector's arithmetic with the shape known)
    rel_refine_null(B, E);
    double nn = 0.0;
    for (int j = 0; j < 9; j++) nn += E[j] * E[j];
    const double scale = __builtin_sqrt(2.0 / nn);
    for (int j = 0; j < 9; j++) E[j] *= scale;
    // 4.
    const double e0[3] = {E[0], E[3], E[6]}, e1[3] = {E[1], E[4], E[7]}, e2[3] = {E[2], E[5], E[8]};
    double x01[3], x12[3], x20[3];
    rel_cross(e0, e1, x01);
    rel_cross(e1, e2, x12);
    rel_cross(e2, e0, x20);
    const double n01 = sac_dot(x01, x01), n12 = sac_dot(x12, x12), n20 = sac_dot(x20, x20);
    double th[3] = {x01[0], x01[1], x01[2]}, tn = n01;
    if (n12 > tn) {
        th[0] = x12[0], th[1] = x12[1], th[2] = x12[2];
        tn = n12;
    }
    if (n20 > tn) {
        th[0] = x20[0], th[1] = x20[1], th[2] = x20[2];
        tn = n20;
    }
    tn = __builtin_sqrt(tn);
    th[0] = th[0] / tn;
    th[1] = th[1] / tn;
    th[2] = th[2] / tn;
    // 5.
    double C[9], TE[9];
    rel_cof(E, C);
    for (int j = 0; j < 3; j++) {
        TE[j] = th[1] * E[6 + j] - th[2] * E[3 + j];
        TE[3 + j] = th[2] * E[j] - th[0] * E[6 + j];
        TE[6 + j] = th[0] * E[3 + j] - th[1] * E[j];
    }
    PoseState cand[2];
    double res[2], det[2], tr[2];
    for (int s = 0; s < 2; s++) {
        double *R = cand[s].R;
        for (int j = 0; j < 9; j++) R[j] = s == 0 ? C[j] - TE[j] : C[j] + TE[j];
        for (int it = 0; it < kRelPolish; it++) {
            double K[9];
            rel_cof(R, K);
            const double dR = (R[0] * K[0] + R[1] * K[1]) + R[2] * K[2];
            for (int j = 0; j < 9; j++) R[j] = 0.5 * (R[j] + K[j] / dR);
        }
        // 6.
        res[s] = rel_translation(R, rays, m1, m2, cand[s].t, det[s], tr[s]);
    }
    const bool minus = res[1] == res[1] && (!(res[0] == res[0]) || res[1] < res[0]);
    const int w = minus ? 1 : 0;
    out = cand[w];
    // (back to the body's origin)
    double Ro[3];
    rel_rot(out.R, o, Ro);
    for (int j = 0; j < 3; j++) out.t[j] = (out.t[j] - Ro[j]) + o[j];
    // 7.
    bool ok = res[w] == res[w];
    for (int j = 0; j < 9; j++) ok = ok && sac_finite(out.R[j]);
    for (int j = 0; j < 3; j++) ok = ok && sac_finite(out.t[j]);
    const double third = tr[w] / 3.0;
    return ok && nq > 0 && det[w] > kRelScale * ((third * third) * third);
}

// OpenGV's distance of the non-central relative problem, recalled: the midpoint of the two rays' closest points, then 1 - cos
// between each ray and the midpoint's direction from its camera, summed.  In frame 1's body frame with a = d1, b = R d2 and
// w = (R c2 + t) - c1.  Parallel rays and a midpoint at a centre give NaN; a point behind either camera scores near 2
MCORB_POSE_HD double rel_score(const PoseState &P, const RelRays &r)
{
    double b[3], Rc[3], w[3], P1[3], P2[3];
    rel_rot(P.R, r.d2, b);
    rel_rot(P.R, r.c2, Rc);
    const double *a = r.d1;
    for (int i = 0; i < 3; i++) w[i] = (Rc[i] + P.t[i]) - r.c1[i];
    const double aa = sac_dot(a, a), ab = sac_dot(a, b), bb = sac_dot(b, b), aw = sac_dot(a, w), bw = sac_dot(b, w);
    const double det = ab * ab - aa * bb;
    const double lambda = (ab * bw - bb * aw) / det;
    const double mu = (aa * bw - ab * aw) / det;
    for (int i = 0; i < 3; i++) {
        P1[i] = 0.5 * ((lambda * a[i]) + (w[i] + mu * b[i]));
        P2[i] = P1[i] - w[i];
    }
    return (1.0 - sac_dot(a, P1) / __builtin_sqrt(sac_dot(P1, P1))) + (1.0 - sac_dot(b, P2) / __builtin_sqrt(sac_dot(P2, P2) * bb));
}

// a hypothesis's record, written member by member: M may be device memory
MCORB_POSE_HD void rel_write_model(RelModel &M, bool ok, const PoseState &P, const int32_t sample[kRelSample])
{
    for (int k = 0; k < 9; k++) M.R[k] = ok ? P.R[k] : 0.0;
    for (int k = 0; k < 3; k++) M.t[k] = ok ? P.t[k] : 0.0;
    M.valid = ok ? 1 : 0;
    for (int k = 0; k < kRelSample; k++) M.sample[k] = sample[k];
    for (int k = 0; k < 6; k++) M.pad[k] = 0;
}

// hypothesis h of a call: its sample, the rays of its matches, its model
MCORB_POSE_HD void rel_hypothesis(const RelJob &job, int h, const RelObs *obs, RelModel &M)
{
    int32_t sample[kRelSample];
    bool ok = rel_sample(job.seed, h, job.S, sample);
    PoseState P = PoseState{};
    if (ok) {
        RelRays rays[kRelSample];
        for (int j = 0; j < kRelSample; j++) rel_rays(job.cams, obs[sample[j]], rays[j]);
        ok = rel_solve17(rays, P);
    }
    rel_write_model(M, ok, P, sample);
}

// The three kernels, serially: what a host-only store runs (mcorb_rel.cpp).  models[H], count[H] and rays[S] are the caller's
// scratch; flags: S, written.  job.S >= 1
inline void rel_run_serial(const RelJob &job, const RelObs *obs, RelModel *models, int32_t *count, RelRays *rays, RelOut &out, uint8_t *flags)
{
    for (int k = 0; k < job.S; k++) rel_rays(job.cams, obs[k], rays[k]);
    PoseState P;
    for (int h = 0; h < job.H; h++) {
        RelModel &M = models[h];
        rel_hypothesis(job, h, obs, M);
        count[h] = 0;
        if (!M.valid) continue;
        pose_load(P, M.R, M.t);
        for (int k = 0; k < job.S; k++) count[h] += sac_is_inlier(rel_score(P, rays[k]), job.threshold) ? 1 : 0;
    }
    const ConsensusBest won = consensus_best<kRelKeyBits>(job.H, [&](int h) { return models[h].valid; }, [&](int h) { return count[h]; });
    const int best = consensus_key_index<kRelKeyBits>(won.key);
    pose_identity(P);
    if (best >= 0) pose_load(P, models[best].R, models[best].t);
    for (int k = 0; k < job.S; k++) flags[k] = best >= 0 && sac_is_inlier(rel_score(P, rays[k]), job.threshold) ? 1 : 0;
    for (int j = 0; j < 9; j++) out.R[j] = P.R[j];
    for (int j = 0; j < 3; j++) out.t[j] = P.t[j];
    out.status = best >= 0 ? MCORB_REL_OK : MCORB_REL_NO_MODEL;
    out.n_inliers = best >= 0 ? count[best] : 0;
    out.best = best;
    out.n_models = won.n_models;
    for (int j = 0; j < kRelSample; j++) out.sample[j] = best >= 0 ? models[best].sample[j] : -1;
    for (int j = 0; j < 3; j++) out.pad[j] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The polish of the winner over its inliers (mcorb_lmap_relative_pose_polished): mcorb_pose.h's Levenberg-Marquardt -- pose_round,
// pose_solve, pose_retract -- on a cost that is stated here (OpenGV's optimizeModelCoefficients for this problem is not in the
// tree and the reference does not call it).
//   the residual of a match at P   with rel_score's a, b = R d2, w, P1 and P2 = P1 - w the 6-vector
//                                  (a - P1 / |P1|, b / |b| - P2 / |P2|) * (1 / sqrt(threshold)): its squared length is 2 score /
//                                  threshold, so an inlier adds less than 2 to the cost and pose_round's absolute stop at 1e-6
//                                  is on the scale of the inlier test.  A NaN residual makes the cost NaN: the trial is rejected
//   the Jacobian                   forward differences through pose_retract itself: column k is (r(retract(P, h e_k)) - r(P)) *
//                                  2^20 with h = 2^-20; the six perturbed poses are computed once per pass (rel_fit_poses)
//   the sums                       mcorb_pose.h's 28: J^T J, J^T r and the cost r.r; match i goes to lane i mod 256 in ascending
//                                  i, the lanes fold as pose_fold
//   the rounds                     one or two: pose_round over the members from the current pose, then all S matches are scored
//                                  at the result with rel_score < threshold; the result replaces the current pose, flags and
//                                  count iff its count is at least the current one, otherwise polishing ends.  Round 1's members
//                                  are the winner's flags, round 2's are round 1's
constexpr int kRelFitPoses = 7;                         // P and its six perturbations
constexpr double kRelFitH = 1.0 / 1048576.0, kRelFitInvH = 1048576.0;
constexpr int kRelFitRounds = MCORB_REL_POLISH_ROUNDS, kRelFitMaxIterations = MCORB_REL_POLISH_MAX_ITERATIONS;

// what the polished path's k_rel_fit leaves for the host next to the RelOut: the layout of mcorb_rel_polish
typedef mcorb_rel_polish RelPolish;

// pose k of a pass: P itself (k = 0) or retract(P, h e_(k - 1)).  k may be a run-time value: nothing is indexed by it
MCORB_POSE_HD void rel_fit_pose(const PoseState &P, int k, PoseState &Q)
{
    const double delta[6] = {k == 1 ? kRelFitH : 0.0, k == 2 ? kRelFitH : 0.0, k == 3 ? kRelFitH : 0.0,
                             k == 4 ? kRelFitH : 0.0, k == 5 ? kRelFitH : 0.0, k == 6 ? kRelFitH : 0.0};
    PoseState T;
    pose_retract(P, delta, T);
#pragma unroll
    for (int j = 0; j < 9; j++) Q.R[j] = k == 0 ? P.R[j] : T.R[j];
#pragma unroll
    for (int j = 0; j < 3; j++) Q.t[j] = k == 0 ? P.t[j] : T.t[j];
}

// 1 / sqrt(threshold), the scale of the residual
MCORB_POSE_HD double rel_fit_scale(double threshold) { return 1.0 / __builtin_sqrt(threshold); }

MCORB_POSE_HD void rel_residual(const PoseState &P, const RelRays &r, double scale, double res[6])
{
    double b[3], Rc[3], w[3], P1[3], P2[3];
    rel_rot(P.R, r.d2, b);
    rel_rot(P.R, r.c2, Rc);
    const double *a = r.d1;
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = (Rc[i] + P.t[i]) - r.c1[i];
    const double aa = sac_dot(a, a), ab = sac_dot(a, b), bb = sac_dot(b, b), aw = sac_dot(a, w), bw = sac_dot(b, w);
    const double det = ab * ab - aa * bb;
    const double lambda = (ab * bw - bb * aw) / det;
    const double mu = (aa * bw - ab * aw) / det;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        P1[i] = 0.5 * ((lambda * a[i]) + (w[i] + mu * b[i]));
        P2[i] = P1[i] - w[i];
    }
    const double n1 = __builtin_sqrt(sac_dot(P1, P1)), n2 = __builtin_sqrt(sac_dot(P2, P2)), nb = __builtin_sqrt(bb);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        res[i] = (a[i] - P1[i] / n1) * scale;
        res[3 + i] = (b[i] / nb - P2[i] / n2) * scale;
    }
}

// one member into a lane's 28 sums.  poses: the kRelFitPoses poses of the pass (LDS on the device), read at constant indices;
// s[k]: the sums, an array or k_rel_fit's column of LDS
template <class Sums>
MCORB_POSE_HD void rel_fit_add(const PoseState *poses, const RelRays &r, double scale, Sums &s)
{
    double r0[6], J[6][6];   // J[k]: column k
    rel_residual(poses[0], r, scale, r0);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        double rk[6];
        rel_residual(poses[1 + k], r, scale, rk);
#pragma unroll
        for (int c = 0; c < 6; c++) J[k][c] = (rk[c] - r0[c]) * kRelFitInvH;
    }
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++, at++) {
            double acc = J[i][0] * J[j][0];
#pragma unroll
            for (int c = 1; c < 6; c++) acc = acc + J[i][c] * J[j][c];
            s[at] = s[at] + acc;
        }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double acc = J[i][0] * r0[0];
#pragma unroll
        for (int c = 1; c < 6; c++) acc = acc + J[i][c] * r0[c];
        s[kPoseG + i] = s[kPoseG + i] + acc;
    }
    double e2 = r0[0] * r0[0];
#pragma unroll
    for (int c = 1; c < 6; c++) e2 = e2 + r0[c] * r0[c];
    s[kPoseCost] = s[kPoseCost] + e2;
}

// a polish record before any round: the winner's pose and count, every round empty
MCORB_POSE_HD void rel_polish_begin(RelPolish &rec, const PoseState &win, int32_t count)
{
    for (int j = 0; j < 9; j++) rec.R[j] = win.R[j];
    for (int j = 0; j < 3; j++) rec.t[j] = win.t[j];
    for (int k = 0; k < kRelFitRounds; k++) {
        mcorb_rel_polish_round &q = rec.round[k];
        q.cost_initial = q.cost_final = 0.0;
        q.n_members = q.iterations = q.status = q.n_inliers = q.accepted = q.reserved = 0;
    }
    rec.n_inliers = count;
    rec.rounds_run = 0;
}

// a pass of the serial run: the fold-ordered sums at P over the members
struct RelFitSerialPass {
    const RelRays *rays;
    const uint8_t *member;
    int S;
    double scale;
    double (*lanes)[kPoseSums];   // [MCORB_POSE_LANES]
    void operator()(const PoseState &P, double sums[kPoseSums])
    {
        PoseState poses[kRelFitPoses];
        for (int k = 0; k < kRelFitPoses; k++) rel_fit_pose(P, k, poses[k]);
        for (int l = 0; l < MCORB_POSE_LANES; l++) {
            for (int k = 0; k < kPoseSums; k++) lanes[l][k] = 0.0;
            for (int i = l; i < S; i += MCORB_POSE_LANES)
                if (member[i]) rel_fit_add(poses, rays[i], scale, lanes[l]);
        }
        pose_fold(lanes, sums);
    }
};

// The rounds, serially: what a host-only store runs behind rel_run_serial, and the hook.  pose / count / flags: the current
// ones (the winner's) in, the accepted ones out; member: round 1's members, S bytes, overwritten; scratch (S bytes) and lanes
// are the caller's
inline void rel_polish_serial(const RelRays *rays, int S, double threshold, int rounds, int max_iterations, PoseState &pose, int32_t &count,
                              uint8_t *flags, uint8_t *member, uint8_t *scratch, double (*lanes)[kPoseSums], RelPolish &rec)
{
    static_assert(MCORB_POSE_LANES == 256, "match i is lane i mod 256's");
    RelFitSerialPass pass{rays, member, S, rel_fit_scale(threshold), lanes};
    rel_polish_begin(rec, pose, count);
    for (int round = 0; round < rounds; round++) {
        mcorb_rel_polish_round &q = rec.round[round];
        int32_t members = 0;
        for (int i = 0; i < S; i++) members += member[i] ? 1 : 0;
        PoseState cand;
        double c0, c1;
        pose_round(pass, pose, max_iterations, cand, q.iterations, q.status, c0, c1);
        int32_t n = 0;
        for (int i = 0; i < S; i++) {
            scratch[i] = sac_is_inlier(rel_score(cand, rays[i]), threshold) ? 1 : 0;
            n += scratch[i];
        }
        q.cost_initial = pose_default_nan(c0);
        q.cost_final = pose_default_nan(c1);
        q.n_members = members;
        q.n_inliers = n;
        q.accepted = n >= count ? 1 : 0;
        rec.rounds_run = round + 1;
        if (!q.accepted) break;
        pose = cand;
        count = n;
        for (int i = 0; i < S; i++) flags[i] = member[i] = scratch[i];
    }
}

}  // namespace mcorb
