// mcorb_sac.h -- the arithmetic of the absolute rig pose by RANSAC in front of the refinement: the consensus step the reference
// runs through OpenGV's sac::Ransac<AbsolutePoseSacProblem>(GP3P) (MCSlam/src/FrontEnd.cpp:4660-4798, threshold_ = 1 -
// cos(atan(sqrt(2) * 0.5 / K[0](0, 2))), max_iterations_ = 100).  OpenGV is not in the tree: its reprojection distance is
// recalled, and three things are stated instead of OpenGV's: the draws, the minimal solver (solver 0: a
// central P3P in the camera of the sample; solver 1: a generalized solver that samples across cameras, Newton on the non-central
// rays from the central solutions, which finds at most 4 of the problem's up to 8 solutions; neither is OpenGV's GP3P) and the
// absence of the adaptive stop.  Same conventions as mcorb_pose.h: no HIP dependency -- the host-only store (mcorb_sac.cpp) and
// k_sac_hypotheses / k_sac_hypotheses_rig / k_sac_score / k_sac_pick (mcorb_sac_gpu.hip) run the same code -- compiled with -ffp-contract=off, fp64, one IEEE operation per operator in the order written, only + - * /,
// comparisons and sqrt, every loop bounded by a count whatever the data holds.
#pragma once
#include <stdint.h>

#include "mcorb_consensus.h"
#include "mcorb_pose.h"

namespace mcorb {

constexpr int kSacDraws = 16;      // the draws of a hypothesis, the first included
constexpr int kSacBisect = 64;     // bracketing steps for the resolvent cubic's root
constexpr int kSacCubicNewton = 4, kSacQuarticNewton = 3;
#ifndef MCORB_SAC_RIG_NEWTON
#define MCORB_SAC_RIG_NEWTON 20   // measured against 8, 10, 12, 16 and 24 (make EXTRA=-DMCORB_SAC_RIG_NEWTON=..)
#endif
constexpr int kSacRigNewton = MCORB_SAC_RIG_NEWTON;   // the rig solver's Newton steps on the three distance equations
constexpr double kSacSelf = 1e-12;   // a solution is kept iff its own three points score below this

// a hypothesis's model: w_T_b, whether there is one, and the observations it was drawn from (-1: not drawn)
struct SacModel {
    double R[9], t[3];
    int32_t valid, sample[4], pad[3];
};
static_assert(sizeof(SacModel) == 128, "the kernels read models at 128-byte strides");

// one call as the kernels read it from device memory: the rig, the threshold, the seed, n observations of which S are the
// consensus set (the first of each match), H hypotheses, the minimal solver (MCORB_SAC_SOLVER_*)
struct SacJob {
    mcorb_track_cam cams[MCORB_MAX_CAMS];
    double threshold;
    uint64_t seed;
    int32_t ncams, n, S, H;
    int32_t solver, pad;
};

// what k_sac_pick leaves for the host: the winner's w_T_b (the identity without one), status MCORB_SAC_*, the winner's count,
// its index (-1: none) and sample, and the hypotheses that had a model
struct SacOut {
    double R[9], t[3];
    int32_t status, n_inliers, best, n_models, sample[4];
};

// draw j of hypothesis h: the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (1 + 16 h + j), 64-bit integers only
MCORB_POSE_HD uint64_t sac_draw(uint64_t seed, int h, int j)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(1 + 16 * h + j);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The sample of hypothesis h.  cons: the S consensus observations in input order; cam_first / cam_cons: the same observations
// camera by camera, each camera's in input order.  Draw 0 mod S picks the first member, whose camera c is the hypothesis's;
// draws 1 .. 15 mod S_c pick from that camera's, a draw equal to an earlier member being dropped.  false: S_c < 4 or the draws
// ran out (the members not drawn are -1)
MCORB_POSE_HD bool sac_sample(uint64_t seed, int h, int S, const int32_t *cons, const PoseObs *obs, const int32_t *cam_first,
                              const int32_t *cam_cons, int32_t &s0, int32_t &s1, int32_t &s2, int32_t &s3)
{
    s0 = cons[sac_draw(seed, h, 0) % (uint64_t)S];
    s1 = s2 = s3 = -1;
    const int c = obs[s0].cam, b = cam_first[c], Sc = cam_first[c + 1] - b;
    if (Sc < 4) return false;
    int have = 1;
    // (selects, not branches: members chosen by `have` under a branch become a run-time-indexed array in scratch)
    for (int j = 1; j < kSacDraws; j++) {
        const int32_t i = cam_cons[b + (int)(sac_draw(seed, h, j) % (uint64_t)Sc)];
        const bool fresh = have < 4 && i != s0 && i != s1 && i != s2;
        s1 = (fresh && have == 1) ? i : s1;
        s2 = (fresh && have == 2) ? i : s2;
        s3 = (fresh && have == 3) ? i : s3;
        have += fresh ? 1 : 0;
    }
    return have == 4;
}

// The sample of hypothesis h for the rig solver: all 16 draws mod S pick from the consensus list in input order, whatever their
// cameras, a draw equal to an earlier member being dropped.  false: fewer than four members after the 16 draws (S < 4 among
// them; the members not drawn are -1)
MCORB_POSE_HD bool sac_sample_rig(uint64_t seed, int h, int S, const int32_t *cons, int32_t &s0, int32_t &s1, int32_t &s2, int32_t &s3)
{
    s0 = cons[sac_draw(seed, h, 0) % (uint64_t)S];
    s1 = s2 = s3 = -1;
    int have = 1;
    for (int j = 1; j < kSacDraws; j++) {
        const int32_t i = cons[sac_draw(seed, h, j) % (uint64_t)S];
        const bool fresh = have < 4 && i != s0 && i != s1 && i != s2;
        s1 = (fresh && have == 1) ? i : s1;
        s2 = (fresh && have == 2) ? i : s2;
        s3 = (fresh && have == 3) ? i : s3;
        have += fresh ? 1 : 0;
    }
    return have == 4;
}

// the bearing of a keypoint (FrontEnd.cpp:4693-4701, with the skew the refinement's calibration has)
MCORB_POSE_HD void sac_bearing(const mcorb_track_cam &cam, float u, float v, double f[3])
{
    const double y = ((double)v - cam.v0) / cam.fy;
    const double x = (((double)u - cam.u0) - cam.s * y) / cam.fx;
    const double n = __builtin_sqrt((x * x + y * y) + 1.0);
    f[0] = x / n;
    f[1] = y / n;
    f[2] = 1.0 / n;
}

// OpenGV's reprojection distance of a non-central adapter, recalled: 1 - f . q / |q| with q the point in the camera's frame
MCORB_POSE_HD double sac_score(const mcorb_track_cam &cam, const PoseState &P, const double X[3], const double f[3])
{
    double pb[3], q[3];
    pose_body(P, X, pb);
    pose_cam(cam, pb, q);
    return 1.0 - ((f[0] * q[0] + f[1] * q[1]) + f[2] * q[2]) / __builtin_sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
}

// strict, and a NaN is not an inlier
MCORB_POSE_HD bool sac_is_inlier(double score, double threshold) { return score < threshold; }

MCORB_POSE_HD bool sac_finite(double x) { return (x - x) == 0.0; }
MCORB_POSE_HD double sac_abs(double x) { return x < 0.0 ? -x : x; }
MCORB_POSE_HD double sac_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the orthonormal triad of a triangle, as columns: e1 along B - A, e3 along e1 x (C - A), e2 = e3 x e1
MCORB_POSE_HD void sac_triad(const double A[3], const double B[3], const double C[3], double e1[3], double e2[3], double e3[3])
{
    const double x0 = B[0] - A[0], x1 = B[1] - A[1], x2 = B[2] - A[2];
    const double y0 = C[0] - A[0], y1 = C[1] - A[1], y2 = C[2] - A[2];
    const double nx = __builtin_sqrt((x0 * x0 + x1 * x1) + x2 * x2);
    e1[0] = x0 / nx;
    e1[1] = x1 / nx;
    e1[2] = x2 / nx;
    const double z0 = e1[1] * y2 - e1[2] * y1, z1 = e1[2] * y0 - e1[0] * y2, z2 = e1[0] * y1 - e1[1] * y0;
    const double nz = __builtin_sqrt((z0 * z0 + z1 * z1) + z2 * z2);
    e3[0] = z0 / nz;
    e3[1] = z1 / nz;
    e3[2] = z2 / nz;
    e2[0] = e3[1] * e1[2] - e3[2] * e1[1];
    e2[1] = e3[2] * e1[0] - e3[0] * e1[2];
    e2[2] = e3[0] * e1[1] - e3[1] * e1[0];
}

// Grunert's quartic of three rays and three points, and what its roots need: shared by the two minimal solvers.
//   With s_i the depths along the unit directions f_i, s2 = u s1, s3 = v s1, a2 = |P2 - P3|^2, b2 = |P1 - P3|^2, c2 = |P1 - P2|^2,
//   ca = f2.f3, cb = f1.f3, cg = f1.f2, K = (a2 - c2) / b2 and Cq = c2 / b2 the law of cosines gives u = N(v) / D(v) with N = (K -
//   1) v^2 - 2 K cb v + (1 + K), D = 2 (cg - ca v), and the quartic E(v) = D^2 + N^2 - 2 cg N D - Cq (v^2 - 2 cb v + 1) D^2 = 0, whose
//   coefficients are multiplied out below.
//   The quartic, made monic (a, b, c, d), is depressed by v = y - a / 4 to y^4 + p y^2 + q y + r and solved after Ferrari: m is
//   a root > 0 of g(m) = m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8, found by kSacBisect halvings of [0, 1 + max(|p|, |p^2 / 4 -
//   r|, q^2 / 8)] (g(0) <= 0 < g(hi)) and kSacCubicNewton Newton steps; with s = sqrt(2 m), e = q / (2 s) the roots are those of
//   y^2 - s y + (p / 2 + m + e) and y^2 + s y + (p / 2 + m - e), root k = 0 .. 3 being (+s + w1) / 2, (+s - w1) / 2, (-s + w2) /
//   2, (-s - w2) / 2 with w the root of the discriminant; a discriminant in [-1e-9 (s^2 + 4 |c|), 0) counts as 0 and gives one
//   root, not two.  q == 0 is the biquadratic: z = (-p +- sqrt(p^2 - 4 r)) / 2, y = +- sqrt(z).  Every v then takes
//   kSacQuarticNewton Newton steps on the monic quartic.
//   A root is used iff v > 0 and u > 0.  s1 = sqrt(b2 / (v^2 - 2 cb v + 1)), s2 = u s1, s3 = v s1.
struct SacQuartic {
    double a2, b2, c2;                  // the squared sides of the world triangle
    double n2, n1, n0, d1, d0, q1;      // N, D and v^2 - 2 cb v + 1
    double a, b, c, d, p;               // the monic quartic, and the depressed one's p
    double s, disc1, disc2, tol1, tol2, discb;
    bool biquadratic;
};

MCORB_POSE_HD void sac_quartic(const double f1[3], const double f2[3], const double f3[3], const double P1[3], const double P2[3],
                               const double P3[3], SacQuartic &Q)
{
    const double d23[3] = {P2[0] - P3[0], P2[1] - P3[1], P2[2] - P3[2]};
    const double d13[3] = {P1[0] - P3[0], P1[1] - P3[1], P1[2] - P3[2]};
    const double d12[3] = {P1[0] - P2[0], P1[1] - P2[1], P1[2] - P2[2]};
    const double a2 = sac_dot(d23, d23), b2 = sac_dot(d13, d13), c2 = sac_dot(d12, d12);
    const double ca = sac_dot(f2, f3), cb = sac_dot(f1, f3), cg = sac_dot(f1, f2);
    const double K = (a2 - c2) / b2, Cq = c2 / b2;
    const double n2 = K - 1.0, n1 = -((2.0 * K) * cb), n0 = 1.0 + K;
    const double d1 = -(2.0 * ca), d0 = 2.0 * cg, q1 = -(2.0 * cb), tg = 2.0 * cg;
    const double D22 = d1 * d1, D21 = 2.0 * (d0 * d1), D20 = d0 * d0;
    const double A4 = n2 * n2 - Cq * D22;
    const double A3 = (2.0 * (n2 * n1) - tg * (n2 * d1)) - Cq * (D21 + q1 * D22);
    const double A2 = (((n1 * n1 + 2.0 * (n2 * n0)) + D22) - tg * (n2 * d0 + n1 * d1)) - Cq * ((D20 + q1 * D21) + D22);
    const double A1 = ((2.0 * (n1 * n0) + D21) - tg * (n1 * d0 + n0 * d1)) - Cq * (q1 * D20 + D21);
    const double A0 = ((n0 * n0 + D20) - tg * (n0 * d0)) - Cq * D20;
    const double a = A3 / A4, b = A2 / A4, c = A1 / A4, d = A0 / A4;
    const double aa = a * a;
    const double p = b - 0.375 * aa;
    const double q = (c - 0.5 * (a * b)) + 0.125 * (aa * a);
    const double r = ((d - 0.25 * (a * c)) + 0.0625 * (aa * b)) - 0.01171875 * (aa * aa);
    // the resolvent cubic
    const double g1 = 0.25 * (p * p) - r, g0 = 0.125 * (q * q);
    double lo = 0.0, hi = sac_abs(p);
    hi = sac_abs(g1) > hi ? sac_abs(g1) : hi;
    hi = g0 > hi ? g0 : hi;
    hi = 1.0 + hi;
    for (int it = 0; it < kSacBisect; it++) {
        const double mid = 0.5 * (lo + hi);
        const double gm = ((mid + p) * mid + g1) * mid - g0;
        const bool below = gm < 0.0;
        lo = below ? mid : lo;
        hi = below ? hi : mid;
    }
    double m = 0.5 * (lo + hi);
    for (int it = 0; it < kSacCubicNewton; it++) {
        const double gm = ((m + p) * m + g1) * m - g0;
        const double dg = (3.0 * m + 2.0 * p) * m + g1;
        const double next = m - gm / dg;
        m = (dg != 0.0 && next > 0.0) ? next : m;
    }
    const double s = __builtin_sqrt(2.0 * m), e = q / (2.0 * s), hm = 0.5 * p + m;
    const double c1 = hm + e, c2q = hm - e;
    Q.a2 = a2, Q.b2 = b2, Q.c2 = c2;
    Q.n2 = n2, Q.n1 = n1, Q.n0 = n0, Q.d1 = d1, Q.d0 = d0, Q.q1 = q1;
    Q.a = a, Q.b = b, Q.c = c, Q.d = d, Q.p = p;
    Q.s = s;
    Q.disc1 = s * s - 4.0 * c1;
    Q.disc2 = s * s - 4.0 * c2q;
    Q.tol1 = -(1e-9 * (s * s + 4.0 * sac_abs(c1)));
    Q.tol2 = -(1e-9 * (s * s + 4.0 * sac_abs(c2q)));
    Q.discb = p * p - 4.0 * r;
    Q.biquadratic = q == 0.0;
}

// root k = 0 .. 3 of the quartic and the depths it gives -> whether it is used (k only selects: no array is indexed by it)
MCORB_POSE_HD bool sac_quartic_root(const SacQuartic &Q, int k, double &s1, double &s2, double &s3)
{
    const bool first = k < 2, plus = (k & 1) == 0;
    double y;
    bool have = true;
    if (Q.biquadratic) {
        const double wb = __builtin_sqrt(Q.discb);
        const double z = 0.5 * (first ? -Q.p + wb : -Q.p - wb);
        const double yz = __builtin_sqrt(z);
        y = plus ? yz : -yz;
        have = plus || yz != 0.0;
    } else {
        double disc = first ? Q.disc1 : Q.disc2;
        const double tol = first ? Q.tol1 : Q.tol2;
        const bool clamped = disc < 0.0 && disc >= tol;
        disc = clamped ? 0.0 : disc;
        have = plus || !clamped;
        const double w = __builtin_sqrt(disc);
        const double sk = first ? Q.s : -Q.s;
        y = 0.5 * (plus ? sk + w : sk - w);
    }
    double v = y - 0.25 * Q.a;
    for (int it = 0; it < kSacQuarticNewton; it++) {
        const double fv = (((v + Q.a) * v + Q.b) * v + Q.c) * v + Q.d;
        const double dv = ((4.0 * v + 3.0 * Q.a) * v + 2.0 * Q.b) * v + Q.c;
        const double next = v - fv / dv;
        v = (dv != 0.0 && sac_finite(next)) ? next : v;
    }
    const double u = ((Q.n2 * v + Q.n1) * v + Q.n0) / (Q.d1 * v + Q.d0);
    const bool used = have && v > 0.0 && u > 0.0;
    s1 = __builtin_sqrt(Q.b2 / ((v * v + Q.q1 * v) + 1.0));
    s2 = u * s1;
    s3 = v * s1;
    return used;
}

// R = W E^T of two triads given as columns, row-major
MCORB_POSE_HD void sac_align(const double w1[3], const double w2[3], const double w3[3], const double e1[3], const double e2[3],
                             const double e3[3], double R[9])
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = (w1[i] * e1[j] + w2[i] * e2[j]) + w3[i] * e3[j];
    }
}

// The central minimal solver (MCORB_SAC_SOLVER_CENTRAL): the rig poses (at most 4) of a central P3P in camera `cam` -- bearings
// f1 .. f3 in the camera's frame, points P1 .. P3 in the world -- handed to visit(pose) in the order of the quartic's roots.
//   For a used root the camera-frame points s_i f_i are aligned to the world's by the triads of the two triangles: R = W E^T, t =
//   P1 - R (s1 f1) is w_T_c, and w_T_b = w_T_c * (b_T_c)^-1.
//   A pose is handed on iff its 12 numbers are finite and its own three points score below kSacSelf (a root that is not one, a
//   degenerate triangle -- a zero norm divides -- and a non-finite pose all end there).
template <class Visit>
MCORB_POSE_HD void sac_solve(const mcorb_track_cam &cam, const double f1[3], const double f2[3], const double f3[3], const double P1[3],
                             const double P2[3], const double P3[3], Visit &visit)
{
    SacQuartic Q;
    sac_quartic(f1, f2, f3, P1, P2, P3, Q);
    // the world triangle's triad, once
    double w1[3], w2[3], w3[3];
    sac_triad(P1, P2, P3, w1, w2, w3);
    for (int k = 0; k < 4; k++) {
        double s1, s2, s3;
        if (!sac_quartic_root(Q, k, s1, s2, s3)) continue;
        const double C1[3] = {s1 * f1[0], s1 * f1[1], s1 * f1[2]};
        const double C2[3] = {s2 * f2[0], s2 * f2[1], s2 * f2[2]};
        const double C3[3] = {s3 * f3[0], s3 * f3[1], s3 * f3[2]};
        double e1[3], e2[3], e3[3];
        sac_triad(C1, C2, C3, e1, e2, e3);
        // w_T_c = (Rc, tc), then w_T_b = w_T_c * (b_T_c)^-1
        double Rc[9], tc[3];
        sac_align(w1, w2, w3, e1, e2, e3, Rc);
#pragma unroll
        for (int i = 0; i < 3; i++) tc[i] = P1[i] - ((Rc[3 * i] * C1[0] + Rc[3 * i + 1] * C1[1]) + Rc[3 * i + 2] * C1[2]);
        PoseState P;
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                P.R[3 * i + j] = (Rc[3 * i] * cam.R[3 * j] + Rc[3 * i + 1] * cam.R[3 * j + 1]) + Rc[3 * i + 2] * cam.R[3 * j + 2];
                ok = ok && sac_finite(P.R[3 * i + j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            P.t[i] = tc[i] - ((P.R[3 * i] * cam.t[0] + P.R[3 * i + 1] * cam.t[1]) + P.R[3 * i + 2] * cam.t[2]);
            ok = ok && sac_finite(P.t[i]);
        }
        ok = ok && sac_score(cam, P, P1, f1) < kSacSelf && sac_score(cam, P, P2, f2) < kSacSelf && sac_score(cam, P, P3, f3) < kSacSelf;
        if (ok) visit(P);
    }
}

// The rig minimal solver (MCORB_SAC_SOLVER_RIG): three observations of any cameras.  Observation i is the ray c_i + l d_i of
// the body's frame, c_i = cam_i.t the camera's centre and d_i = cam_i.R f_i its bearing there; the pose puts B_i = c_i + l_i d_i
// on P_i.  What is shared by the four roots:
struct SacRig {
    double c1[3], c2[3], c3[3], d1[3], d2[3], d3[3];   // the rays
    double w1[3], w2[3], w3[3];                        // the world triangle's triad
    SacQuartic Q;                                      // Grunert's quartic on (d_i, P_i): the rays as if they met in one point
};

MCORB_POSE_HD void sac_ray(const mcorb_track_cam &cam, const double f[3], double c[3], double d[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        c[i] = cam.t[i];
        d[i] = (cam.R[3 * i] * f[0] + cam.R[3 * i + 1] * f[1]) + cam.R[3 * i + 2] * f[2];
    }
}

MCORB_POSE_HD void sac_rig_prepare(const mcorb_track_cam &cam1, const mcorb_track_cam &cam2, const mcorb_track_cam &cam3, const double f1[3],
                                   const double f2[3], const double f3[3], const double P1[3], const double P2[3], const double P3[3],
                                   SacRig &G)
{
    sac_ray(cam1, f1, G.c1, G.d1);
    sac_ray(cam2, f2, G.c2, G.d2);
    sac_ray(cam3, f3, G.c3, G.d3);
    sac_quartic(G.d1, G.d2, G.d3, P1, P2, P3, G.Q);
    sac_triad(P1, P2, P3, G.w1, G.w2, G.w3);
}

// Root k of the rig solver -> whether it gives a pose.
//   Start: the depths (s1, s2, s3) of the quartic's root k, used iff v > 0 and u > 0 as in the central solver.
//   Newton: kSacRigNewton steps on F12, F13, F23 with F_ij(l) = |B_i - B_j|^2 - |P_i - P_j|^2.  With D_ij = B_i - B_j the Jacobian is
//       | a b 0 |     a = 2 D12.d1   b = -(2 D12.d2)
//       | c 0 e |     c = 2 D13.d1   e = -(2 D13.d3)
//       | 0 g h |     g = 2 D23.d2   h = -(2 D23.d3)
//   and J x = F is solved by cofactors along the first row: det = -(a (e g) + b (c h)), m = F13 h - e F23,
//   x1 = (-(F12 (e g)) - b m) / det, x2 = (a m - F12 (c h)) / det, x3 = ((F12 (c g) - a (F13 g)) - b (c F23)) / det, l <- l - x.  A
//   step is taken iff det != 0 and all three next values are finite.  The root is used iff all l_i > 0.
//   Pose: R = W E^T from the triads of (P_i) and (B_i) is w_R_b directly, t = P1 - R B1.
//   Kept iff the 12 numbers are finite and each of the three points scores below kSacSelf in its own camera.
// When the three cameras are one camera the start already solves F = 0; there is no special case.
MCORB_POSE_HD bool sac_rig_root(const SacRig &G, int k, const mcorb_track_cam &cam1, const mcorb_track_cam &cam2, const mcorb_track_cam &cam3,
                                const double f1[3], const double f2[3], const double f3[3], const double P1[3], const double P2[3],
                                const double P3[3], PoseState &P)
{
    double l1, l2, l3;
    bool ok = sac_quartic_root(G.Q, k, l1, l2, l3);
    double B1[3], B2[3], B3[3];
    for (int it = 0; it < kSacRigNewton; it++) {
        double D12[3], D13[3], D23[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            B1[i] = G.c1[i] + l1 * G.d1[i];
            B2[i] = G.c2[i] + l2 * G.d2[i];
            B3[i] = G.c3[i] + l3 * G.d3[i];
            D12[i] = B1[i] - B2[i];
            D13[i] = B1[i] - B3[i];
            D23[i] = B2[i] - B3[i];
        }
        const double F12 = sac_dot(D12, D12) - G.Q.c2, F13 = sac_dot(D13, D13) - G.Q.b2, F23 = sac_dot(D23, D23) - G.Q.a2;
        const double a = 2.0 * sac_dot(D12, G.d1), b = -(2.0 * sac_dot(D12, G.d2));
        const double c = 2.0 * sac_dot(D13, G.d1), e = -(2.0 * sac_dot(D13, G.d3));
        const double g = 2.0 * sac_dot(D23, G.d2), h = -(2.0 * sac_dot(D23, G.d3));
        const double eg = e * g, ch = c * h;
        const double det = -(a * eg + b * ch);
        const double m = F13 * h - e * F23;
        const double x1 = (-(F12 * eg) - b * m) / det;
        const double x2 = (a * m - F12 * ch) / det;
        const double x3 = ((F12 * (c * g) - a * (F13 * g)) - b * (c * F23)) / det;
        const double t1 = l1 - x1, t2 = l2 - x2, t3 = l3 - x3;
        const bool take = det != 0.0 && sac_finite(t1) && sac_finite(t2) && sac_finite(t3);
        l1 = take ? t1 : l1;
        l2 = take ? t2 : l2;
        l3 = take ? t3 : l3;
    }
    ok = ok && l1 > 0.0 && l2 > 0.0 && l3 > 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        B1[i] = G.c1[i] + l1 * G.d1[i];
        B2[i] = G.c2[i] + l2 * G.d2[i];
        B3[i] = G.c3[i] + l3 * G.d3[i];
    }
    double e1[3], e2[3], e3[3];
    sac_triad(B1, B2, B3, e1, e2, e3);
    sac_align(G.w1, G.w2, G.w3, e1, e2, e3, P.R);
#pragma unroll
    for (int i = 0; i < 9; i++) ok = ok && sac_finite(P.R[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        P.t[i] = P1[i] - ((P.R[3 * i] * B1[0] + P.R[3 * i + 1] * B1[1]) + P.R[3 * i + 2] * B1[2]);
        ok = ok && sac_finite(P.t[i]);
    }
    const bool self = sac_score(cam1, P, P1, f1) < kSacSelf && sac_score(cam2, P, P2, f2) < kSacSelf && sac_score(cam3, P, P3, f3) < kSacSelf;
    return ok && self;
}

// the rig poses (at most 4 of the problem's up to 8: those that continue the central solutions) handed to visit(pose) in root order
template <class Visit>
MCORB_POSE_HD void sac_solve_rig(const mcorb_track_cam *cams, int cam1, int cam2, int cam3, const double f1[3], const double f2[3],
                                 const double f3[3], const double P1[3], const double P2[3], const double P3[3], Visit &visit)
{
    SacRig G;
    sac_rig_prepare(cams[cam1], cams[cam2], cams[cam3], f1, f2, f3, P1, P2, P3, G);
    for (int k = 0; k < 4; k++) {
        PoseState P;
        if (sac_rig_root(G, k, cams[cam1], cams[cam2], cams[cam3], f1, f2, f3, P1, P2, P3, P)) visit(P);
    }
}

// the fourth point disambiguates as OpenGV does: the solution with the smallest score there wins, a tie goes to the lowest
// solution index and a NaN never wins.  `cam` is the fourth point's camera
struct SacDisambiguate {
    const mcorb_track_cam &cam;
    const double *X4, *f4;
    PoseState best;
    double best_score;
    bool have;
    MCORB_POSE_HD void operator()(const PoseState &P)
    {
        const double sc = sac_score(cam, P, X4, f4);
        const bool better = have ? sc < best_score : sc == sc;
        if (better) {
            best = P;
            best_score = sc;
            have = true;
        }
    }
};

// the same rule between two roots that each hold a candidate (has, score, k), for lanes that took one root each: whether the
// other's beats this one's
MCORB_POSE_HD bool sac_root_beats(bool o_has, double o_score, int o_k, bool has, double score, int k)
{
    return o_has && (!has || o_score < score || (o_score == score && o_k < k));
}

// A hypothesis's model from its four observations: keypoints (u, v), points X, all in camera `cam`.  -> whether there is one
MCORB_POSE_HD bool sac_model(const mcorb_track_cam &cam, const float uv[4][2], const double X[4][3], PoseState &out)
{
    double f1[3], f2[3], f3[3], f4[3];
    sac_bearing(cam, uv[0][0], uv[0][1], f1);
    sac_bearing(cam, uv[1][0], uv[1][1], f2);
    sac_bearing(cam, uv[2][0], uv[2][1], f3);
    sac_bearing(cam, uv[3][0], uv[3][1], f4);
    SacDisambiguate pick{cam, X[3], f4, PoseState{}, 0.0, false};
    sac_solve(cam, f1, f2, f3, X[0], X[1], X[2], pick);
    out = pick.best;
    return pick.have;
}

// the same with the rig solver: observation i in camera ci[i], the fourth point scored in its own
MCORB_POSE_HD bool sac_model_rig(const mcorb_track_cam *cams, int c0, int c1, int c2, int c3, const float uv[4][2], const double X[4][3],
                                 PoseState &out)
{
    double f1[3], f2[3], f3[3], f4[3];
    sac_bearing(cams[c0], uv[0][0], uv[0][1], f1);
    sac_bearing(cams[c1], uv[1][0], uv[1][1], f2);
    sac_bearing(cams[c2], uv[2][0], uv[2][1], f3);
    sac_bearing(cams[c3], uv[3][0], uv[3][1], f4);
    SacDisambiguate pick{cams[c3], X[3], f4, PoseState{}, 0.0, false};
    sac_solve_rig(cams, c0, c1, c2, f1, f2, f3, X[0], X[1], X[2], pick);
    out = pick.best;
    return pick.have;
}

// a hypothesis's record, written member by member: M may be device memory
MCORB_POSE_HD void sac_write_model(SacModel &M, bool ok, const PoseState &P, int32_t s0, int32_t s1, int32_t s2, int32_t s3)
{
#pragma unroll
    for (int k = 0; k < 9; k++) M.R[k] = ok ? P.R[k] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) M.t[k] = ok ? P.t[k] : 0.0;
    M.valid = ok ? 1 : 0;
    M.sample[0] = s0;
    M.sample[1] = s1;
    M.sample[2] = s2;
    M.sample[3] = s3;
    M.pad[0] = M.pad[1] = M.pad[2] = 0;
}

// Hypothesis h of a call with the central solver: its sample, its four points through point(i, X), its model
template <class Point>
MCORB_POSE_HD void sac_hypothesis_central(const SacJob &job, int h, const PoseObs *obs, const Point &point, const int32_t *cons,
                                          const int32_t *cam_first, const int32_t *cam_cons, SacModel &M)
{
    int32_t s0, s1, s2, s3;
    bool ok = sac_sample(job.seed, h, job.S, cons, obs, cam_first, cam_cons, s0, s1, s2, s3);
    PoseState P = PoseState{};
    if (ok) {
        const PoseObs o0 = obs[s0], o1 = obs[s1], o2 = obs[s2], o3 = obs[s3];
        const float uv[4][2] = {{o0.u, o0.v}, {o1.u, o1.v}, {o2.u, o2.v}, {o3.u, o3.v}};
        double X[4][3];
        point(s0, X[0]);
        point(s1, X[1]);
        point(s2, X[2]);
        point(s3, X[3]);
        ok = sac_model(job.cams[o0.cam], uv, X, P);
    }
    sac_write_model(M, ok, P, s0, s1, s2, s3);
}

// the same with the rig solver (cam_first and cam_cons are not used)
template <class Point>
MCORB_POSE_HD void sac_hypothesis_rig(const SacJob &job, int h, const PoseObs *obs, const Point &point, const int32_t *cons, SacModel &M)
{
    int32_t s0, s1, s2, s3;
    bool ok = sac_sample_rig(job.seed, h, job.S, cons, s0, s1, s2, s3);
    PoseState P = PoseState{};
    if (ok) {
        const PoseObs o0 = obs[s0], o1 = obs[s1], o2 = obs[s2], o3 = obs[s3];
        const float uv[4][2] = {{o0.u, o0.v}, {o1.u, o1.v}, {o2.u, o2.v}, {o3.u, o3.v}};
        double X[4][3];
        point(s0, X[0]);
        point(s1, X[1]);
        point(s2, X[2]);
        point(s3, X[3]);
        ok = sac_model_rig(job.cams, o0.cam, o1.cam, o2.cam, o3.cam, uv, X, P);
    }
    sac_write_model(M, ok, P, s0, s1, s2, s3);
}

// hypothesis h by the job's solver
template <class Point>
MCORB_POSE_HD void sac_hypothesis(const SacJob &job, int h, const PoseObs *obs, const Point &point, const int32_t *cons,
                                  const int32_t *cam_first, const int32_t *cam_cons, SacModel &M)
{
    if (job.solver == MCORB_SAC_SOLVER_RIG)
        sac_hypothesis_rig(job, h, obs, point, cons, M);
    else
        sac_hypothesis_central(job, h, obs, point, cons, cam_first, cam_cons, M);
}

// the winner among H hypotheses: consensus_key (mcorb_consensus.h) over h
constexpr int kSacKeyBits = 10;
static_assert((1 << kSacKeyBits) == MCORB_SAC_MAX_ITERATIONS, "the key holds every hypothesis index");

// The three kernels, serially: what a host-only store runs (mcorb_sac.cpp).  X: the n points, gathered; models[H], count[H] and
// f[3 S] are the caller's scratch; flags: n, written
struct SacHostPoint {
    const double *X;
    inline void operator()(int i, double out[3]) const
    {
        out[0] = X[3 * (size_t)i];
        out[1] = X[3 * (size_t)i + 1];
        out[2] = X[3 * (size_t)i + 2];
    }
};
inline void sac_run_serial(const SacJob &job, const PoseObs *obs, const double *X, const int32_t *cons, const int32_t *cam_first,
                           const int32_t *cam_cons, SacModel *models, int32_t *count, double *f, SacOut &out, uint8_t *flags)
{
    const SacHostPoint point{X};
    for (int k = 0; k < job.S; k++) {
        const PoseObs &o = obs[cons[k]];
        sac_bearing(job.cams[o.cam], o.u, o.v, f + 3 * (size_t)k);
    }
    PoseState P;
    for (int h = 0; h < job.H; h++) {
        SacModel &M = models[h];
        sac_hypothesis(job, h, obs, point, cons, cam_first, cam_cons, M);
        count[h] = 0;
        if (!M.valid) continue;
        pose_load(P, M.R, M.t);
        for (int k = 0; k < job.S; k++) {
            const int i = cons[k];
            count[h] += sac_is_inlier(sac_score(job.cams[obs[i].cam], P, X + 3 * (size_t)i, f + 3 * (size_t)k), job.threshold) ? 1 : 0;
        }
    }
    const ConsensusBest won = consensus_best<kSacKeyBits>(job.H, [&](int h) { return models[h].valid; }, [&](int h) { return count[h]; });
    const int best = consensus_key_index<kSacKeyBits>(won.key);
    pose_identity(P);
    if (best >= 0) pose_load(P, models[best].R, models[best].t);
    for (int i = 0; i < job.n; i++) flags[i] = 0;
    if (best >= 0)
        for (int k = 0; k < job.S; k++) {
            const int i = cons[k];
            flags[i] = sac_is_inlier(sac_score(job.cams[obs[i].cam], P, X + 3 * (size_t)i, f + 3 * (size_t)k), job.threshold) ? 1 : 0;
        }
    for (int j = 0; j < 9; j++) out.R[j] = P.R[j];
    for (int j = 0; j < 3; j++) out.t[j] = P.t[j];
    out.status = best >= 0 ? MCORB_SAC_OK : MCORB_SAC_NO_MODEL;
    out.n_inliers = best >= 0 ? count[best] : 0;
    out.best = best;
    out.n_models = won.n_models;
    for (int j = 0; j < 4; j++) out.sample[j] = best >= 0 ? models[best].sample[j] : -1;
}

}  // namespace mcorb
