// mcorb_ess.h -- the arithmetic of the pose of one camera between two frames from 2D-2D matches: what the reference gets from
// cv::findEssentialMat(..., RANSAC, prob, thr, mask) and cv::recoverPose(...) in the one-camera arm of its bootstrap
// (MCSlam/src/FrontEnd.cpp:2591-2628) and at :2105, :3023, :6842, :6959, :7142, :7172.  OpenCV is not in the tree: the Sampson
// distance and recoverPose's cheirality vote are recalled, and five things are stated instead of OpenCV's:
// the draws, the minimal solver (a hidden-variable five-point solver: nothing of Nister's elimination is recalled), the absence
// of the adaptive stop, the triangulation inside the vote (mcorb_rel.h's midpoint) and the rotations from E (mcorb_rel.h's steps
// 4-5 in place of an SVD).  Same conventions as mcorb_rel.h: no HIP dependency -- the host-only store (mcorb_ess.cpp) and
// k_ess_hypotheses / k_ess_score / k_ess_pick / k_ess_finish (mcorb_ess_gpu.hip) run the same code -- compiled with
// -ffp-contract=off, fp64, one IEEE operation per operator in the order written, only + - * /, comparisons and sqrt, every loop
// bounded by a count whatever the data holds.
//   The unknown is (R, t) = c1_T_c2: X_c1 = R X_c2 + t, |t| = 1, E = [t]x R, x1^T E x2 = 0.  The solver is cut into the pieces the
//   kernel hands to the 16 lanes of a hypothesis; the lanes only move values, every chain of operations is one of the functions
//   below, and ess_hypothesis runs them one after the other.
#pragma once
#include <stdint.h>

#include "mcorb_ess_table.inc"
#include "mcorb_rel.h"

namespace mcorb {

constexpr int kEssSample = MCORB_ESS_SAMPLE;   // the matches of a minimal sample
constexpr int kEssRoots = MCORB_ESS_MAX_ROOTS; // the models of a hypothesis at most
constexpr int kEssNodes = 11;                  // the values of det C(z) that give its 11 coefficients
constexpr int kEssBisect = 48;                 // halvings of a bracket of the derivative chain
constexpr int kEssPolish = 3;                  // Gauss-Newton steps on (x, y, z) against the ten cubics
constexpr double kEssSelf = 1e-9;              // a model is kept iff its five rows and its ten cubics are below this
constexpr int kEssKeyBits = 18;
static_assert(MCORB_ESS_MAX_ITERATIONS * kEssRoots <= (1 << kEssKeyBits), "the key holds every slot");

// a match as the kernels read it
struct EssObs { float u1, v1, u2, v2; };

// a slot's model: E with |E|_F^2 = 2 (zeros without one) and whether there is one
struct EssModel {
    double E[9];
    int32_t valid, pad;
};
static_assert(sizeof(EssModel) == 80, "the kernels read models at 80-byte strides");

// one call as the kernels read it from device memory: the calibration, the squared threshold on normalised points, recoverPose's
// distance, the seed, S matches, H hypotheses
struct EssJob {
    double fx, fy, s, u0, v0;
    double threshold2, distance;
    uint64_t seed;
    int32_t S, H;
};

// what k_ess_pick leaves for k_ess_finish: the winning slot (-1: none), its count, the slots that had a model, the model and its
// candidates
struct EssPick {
    double E[9], Rp[9], Rm[9], t[3];
    int32_t slot, count, n_models, pad;
};

// what k_ess_finish leaves for the host
struct EssOut {
    double R[9], t[3], E[9];
    int32_t status, n_ransac_inliers, n_inliers, best_hypothesis, best_root, sample[kEssSample], n_models, cheirality[4], pad;
};

// a match's normalised points and unit bearings
struct EssPt { double x1, y1, x2, y2; };

MCORB_POSE_HD void ess_normalise(const EssJob &job, double u, double v, double &x, double &y)
{
    y = (v - job.v0) / job.fy;
    x = ((u - job.u0) - job.s * y) / job.fx;
}
MCORB_POSE_HD void ess_point(const EssJob &job, double u1, double v1, double u2, double v2, EssPt &p)
{
    ess_normalise(job, u1, v1, p.x1, p.y1);
    ess_normalise(job, u2, v2, p.x2, p.y2);
}
MCORB_POSE_HD void ess_bearing(double x, double y, double f[3])
{
    const double n = __builtin_sqrt((x * x + y * y) + 1.0);
    f[0] = x / n;
    f[1] = y / n;
    f[2] = 1.0 / n;
}

// ---------------------------------------------------------------------------------------------------------------------------
// polynomials in x, y, z.  A linear one is its coefficients of x, y, z, 1.  A quadratic has 10 coefficients and a cubic 20, grouped
// by their monomial in (x, y) -- in the order x^3, x^2 y, x y^2, y^3, x^2, x y, y^2, x, y, 1 for a cubic and x^2, x y, y^2, x, y, 1
// for a quadratic -- and inside a group by ascending power of z: a cubic's row of C(z) is read off by Horner's rule per group
// ---------------------------------------------------------------------------------------------------------------------------
MCORB_POSE_HD constexpr int ess_pos3(int a, int b, int c) { return (a + b == 3 ? b : a + b == 2 ? 4 + 2 * b : a + b == 1 ? 10 + 3 * b : 16) + c; }
MCORB_POSE_HD constexpr int ess_pos2(int a, int b, int c) { return (a + b == 2 ? b : a + b == 1 ? 3 + 2 * b : 7) + c; }

// q += a b, the 16 products in the order (i, j) = (0, 0), (0, 1) .. (3, 3)
MCORB_POSE_HD void ess_mul11(const double a[4], const double b[4], double q[10])
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            q[ess_pos2((i == 0) + (j == 0), (i == 1) + (j == 1), (i == 2) + (j == 2))] += a[i] * b[j];
}

// c += q l, the 40 products in the order (u, k) = (0, 0), (0, 1) .. (9, 3)
MCORB_POSE_HD void ess_mul21(const double q[10], const double l[4], double c[20])
{
    constexpr int qa[10] = {2, 1, 0, 1, 1, 0, 0, 0, 0, 0}, qb[10] = {0, 1, 2, 0, 0, 1, 1, 0, 0, 0}, qc[10] = {0, 0, 0, 0, 1, 0, 1, 0, 1, 2};
    for (int u = 0; u < 10; u++)
        for (int k = 0; k < 4; k++) c[ess_pos3(qa[u] + (k == 0), qb[u] + (k == 1), qc[u] + (k == 2))] += q[u] * l[k];
}

// entry k of E = x X + y Y + z Z + W as a linear polynomial; B: the basis, X at B, Y at B + 9, Z at B + 18, W at B + 27
MCORB_POSE_HD void ess_entry(const double *B, int k, double l[4])
{
    l[0] = B[k];
    l[1] = B[9 + k];
    l[2] = B[18 + k];
    l[3] = B[27 + k];
}

// The null space of the five rows vec(d1 d2^T) (row-major: entry 3 a + b is d1[a] d2[b]) as an orthonormal basis, B[36].  The rows
// are orthonormalised by modified Gram-Schmidt, two passes (a row without a remainder divides by zero: the NaN ends in a model
// that is not kept); P = I - sum q q^T is the projector on the null space; four times the largest diagonal entry of P (the
// first of equals) picks a column, v = P e_k / sqrt(P_kk) is the next basis vector and P <- P - v v^T
MCORB_POSE_HD void ess_basis(const double (*d1)[3], const double (*d2)[3], double *B)
{
    double Q[kEssSample][9], P[81];
    for (int i = 0; i < kEssSample; i++) {
        double *v = Q[i];
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) v[3 * a + b] = d1[i][a] * d2[i][b];
        for (int pass = 0; pass < 2; pass++)
            for (int k = 0; k < i; k++) {
                double dot = 0.0;
                for (int j = 0; j < 9; j++) dot += Q[k][j] * v[j];
                for (int j = 0; j < 9; j++) v[j] -= dot * Q[k][j];
            }
        double nn = 0.0;
        for (int j = 0; j < 9; j++) nn += v[j] * v[j];
        const double inv = 1.0 / __builtin_sqrt(nn);
        for (int j = 0; j < 9; j++) v[j] *= inv;
    }
    for (int p = 0; p < 9; p++)
        for (int q = 0; q < 9; q++) {
            double acc = p == q ? 1.0 : 0.0;
            for (int i = 0; i < kEssSample; i++) acc -= Q[i][p] * Q[i][q];
            P[9 * p + q] = acc;
        }
    for (int s = 0; s < 4; s++) {
        int k = 0;
        for (int j = 1; j < 9; j++) k = P[10 * j] > P[10 * k] ? j : k;
        const double inv = 1.0 / __builtin_sqrt(P[10 * k]);
        double *v = B + 9 * s;
        for (int j = 0; j < 9; j++) v[j] = P[9 * j + k] * inv;
        for (int p = 0; p < 9; p++)
            for (int q = 0; q < 9; q++) P[9 * p + q] -= v[p] * v[q];
    }
}

// cubic k of the ten: k = 3 i + j < 9 is entry (i, j) of 2 (E E^T) E - tr(E E^T) E -- T1 = sum over m of (sum over l of E_il E_ml)
// E_mj, T2 = (sum over r of E_r E_r) E_ij, c = 2 T1 - T2 -- and k = 9 is det E = (E4 E8 - E5 E7) E0 + (E5 E6 - E3 E8) E1 + (E3 E7 -
// E4 E6) E2
MCORB_POSE_HD void ess_cubic(const double *B, int k, double *c)
{
    double T1[20], T2[20], q[10], a[4], b[4];
    for (int v = 0; v < 20; v++) T1[v] = T2[v] = 0.0;
    if (k < 9) {
        const int i = k / 3, j = k % 3;
        for (int m = 0; m < 3; m++) {
            for (int u = 0; u < 10; u++) q[u] = 0.0;
            for (int l = 0; l < 3; l++) {
                ess_entry(B, 3 * i + l, a);
                ess_entry(B, 3 * m + l, b);
                ess_mul11(a, b, q);
            }
            ess_entry(B, 3 * m + j, a);
            ess_mul21(q, a, T1);
        }
        for (int u = 0; u < 10; u++) q[u] = 0.0;
        for (int r = 0; r < 9; r++) {
            ess_entry(B, r, a);
            ess_mul11(a, a, q);
        }
        ess_entry(B, k, a);
        ess_mul21(q, a, T2);
        for (int v = 0; v < 20; v++) c[v] = 2.0 * T1[v] - T2[v];
    } else {
        constexpr int first[3][2] = {{4, 8}, {5, 6}, {3, 7}}, second[3][2] = {{5, 7}, {3, 8}, {4, 6}};
        for (int m = 0; m < 3; m++) {
            double qa[10], qb[10];
            for (int u = 0; u < 10; u++) qa[u] = qb[u] = 0.0;
            ess_entry(B, first[m][0], a);
            ess_entry(B, first[m][1], b);
            ess_mul11(a, b, qa);
            ess_entry(B, second[m][0], a);
            ess_entry(B, second[m][1], b);
            ess_mul11(a, b, qb);
            for (int u = 0; u < 10; u++) q[u] = qa[u] - qb[u];
            ess_entry(B, m, a);
            ess_mul21(q, a, T1);
        }
        for (int v = 0; v < 20; v++) c[v] = T1[v];
    }
}

// a cubic's row of C(z): the ten coefficients of x^3 .. 1 at z, by Horner's rule
MCORB_POSE_HD void ess_row(const double *c, double z, double *row)
{
    for (int m = 0; m < 4; m++) row[m] = c[m];
    for (int m = 0; m < 3; m++) row[4 + m] = c[5 + 2 * m] * z + c[4 + 2 * m];
    for (int m = 0; m < 2; m++) row[7 + m] = (c[12 + 3 * m] * z + c[11 + 3 * m]) * z + c[10 + 3 * m];
    row[9] = ((c[19] * z + c[18]) * z + c[17]) * z + c[16];
}

// LU with partial pivoting of the 10 x 10 matrix M in place (the largest |entry| of the column, the first of equals; a zero
// pivot leaves its column as it is) -> the determinant: the product of the pivots in order, its sign turned by every exchange
MCORB_POSE_HD double ess_lu(double *M)
{
    double det = 1.0;
    for (int k = 0; k < 10; k++) {
        int pk = k;
        double best = sac_abs(M[10 * k + k]);
        for (int i = k + 1; i < 10; i++) {
            const double v = sac_abs(M[10 * i + k]);
            pk = v > best ? i : pk;
            best = v > best ? v : best;
        }
        if (pk != k) {
            for (int j = 0; j < 10; j++) {
                const double tmp = M[10 * k + j];
                M[10 * k + j] = M[10 * pk + j];
                M[10 * pk + j] = tmp;
            }
            det = -det;
        }
        const double d = M[10 * k + k];
        det = det * d;
        if (d == 0.0) continue;
        for (int i = k + 1; i < 10; i++) {
            const double f = M[10 * i + k] / d;
            for (int j = k + 1; j < 10; j++) M[10 * i + j] -= f * M[10 * k + j];
        }
    }
    return det;
}

MCORB_POSE_HD double ess_node(int k)
{
    constexpr double node[kEssNodes] = MCORB_ESS_NODES;
    return node[k];
}

// det C(z) at z = rho * node k; table: the ten cubics, 20 coefficients each
MCORB_POSE_HD double ess_det_at(const double *table, int k, double rho)
{
    double M[100];
    const double z = rho * ess_node(k);
    for (int r = 0; r < 10; r++) ess_row(table + 20 * r, z, M + 10 * r);
    return ess_lu(M);
}

// coefficient j of det C(z) from its values at the nodes, summed in node order
MCORB_POSE_HD double ess_coefficient(const double *det, int j)
{
    constexpr double interp[kEssNodes][kEssNodes] = MCORB_ESS_INTERP;
    double acc = 0.0;
    for (int k = 0; k < kEssNodes; k++) acc += interp[j][k] * det[k];
    return acc;
}

// The scale of the roots from a first pass at rho = 1: the power of two rho = 2^e with |p[0] / p[10]| / rho^10 in [2^-5, 2^5) -- the
// geometric mean of the ten roots' moduli within a factor sqrt(2) of rho -- or 1 where that ratio is not finite and positive.
// The nodes lie in [-2, 2] and the table's rounding is relative to the largest of the 11 values: roots that all lie in a
// disc far smaller (or larger) than that would drown in it, so a second pass takes the values at rho * node and finds the
// roots of the polynomial in w = z / rho.  At most 24 steps either way
MCORB_POSE_HD double ess_scale(const double *p)
{
    double r = sac_abs(p[0] / p[10]), rho = 1.0;
    if (!(sac_finite(r) && r > 0.0)) return 1.0;
    for (int it = 0; it < 24; it++) {
        const bool big = r >= 32.0, small = r < 0.03125;
        r = big ? r * 0.0009765625 : small ? r * 1024.0 : r;
        rho = big ? rho * 2.0 : small ? rho * 0.5 : rho;
    }
    return rho;
}

// The real roots of p (degree 10, p[j] the coefficient of z^j) by the chain of derivatives.  Level L = 9 .. 0 is q = the L-th
// derivative of p, degree n = 10 - L: q[j] = p[j + L] (j + 1) .. (j + L).  The roots of level L + 1 (m <= n - 1 of them, ascending)
// cut [-b, b], b = 1 + max |q[j] / q[n]| (Cauchy's bound), into m + 1 intervals, in each of which q is monotonic; interval i holds
// a root iff q(lo) <= 0 < q(hi) or q(lo) >= 0 > q(hi), found by kEssBisect halvings (mid = (lo + hi) / 2 replaces the end whose
// side it is on) and returned as the last bracket's middle.  A root of even multiplicity changes no sign and is not found.
MCORB_POSE_HD void ess_level(const double *p, int L, double *q, double &bound)
{
    const int n = 10 - L;
    for (int j = 0; j <= n; j++) {
        double f = 1.0;
        for (int s = 1; s <= L; s++) f *= (double)(j + s);
        q[j] = p[j + L] * f;
    }
    double b = 0.0;
    for (int j = 0; j < n; j++) {
        const double r = sac_abs(q[j] / q[n]);
        b = r > b ? r : b;
    }
    bound = 1.0 + b;
}
MCORB_POSE_HD double ess_horner(const double *q, int n, double z)
{
    double v = q[n];
    for (int j = n - 1; j >= 0; j--) v = v * z + q[j];
    return v;
}
MCORB_POSE_HD bool ess_interval(const double *q, int n, const double *crit, int m, double bound, int i, double &root)
{
    double lo = i == 0 ? -bound : crit[i - 1], hi = i == m ? bound : crit[i];
    const double flo = ess_horner(q, n, lo), fhi = ess_horner(q, n, hi);
    const bool up = flo <= 0.0 && fhi > 0.0, down = flo >= 0.0 && fhi < 0.0;
    for (int it = 0; it < kEssBisect; it++) {
        const double mid = 0.5 * (lo + hi);
        const double fm = ess_horner(q, n, mid);
        const bool above = up ? fm > 0.0 : fm < 0.0;
        hi = above ? mid : hi;
        lo = above ? lo : mid;
    }
    root = 0.5 * (lo + hi);
    return (up || down) && sac_finite(root);
}
// -> the number of roots, ascending in roots[10]
MCORB_POSE_HD int ess_real_roots(const double *p, double *roots)
{
    double crit[10], next[10], q[11];
    int m = 0;
    if (!(sac_finite(p[10]) && p[10] != 0.0)) return 0;
    for (int L = 9; L >= 0; L--) {
        const int n = 10 - L;
        double bound;
        ess_level(p, L, q, bound);
        int found = 0;
        for (int i = 0; i <= m; i++) {
            double r;
            if (ess_interval(q, n, crit, m, bound, i, r)) next[found++] = r;
        }
        for (int i = 0; i < found; i++) crit[i] = next[i];
        m = found;
    }
    for (int i = 0; i < m; i++) roots[i] = crit[i];
    return m;
}

// a cubic at (x, y, z) with its three derivatives, its 20 terms in order; X, Y, Z: the powers 0 .. 3
MCORB_POSE_HD void ess_cubic_at(const double *c, const double X[4], const double Y[4], const double Z[4], double &r, double &gx, double &gy,
                                double &gz)
{
    constexpr int ea[20] = {3, 2, 1, 0, 2, 2, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    constexpr int eb[20] = {0, 1, 2, 3, 0, 0, 1, 1, 2, 2, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0};
    constexpr int ec[20] = {0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 2, 0, 1, 2, 0, 1, 2, 3};
    r = gx = gy = gz = 0.0;
    for (int v = 0; v < 20; v++) {
        const int a = ea[v], b = eb[v], e = ec[v];
        r += c[v] * ((X[a] * Y[b]) * Z[e]);
        if (a > 0) gx += c[v] * ((((double)a * X[a - 1]) * Y[b]) * Z[e]);
        if (b > 0) gy += c[v] * ((X[a] * ((double)b * Y[b - 1])) * Z[e]);
        if (e > 0) gz += c[v] * ((X[a] * Y[b]) * ((double)e * Z[e - 1]));
    }
}

// the largest |residual| of E on the sample's five rows d1^T E d2 and on the ten cubics
MCORB_POSE_HD double ess_residual(const double *E, const double (*d1)[3], const double (*d2)[3])
{
    double worst = 0.0;
    for (int i = 0; i < kEssSample; i++) {
        double a[3];
        rel_rot(E, d2[i], a);
        const double r = sac_abs(sac_dot(d1[i], a));
        worst = r > worst || r != r ? r : worst;
    }
    double G[9], tr;
    for (int i = 0; i < 3; i++)
        for (int m = 0; m < 3; m++) G[3 * i + m] = (E[3 * i] * E[3 * m] + E[3 * i + 1] * E[3 * m + 1]) + E[3 * i + 2] * E[3 * m + 2];
    tr = (G[0] + G[4]) + G[8];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double ge = (G[3 * i] * E[j] + G[3 * i + 1] * E[3 + j]) + G[3 * i + 2] * E[6 + j];
            const double r = sac_abs(2.0 * ge - tr * E[3 * i + j]);
            worst = r > worst || r != r ? r : worst;
        }
    double x[3];
    rel_cross(E + 3, E + 6, x);
    const double r = sac_abs(sac_dot(E, x));
    worst = r > worst || r != r ? r : worst;
    return worst;
}

// The model of the root z: C(z) is factored by ess_lu and (x, y) read from its rows 8 and 7 with the last monomial 1 -- y = -U89 /
// U88, x = (-U79 - U78 y) / U77 --; kEssPolish Gauss-Newton steps on (x, y, z) against the ten cubics, the 3 x 3 normal equations
// solved by cofactors, a step taken iff det != 0 and the three next values are finite; E = ((x X + y Y) + z Z) + W scaled to |E|_F^2
// = 2.  Kept iff its nine numbers are finite and ess_residual < kEssSelf (false for a NaN)
MCORB_POSE_HD bool ess_root_model(const double *table, const double *B, const double (*d1)[3], const double (*d2)[3], double z, double *E)
{
    double M[100];
    for (int r = 0; r < 10; r++) ess_row(table + 20 * r, z, M + 10 * r);
    ess_lu(M);
    double y = -M[89] / M[88];
    double x = (-M[79] - M[78] * y) / M[77];
    for (int it = 0; it < kEssPolish; it++) {
        const double X[4] = {1.0, x, x * x, (x * x) * x}, Y[4] = {1.0, y, y * y, (y * y) * y}, Z[4] = {1.0, z, z * z, (z * z) * z};
        double N00 = 0.0, N01 = 0.0, N02 = 0.0, N11 = 0.0, N12 = 0.0, N22 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
        for (int k = 0; k < 10; k++) {
            double h, g0, g1, g2;
            ess_cubic_at(table + 20 * k, X, Y, Z, h, g0, g1, g2);
            N00 += g0 * g0;
            N01 += g0 * g1;
            N02 += g0 * g2;
            N11 += g1 * g1;
            N12 += g1 * g2;
            N22 += g2 * g2;
            r0 += g0 * h;
            r1 += g1 * h;
            r2 += g2 * h;
        }
        const double c00 = N11 * N22 - N12 * N12, c01 = N12 * N02 - N01 * N22, c02 = N01 * N12 - N11 * N02;
        const double c11 = N00 * N22 - N02 * N02, c12 = N01 * N02 - N00 * N12, c22 = N00 * N11 - N01 * N01;
        const double det = (N00 * c00 + N01 * c01) + N02 * c02;
        const double nx = x - ((c00 * r0 + c01 * r1) + c02 * r2) / det;
        const double ny = y - ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        const double nz = z - ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        const bool take = det != 0.0 && sac_finite(nx) && sac_finite(ny) && sac_finite(nz);
        x = take ? nx : x;
        y = take ? ny : y;
        z = take ? nz : z;
    }
    double nn = 0.0;
    for (int k = 0; k < 9; k++) {
        E[k] = ((x * B[k] + y * B[9 + k]) + z * B[18 + k]) + B[27 + k];
        nn += E[k] * E[k];
    }
    const double scale = __builtin_sqrt(2.0 / nn);
    bool ok = true;
    for (int k = 0; k < 9; k++) {
        E[k] *= scale;
        ok = ok && sac_finite(E[k]);
    }
    return ok && ess_residual(E, d1, d2) < kEssSelf;
}

// the sample of hypothesis h and its bearings -> whether it has five members
MCORB_POSE_HD bool ess_sample(const EssJob &job, int h, const EssObs *obs, int32_t sample[kEssSample], double (*d1)[3], double (*d2)[3])
{
    const bool ok = rel_sample_k<kEssSample>(job.seed, h, job.S, sample);
    for (int j = 0; j < kEssSample; j++) {
        EssPt p = EssPt{0.0, 0.0, 0.0, 0.0};
        if (ok) {
            const EssObs o = obs[sample[j]];
            ess_point(job, (double)o.u1, (double)o.v1, (double)o.u2, (double)o.v2, p);
        }
        ess_bearing(p.x1, p.y1, d1[j]);
        ess_bearing(p.x2, p.y2, d2[j]);
    }
    return ok;
}

// The solver on five pairs of bearings -> the number of models; E: 9 doubles per model, in ascending order of the root each
// began from (z0, may be NULL: those roots)
MCORB_POSE_HD int ess_solve5(const double (*d1)[3], const double (*d2)[3], double *E, double *z0)
{
    double B[36], table[200], det[kEssNodes], p[kEssNodes], roots[kEssRoots];
    ess_basis(d1, d2, B);
    for (int k = 0; k < 10; k++) ess_cubic(B, k, table + 20 * k);
    for (int k = 0; k < kEssNodes; k++) det[k] = ess_det_at(table, k, 1.0);
    for (int j = 0; j < kEssNodes; j++) p[j] = ess_coefficient(det, j);
    const double rho = ess_scale(p);
    for (int k = 0; k < kEssNodes; k++) det[k] = ess_det_at(table, k, rho);
    for (int j = 0; j < kEssNodes; j++) p[j] = ess_coefficient(det, j);
    const int nr = ess_real_roots(p, roots);
    int n = 0;
    for (int r = 0; r < nr; r++)
        if (ess_root_model(table, B, d1, d2, rho * roots[r], E + 9 * n)) {
            if (z0) z0[n] = rho * roots[r];
            n++;
        }
    return n;
}

// a slot's record, written member by member: M may be device memory
MCORB_POSE_HD void ess_write_model(EssModel &M, bool ok, const double *E)
{
    for (int k = 0; k < 9; k++) M.E[k] = ok ? E[k] : 0.0;
    M.valid = ok ? 1 : 0;
    M.pad = 0;
}

// hypothesis h of a call: its sample and its ten slots, the models first in root order
MCORB_POSE_HD void ess_hypothesis(const EssJob &job, int h, const EssObs *obs, EssModel *slots, int32_t *sample)
{
    double d1[kEssSample][3], d2[kEssSample][3], E[9 * kEssRoots];
    int32_t smp[kEssSample];
    const bool ok = ess_sample(job, h, obs, smp, d1, d2);
    const int n = ok ? ess_solve5(d1, d2, E, nullptr) : 0;
    for (int c = 0; c < kEssRoots; c++) ess_write_model(slots[c], c < n, E + 9 * (c < n ? c : 0));
    for (int j = 0; j < kEssSample; j++) sample[j] = smp[j];
}

// OpenCV's Sampson distance, recalled
MCORB_POSE_HD double ess_sampson(const double *E, const EssPt &p)
{
    const double a0 = (E[0] * p.x2 + E[1] * p.y2) + E[2], a1 = (E[3] * p.x2 + E[4] * p.y2) + E[5], a2 = (E[6] * p.x2 + E[7] * p.y2) + E[8];
    const double b0 = (E[0] * p.x1 + E[3] * p.y1) + E[6], b1 = (E[1] * p.x1 + E[4] * p.y1) + E[7];
    const double r = (p.x1 * a0 + p.y1 * a1) + a2;
    return (r * r) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1);
}

// The four candidates of E, mcorb_rel.h's steps 4-5: E is scaled to |E|_F^2 = 2, t^ is the longest of the three cross products of
// its columns (the first of equals), normalised; R+- = cof(E) -+ [t^]x E, each with kRelPolish steps of R <- (R + R^-T) / 2
MCORB_POSE_HD void ess_decompose(const double *E_in, double *Rp, double *Rm, double *th)
{
    double E[9], nn = 0.0;
    for (int j = 0; j < 9; j++) nn += E_in[j] * E_in[j];
    const double scale = __builtin_sqrt(2.0 / nn);
    for (int j = 0; j < 9; j++) E[j] = E_in[j] * scale;
    const double e0[3] = {E[0], E[3], E[6]}, e1[3] = {E[1], E[4], E[7]}, e2[3] = {E[2], E[5], E[8]};
    double x01[3], x12[3], x20[3];
    rel_cross(e0, e1, x01);
    rel_cross(e1, e2, x12);
    rel_cross(e2, e0, x20);
    const double n01 = sac_dot(x01, x01), n12 = sac_dot(x12, x12), n20 = sac_dot(x20, x20);
    double tn = n01;
    th[0] = x01[0], th[1] = x01[1], th[2] = x01[2];
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
    double C[9], TE[9];
    rel_cof(E, C);
    for (int j = 0; j < 3; j++) {
        TE[j] = th[1] * E[6 + j] - th[2] * E[3 + j];
        TE[3 + j] = th[2] * E[j] - th[0] * E[6 + j];
        TE[6 + j] = th[0] * E[3 + j] - th[1] * E[j];
    }
    for (int s = 0; s < 2; s++) {
        double *R = s == 0 ? Rp : Rm;
        for (int j = 0; j < 9; j++) R[j] = s == 0 ? C[j] - TE[j] : C[j] + TE[j];
        for (int it = 0; it < kRelPolish; it++) {
            double K[9];
            rel_cof(R, K);
            const double dR = (R[0] * K[0] + R[1] * K[1]) + R[2] * K[2];
            for (int j = 0; j < 9; j++) R[j] = 0.5 * (R[j] + K[j] / dR);
        }
    }
}

// the depths of a match in both cameras at (R, t): mcorb_rel.h's midpoint with a = d1, b = R d2, w = t; z1 is P1's z, z2 that of
// R^T P2
MCORB_POSE_HD void ess_depths(const double *R, const double *t, const EssPt &p, double &z1, double &z2)
{
    double a[3], d2[3], b[3], P1[3], P2[3];
    ess_bearing(p.x1, p.y1, a);
    ess_bearing(p.x2, p.y2, d2);
    rel_rot(R, d2, b);
    const double aa = sac_dot(a, a), ab = sac_dot(a, b), bb = sac_dot(b, b), aw = sac_dot(a, t), bw = sac_dot(b, t);
    const double det = ab * ab - aa * bb;
    const double lambda = (ab * bw - bb * aw) / det;
    const double mu = (aa * bw - ab * aw) / det;
    for (int i = 0; i < 3; i++) {
        P1[i] = 0.5 * ((lambda * a[i]) + (t[i] + mu * b[i]));
        P2[i] = P1[i] - t[i];
    }
    z1 = P1[2];
    z2 = (R[2] * P2[0] + R[5] * P2[1]) + R[8] * P2[2];
}
// recoverPose's test, recalled: strictly inside (0, distance) in both cameras; a NaN fails
MCORB_POSE_HD bool ess_in_front(double z1, double z2, double distance) { return z1 > 0.0 && z1 < distance && z2 > 0.0 && z2 < distance; }

// candidate c = 0 .. 3: (R+, t^), (R-, t^), (R+, -t^), (R-, -t^)
MCORB_POSE_HD bool ess_candidate_passes(const EssPick &P, int c, const EssPt &p, double distance)
{
    const double *R = (c & 1) ? P.Rm : P.Rp;
    const double t[3] = {c < 2 ? P.t[0] : -P.t[0], c < 2 ? P.t[1] : -P.t[1], c < 2 ? P.t[2] : -P.t[2]};
    double z1, z2;
    ess_depths(R, t, p, z1, z2);
    return ess_in_front(z1, z2, distance);
}

// the winner among the slots: the largest count of those with a model, a tie to the lowest hypothesis, then to the lowest root --
// the order by slot = h * kEssRoots + c, so consensus_key (mcorb_consensus.h) over the slot

// what k_ess_pick writes once the winner is known
MCORB_POSE_HD void ess_pick(const EssModel *models, const int32_t *count, int slot, int n_models, EssPick &P)
{
    for (int j = 0; j < 9; j++) P.E[j] = slot >= 0 ? models[slot].E[j] : 0.0;
    for (int j = 0; j < 9; j++) P.Rp[j] = P.Rm[j] = (j % 4 == 0) ? 1.0 : 0.0;
    for (int j = 0; j < 3; j++) P.t[j] = 0.0;
    if (slot >= 0) ess_decompose(P.E, P.Rp, P.Rm, P.t);
    P.slot = slot;
    P.count = slot >= 0 ? count[slot] : 0;
    P.n_models = n_models;
    P.pad = 0;
}

// the winning candidate: the largest of the four counts, a tie to the lowest index
MCORB_POSE_HD int ess_vote(const int32_t cheir[4])
{
    int w = 0;
    for (int c = 1; c < 4; c++) w = cheir[c] > cheir[w] ? c : w;
    return w;
}

// what k_ess_finish writes for the host
MCORB_POSE_HD void ess_finish(const EssPick &P, const int32_t cheir[4], const int32_t *samples, EssOut &out)
{
    const bool have = P.slot >= 0;
    const int w = ess_vote(cheir);
    const double *R = (w & 1) ? P.Rm : P.Rp;
    for (int j = 0; j < 9; j++) out.R[j] = R[j];
    for (int j = 0; j < 3; j++) out.t[j] = have ? (w < 2 ? P.t[j] : -P.t[j]) : 0.0;
    for (int j = 0; j < 9; j++) out.E[j] = P.E[j];
    out.status = have ? MCORB_ESS_OK : MCORB_ESS_NO_MODEL;
    out.n_ransac_inliers = P.count;
    out.n_inliers = have ? cheir[w] : 0;
    out.best_hypothesis = have ? P.slot / kEssRoots : -1;
    out.best_root = have ? P.slot % kEssRoots : -1;
    for (int j = 0; j < kEssSample; j++) out.sample[j] = have ? samples[kEssSample * (P.slot / kEssRoots) + j] : -1;
    out.n_models = P.n_models;
    for (int c = 0; c < 4; c++) out.cheirality[c] = have ? cheir[c] : 0;
    out.pad = 0;
}

// The four kernels, serially: what a host-only store runs (mcorb_ess.cpp).  models[10 H], samples[5 H], count[10 H] and pts[S] are
// the caller's scratch; flags: S, written.  job.S >= 1
inline void ess_run_serial(const EssJob &job, const EssObs *obs, EssModel *models, int32_t *samples, int32_t *count, EssPt *pts, EssOut &out,
                           uint8_t *flags)
{
    for (int k = 0; k < job.S; k++) ess_point(job, (double)obs[k].u1, (double)obs[k].v1, (double)obs[k].u2, (double)obs[k].v2, pts[k]);
    for (int h = 0; h < job.H; h++) {
        ess_hypothesis(job, h, obs, models + kEssRoots * h, samples + kEssSample * h);
        for (int c = 0; c < kEssRoots; c++) {
            const int slot = kEssRoots * h + c;
            const EssModel &M = models[slot];
            count[slot] = 0;
            if (M.valid)
                for (int k = 0; k < job.S; k++) count[slot] += sac_is_inlier(ess_sampson(M.E, pts[k]), job.threshold2) ? 1 : 0;
        }
    }
    const ConsensusBest won =
        consensus_best<kEssKeyBits>(job.H * kEssRoots, [&](int s) { return models[s].valid; }, [&](int s) { return count[s]; });
    EssPick P;
    ess_pick(models, count, consensus_key_index<kEssKeyBits>(won.key), won.n_models, P);
    int32_t cheir[4] = {0, 0, 0, 0};
    if (P.slot >= 0)
        for (int k = 0; k < job.S; k++)
            if (sac_is_inlier(ess_sampson(P.E, pts[k]), job.threshold2))
                for (int c = 0; c < 4; c++) cheir[c] += ess_candidate_passes(P, c, pts[k], job.distance) ? 1 : 0;
    const int w = ess_vote(cheir);
    for (int k = 0; k < job.S; k++)
        flags[k] = P.slot >= 0 && sac_is_inlier(ess_sampson(P.E, pts[k]), job.threshold2) && ess_candidate_passes(P, w, pts[k], job.distance) ? 1 : 0;
    ess_finish(P, cheir, samples, out);
}

}  // namespace mcorb
