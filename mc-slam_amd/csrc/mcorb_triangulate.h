// mcorb_triangulate.h -- the arithmetic of FrontEnd::obtainLfFeatures' per-track work (MCSlam/src/FrontEnd.cpp:280-349) for one
// track: cv::sfm::triangulatePoints restated as the null vector of the DLT design (inverse iteration on its Gram matrix), and
// MultiCameraFrame::computeRepresentativeDesc (MultiCameraFrame.cpp:530-567).  No HIP dependency: the host path
// (mcorb_lf.cpp: mcorb_rig_obtain_lf_features, mcorb_host_triangulate), the device path (k_lf_tracks, mcorb_lf_gpu.hip) and a
// plain g++ test include the same code.  Compile with -ffp-contract=off (the library's flag): every product and sum below is one
// IEEE double operation in the order written.  The only other operations are double division and sqrt, both correctly rounded
// on gfx950 (LLVM expands f64 fdiv into the v_div_scale / v_div_fmas / v_div_fixup sequence and f64 sqrt into v_sqrt_f64 with
// scaling and Newton correction steps), so the device and the host agree bit for bit; tests/test_gpu_live_lf.py checks it on
// 10^5 problems that reach every exit of null_vector_t.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MCORB_TRI_HD __host__ __device__
#else
#define MCORB_TRI_HD
#endif

#ifndef MCORB_MAX_CAMS
#define MCORB_MAX_CAMS 16   // (include/mcorb.h)
#endif

namespace mcorb {

constexpr int kLfMaxN = 4 + MCORB_MAX_CAMS, kLfMaxM = 3 * MCORB_MAX_CAMS;

// which exit null_vector_t took (the device self-test asserts that each is reached)
enum TriBranch { kTriZeroTrace = 0, kTriUnshifted = 1, kTriRayleigh = 2, kTriSylvester = 3 };

template <typename T>
MCORB_TRI_HD inline void tri_swap(T &a, T &b) { T t = a; a = b; b = t; }
MCORB_TRI_HD inline double tri_max(double a, double b) { return a < b ? b : a; }   // std::max(a, b)

// right singular vector of the smallest singular value of the m x n matrix A (row-major, m >= n, n <= 20)
// = eigenvector of the smallest eigenvalue of G = A^T A, found by inverse iteration: G + delta I is factored ONCE (LU with
// partial pivoting, n^3 / 3 multiplications), every further step is two triangular solves.  The design matrices of the
// triangulation have one singular value far below the rest (zero for exact correspondences): unshifted steps until the
// iterate has settled, then Rayleigh-quotient shifts (a fresh n^3 / 3 factorisation per step, nothing at n = 4 .. 8) until
// two successive iterates agree to 1e-15.  Accuracy: eps |G| / (lambda_2 - lambda_1) on the unit vector, 1e-12 .. 1e-11
// for this geometry (the one-sided Jacobi SVD it replaces worked on A itself, eps / sigma_2, at 50 x the cost: 60 sweeps
// of 6 .. 28 column pairs per track were 10 of the 13 ms a 4-camera frame took in round 2).  The test against LAPACK's SVD
// (600 cases of 2 .. 6 views, small and gross noise) holds its 1e-9.
// M, N > 0: compile-time shape (the 2-, 3- and 4-view designs are almost all the tracks of a 4-camera rig: with the loop
// bounds known the compiler unrolls and keeps G / LU in registers); M = N = 0: run-time shape.  Returns the TriBranch taken.
template <int M, int N>
MCORB_TRI_HD inline int null_vector_t(const double *A, int m_rt, int n_rt, double *x)
{
    const int m = M > 0 ? M : m_rt, n = N > 0 ? N : n_rt;
    constexpr int NN = N > 0 ? N : kLfMaxN;
    double G[NN * NN], LU[NN * NN];
    int piv[NN];
    double tr = 0.0;
    for (int p = 0; p < n; p++)
        for (int q = p; q < n; q++) {
            double sacc = 0.0;
            for (int i = 0; i < m; i++) sacc += A[i * n + p] * A[i * n + q];
            G[p * n + q] = G[q * n + p] = sacc;
            if (p == q) tr += sacc;
        }
    if (!(tr > 0.0)) { for (int i = 0; i < n; i++) x[i] = i == n - 1 ? 1.0 : 0.0; return kTriZeroTrace; }
    const double pivmin = 1e-30 * tr;
    // factor G - shift I (LU, partial pivoting); a vanishing pivot is nudged: the solve then blows up along the null vector,
    // which is the point of inverse iteration
    auto factor = [&](double shift) {
        for (int i = 0; i < n * n; i++) LU[i] = G[i];
        for (int i = 0; i < n; i++) LU[i * n + i] -= shift;
        for (int k = 0; k < n; k++) {
            int pk = k;
            for (int i = k + 1; i < n; i++) if (fabs(LU[i * n + k]) > fabs(LU[pk * n + k])) pk = i;
            piv[k] = pk;
            if (pk != k) for (int j = 0; j < n; j++) tri_swap(LU[k * n + j], LU[pk * n + j]);
            double d = LU[k * n + k];
            // (a shift that IS an eigenvalue to the last bit can leave an exactly zero pivot; the nudge must keep the solve
            // finite -- 1 / 1e-300 squared overflows, and the normalisation then turns the iterate into NaNs)
            if (fabs(d) < pivmin) { d = d < 0 ? -pivmin : pivmin; LU[k * n + k] = d; }
            const double inv = 1.0 / d;
            for (int i = k + 1; i < n; i++) {
                const double f = LU[i * n + k] * inv;
                LU[i * n + k] = f;
                if (f != 0.0) for (int j = k + 1; j < n; j++) LU[i * n + j] -= f * LU[k * n + j];
            }
        }
    };
    double v[NN], y[NN];
    auto solve_step = [&]() -> double {   // v <- normalised (G - shift I)^-1 v, sign kept; returns the largest change of a component
        for (int i = 0; i < n; i++) y[i] = v[i];
        for (int k = 0; k < n; k++)            // P (all row exchanges first: the multipliers sit in their final rows)
            if (piv[k] != k) tri_swap(y[k], y[piv[k]]);
        for (int k = 0; k < n; k++)            // L
            for (int i = k + 1; i < n; i++) y[i] -= LU[i * n + k] * y[k];
        for (int k = n - 1; k >= 0; k--) {     // U
            double t = y[k];
            for (int j = k + 1; j < n; j++) t -= LU[k * n + j] * y[j];
            y[k] = t / LU[k * n + k];
        }
        double nn = 0.0, dotp = 0.0;
        for (int i = 0; i < n; i++) nn += y[i] * y[i];
        nn = 1.0 / sqrt(nn);
        for (int i = 0; i < n; i++) { y[i] *= nn; dotp += y[i] * v[i]; }
        const double sgn = dotp < 0 ? -1.0 : 1.0;
        double diff = 0.0;
        for (int i = 0; i < n; i++) { y[i] *= sgn; diff = tri_max(diff, fabs(y[i] - v[i])); v[i] = y[i]; }
        return diff;
    };
    auto rayleigh = [&]() {
        double r = 0.0;
        for (int p = 0; p < n; p++) {
            double gp = 0.0;
            for (int q = 0; q < n; q++) gp += G[p * n + q] * v[q];
            r += v[p] * gp;
        }
        return r;
    };
    for (int i = 0; i < n; i++) v[i] = 1.0 / sqrt((double)n) * (1.0 + 0.01 * i);   // any start with a component along the answer
    // Unshifted steps -- which can only converge to the eigenvector of the eigenvalue nearest zero, the smallest (G is positive
    // semi-definite) -- until the iterate has settled to 1e-3; only then Rayleigh-quotient shifts (cubic from there: two or
    // three steps where the unshifted iteration, contracting by lambda_1 / lambda_2 = 0.1 .. 0.5 on tracks with a wrong
    // correspondence, needs dozens).  Shifting earlier is not safe: a start vector that happens to be nearly orthogonal to the
    // answer still has its quotient near lambda_2 after a few steps, and the shifted iteration then converges THERE (seen on 2 %
    // of real tracks).  Should a shifted step move the iterate by more than 1e-2 it has left the basin: back to unshifted steps.
    factor(-1e-14 * tr);   // (keeps the factorisation away from an exactly singular matrix)
    double diff = 1.0;
    for (int it = 0; it < 400 && diff >= 1e-3; it++) diff = solve_step();
    bool shifted = false;
    int branch = kTriUnshifted;
    for (int it = 0; it < 8 && diff >= 1e-15; it++) {
        factor(rayleigh());
        diff = solve_step();
        shifted = true;
        if (diff > 1e-2) break;
    }
    if (shifted) {
        // "settled" can also mean: sitting next to ANOTHER eigenvector with a tiny component along the wanted one (an unlucky
        // start); the shifted steps then polish that one.  Sylvester: G - (rho - tol) I has as many negative pivots in its LDL^T
        // as G has eigenvalues below rho - tol -- none when rho is the smallest.  Otherwise: unshifted iteration to the end.
        branch = kTriRayleigh;
        const double rho = rayleigh(), tol = 1e-10 * tr + 1e-3 * fabs(rho);
        bool smallest = diff <= 1e-2;   // (false for a NaN too)
        if (smallest) {
            for (int i = 0; i < n * n; i++) LU[i] = G[i];
            for (int i = 0; i < n; i++) LU[i * n + i] -= rho - tol;
            for (int k = 0; k < n && smallest; k++) {
                const double d = LU[k * n + k];
                if (!(d > 0.0)) { smallest = false; break; }
                for (int i = k + 1; i < n; i++) {
                    const double f = LU[i * n + k] / d;
                    for (int j = k + 1; j < n; j++) LU[i * n + j] -= f * LU[k * n + j];
                }
            }
        }
        if (!smallest) {
            branch = kTriSylvester;
            for (int i = 0; i < n; i++) v[i] = 1.0 / sqrt((double)n) * (1.0 + 0.01 * i);
            factor(-1e-14 * tr);
            diff = 1.0;
            for (int k = 0; k < 2000 && diff >= 1e-15; k++) diff = solve_step();
        }
    }
    for (int i = 0; i < n; i++) x[i] = v[i];
    return branch;
}
MCORB_TRI_HD inline int null_vector(const double *A, int m, int n, double *x)
{
    if (m == 4 && n == 4) return null_vector_t<4, 4>(A, m, n, x);
    else if (m == 9 && n == 7) return null_vector_t<9, 7>(A, m, n, x);
    else if (m == 12 && n == 8) return null_vector_t<12, 8>(A, m, n, x);
    else return null_vector_t<0, 0>(A, m, n, x);
}

// triangulateNViews' design [-P_i | x_i in column 4+i] (X, alpha_1..alpha_n)^T = 0 for NV views (NV > 0: compile-time, the
// design sized to it; NV = 0: nv_rt views in the largest design), and its null vector's first four entries
template <int NV>
MCORB_TRI_HD inline int triangulate_nviews(const double *x, const double *const *P, int nv_rt, double h[4])
{
    const int nv = NV > 0 ? NV : nv_rt, m = 3 * nv, n = 4 + nv;
    constexpr int DM = NV > 0 ? 3 * NV : kLfMaxM, DN = NV > 0 ? 4 + NV : kLfMaxN;
    double D[DM * DN], sol[DN];
    for (int i = 0; i < m * n; i++) D[i] = 0.0;
    for (int i = 0; i < nv; i++) {
        for (int jj = 0; jj < 3; jj++)
            for (int ii = 0; ii < 4; ii++) D[(size_t)(3 * i + jj) * n + ii] = -P[i][4 * jj + ii];
        D[(size_t)(3 * i + 0) * n + 4 + i] = x[2 * i];
        D[(size_t)(3 * i + 1) * n + 4 + i] = x[2 * i + 1];
        D[(size_t)(3 * i + 2) * n + 4 + i] = 1.0;
    }
    const int br = null_vector(D, m, n, sol);
    for (int i = 0; i < 4; i++) h[i] = sol[i];
    return br;
}

// cv::sfm::triangulatePoints for one point seen in nv views: x = normalised image coordinates, P = 3x4 [R|t] (row-major).
// Returns the TriBranch of its null vector.  kAnyViews = false: nv <= 4 only (the run-time-shaped solver and its 48 x 20 design
// are not compiled in; k_lf_tracks' instance for rigs of up to four cameras, whose scratch is then a few hundred bytes per lane).
template <bool kAnyViews = true>
MCORB_TRI_HD inline int triangulate(const double *x, const double *const *P, int nv, double X[3])
{
    double h[4];
    int br;
    if (nv == 2) {   // triangulateDLT
        double D[16];
        for (int i = 0; i < 4; i++) {
            D[0 * 4 + i] = x[0] * P[0][8 + i] - P[0][0 + i];
            D[1 * 4 + i] = x[1] * P[0][8 + i] - P[0][4 + i];
            D[2 * 4 + i] = x[2] * P[1][8 + i] - P[1][0 + i];
            D[3 * 4 + i] = x[3] * P[1][8 + i] - P[1][4 + i];
        }
        br = null_vector(D, 4, 4, h);
    } else if (nv == 3) {
        br = triangulate_nviews<3>(x, P, nv, h);
    } else if (nv == 4) {
        br = triangulate_nviews<4>(x, P, nv, h);
    } else if (kAnyViews) {
        br = triangulate_nviews<0>(x, P, nv, h);
    } else {
        br = kTriZeroTrace;
        h[0] = h[1] = h[2] = 0.0; h[3] = 1.0;
    }
    for (int i = 0; i < 3; i++) X[i] = h[i] / h[3];   // homogeneousToEuclidean
    return br;
}

// ORBextractor::DescriptorDistance (ORBextractor.cpp:1202-1218) on two 32-byte rows
MCORB_TRI_HD inline int tri_hamming256(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int i = 0; i < 32; i += 4) {
        uint32_t u = (uint32_t)a[i] | (uint32_t)a[i + 1] << 8 | (uint32_t)a[i + 2] << 16 | (uint32_t)a[i + 3] << 24;
        uint32_t w = (uint32_t)b[i] | (uint32_t)b[i + 1] << 8 | (uint32_t)b[i + 2] << 16 | (uint32_t)b[i + 3] << 24;
        uint32_t v = u ^ w;
        v = v - ((v >> 1) & 0x55555555u);
        v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
        d += (int)((((v + (v >> 4)) & 0xF0F0F0Fu) * 0x1010101u) >> 24);
    }
    return d;
}

// computeRepresentativeDesc (MultiCameraFrame.cpp:530-567): the row whose median Hamming distance to all n rows (itself included,
// at 0) is smallest, median = sorted[(size_t)(0.5 * (n - 1))], the first minimum wins.  rows[i]: the i-th 32-byte row;
// 1 <= n <= MCORB_MAX_CAMS.  The same integer as mcorb_representative_desc.
MCORB_TRI_HD inline int representative_desc(const uint8_t *const *rows, int n)
{
    int best_median = 0x7fffffff, best_idx = 0;
    for (int i = 0; i < n; i++) {
        int row[MCORB_MAX_CAMS];
        for (int j = 0; j < n; j++) row[j] = i == j ? 0 : tri_hamming256(rows[i], rows[j]);
        for (int a = 1; a < n; a++) {   // (any sort gives the same sorted ints)
            const int t = row[a];
            int b = a - 1;
            while (b >= 0 && row[b] > t) { row[b + 1] = row[b]; b--; }
            row[b + 1] = t;
        }
        const int median = row[(size_t)(0.5 * (n - 1))];
        if (median < best_median) { best_median = median; best_idx = i; }
    }
    return best_idx;
}

}  // namespace mcorb
