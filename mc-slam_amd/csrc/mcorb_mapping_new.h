// mcorb_mapping_new.h -- the arithmetic of one inter-frame match of FrontEnd::TriangulateNewLandmarks (MCSlam/src/FrontEnd.cpp:
// 6465-6700): the views (getDataForGTSAMTriangulation, :4802-4827), the initial point (triangulateSafe), the 3-unknown
// Levenberg-Marquardt over TriangulationFactor<PinholeCamera<Cal3_S2>> (:6521-6546), the chi-square cull (:6550-6572), the
// parallax gate (:6597-6618) and the new landmark's normal (:6680-6682).  No HIP dependency: the host-only store
// (mcorb_mapping.cpp), k_map_refine_new (mcorb_mapping_gpu.hip) and a plain g++ program include the same code.  Compile with
// -ffp-contract=off: every product, sum, division and sqrt below is one IEEE operation in the order written, in the type
// written, so the device and the host agree bit for bit.  DESIGN.md section 9h has the stated deviations from gtsam.
//
// Per match, in order:
//   views            the previous keyframe's views of queryIdx, cameras ascending, then the current frame's of trainIdx (map_gather);
//                    a view's camera is its frame's proj row (world to camera) and K with skew 0: K[1] is not read
//   initial point    X0 = mcorb::triangulate on x = ((kx - K02) / K00, (ky - K12) / K11), as map_match calls it (map_dlt); a component of X0
//                    that is not finite: verdict 8; p.z <= 0 in any view at X0 (a NaN does not take it): verdict 3
//   factor           p = P[:, :3] * X + P[:, 3] (sum over k from 0.0, then the addend); d = 1.0 / p.z, u = p.x d, v = p.y d;
//                    r = ((fx u + u0) - kx, (fy v + v0) - ky); J = Dpi * P[:, :3], Dpi = ((fx d, 0, -((fx u) d)), (0, fy d,
//                    -((fy v) d))), an entry (D0 B0 + D1 B1) + D2 B2; p.z <= 0: r = (2 fx, 2 fx), J = 0 (gtsam with throwCheirality
//                    false); both are computed and one is selected
//   normal equations over the views in order, each into +0.0: H (6 upper entries, a term J0i J0j + J1i J1j), g (a term J0i rx +
//                    J1i ry), cost = 0.5 * sum (rx rx + ry ry)
//   optimizer        lambda = 1; a trial solves (H + lambda I) delta = -g by a 3 x 3 LDL^T without sqrt (a pivot that is not > 0,
//                    a NaN included, rejects the trial), X' = X + delta, accepted iff cost' < cost; accepted: lambda = lambda / 10,
//                    and the loop ends when cost - cost' <= 1.0 or <= 1e-5 * cost; rejected: lambda = lambda * 10, and the loop
//                    ends when lambda > 1e5; at most 50 solves.  The result is the last accepted X, or X0
//   cull             views in order: (rx rx + ry ry) * (double)inv_sigma2[octave] > 5.991 (a NaN passes): verdict 4
//   parallax         ray = X - cur->twc, dist = sqrt of three squares added in order; ray1 = X - prev->twc, dist1 = (float)sqrt(..);
//                    cos = (float)(dot / ((double)dist1 * dist)); (double)cos >= 0.99998 (a NaN passes): verdict 5, not an inlier
//   landmark         the point is X; normal and n_rays are lm_normal_first over the previous keyframe's views, then lm_normal_add over
//                    the current frame's (map_new_normal)
// Doubles that leave a record go through lm_default_nan: the host and the device give a NaN different signs.
#pragma once
#include "mcorb_mapping.h"

namespace mcorb {

constexpr int kMapDegenerate = 8;   // a component of X0 is not finite (MapVerdict has 0 .. 7)
constexpr int kNewMaxSolves = 50;

// what a match leaves behind next to its MapOut (whose dist2 holds dist and whose cos holds (double)cos): valid for verdicts 0, 4, 5
struct MapNewExtra {
    double cost_initial, cost_final;
    float cos;
    int32_t solves;
};

struct NewSums { double H[6], g[3], cost; };   // H: 00 01 02 11 12 22

MCORB_TRI_HD inline bool new_finite(double x) { return (x - x) == 0.0; }

MCORB_TRI_HD inline float new_default_nan(float x)
{
    uint32_t b;
    __builtin_memcpy(&b, &x, sizeof(b));
    if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;
    __builtin_memcpy(&x, &b, sizeof(b));
    return x;
}

// p.z of a view at X
MCORB_TRI_HD inline double new_depth(const double *P, const double X[3])
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += P[8 + k] * X[k];
    return s + P[11];
}

// the factor's residual and, with J, its Jacobian by X
template <bool WithJ>
MCORB_TRI_HD inline void new_residual(const double *P, const double *K, float kx, float ky, const double X[3], double &rx, double &ry,
                                      double J[2][3])
{
    double p[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += P[4 * r + k] * X[k];
        p[r] = s + P[4 * r + 3];
    }
    const double fx = K[0], fy = K[4], u0 = K[2], v0 = K[5];
    // (no branch: both values of every output are computed and one is taken)
    const bool behind = p[2] <= 0;
    const double d = 1.0 / p[2];
    const double u = p[0] * d, v = p[1] * d;
    const double behind_r = 2.0 * fx;
    rx = behind ? behind_r : (fx * u + u0) - (double)kx;
    ry = behind ? behind_r : (fy * v + v0) - (double)ky;
    if (!WithJ) return;
    const double D00 = fx * d, D02 = -((fx * u) * d), D11 = fy * d, D12 = -((fy * v) * d);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        J[0][c] = behind ? 0.0 : (D00 * P[c] + 0.0 * P[4 + c]) + D02 * P[8 + c];
        J[1][c] = behind ? 0.0 : (0.0 * P[c] + D11 * P[4 + c]) + D12 * P[8 + c];
    }
}

// the normal equations at X over the views in order
MCORB_TRI_HD inline void new_pass(const MapViews &v, const double X[3], NewSums &S)
{
#pragma unroll
    for (int k = 0; k < 6; k++) S.H[k] = 0.0;
    S.g[0] = S.g[1] = S.g[2] = 0.0;
    double sq = 0.0;
    for (int i = 0; i < v.nv; i++) {
        double rx, ry, J[2][3];
        new_residual<true>(v.P[i], v.K[i], v.kx[i], v.ky[i], X, rx, ry, J);
        int at = 0;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a; b < 3; b++, at++) S.H[at] = S.H[at] + (J[0][a] * J[0][b] + J[1][a] * J[1][b]);
#pragma unroll
        for (int a = 0; a < 3; a++) S.g[a] = S.g[a] + (J[0][a] * rx + J[1][a] * ry);
        sq = sq + (rx * rx + ry * ry);
    }
    S.cost = 0.5 * sq;
}

// (H + lambda I) delta = -g by an LDL^T written out; false when a pivot is not > 0, a NaN included
MCORB_TRI_HD inline bool new_solve(const NewSums &S, double lambda, double delta[3])
{
    const double a00 = S.H[0] + lambda, a01 = S.H[1], a02 = S.H[2], a11 = S.H[3] + lambda, a12 = S.H[4], a22 = S.H[5] + lambda;
    const double d0 = a00;
    const double l10 = a01 / d0, l20 = a02 / d0;
    const double d1 = a11 - (l10 * l10) * d0;
    const double l21 = (a12 - (l20 * l10) * d0) / d1;
    const double d2 = (a22 - (l20 * l20) * d0) - (l21 * l21) * d1;
    const bool ok = (d0 > 0) & (d1 > 0) & (d2 > 0);
    const double y0 = -S.g[0];
    const double y1 = -S.g[1] - l10 * y0;
    const double y2 = (-S.g[2] - l20 * y0) - l21 * y1;
    delta[2] = y2 / d2;
    delta[1] = y1 / d1 - l21 * delta[2];
    delta[0] = (y0 / d0 - l10 * delta[1]) - l20 * delta[2];
    return ok;
}

// the optimizer from X0: every loop is bounded by the counts above whatever the data holds
MCORB_TRI_HD inline void new_optimize(const MapViews &v, const double X0[3], double X[3], int32_t &solves, double &cost_initial,
                                      double &cost_final)
{
    NewSums S, T;
    X[0] = X0[0]; X[1] = X0[1]; X[2] = X0[2];
    new_pass(v, X, S);
    double cost = S.cost, lambda = 1.0;
    cost_initial = cost;
    solves = 0;
    for (int it = 0; it < kNewMaxSolves; it++) {
        solves = it + 1;
        double delta[3], Xt[3];
        bool accept = false;
        if (new_solve(S, lambda, delta)) {
#pragma unroll
            for (int k = 0; k < 3; k++) Xt[k] = X[k] + delta[k];
            new_pass(v, Xt, T);
            accept = T.cost < cost;
        }
        if (accept) {
            const double dec = cost - T.cost;
            const bool stop = dec <= 1.0 || dec <= 1e-5 * cost;
#pragma unroll
            for (int k = 0; k < 3; k++) X[k] = Xt[k];
            S = T;
            cost = T.cost;
            lambda = lambda / 10.0;
            if (stop) break;
        } else {
            lambda = lambda * 10.0;
            if (lambda > 1e5) break;
        }
    }
    cost_final = cost;
}

MCORB_TRI_HD inline void new_clear(MapOut &o, MapNewExtra &e)
{
    map_clear(o);
    e.cost_initial = e.cost_final = 0.0;
    e.cos = 0.f;
    e.solves = 0;
}

// everything after the DLT
MCORB_TRI_HD inline void map_refine(const MapViews &v, const double X0[3], const double twc_cur[3], const double twc_prev[3],
                                    const float *inv_sigma2, MapOut &o, MapNewExtra &e)
{
    new_clear(o, e);
    if (!(new_finite(X0[0]) && new_finite(X0[1]) && new_finite(X0[2]))) { o.verdict = kMapDegenerate; return; }
    for (int k = 0; k < 3; k++) o.X[k] = X0[k];
    for (int i = 0; i < v.nv; i++)
        if (new_depth(v.P[i], X0) <= 0) { o.verdict = kMapBehind; return; }
    double X[3];
    new_optimize(v, X0, X, e.solves, e.cost_initial, e.cost_final);
    e.cost_initial = lm_default_nan(e.cost_initial);
    e.cost_final = lm_default_nan(e.cost_final);
    for (int k = 0; k < 3; k++) o.X[k] = lm_default_nan(X[k]);
    for (int i = 0; i < v.nv; i++) {
        double rx, ry;
        new_residual<false>(v.P[i], v.K[i], v.kx[i], v.ky[i], X, rx, ry, nullptr);
        const double err = (rx * rx + ry * ry) * (double)inv_sigma2[v.octave[i]];
        if (err > 5.991) { o.verdict = kMapChi2; return; }
    }
    double ray[3], ray1[3], s = 0.0, s1 = 0.0, dot = 0.0;
    for (int k = 0; k < 3; k++) { ray[k] = X[k] - twc_cur[k]; ray1[k] = X[k] - twc_prev[k]; }
    for (int k = 0; k < 3; k++) s += ray[k] * ray[k];
    for (int k = 0; k < 3; k++) s1 += ray1[k] * ray1[k];
    for (int k = 0; k < 3; k++) dot += ray1[k] * ray[k];
    const double dist = sqrt(s);
    const float dist1 = (float)sqrt(s1);
    const float cosp = (float)(dot / ((double)dist1 * dist));
    o.dist2 = lm_default_nan(dist);
    e.cos = new_default_nan(cosp);
    o.cos = (double)e.cos;
    if ((double)cosp >= 0.99998) { o.verdict = kMapParallax; return; }
    map_new_normal(v, X, o.normal, o.n_rays);
    for (int k = 0; k < 3; k++) o.normal[k] = lm_default_nan(o.normal[k]);
    o.verdict = kMapLandmark;
}

// a call's arguments: MapArgs with frames[0] the current frame and frames[1] the previous keyframe (F is not read), the two poses'
// translation columns and the second half of the records
struct MapNewArgs {
    MapArgs a;
    double twc_cur[3], twc_prev[3];
    MapNewExtra *extra;
};

// one match from the views to the normal.  kAnyViews = false: nv <= 4 only, as triangulate<false>
template <bool kAnyViews>
MCORB_TRI_HD inline void map_new_item(const MapNewArgs &n, const MapItem &it)
{
    const MapArgs &a = n.a;
    MapViews v;
    map_gather_pair(a, it.q, it.t, v);
    double X0[3];
    map_dlt<kAnyViews>(v, X0);
    MapOut o;
    MapNewExtra e;
    map_refine(v, X0, n.twc_cur, n.twc_prev, a.inv_sigma2, o, e);
    a.out[it.rec] = o;
    n.extra[it.rec] = e;
}

// the test hooks (mcorb_host_map_refine, mcorb_dev_map_refine_selftest): everything after the DLT for caller-given X0 (MapCases'
// X), views, the two twc (3 per case each) and the constants
struct MapRefineCases : MapCases { const double *twc_cur, *twc_prev; };

MCORB_TRI_HD inline void map_refine_case(const MapRefineCases &c, int i, MapOut &o, MapNewExtra &e)
{
    MapViews v;
    map_case_views(c, i, v);
    map_refine(v, c.X + 3 * (size_t)i, c.twc_cur + 3 * (size_t)i, c.twc_prev + 3 * (size_t)i, c.inv_sigma2, o, e);
}

}  // namespace mcorb
