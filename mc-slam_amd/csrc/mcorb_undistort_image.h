// mcorb_undistort_image.h -- the RECTIFY branch of MultiCameraFrame::setData (MCSlam/src/MultiCameraFrame.cpp:123-136):
// cv::undistort(img, undistImg, K, dist) on an 8-bit one-channel image, in its two halves.  (a) The fixed-point map, which depends
// on the calibration alone: built once per camera on the host (its row loop is a serial sum).  (b) The resampling of one pixel,
// remap(.., INTER_LINEAR, BORDER_CONSTANT): the hot path, shared by k_remap_u8 (mcorb_handoff_gpu.hip), the host form and a plain g++
// test (tests/cpp/test_undistort_image.cpp).  No HIP dependency.  Compile with -ffp-contract=off (the library's flag): every
// product and sum of the map is one IEEE double operation in the order written.
// Restated from OpenCV 4.x (modules/calib3d/src/undistort.dispatch.cpp, undistort.simd.hpp, core/src/lapack.cpp) as recalled:
// no cv::undistort has been executed against it (docs/design/02_oracle.md).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MCORB_UDI_HD __host__ __device__
#else
#define MCORB_UDI_HD
#endif

namespace mcorb {

// One camera as cv::undistort sees it: K and dist are the CV_64F values they are (convertTo(CV_64F) / Mat_<double>() of a CV_64F
// Mat is a copy) -- unlike UndistortKeyPoints there is no trip through float.
struct UndistImageCam {
    double K[9];    // row-major 3x3
    double k[14];   // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tauX tauY, zero-filled (OpenCV's k[14]; the tilt pair stays 0)
};

// n = 4, 5, 8 or 12; the 14-coefficient tilt model is refused as in mcorb_undistort.h.  Returns 0, or -1 for a count not taken.
inline int undist_image_prepare(const double *K, const double *dist, int n, UndistImageCam &c)
{
    if (n != 4 && n != 5 && n != 8 && n != 12) return -1;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < 9; i++) c.K[i] = K[i];
    for (int i = 0; i < n; i++) c.k[i] = dist[i];
    return 0;
}

// rows per stripe of cv::undistort: min(max(1, (1 << 12) / max(cols, 1)), rows)
inline int undist_image_stripe(int cols, int rows)
{
    int s = 4096 / (cols > 1 ? cols : 1);
    if (s < 1) s = 1;
    return s < rows ? s : rows;
}

// saturate_cast<int>(double) = cvRound: round half to even (the default rounding mode); what does not fit an int is the
// "integer indefinite" 0x80000000 of cvtsd2si, NaN included
inline int32_t undist_image_round(double v)
{
    const double r = nearbyint(v);
    if (!(r >= -2147483648. && r <= 2147483647.)) return INT32_MIN;
    return (int32_t)r;
}

// (Ar * I).inv(DECOMP_LU) of a 3x3 CV_64F matrix: the product by gemm's s = 0; s += a(i, k) * b(k, j) and cv::invert's closed
// form for n == 3 (det3, then the adjugate times 1/det).  false: singular (d == 0), where OpenCV returns zeros.
inline bool undist_image_inv3(const double *Ar, double *ir)
{
    static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double S[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += Ar[i * 3 + k] * I[k * 3 + j];
            S[i * 3 + j] = s;
        }
#define MCORB_SD(y, x) S[(y) * 3 + (x)]
    double d = MCORB_SD(0, 0) * (MCORB_SD(1, 1) * MCORB_SD(2, 2) - MCORB_SD(1, 2) * MCORB_SD(2, 1)) -
               MCORB_SD(0, 1) * (MCORB_SD(1, 0) * MCORB_SD(2, 2) - MCORB_SD(1, 2) * MCORB_SD(2, 0)) +
               MCORB_SD(0, 2) * (MCORB_SD(1, 0) * MCORB_SD(2, 1) - MCORB_SD(1, 1) * MCORB_SD(2, 0));
    if (d == 0.) { for (int i = 0; i < 9; i++) ir[i] = 0.; return false; }
    d = 1. / d;
    ir[0] = (MCORB_SD(1, 1) * MCORB_SD(2, 2) - MCORB_SD(1, 2) * MCORB_SD(2, 1)) * d;
    ir[1] = (MCORB_SD(0, 2) * MCORB_SD(2, 1) - MCORB_SD(0, 1) * MCORB_SD(2, 2)) * d;
    ir[2] = (MCORB_SD(0, 1) * MCORB_SD(1, 2) - MCORB_SD(0, 2) * MCORB_SD(1, 1)) * d;
    ir[3] = (MCORB_SD(1, 2) * MCORB_SD(2, 0) - MCORB_SD(1, 0) * MCORB_SD(2, 2)) * d;
    ir[4] = (MCORB_SD(0, 0) * MCORB_SD(2, 2) - MCORB_SD(0, 2) * MCORB_SD(2, 0)) * d;
    ir[5] = (MCORB_SD(0, 2) * MCORB_SD(1, 0) - MCORB_SD(0, 0) * MCORB_SD(1, 2)) * d;
    ir[6] = (MCORB_SD(1, 0) * MCORB_SD(2, 1) - MCORB_SD(1, 1) * MCORB_SD(2, 0)) * d;
    ir[7] = (MCORB_SD(0, 1) * MCORB_SD(2, 0) - MCORB_SD(0, 0) * MCORB_SD(2, 1)) * d;
    ir[8] = (MCORB_SD(0, 0) * MCORB_SD(1, 1) - MCORB_SD(0, 1) * MCORB_SD(1, 0)) * d;
#undef MCORB_SD
    return true;
}

// The maps of a cols x rows image: map1 (cols * rows pairs of shorts, x then y), map2 (cols * rows), row-major without padding.
// cv::undistort's stripe loop around initUndistortRectifyMap(A, dist, I, Ar, Size(cols, stripe), CV_16SC2, ..), scalar row loop.
inline void undist_image_map(const UndistImageCam &c, int cols, int rows, int16_t *map1, uint16_t *map2)
{
    const double *A = c.K, *k = c.k;
    const double u0 = A[2], v0 = A[5], fx = A[0], fy = A[4];
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    const double s1 = k[8], s2 = k[9], s3 = k[10], s4 = k[11];
    const int stripe0 = undist_image_stripe(cols, rows);
    double Ar[9];
    for (int i = 0; i < 9; i++) Ar[i] = A[i];
    const double v0r = Ar[5];   // double v0 = Ar(1, 2);
    for (int y0 = 0; y0 < rows; y0 += stripe0) {
        const int stripe = stripe0 < rows - y0 ? stripe0 : rows - y0;
        Ar[5] = v0r - y0;   // Ar(1, 2) = v0 - y;
        double ir[9];
        undist_image_inv3(Ar, ir);
        for (int i = 0; i < stripe; i++) {
            int16_t *m1 = map1 + (size_t)(y0 + i) * cols * 2;
            uint16_t *m2 = map2 + (size_t)(y0 + i) * cols;
            // double _x = i*ir[1] + ir[2], _y = i*ir[4] + ir[5], _w = i*ir[7] + ir[8];
            double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
            // for( ; j < size.width; j++, _x += ir[0], _y += ir[3], _w += ir[6] )
            for (int j = 0; j < cols; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
                const double w = 1. / _w, x = _x * w, y = _y * w;
                const double x2 = x * x, y2 = y * y;
                const double r2 = x2 + y2, _2xy = 2 * x * y;
                const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
                const double xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2);
                const double yd = (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2);
                // cv::Vec3d vecTilt = matTilt*cv::Vec3d(xd, yd, 1);   matTilt = Matx33d::eye() (tauX == tauY == 0), written out as
                // Matx * Vec accumulates it (mcorb_undistort.h)
                double vt0 = 0, vt1 = 0, vt2 = 0;
                vt0 += 1. * xd; vt0 += 0. * yd; vt0 += 0. * 1.;
                vt1 += 0. * xd; vt1 += 1. * yd; vt1 += 0. * 1.;
                vt2 += 0. * xd; vt2 += 0. * yd; vt2 += 1. * 1.;
                const double invProj = vt2 != 0. ? 1. / vt2 : 1.;
                const double u = fx * invProj * vt0 + u0;
                const double v = fy * invProj * vt1 + v0;
                const int32_t iu = undist_image_round(u * 32);   // saturate_cast<int>(u*INTER_TAB_SIZE)
                const int32_t iv = undist_image_round(v * 32);
                m1[j * 2] = (int16_t)(iu >> 5);
                m1[j * 2 + 1] = (int16_t)(iv >> 5);
                m2[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
            }
        }
    }
}

// The four bilinear weights of fractional position m2 (fx = m2 & 31, fy = m2 >> 5), taps (0,0) (1,0) (0,1) (1,1): exact integers
// that sum to 32768 (INTER_REMAP_COEF_SCALE), held in int -- position (0, 0) weighs its pixel with the full 32768.
MCORB_UDI_HD inline void remap_weights(unsigned m2, int w[4])
{
    const int fx = (int)(m2 & 31u), fy = (int)((m2 >> 5) & 31u);
    w[0] = (32 - fx) * (32 - fy) * 32;
    w[1] = fx * (32 - fy) * 32;
    w[2] = (32 - fx) * fy * 32;
    w[3] = fx * fy * 32;
}

// One pixel of one output position: where its four taps lie (byte offsets into a plane of row stride `stride`; a tap outside the
// w x h source gets offset 0 and weight 0 -- BORDER_CONSTANT with value 0) and what they weigh.  Depends on the map alone.
struct RemapTaps {
    int32_t off[4];
    int32_t wt[4];
};
MCORB_UDI_HD inline void remap_taps(int sx, int sy, unsigned m2, int w, int h, int stride, RemapTaps &t)
{
    remap_weights(m2, t.wt);
    const bool x0 = sx >= 0 && sx < w, x1 = sx + 1 >= 0 && sx + 1 < w;
    const bool y0 = sy >= 0 && sy < h, y1 = sy + 1 >= 0 && sy + 1 < h;
    const bool in[4] = {x0 && y0, x1 && y0, x0 && y1, x1 && y1};
    for (int i = 0; i < 4; i++) {
        t.off[i] = in[i] ? (sy + (i >> 1)) * stride + sx + (i & 1) : 0;
        if (!in[i]) t.wt[i] = 0;
    }
}
// dst = (sum w * p + 16384) >> 15 (FixedPtCast<int, uchar, INTER_REMAP_COEF_BITS>; the sum is at most 255 * 32768)
MCORB_UDI_HD inline uint8_t remap_pixel(const uint8_t *src, const RemapTaps &t)
{
    const int s = t.wt[0] * src[t.off[0]] + t.wt[1] * src[t.off[1]] + t.wt[2] * src[t.off[2]] + t.wt[3] * src[t.off[3]];
    return (uint8_t)((s + 16384) >> 15);
}

// remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) of a w x h 8UC1 image (the maps as undist_image_map lays them out)
inline void remap_u8(const uint8_t *src, int src_stride, int w, int h, const int16_t *map1, const uint16_t *map2, uint8_t *dst,
                     int dst_stride)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            RemapTaps t;
            remap_taps(map1[2 * i], map1[2 * i + 1], map2[i], w, h, src_stride, t);
            dst[(size_t)y * dst_stride + x] = remap_pixel(src, t);
        }
}

}  // namespace mcorb
