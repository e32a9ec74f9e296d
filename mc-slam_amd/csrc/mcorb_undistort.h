// mcorb_undistort.h -- MultiCameraFrame::UndistortKeyPoints (MCSlam/src/MultiCameraFrame.cpp:300-347) for one keypoint: the
// arithmetic of cv::undistortPoints as the reference calls it.  No HIP dependency: k_undistort (mcorb_handoff_gpu.hip) and a plain
// g++ test (tests/cpp/test_undistort.cpp) include the same code.  Compile with -ffp-contract=off (the library's flag): every
// product and sum below is one IEEE double operation in the order written, so device, host and a numpy restatement agree bit
// for bit.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MCORB_UD_HD __host__ __device__
#else
#define MCORB_UD_HD
#endif

namespace mcorb {

// One camera as cv::undistortPoints sees it.  The reference keeps K and the coefficients as CV_64F (DatasetReader.cpp:108-111,
// 192-203), converts both to CV_32F before the call (MultiCameraFrame.cpp:324-325), and undistortPoints converts them back to
// double (cvConvert into double A[3][3], k[14]): every value here is (double)(float)value.
struct UndistCam {
    double K[9];    // row-major 3x3
    double k[12];   // k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]], zero-filled (OpenCV's k[0..11])
    int32_t mode;   // 0: copy the point (camera not set, or the reference's zero test says so), 1: undistort
    int32_t pad;
};

// The reference's zero test (MultiCameraFrame.cpp:302): dist_coeffs_[cam].at<float>(0) == 0.0 on a CV_64F Mat.  Release OpenCV
// does not check the element type, so it reads the low 4 bytes of the double k1 (little-endian) as a float: the camera is passed
// through unchanged iff those 32 bits are +0 or -0.  True for k1 == 0, but also for any k1 with a short binary mantissa
// (k1 = -0.25, 0.5, ...), and false for almost every calibrated value.
inline bool undist_zero_test(double k1)
{
    uint64_t b;
    memcpy(&b, &k1, sizeof(b));
    return ((uint32_t)b & 0x7fffffffu) == 0;
}

// Fills c from camconfig's CV_64F values (K: 3x3 row-major, dist: n coefficients).  n = 4, 5, 8 or 12 (zero-filled to 12); the
// 14-coefficient tilt model is refused (no reference reader produces it).  Returns 0, or -1 for a count it does not take.
inline int undist_prepare(const double *K, const double *dist, int n, UndistCam &c)
{
    if (n != 4 && n != 5 && n != 8 && n != 12) return -1;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < 9; i++) c.K[i] = (double)(float)K[i];
    for (int i = 0; i < n; i++) c.k[i] = (double)(float)dist[i];
    c.mode = undist_zero_test(dist[0]) ? 0 : 1;
    return 0;
}

// cvUndistortPointsInternal, OpenCV 4.x (modules/calib3d/src/undistort.dispatch.cpp), for one CV_32FC2 point with
// R = noArray(), P = K, and the criteria of the undistortPoints(src, dst, K, D, R, P) overload,
// TermCriteria(MAX_ITER, 5, 0.01): COUNT only, so exactly 5 iterations and no EPS test.  Line by line:
MCORB_UD_HD inline void undistort_point(const UndistCam &c, float px, float py, float &ox, float &oy)
{
    if (c.mode == 0) { ox = px; oy = py; return; }   // (the reference copies the keypoint, :302-307)
    const double *A = c.K, *k = c.k;
    // double fx = A[0][0]; double fy = A[1][1]; double ifx = 1./fx; double ify = 1./fy; double cx = A[0][2]; double cy = A[1][2];
    const double fx = A[0], fy = A[4];
    const double ifx = 1. / fx, ify = 1. / fy;
    const double cx = A[2], cy = A[5];
    // x = srcf[i*sstep].x; y = srcf[i*sstep].y; u = x; v = y;
    double x = (double)px, y = (double)py;
    const double u = x, v = y;
    // x = (x - cx)*ifx; y = (y - cy)*ify;
    x = (x - cx) * ifx;
    y = (y - cy) * ify;
    // cv::Vec3d vecUntilt = invMatTilt * cv::Vec3d(x, y, 1);   invMatTilt = Matx33d::eye() (k[12] == k[13] == 0).
    // Matx * Vec accumulates s = 0; s += a(i, j) * b(j) over j (Matx_MatMulOp): written out, signed zeros included.
    double vu0 = 0, vu1 = 0, vu2 = 0;
    vu0 += 1. * x; vu0 += 0. * y; vu0 += 0. * 1.;
    vu1 += 0. * x; vu1 += 1. * y; vu1 += 0. * 1.;
    vu2 += 0. * x; vu2 += 0. * y; vu2 += 1. * 1.;
    // double invProj = vecUntilt(2) ? 1./vecUntilt(2) : 1;
    const double invProj = vu2 != 0. ? 1. / vu2 : 1.;
    // x0 = x = invProj * vecUntilt(0); y0 = y = invProj * vecUntilt(1);
    x = invProj * vu0;
    y = invProj * vu1;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {   // for (int j = 0; ; j++) { if ((criteria.type & COUNT) && j >= criteria.maxCount) break; ...
        // double r2 = x*x + y*y;
        const double r2 = x * x + y * y;
        // double icdist = (1 + ((k[7]*r2 + k[6])*r2 + k[5])*r2)/(1 + ((k[4]*r2 + k[1])*r2 + k[0])*r2);
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        // if (icdist < 0) { x = (u - cx)*ifx; y = (v - cy)*ify; break; }   (test: undistortPoints.regression_14583)
        if (icdist < 0) {
            x = (u - cx) * ifx;
            y = (v - cy) * ify;
            break;
        }
        // double deltaX = 2*k[2]*x*y + k[3]*(r2 + 2*x*x)+ k[8]*r2+k[9]*r2*r2;
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        // double deltaY = k[2]*(r2 + 2*y*y) + 2*k[3]*x*y+ k[10]*r2+k[11]*r2*r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        // x = (x0 - deltaX)*icdist; y = (y0 - deltaY)*icdist;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    // RR = P(3x3) * R = K * I: RR[i][j] == K[i][j]
    // double xx = RR[0][0]*x + RR[0][1]*y + RR[0][2];
    const double xx = A[0] * x + A[1] * y + A[2];
    // double yy = RR[1][0]*x + RR[1][1]*y + RR[1][2];
    const double yy = A[3] * x + A[4] * y + A[5];
    // double ww = 1./(RR[2][0]*x + RR[2][1]*y + RR[2][2]);
    const double ww = 1. / (A[6] * x + A[7] * y + A[8]);
    // x = xx*ww; y = yy*ww;  dstf[i*dstep].x = (float)x; dstf[i*dstep].y = (float)y;
    ox = (float)(xx * ww);
    oy = (float)(yy * ww);
}

}  // namespace mcorb
