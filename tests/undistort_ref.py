"""Independent numpy float64 restatement of MultiCameraFrame::UndistortKeyPoints (MultiCameraFrame.cpp:300-347): the zero test
and cv::undistortPoints(pts, pts, K, dist, noArray(), K) as OpenCV 4.x's cvUndistortPointsInternal computes it
(modules/calib3d/src/undistort.dispatch.cpp, TermCriteria(MAX_ITER, 5, 0.01)).  Written from the OpenCV source, not from
mcorb_undistort.h; numpy evaluates every array expression one IEEE operation at a time, left to right, without contraction,
so the result is bit-comparable with the library's."""
import numpy as np


def zero_test(k1):
    """dist_coeffs_[cam].at<float>(0) == 0.0 on a CV_64F Mat (:302): the low 32 bits of the double k1 read as a float"""
    lo = int(np.array([k1], "<f8").view("<u4")[0])
    return (lo & 0x7FFFFFFF) == 0


def coeffs(dist):
    """OpenCV's k[14] after cvConvert of the CV_32F copy (:324-325): float-rounded, zero-filled"""
    dist = np.asarray(dist, np.float64).ravel()
    if dist.size not in (4, 5, 8, 12):
        raise ValueError("coefficient count %d" % dist.size)
    k = np.zeros(14, np.float64)
    k[:dist.size] = dist.astype(np.float32).astype(np.float64)
    return k


def undistort(u32, v32, K, dist):
    """u32, v32: float32 arrays (the keypoints' pt); K: 3x3 CV_64F, dist: 4/5/8/12 CV_64F coefficients.
    Returns float32 (x, y) arrays, or the input unchanged when the zero test passes the camera through."""
    u32 = np.asarray(u32, np.float32)
    v32 = np.asarray(v32, np.float32)
    if zero_test(np.asarray(dist, np.float64).ravel()[0]):
        return u32.copy(), v32.copy()
    A = np.asarray(K, np.float64).reshape(3, 3).astype(np.float32).astype(np.float64)
    k = coeffs(dist)
    one = np.float64(1.0)
    zero = np.float64(0.0)
    fx, fy = A[0, 0], A[1, 1]
    ifx, fy_inv = one / fx, one / fy
    cx, cy = A[0, 2], A[1, 2]
    x = u32.astype(np.float64)
    y = v32.astype(np.float64)
    u, v = x.copy(), y.copy()
    x = (x - cx) * ifx
    y = (y - cy) * fy_inv
    # invMatTilt (identity) * Vec3d(x, y, 1), accumulated from s = 0
    e = np.eye(3)
    vec = [np.zeros_like(x) for _ in range(3)]
    for i in range(3):
        s = np.full_like(x, zero)
        s = s + e[i, 0] * x
        s = s + e[i, 1] * y
        s = s + e[i, 2] * one
        vec[i] = s
    inv_proj = np.where(vec[2] != 0, one / np.where(vec[2] != 0, vec[2], one), one)
    x = inv_proj * vec[0]
    y = inv_proj * vec[1]
    x0, y0 = x.copy(), y.copy()
    done = np.zeros(x.shape, bool)
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        neg = (icdist < 0) & ~done
        x = np.where(neg, (u - cx) * ifx, x)
        y = np.where(neg, (v - cy) * fy_inv, y)
        done |= neg
        deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = np.where(done, x, (x0 - deltaX) * icdist)
        y = np.where(done, y, (y0 - deltaY) * icdist)
    RR = A   # P * R = K * I
    xx = RR[0, 0] * x + RR[0, 1] * y + RR[0, 2]
    yy = RR[1, 0] * x + RR[1, 1] * y + RR[1, 2]
    ww = one / (RR[2, 0] * x + RR[2, 1] * y + RR[2, 2])
    return (xx * ww).astype(np.float32), (yy * ww).astype(np.float32)


def undistort_records(kps, K, dist):
    """image_kps_undist of one image: the keypoint records with pt replaced (:336-344)"""
    out = np.array(kps, copy=True)
    if len(out):
        out["x"], out["y"] = undistort(out["x"], out["y"], K, dist)
    return out


def distort(xn, yn, dist):
    """forward radtan / rational / thin-prism model on normalised coordinates (float64), for the round-trip check"""
    k = coeffs(dist)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = k[:12]
    r2 = xn * xn + yn * yn
    r4, r6 = r2 * r2, r2 * r2 * r2
    rad = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn) + s1 * r2 + s2 * r4
    yd = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn + s3 * r2 + s4 * r4
    return xd, yd
