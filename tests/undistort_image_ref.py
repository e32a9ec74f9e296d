"""Independent numpy float64 restatement of the RECTIFY branch of MultiCameraFrame::setData (MultiCameraFrame.cpp:123-136):
cv::undistort(img, undistImg, K, dist) on an 8-bit one-channel image as OpenCV 4.x computes it -- the fixed-point map
(undistort's stripe loop around initUndistortRectifyMap to CV_16SC2) and remap(INTER_LINEAR, BORDER_CONSTANT 0).  Written from
the description of those functions, not from mcorb_undistort_image.h; numpy evaluates every array expression one IEEE operation
at a time, left to right, without contraction, and np.add.accumulate sums sequentially, so the maps are bit-comparable with
the library's."""
import numpy as np

INT_MIN = -2 ** 31


def coeffs(dist):
    """OpenCV's k[14]: the CV_64F values as they are, zero-filled; 4, 5, 8 or 12 of them"""
    dist = np.asarray(dist, np.float64).ravel()
    if dist.size not in (4, 5, 8, 12):
        raise ValueError("coefficient count %d" % dist.size)
    k = np.zeros(14, np.float64)
    k[:dist.size] = dist
    return k


def stripe_height(cols, rows):
    return min(max(1, 4096 // max(cols, 1)), rows)


def inv3(M):
    """cv::invert of a 3x3 CV_64F matrix (DECOMP_LU takes the closed form for n == 3): det by the first row's cofactors, then
    the adjugate times 1/det"""
    m = [[np.float64(M[i][j]) for j in range(3)] for i in range(3)]
    d = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
         + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    if d == 0:
        return np.zeros(9)
    d = np.float64(1.0) / d
    t = np.empty(9, np.float64)
    t[0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) * d
    t[1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * d
    t[2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * d
    t[3] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) * d
    t[4] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * d
    t[5] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * d
    t[6] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) * d
    t[7] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * d
    t[8] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * d
    return t


def times_identity(M):
    """Ar * I as gemm accumulates it: s = 0; s += a[i][k] * b[k][j]"""
    eye = np.eye(3)
    out = np.zeros((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            s = np.float64(0.0)
            for k in range(3):
                s = s + np.float64(M[i][k]) * eye[k][j]
            out[i][j] = s
    return out


def round_to_int(v):
    """saturate_cast<int>(double): round half to even; what an int cannot hold (NaN included) is 0x80000000"""
    r = np.rint(v)
    ok = (r >= -2147483648.0) & (r <= 2147483647.0)
    return np.where(ok, np.where(ok, r, 0.0).astype(np.int64), INT_MIN)


def running(start, step, n):
    """start, start + step, (start + step) + step, ..: the row loop's serial sum"""
    a = np.full(n, step, np.float64)
    a[0] = start
    return np.add.accumulate(a)


def undistort_map(K, dist, cols, rows):
    """(map1 (rows, cols, 2) int16, map2 (rows, cols) uint16)"""
    A = np.asarray(K, np.float64).reshape(3, 3)
    k = coeffs(dist)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = k[:12]
    u0, v0, fx, fy = A[0, 2], A[1, 2], A[0, 0], A[1, 1]
    one, zero = np.float64(1.0), np.float64(0.0)
    map1 = np.zeros((rows, cols, 2), np.int16)
    map2 = np.zeros((rows, cols), np.uint16)
    sh = stripe_height(cols, rows)
    for y0 in range(0, rows, sh):
        Ar = A.copy()
        Ar[1, 2] = A[1, 2] - np.float64(y0)
        ir = inv3(times_identity(Ar))
        for i in range(min(sh, rows - y0)):
            fi = np.float64(i)
            _x = running(fi * ir[1] + ir[2], ir[0], cols)
            _y = running(fi * ir[4] + ir[5], ir[3], cols)
            _w = running(fi * ir[7] + ir[8], ir[6], cols)
            w = one / _w
            x = _x * w
            y = _y * w
            x2 = x * x
            y2 = y * y
            r2 = x2 + y2
            _2xy = 2 * x * y
            kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
            xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2
            yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
            # the identity tilt matrix times (xd, yd, 1), accumulated from s = 0
            e = np.eye(3)
            vec = []
            for r in range(3):
                s = np.full_like(xd, zero)
                s = s + e[r, 0] * xd
                s = s + e[r, 1] * yd
                s = s + e[r, 2] * one
                vec.append(s)
            inv_proj = np.where(vec[2] != 0, one / np.where(vec[2] != 0, vec[2], one), one)
            u = fx * inv_proj * vec[0] + u0
            v = fy * inv_proj * vec[1] + v0
            iu = round_to_int(u * 32)
            iv = round_to_int(v * 32)
            map1[y0 + i, :, 0] = (iu >> 5).astype(np.int16)      # plain casts: the low 16 bits
            map1[y0 + i, :, 1] = (iv >> 5).astype(np.int16)
            map2[y0 + i] = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map1, map2


def weights(map2):
    """the four integer weights of every fractional position, taps (0,0) (1,0) (0,1) (1,1)"""
    fx = (map2.astype(np.int64) & 31)
    fy = (map2.astype(np.int64) >> 5)
    return [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]


def remap(src, map1, map2):
    """remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) of an (h, w) uint8 image; also returns the count of taps
    that fell outside the source"""
    src = np.asarray(src, np.uint8)
    h, w = src.shape
    sx = map1[..., 0].astype(np.int64)
    sy = map1[..., 1].astype(np.int64)
    acc = np.zeros(sx.shape, np.int64)
    outside = 0
    for wt, (dx, dy) in zip(weights(map2), [(0, 0), (1, 0), (0, 1), (1, 1)]):
        x, y = sx + dx, sy + dy
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        outside += int((~inside).sum())
        p = np.where(inside, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64), 0)
        acc += wt * p
    return ((acc + 16384) >> 15).astype(np.uint8), outside


def undistort(src, K, dist):
    m1, m2 = undistort_map(K, dist, src.shape[1], src.shape[0])
    return remap(src, m1, m2)[0]
