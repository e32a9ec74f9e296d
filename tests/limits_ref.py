"""Reference helpers of the limit tests (test_limits_cpu.py, test_gpu_limits.py): descriptors at exact Hamming
distances, BruteForceMatch's accept test restated in float32, and computeOrbDescriptor (ORBextractor.cpp:105-145)
restated in numpy with the cos / sin source as a parameter.  No GPU, no oracle: plain numpy."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATTERN_INC = os.path.join(os.path.dirname(HERE), "mc-slam_amd", "csrc", "brief_pattern_31.inc")


# (dist_thresh, ratio): BruteForceMatch (MultiCameraFrame.cpp:1061), findInterMatches (FrontEnd.cpp:3344-3500), a zero
# threshold, no threshold with ratio 1, and a ratio whose float32 value is far from its decimal
ACCEPT_SETTINGS = [(75.0, 0.85), (50.0, 0.7), (0.0, 0.85), (256.0, 1.0), (75.0, 0.6)]


# --------------------------------------------------------------------------------------------
# descriptors at exact distances
# --------------------------------------------------------------------------------------------
def bits_desc(bits):
    """rows of 256 0/1 values (bit i = byte i // 8, bit i % 8) -> (n, 32) uint8 descriptors"""
    return np.packbits(np.asarray(bits, np.uint8).reshape(-1, 256), axis=1, bitorder="little")


def popcount_dist(q, t):
    """exact Hamming distance matrix (nq, nt) by unpacking the bits"""
    qb = np.unpackbits(np.asarray(q, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    tb = np.unpackbits(np.asarray(t, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    return qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2 * qb @ tb.T


def accept_case(D, swap=False):
    """The (d0, d1) = (a, a + D) table of one train distance D (0 <= D <= 256):
    trains t0 = 0 and t1 = the first D bits set (swapped: t1, t0, so the best index is 1);
    query a (a = 0 .. 256 - D) = the last a bits set, i.e. a bits outside the first D.
    -> (queries (257 - D, 32), trains (2, 32))"""
    n = 257 - D
    qb = np.zeros((n, 256), np.uint8)
    for a in range(n):
        qb[a, 256 - a:] = 1
    tb = np.zeros((2, 256), np.uint8)
    tb[1, :D] = 1
    if swap:
        tb = tb[::-1]
    return bits_desc(qb), bits_desc(tb)


def accept_restated(d0, d1, dist_thresh, ratio):
    """m0.distance < ratio * m1.distance && !(m0.distance > dist_thresh) (MultiCameraFrame.cpp:1061-1063) in float32,
    one rounded product, no contraction: what the reference computes with DMatch::distance (float)"""
    f0, f1 = np.asarray(d0, np.float32), np.asarray(d1, np.float32)
    return (f0 < np.float32(ratio) * f1) & ~(f0 > np.float32(dist_thresh))


def knn2_restated(q, t):
    """knnMatch(k = 2) from the exact distance matrix: stable order, so the lower train index wins ties"""
    d = popcount_dist(q, t)
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), -1, np.int32)
    if nt:
        o = np.argsort(d, axis=1, kind="stable")[:, :2]
        k = o.shape[1]
        idx[:, :k] = o
        dist[:, :k] = np.take_along_axis(d, o, axis=1)
    return idx, dist


def match_restated(q, t, dist_thresh, ratio):
    """BruteForceMatch's accepted (query, train) pairs from the restated k-NN table"""
    idx, dist = knn2_restated(q, t)
    ok = (idx[:, 1] >= 0) & accept_restated(dist[:, 0], dist[:, 1], dist_thresh, ratio)
    qi = np.nonzero(ok)[0]
    return qi.astype(np.uint32), idx[qi, 0].astype(np.uint32)


def first_diff(a, b):
    """index of the first differing row of two arrays (None: equal)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return "shape %s != %s" % (a.shape, b.shape)
    if a.size == 0:
        return None
    bad = np.nonzero(np.any((a != b).reshape(len(a), -1), axis=1))[0]
    return None if len(bad) == 0 else int(bad[0])


# --------------------------------------------------------------------------------------------
# rotated BRIEF
# --------------------------------------------------------------------------------------------
# synth_rig_frame(frame, 4, cam, 1280, 720) images whose 8000 rotated keypoints include descriptor bits that depend on the
# tap arithmetic's last bit (fragile_bits > 0; frames 58 and 99 among them where an fma in cvRound(x*a - y*b) flips a bit).
# A few in a million keypoints have one, so these were found by scanning frames 40-103 on the oracle.
FRAGILE_IMAGES = [(43, 0), (53, 1), (58, 2), (69, 2), (86, 3), (94, 0), (99, 0), (99, 3)]
FRAGILE_SHAPE = (1280, 720, 8000)

def brief_pattern():
    """the 256 test pairs of brief_pattern_31.inc as (512, 2) int8 (x, y) points: pair i = rows 2i, 2i + 1"""
    with open(PATTERN_INC) as f:
        text = f.read()
    body = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith(("/*", "*")))
    vals = [int(v) for v in body.replace("\n", ",").split(",") if v.strip()]
    assert len(vals) == 1024, len(vals)
    return np.array(vals, np.int8).reshape(512, 2)


FACTOR_PI = np.float32(np.pi / 180.0)   # (float)(M_PI / 180.f)


def _rad(angles):
    return np.asarray(angles, np.float32) * FACTOR_PI


_libm = None


def trig_glibc(angles):
    """cosf / sinf of glibc (the oracle's and the reference's libm) on angle * factorPI"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL("libm.so.6")
        for fn in ("cosf", "sinf"):
            getattr(_libm, fn).restype = ctypes.c_float
            getattr(_libm, fn).argtypes = [ctypes.c_float]
    rad = _rad(angles)
    c = np.array([_libm.cosf(float(r)) for r in rad], np.float32)
    s = np.array([_libm.sinf(float(r)) for r in rad], np.float32)
    return c, s


def trig_double(angles):
    """(float)cos((double)rad), (float)sin((double)rad): what k_describe_oriented computes"""
    rad = _rad(angles).astype(np.float64)
    return np.cos(rad).astype(np.float32), np.sin(rad).astype(np.float32)


def rotated_taps(cos_a, sin_b):
    """per keypoint and pattern point: (dy, dx) = (cvRound(x*b + y*a), cvRound(x*a - y*b)), float32 products and sums,
    round half to even (lrintf, __float2int_rn) -> two (n, 512) int arrays"""
    P = brief_pattern().astype(np.float32)
    x, y = P[None, :, 0], P[None, :, 1]
    a = np.asarray(cos_a, np.float32)[:, None]
    b = np.asarray(sin_b, np.float32)[:, None]
    dy = np.rint((x * b).astype(np.float32) + (y * a).astype(np.float32)).astype(np.int64)
    dx = np.rint((x * a).astype(np.float32) - (y * b).astype(np.float32)).astype(np.int64)
    return dy, dx


def describe_restated(blurred, kx, ky, angles, trig):
    """computeOrbDescriptor on one level: blurred = the level's GaussianBlur output (interior, h x w), kx / ky / angles =
    level-coordinate keypoints (float32), trig = trig_glibc or trig_double -> (n, 32) uint8"""
    blurred = np.asarray(blurred, np.uint8)
    h, w = blurred.shape
    n = len(kx)
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    cx = np.rint(np.asarray(kx, np.float32)).astype(np.int64)
    cy = np.rint(np.asarray(ky, np.float32)).astype(np.int64)
    a, b = trig(angles)
    dy, dx = rotated_taps(a, b)
    yy, xx = cy[:, None] + dy, cx[:, None] + dx
    assert yy.min() >= 0 and yy.max() < h and xx.min() >= 0 and xx.max() < w, "a tap leaves the level"
    v = blurred[yy, xx].astype(np.int32)                       # (n, 512)
    bits = (v[:, 0::2] < v[:, 1::2]).astype(np.uint8)          # (n, 256): test i -> bit i % 8 of byte i // 8
    return np.packbits(bits, axis=1, bitorder="little")


def fragile_bits(blurred, kx, ky, cos_a, sin_b):
    """Descriptor bits that depend on the tap arithmetic's roundings: a tap is fragile when evaluating cvRound(x*a - y*b) /
    cvRound(x*b + y*a) with one product kept exact (a contraction into an fma) or both (a double evaluation) moves the
    rounded offset; the bit counts when the pixel at the moved tap flips the comparison.  -> number of such bits"""
    blurred = np.asarray(blurred, np.uint8)
    if len(kx) == 0:
        return 0
    P = brief_pattern().astype(np.float32)
    x, y = P[None, :, 0], P[None, :, 1]
    a = np.asarray(cos_a, np.float32)[:, None]
    b = np.asarray(sin_b, np.float32)[:, None]
    dy, dx = rotated_taps(cos_a, sin_b)
    X, Y, A, B = (v.astype(np.float64) for v in (x, y, a, b))
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)
    xa, yb, xb, ya = f32(X * A), f32(Y * B), f32(X * B), f32(Y * A)
    alt_dx = [np.rint(f32(X * A - Y * B)), np.rint(f32(X * A - yb)), np.rint(f32(xa - Y * B))]
    alt_dy = [np.rint(f32(X * B + Y * A)), np.rint(f32(X * B + ya)), np.rint(f32(xb + Y * A))]
    cx = np.rint(np.asarray(kx, np.float32)).astype(np.int64)[:, None]
    cy = np.rint(np.asarray(ky, np.float32)).astype(np.int64)[:, None]
    h, w = blurred.shape

    def val(yy, xx):
        return blurred[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int32)

    v = val(cy + dy, cx + dx)
    bit = v[:, 0::2] < v[:, 1::2]
    changed = np.zeros(bit.shape, bool)
    for ady, adx in zip(alt_dy, alt_dx):
        ady, adx = ady.astype(np.int64), adx.astype(np.int64)
        moved = (ady != dy) | (adx != dx)
        if not moved.any():
            continue
        u = val(cy + ady, cx + adx)
        u = np.where(moved, u, v)
        changed |= (u[:, 0::2] < u[:, 1::2]) != bit
    return int(changed.sum())
