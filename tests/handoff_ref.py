"""Independent numpy restatement of the CV_32F frame hand-off of MultiCameraFrame::setData (MultiCameraFrame.cpp:108-116):
multiply(img, 255) -> convertTo(CV_8U) -> cvtColor(BGR2GRAY), and the value set its tests feed it.  Plain numpy, not the oracle
library: numpy's float32 multiply is one correctly rounded IEEE operation and np.rint rounds half to even.

Out-of-range rule: a product that is NaN, +-Inf or outside [-2^31, 2^31) gives 0 -- x86 OpenCV converts through cvtss2si /
cvtps2dq, whose "integer indefinite" 0x80000000 the saturating packs then clamp to 0.  Recalled, not executed
(docs/design/02_oracle.md)."""
import numpy as np

TWO31 = np.float32(2.0 ** 31)


def stage_f32(img):
    """(h, w) or (h, w, 3) float32 -> (h, w) uint8"""
    img = np.asarray(img)
    assert img.dtype == np.float32 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3))
    with np.errstate(all="ignore"):
        p = img * np.float32(255)
        ok = np.isfinite(p) & (p >= -TWO31) & (p < TWO31)
    r = np.rint(np.where(ok, p, np.float32(0))).astype(np.int64)   # exact: |p| < 2^31 is an integer-valued float32 after rint
    v = np.clip(r, 0, 255)
    if img.ndim == 3:
        v = (v[..., 0] * 1868 + v[..., 1] * 9617 + v[..., 2] * 4899 + 8192) >> 14
    return v.astype(np.uint8)


def _step(f, n):
    """f moved by n float32 ulps (n may be negative)"""
    to = np.float32(np.inf if n > 0 else -np.inf)
    for _ in range(abs(n)):
        f = np.nextafter(f, to)
    return f


def tie_inputs():
    """255 float32 values, the k-th of which times float32(255) is exactly k + 0.5 in float32 arithmetic"""
    out = np.zeros(255, np.float32)
    for k in range(255):
        want = np.float32(k + 0.5)
        c = np.float32((k + 0.5) / 255.0)
        hit = [f for f in (_step(c, n) for n in (0, -1, 1, -2, 2, -3, 3, -4, 4)) if f * np.float32(255) == want]
        assert hit, "no float32 within 4 ulp of (%d + 0.5) / 255 whose product with 255 is the tie" % k
        out[k] = hit[0]
    r = np.rint(out * np.float32(255)).astype(np.int64)
    assert np.array_equal(r, np.arange(255) + (np.arange(255) & 1))   # even k stays, odd k goes up: both parities occur
    return out


def value_set():
    """every value class of the hand-off, once each, as one float32 vector"""
    ties = tie_inputs()
    below = np.nextafter(ties, np.float32(-np.inf))
    above = np.nextafter(ties, np.float32(np.inf))
    special = np.array([-0.0, 1e-40, -0.3, 1.0000001, 1.7, -1e-3,
                        8.4e6, 8.5e6, 1e10, -1e10, np.inf, -np.inf, np.nan], np.float32)
    with np.errstate(all="ignore"):
        p = special * np.float32(255)
    assert 0 < special[1] < np.finfo(np.float32).tiny and special[3] > 1            # a denormal; 1.0000001 is not 1
    assert p[6] < TWO31 <= p[7] and np.isfinite(p[8]) and p[9] < -TWO31             # 8.4e6 just inside, 8.5e6 just outside
    u8 = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.concatenate([u8, ties, below, above, special]).astype(np.float32)


def value_image(w, h, channels=1):
    """the value set tiled over an (h, w[, 3]) float32 image so that every value lands in every column position mod 4 and in
    every channel: the quads of 4 columns are numbered row by row, and element (x, c) of quad q holds value q + x % 4 + 345 c
    (mod the set's length) -- the set passes through each column position as q runs through the image"""
    vals = value_set()
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(channels), indexing="ij")
    idx = (y * ((w + 3) // 4) + x // 4 + (x & 3) + 345 * c) % len(vals)
    seen = np.zeros((len(vals), 4, channels), bool)
    seen[idx, x & 3, c] = True
    assert seen.all(), "%dx%dx%d: a value misses a column position mod 4 or a channel" % (w, h, channels)
    img = vals[idx]
    return img[..., 0] if channels == 1 else img
