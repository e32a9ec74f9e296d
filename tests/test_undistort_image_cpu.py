"""cv::undistort's two halves (mc-slam_amd/csrc/mcorb_undistort_image.h: the fixed-point map built once per camera on the host,
and the resampling k_remap_u8 runs) on the host: mcorb_host_undistort_map / mcorb_host_remap_u8 bit-equal to the independent
numpy restatement tests/undistort_image_ref.py at every size and coefficient model; answers that need no restatement (identity
map, constant images, the weights, a 4x4 example computed by hand); the argument checks; and the header alone under plain g++."""
import ctypes as C
import os
import subprocess
import zlib
from importlib import import_module

import numpy as np
import pytest

import undistort_image_ref as R

pkg = import_module("mc-slam_amd")
_lib = pkg._lib
L = _lib.load()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mc-slam_amd", "csrc")

# the last four: widths with w % 4 in {1, 2, 3}, where the row of quads k_remap_u8 and a vectorised host loop walk ends in a
# scalar tail (323: wider than one 256-lane block, w % 64 != 0)
SIZES = [(160, 120), (640, 480), (752, 480), (1280, 720), (1920, 1080), (161, 120), (162, 121), (163, 123), (323, 243)]
# cv::undistort's min(max(1, 4096 / cols), rows), worked out by hand: 4096 = 25 * 163 + 21 = 12 * 323 + 220
STRIPES = {160: 25, 640: 6, 752: 5, 1280: 3, 1920: 2, 161: 25, 162: 25, 163: 25, 323: 12}

# (name, coefficients): 4 / 5 / 8 / 12 coefficients; the strong ones push corners out of the source (pincushion) or fold the
# far field back over the centre (barrel)
MODELS = [
    ("radtan4_barrel", [-0.2873, 0.0912, 0.00031, -0.00047]),
    ("radtan4_pincushion_strong", [0.4841, 0.1422, -0.00112, 0.00083]),
    ("radtan5_barrel_strong", [-0.9517, 0.0703, 0.00052, 0.00021, -0.0451]),
    ("radtan5_tangential", [-0.0813, 0.0274, 0.0061, -0.0049, 0.0032]),
    ("rational8", [0.5213, -0.1274, 0.00041, -0.00037, 0.0089, 0.8723, -0.0612, 0.0301]),
    ("thinprism12", [-0.2791, 0.0833, 0.00027, -0.00061, -0.0175, 0.0213, -0.0034, 0.0011, 0.0017, -0.0008, -0.0012, 0.0004]),
]


def camera(w, h):
    """a plausible K for a w x h sensor: ~75 degrees across, principal point off centre, fx != fy"""
    return np.array([[0.651 * w + 0.37, 0.0, 0.503 * w - 0.21], [0.0, 0.649 * w - 0.13, 0.497 * h + 0.43], [0.0, 0.0, 1.0]])


def image(seed, w, h):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx * 3 + yy * 5 + rng.integers(0, 96, (h, w))) & 255).astype(np.uint8)


def host_map(K, dist, w, h):
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    d = np.ascontiguousarray(dist, np.float64).ravel()
    m1 = np.zeros((h, w, 2), np.int16)
    m2 = np.zeros((h, w), np.uint16)
    st = L.mcorb_host_undistort_map(K.ctypes.data, d.ctypes.data, d.size, w, h, m1.ctypes.data, m2.ctypes.data)
    return st, m1, m2


def host_remap(src, m1, m2):
    h, w = src.shape
    src = np.ascontiguousarray(src)
    m1 = np.ascontiguousarray(m1, np.int16)
    m2 = np.ascontiguousarray(m2, np.uint16)
    dst = np.full((h, w), 0xAB, np.uint8)
    st = L.mcorb_host_remap_u8(src.ctypes.data, w, w, h, m1.ctypes.data, m2.ctypes.data, dst.ctypes.data, w)
    return st, dst


SEEN = {"outside": {}, "fractions": {}}


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name,dist", MODELS, ids=[m[0] for m in MODELS])
def test_map_and_remap_bit_equal_to_numpy_restatement(name, dist, w, h):
    assert R.stripe_height(w, h) == STRIPES[w]
    K = camera(w, h)
    st, m1, m2 = host_map(K, dist, w, h)
    assert st == 0
    with np.errstate(all="ignore"):
        r1, r2 = R.undistort_map(K, dist, w, h)
    bad = np.argwhere((m1 != r1).any(axis=2) | (m2 != r2))
    assert bad.size == 0, "%d of %d map entries differ, first at row %d col %d: %r %r vs %r %r" % (
        len(bad), w * h, bad[0][0], bad[0][1], m1[tuple(bad[0])], m2[tuple(bad[0])], r1[tuple(bad[0])], r2[tuple(bad[0])])
    assert not np.array_equal(m1[..., 0], np.broadcast_to(np.arange(w, dtype=np.int16), (h, w)))   # the model did move the pixels
    src = image(zlib.crc32(("%s%d" % (name, w)).encode()), w, h)
    st, dst = host_remap(src, m1, m2)
    assert st == 0
    ref, outside = R.remap(src, r1, r2)
    assert np.array_equal(dst, ref), "%d pixels differ" % int((dst != ref).sum())
    SEEN["outside"][(name, w)] = outside
    SEEN["fractions"][(name, w)] = len(np.unique(m2))
    assert int(m2.max()) < 1024


def test_cases_cover_out_of_source_taps_and_every_fractional_position():
    """(reads what the parametrised test above recorded: run the file as a whole)"""
    assert len(SEEN["outside"]) == len(SIZES) * len(MODELS), "run after test_map_and_remap_bit_equal_to_numpy_restatement"
    assert any(v > 0 for v in SEEN["outside"].values()), SEEN["outside"]
    assert any(v > 0 for (n, _), v in SEEN["outside"].items() if "pincushion" in n)
    assert any(v == 1024 for v in SEEN["fractions"].values()), SEEN["fractions"]


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("ncoef", [4, 5, 8, 12])
def test_zero_distortion_is_the_identity_map(w, h, ncoef):
    """all-zero coefficients: the accumulated error of the row sums is ~1e-12 px against a quantum of 1/32, so map1 is (j, i) and
    map2 is 0 everywhere, and the remap of any image is the image"""
    st, m1, m2 = host_map(camera(w, h), np.zeros(ncoef), w, h)
    assert st == 0
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(m1[..., 0], xx) and np.array_equal(m1[..., 1], yy) and not m2.any()
    src = image(w + ncoef, w, h)
    st, dst = host_remap(src, m1, m2)
    assert st == 0 and np.array_equal(dst, src)


@pytest.mark.parametrize("v", [0, 1, 127, 128, 254, 255])
def test_constant_image_stays_constant_where_all_taps_are_inside(v):
    w, h = 640, 480
    st, m1, m2 = host_map(camera(w, h), MODELS[1][1], w, h)
    assert st == 0
    st, dst = host_remap(np.full((h, w), v, np.uint8), m1, m2)
    assert st == 0
    sx, sy = m1[..., 0].astype(int), m1[..., 1].astype(int)
    inside = (sx >= 0) & (sx + 1 < w) & (sy >= 0) & (sy + 1 < h)
    assert inside.any() and not inside.all()
    assert np.all(dst[inside] == v)
    allout = (sx + 1 < 0) | (sx >= w) | (sy + 1 < 0) | (sy >= h)
    assert np.all(dst[allout] == 0) and np.all(dst <= v)


def test_weights_of_all_1024_positions_sum_to_32768():
    """through the library: a source with a single 255 at one tap returns that tap's weight for every fractional position,
    (w * 255 + 16384) >> 15; the four weights sum to 32768 everywhere; a 2x2 block of 255s comes back 255 everywhere"""
    m2 = np.arange(1024, dtype=np.uint16).reshape(32, 32)
    m1 = np.zeros((32, 32, 2), np.int16)
    for tap, wt in enumerate(R.weights(m2)):
        src = np.zeros((32, 32), np.uint8)
        src[tap >> 1, tap & 1] = 255
        st, dst = host_remap(src, m1, m2)
        assert st == 0 and np.array_equal(dst.astype(np.int64), (wt * 255 + 16384) >> 15)
    assert np.array_equal(sum(R.weights(m2)), np.full((32, 32), 32768))
    assert R.weights(np.zeros(1, np.uint16))[0][0] == 32768   # position (0, 0) weighs its pixel fully: more than a short holds
    src = np.zeros((32, 32), np.uint8)
    src[:2, :2] = 255
    st, dst = host_remap(src, m1, m2)
    assert st == 0 and np.all(dst == 255)


def test_hand_computed_4x4_example():
    """p[y][x] = 10 * (4 y + x).
    (0,0) <- source (1, 1) + (8, 16)/32: weights 12288, 4096, 12288, 4096 on 50, 60, 90, 100
             = 2375680; + 16384 = 2392064 = 73 * 32768 -> 73 (72.5 rounds up).
    (1,0) <- source (3, 0) + (16, 0)/32, on the right edge: weights 16384, 16384, 0, 0 on 30 and the border's 0
             = 491520; + 16384 = 507904 = 15.5 * 32768 -> 15.
    (2,0) <- source (-1, 3) + (24, 8)/32, the bottom left corner: only tap (0, 3) = 120 is inside, weight 24 * 24 * 32 = 18432
             = 2211840; + 16384 = 2228224 = 68 * 32768 -> 68.
    (3,0) <- source (-5, 7): fully outside -> 0.     (0,1) <- source (2, 2) exactly -> 100.
    Everything else <- source (0, 0) exactly -> 0, (3, 3) exactly -> 150 in the last row."""
    p = (10 * np.arange(16)).reshape(4, 4).astype(np.uint8)
    m1 = np.zeros((4, 4, 2), np.int16)
    m2 = np.zeros((4, 4), np.uint16)
    m1[0, 0], m2[0, 0] = (1, 1), 16 * 32 + 8
    m1[0, 1], m2[0, 1] = (3, 0), 16
    m1[0, 2], m2[0, 2] = (-1, 3), 8 * 32 + 24
    m1[0, 3], m2[0, 3] = (-5, 7), 5 * 32 + 9
    m1[1, 0] = (2, 2)
    m1[3, :] = (3, 3)
    st, dst = host_remap(p, m1, m2)
    assert st == 0
    expect = np.zeros((4, 4), np.uint8)
    expect[0] = [73, 15, 68, 0]
    expect[1, 0] = 100
    expect[3, :] = 150
    assert np.array_equal(dst, expect), dst
    assert np.array_equal(R.remap(p, m1, m2)[0], expect)


def test_values_past_a_short_and_past_an_int_cast_like_opencv():
    """k1 = 1e3 throws the far field tens of thousands of pixels out: (short)(iu >> 5) keeps the low 16 bits.  k1 = 1e300 throws it
    past what an int holds: saturate_cast<int> gives 0x80000000 there, whose (short)(iu >> 5) and iu & 31 are 0"""
    w, h = 160, 120
    K = camera(w, h)
    for k1 in (1e3, 1e300):
        dist = [k1, 0.0, 0.0, 0.0]
        st, m1, m2 = host_map(K, dist, w, h)
        with np.errstate(all="ignore"):
            r1, r2 = R.undistort_map(K, dist, w, h)
        assert st == 0 and np.array_equal(m1, r1) and np.array_equal(m2, r2)
        if k1 == 1e3:   # the wrap shows: along the top row the source column is not monotonic
            assert np.any(np.diff(m1[0, :, 0].astype(int)) < 0)
        else:
            far = np.hypot(*np.mgrid[0:h, 0:w][::-1] - np.array([K[0, 2], K[1, 2]])[:, None, None]) > 8
            assert not m1[far].any() and not m2[far].any()
        src = image(9, w, h)
        assert np.array_equal(host_remap(src, m1, m2)[1], R.remap(src, r1, r2)[0])


def test_argument_checks():
    w, h = 16, 8
    K = camera(w, h)
    E_ARG = _lib.E_ARG
    for n in (1, 3, 6, 7, 9, 13, 14):   # 14 is the tilt model
        assert host_map(K, np.full(n, 0.01), w, h)[0] == E_ARG
    for n in (0, 1, 3, 6, 7, 9, 13, 14):
        with pytest.raises(ValueError):
            R.coeffs([0.01] * n)
    d = np.zeros(1)
    m1 = np.zeros((h, w, 2), np.int16)
    m2 = np.zeros((h, w), np.uint16)
    Kc = np.ascontiguousarray(K).reshape(9)
    assert L.mcorb_host_undistort_map(Kc.ctypes.data, d.ctypes.data, 0, w, h, m1.ctypes.data, m2.ctypes.data) == E_ARG
    for bad in (np.nan, np.inf, -np.inf):
        Kb = K.copy()
        Kb[0, 2] = bad
        assert host_map(Kb, [0.1, 0, 0, 0], w, h)[0] == E_ARG
        assert host_map(K, [0.1, bad, 0, 0], w, h)[0] == E_ARG
    for i in (0, 1):
        Kb = K.copy()
        Kb[i, i] = 0.0
        assert host_map(Kb, [0.1, 0, 0, 0], w, h)[0] == E_ARG
    d4 = np.zeros(4)
    assert L.mcorb_host_undistort_map(None, d4.ctypes.data, 4, w, h, m1.ctypes.data, m2.ctypes.data) == E_ARG
    assert L.mcorb_host_undistort_map(Kc.ctypes.data, None, 4, w, h, m1.ctypes.data, m2.ctypes.data) == E_ARG
    assert L.mcorb_host_undistort_map(Kc.ctypes.data, d4.ctypes.data, 4, w, h, None, m2.ctypes.data) == E_ARG
    assert L.mcorb_host_undistort_map(Kc.ctypes.data, d4.ctypes.data, 4, 0, h, m1.ctypes.data, m2.ctypes.data) == E_ARG
    assert L.mcorb_host_undistort_map(Kc.ctypes.data, d4.ctypes.data, 4, w, -1, m1.ctypes.data, m2.ctypes.data) == E_ARG
    assert L.mcorb_host_undistort_map(Kc.ctypes.data, d4.ctypes.data, 4, w, h, m1.ctypes.data, m2.ctypes.data) == 0
    src = np.zeros((h, w), np.uint8)
    dst = np.zeros((h, w), np.uint8)
    assert L.mcorb_host_remap_u8(None, w, w, h, m1.ctypes.data, m2.ctypes.data, dst.ctypes.data, w) == E_ARG
    assert L.mcorb_host_remap_u8(src.ctypes.data, w - 1, w, h, m1.ctypes.data, m2.ctypes.data, dst.ctypes.data, w) == E_ARG
    assert L.mcorb_host_remap_u8(src.ctypes.data, w, w, h, m1.ctypes.data, m2.ctypes.data, dst.ctypes.data, w - 1) == E_ARG
    assert L.mcorb_host_remap_u8(src.ctypes.data, w, 0, h, m1.ctypes.data, m2.ctypes.data, dst.ctypes.data, w) == E_ARG
    assert L.mcorb_host_remap_u8(src.ctypes.data, w, w, h, None, m2.ctypes.data, dst.ctypes.data, w) == E_ARG
    assert L.mcorb_host_remap_u8(src.ctypes.data, w, w, h, m1.ctypes.data, m2.ctypes.data, dst.ctypes.data, w) == 0


def test_strided_remap(w=160, h=120, src_pad=24, dst_pad=8):
    st, m1, m2 = host_map(camera(w, h), MODELS[0][1], w, h)
    src = image(3, w + src_pad, h)
    dst = np.full((h, w + dst_pad), 0xCD, np.uint8)
    assert L.mcorb_host_remap_u8(src.ctypes.data, w + src_pad, w, h, m1.ctypes.data, m2.ctypes.data, dst.ctypes.data, w + dst_pad) == 0
    assert np.array_equal(dst[:, :w], R.remap(np.ascontiguousarray(src[:, :w]), m1, m2)[0]) and np.all(dst[:, w:] == 0xCD)


@pytest.mark.parametrize("w,h", [(161, 120), (162, 121), (163, 123)])
def test_strided_remap_at_unaligned_widths(w, h):
    """odd paddings too: no row of either plane starts on a multiple of 4"""
    test_strided_remap(w, h, 13, 5)


# -- the header alone, plain g++ ------------------------------------------------------------------------------------------------
def build_exe(out, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_undistort_image.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(str(tmp_path_factory.mktemp("undist_image") / "test_undistort_image"))


def run_exe(exe, tmp, K, dist, src):
    h, w = src.shape
    d = np.zeros(12, np.float64)
    d[:len(dist)] = dist
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(K, "<f8").tobytes() + np.int32(len(dist)).tobytes() + d.astype("<f8").tobytes()
                + np.int32(w).tobytes() + np.int32(h).tobytes() + np.ascontiguousarray(src).tobytes())
    subprocess.check_call([exe, fin, fout], timeout=300)
    raw = np.fromfile(fout, np.uint8)
    st = int(raw[:4].view("<i4")[0])
    n = w * h
    m1 = raw[4:4 + 4 * n].view("<i2").reshape(h, w, 2)
    m2 = raw[4 + 4 * n:4 + 6 * n].view("<u2").reshape(h, w)
    return st, m1, m2, raw[4 + 6 * n:].reshape(h, w)


def test_header_self_check(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("name,dist", MODELS, ids=[m[0] for m in MODELS])
def test_header_under_plain_gxx_equals_restatement_and_library(exe, tmp_path, name, dist):
    w, h = 752, 480
    K = camera(w, h)
    src = image(17, w, h)
    st, m1, m2, dst = run_exe(exe, str(tmp_path), K, dist, src)
    assert st == 0
    with np.errstate(all="ignore"):
        r1, r2 = R.undistort_map(K, dist, w, h)
    assert np.array_equal(m1, r1) and np.array_equal(m2, r2) and np.array_equal(dst, R.remap(src, r1, r2)[0])
    st, l1, l2 = host_map(K, dist, w, h)
    assert st == 0 and np.array_equal(m1, l1) and np.array_equal(m2, l2)


@pytest.mark.parametrize("w,h", [(161, 120), (163, 123)])
def test_header_under_plain_gxx_at_widths_with_a_scalar_tail(exe, tmp_path, w, h):
    name, dist = MODELS[1]   # the strong pincushion: taps outside the plane
    K = camera(w, h)
    src = image(23, w, h)
    st, m1, m2, dst = run_exe(exe, str(tmp_path), K, dist, src)
    assert st == 0
    with np.errstate(all="ignore"):
        r1, r2 = R.undistort_map(K, dist, w, h)
    ref, outside = R.remap(src, r1, r2)
    assert outside > 0 and np.array_equal(m1, r1) and np.array_equal(m2, r2) and np.array_equal(dst, ref)
    st, l1, l2 = host_map(K, dist, w, h)
    assert st == 0 and np.array_equal(m1, l1) and np.array_equal(m2, l2)


def test_header_refuses_counts(exe, tmp_path):
    for n in (0, 3, 6, 9):
        st, _, _, _ = run_exe(exe, str(tmp_path), camera(8, 8), [0.1] * n, np.zeros((8, 8), np.uint8))
        assert st == -1


def test_opencv_crosscheck_of_undistort_is_well_formed():
    """tools/crosscheck/crosscheck_undistort.cpp (the program that would pin this restatement against a real cv::undistort) must
    at least be well-formed C++: -fsyntax-only against tests/cpp/cvmock (declarations, no behaviour).  Pins nothing, says so."""
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "cpp", "cvmock"),
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tools", "crosscheck", "crosscheck_undistort.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "PINS NOTHING UNTIL SOMEONE RUNS IT" in open(cmd[-1]).read()
