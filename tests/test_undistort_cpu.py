"""UndistortKeyPoints' arithmetic (mc-slam_amd/csrc/mcorb_undistort.h, the code k_undistort runs) on the host: bit-equal to the
independent numpy restatement tests/undistort_ref.py on 10^6 seeded points per distortion model, the icdist < 0 branch and the
reference's zero test; and, with no code in common, a round trip through the forward distortion model."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import undistort_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mc-slam_amd", "csrc")
NPTS = 1_000_000

K_HD = np.array([[1150.3, 0.0, 962.7], [0.0, 1148.9, 541.2], [0.0, 0.0, 1.0]])

# (name, coefficients): 4 / 5 / 8 / 12 coefficients, barrel and pincushion, tangential, rational, thin prism
MODELS = [
    ("radtan4_barrel", [-0.2873, 0.0912, 0.00031, -0.00047]),
    ("radtan4_pincushion", [0.1841, -0.0422, -0.00112, 0.00083]),
    ("radtan5_barrel", [-0.3517, 0.1703, 0.00052, 0.00021, -0.0451]),
    ("radtan5_tangential", [-0.0813, 0.0274, 0.0061, -0.0049, 0.0032]),
    ("rational8", [0.5213, -0.1274, 0.00041, -0.00037, 0.0089, 0.8723, -0.0612, 0.0301]),
    ("thinprism12", [-0.2791, 0.0833, 0.00027, -0.00061, -0.0175, 0.0213, -0.0034, 0.0011, 0.0017, -0.0008, -0.0012, 0.0004]),
]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("undist") / "test_undistort")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_undistort.cpp"), "-o", out])
    return out


def run_host(exe, tmp, K, dist, u, v):
    """returns (status, mode, x, y) of the header's code"""
    d = np.zeros(12, np.float64)
    d[:len(dist)] = dist
    pts = np.empty(2 * len(u), np.float32)
    pts[0::2], pts[1::2] = u, v
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray(K, "<f8").tobytes() + np.int32(len(dist)).tobytes() + d.astype("<f8").tobytes()
                + np.int64(len(u)).tobytes() + pts.tobytes())
    subprocess.check_call([exe, fin, fout], timeout=300)
    raw = np.fromfile(fout, np.uint8)
    st, mode = raw[:8].view("<i4")
    out = raw[8:].view("<f4")
    return int(st), int(mode), out[0::2], out[1::2]


def points(seed, n, W=1920, H=1080):
    """points across and beyond a W x H frame: the frame itself, a margin of half a frame, and exact pixel centres"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.5 * W, 1.5 * W, n).astype(np.float32)
    v = rng.uniform(-0.5 * H, 1.5 * H, n).astype(np.float32)
    q = n // 4
    u[:q] = rng.integers(0, W, q).astype(np.float32)
    v[:q] = rng.integers(0, H, q).astype(np.float32)
    u[q:2 * q] = (rng.integers(0, W, q) * np.float32(1.2) ** rng.integers(1, 8, q)).astype(np.float32)   # scaled pyramid coordinates
    return u, v


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("name,dist", MODELS, ids=[m[0] for m in MODELS])
def test_bit_equal_to_numpy_restatement(exe, tmp_path, name, dist):
    u, v = points(zlib.crc32(name.encode()), NPTS)
    st, mode, x, y = run_host(exe, str(tmp_path), K_HD, dist, u, v)
    assert st == 0 and mode == 1
    with np.errstate(all="ignore"):
        rx, ry = U.undistort(u, v, K_HD, dist)
    bad = np.flatnonzero((x.view(np.uint32) != rx.view(np.uint32)) | (y.view(np.uint32) != ry.view(np.uint32)))
    assert bad.size == 0, "%d of %d points differ, first at (%r, %r): %r vs %r" % (bad.size, NPTS, u[bad[0]], v[bad[0]],
                                                                                 (x[bad[0]], y[bad[0]]), (rx[bad[0]], ry[bad[0]]))
    assert not np.array_equal(x, u)   # the model did move the points


def test_negative_icdist_branch(exe, tmp_path):
    """points far outside the frame under strong barrel distortion make the denominator of icdist negative: OpenCV resets to the
    plain normalised point (regression_14583), i.e. ((u - cx) * ifx) * fx + cx"""
    dist = [-0.6, -0.01, 0.0, 0.0]
    K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
    u = np.array([4000.0, -3000.0, 320.0, 5200.5, 2500.25], np.float32)
    v = np.array([240.0, 3100.0, -4000.0, 2200.0, 2600.0], np.float32)
    st, mode, x, y = run_host(exe, str(tmp_path), K, dist, u, v)
    assert st == 0 and mode == 1
    Kf = K.astype(np.float32).astype(np.float64)
    ex = ((u.astype(np.float64) - Kf[0, 2]) * (1.0 / Kf[0, 0]) * Kf[0, 0] + Kf[0, 2]).astype(np.float32)
    ey = ((v.astype(np.float64) - Kf[1, 2]) * (1.0 / Kf[1, 1]) * Kf[1, 1] + Kf[1, 2]).astype(np.float32)
    # every point takes the branch on the first iteration: r2 of the normalised point already has 1 + k1 r2 + k2 r4 < 0
    xn = (u.astype(np.float64) - 320) / 500
    yn = (v.astype(np.float64) - 240) / 500
    r2 = xn * xn + yn * yn
    assert np.all(1 + (-0.01 * r2 - 0.6) * r2 < 0)
    assert same_bits(x, ex) and same_bits(y, ey)
    with np.errstate(all="ignore"):
        rx, ry = U.undistort(u, v, K, dist)
    assert same_bits(x, rx) and same_bits(y, ry)


@pytest.mark.parametrize("k1,active", [(0.0, False), (-0.0, False), (-0.25, False), (0.5, False), (-0.25 + 2.0 ** -40, True),
                                       (-0.2873, True), (1e-300, True)])
def test_zero_test_quirk(exe, tmp_path, k1, active):
    """the reference's dist_coeffs_[cam].at<float>(0) == 0.0 on a CV_64F Mat reads the low 32 bits of k1: pass-through for k1 = 0,
    and for short binary values like -0.25, whatever k2 says"""
    dist = [k1, 0.091, 0.0003, -0.0004]
    u, v = points(5, 1000)
    st, mode, x, y = run_host(exe, str(tmp_path), K_HD, dist, u, v)
    assert st == 0 and mode == (1 if active else 0)
    assert U.zero_test(k1) == (not active)
    if not active:
        assert same_bits(x, u) and same_bits(y, v)
    with np.errstate(all="ignore"):
        rx, ry = U.undistort(u, v, K_HD, dist)
    assert same_bits(x, rx) and same_bits(y, ry)


def test_zero_k1_with_nonzero_k2_passes_through(exe, tmp_path):
    u, v = points(6, 1000)
    st, mode, x, y = run_host(exe, str(tmp_path), K_HD, [0.0, 0.2, 0.01, 0.01, 0.3], u, v)
    assert st == 0 and mode == 0 and same_bits(x, u) and same_bits(y, v)


@pytest.mark.parametrize("n", [0, 1, 3, 6, 7, 9, 13, 14])
def test_coefficient_counts_refused(exe, tmp_path, n):
    """4, 5, 8 and 12 coefficients only; 14 (the tilt model) is refused like every other count"""
    st, _, _, _ = run_host(exe, str(tmp_path), K_HD, [0.1] * min(n, 12), np.zeros(1, np.float32), np.zeros(1, np.float32)) \
        if n <= 12 else (None, None, None, None)
    if n <= 12:
        assert st == -1
    with pytest.raises(ValueError):
        U.coeffs([0.1] * n)


@pytest.mark.parametrize("name,dist", MODELS, ids=[m[0] for m in MODELS])
def test_round_trip_through_forward_model(exe, tmp_path, name, dist):
    """no code in common with either restatement: distorting the undistorted point with the forward model returns the input.
    Moderate distortion (the models above at a quarter of their strength) inside the frame, where OpenCV's 5 fixed-point
    iterations converge: within 0.1 px everywhere (the rational model's worst corner is 0.08 px), within 1e-4 px at the median."""
    dist = [0.25 * c for c in dist]
    rng = np.random.default_rng(11)
    u = rng.uniform(0, 1920, 200_000).astype(np.float32)
    v = rng.uniform(0, 1080, 200_000).astype(np.float32)
    st, mode, x, y = run_host(exe, str(tmp_path), K_HD, dist, u, v)
    assert st == 0 and mode == 1
    Kf = K_HD.astype(np.float32).astype(np.float64)
    xn = (x.astype(np.float64) - Kf[0, 2]) / Kf[0, 0]
    yn = (y.astype(np.float64) - Kf[1, 2]) / Kf[1, 1]
    xd, yd = U.distort(xn, yn, dist)
    err = np.hypot(xd * Kf[0, 0] + Kf[0, 2] - u, yd * Kf[1, 1] + Kf[1, 2] - v)
    assert err.max() < 0.1 and np.median(err) < 1e-4, np.quantile(err, [0.5, 0.999, 1.0])
    assert np.median(np.hypot(x - u, y - v)) > 1.0   # (and the points did move)
