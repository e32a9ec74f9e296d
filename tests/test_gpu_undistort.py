"""UndistortKeyPoints on the device (k_undistort, inside every extraction job): the rig's image_kps_undist equals the numpy
restatement (tests/undistort_ref.py) applied to the rig's own raw records, bit for bit, on every path a job takes; the consumers'
NULL defaults read that set; set / clear / re-set between jobs; the C ABI's argument and state checks."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import undistort_ref as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


def kmat(W, H, f=0.9):
    return np.array([[f * W, 0.0, W / 2 + 3.3], [0.0, f * W * 1.002, H / 2 - 2.1], [0.0, 0.0, 1.0]])


# per camera: pass-through (k1 = 0), the k1 = -0.25 quirk (passed through too), 5 coefficients, 8 coefficients
DISTS = [
    [0.0, 0.051, 0.0011, -0.0009],
    [-0.25, 0.072, 0.0002, 0.0001],
    [-0.2873, 0.0912, 0.00031, -0.00047, -0.0312],
    [0.4213, -0.1274, 0.00041, -0.00037, 0.0089, 0.7723, -0.0612, 0.0301],
]


def set_all(rig, W, H, dists):
    Ks = [kmat(W, H, 0.85 + 0.03 * c) for c in range(len(dists))]
    for c, d in enumerate(dists):
        rig.set_undistortion(c, Ks[c], d)
    return Ks


def expected(rig, m, K, dist, slot=0):
    return U.undistort_records(rig.features(m, slot=slot)[1], K, dist)


def check_images(rig, nimg, Ks, dists, slot=0):
    C = len(Ks)
    moved = 0
    for m in range(nimg):
        c = m % C
        got = rig.features_undist(m, slot=slot)
        with np.errstate(all="ignore"):
            want = expected(rig, m, Ks[c], dists[c], slot)
        assert len(got) > 0
        assert got.tobytes() == want.tobytes(), "image %d (camera %d, slot %d)" % (m, c, slot)
        moved += int(not np.array_equal(got["x"], rig.features(m, slot=slot)[1]["x"]))
    return moved


def frames(mc, F, C, W, H, f0=0):
    return [mc.synth_rig_frame(f0 + f, C, c, W, H) for f in range(F) for c in range(C)]


@pytest.mark.parametrize("selection,graph", [(2, 0), (2, 1), (1, 0)], ids=["gpu", "gpu-graph", "host"])
def test_one_frame_four_models_bit_exact(mc, selection, graph):
    """4 cameras at 1280x720, one model per camera, one rig frame per job (the small path: host-mapped results); twice per rig so
    a captured graph is replayed"""
    C, W, H = 4, 1280, 720
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=2000, selection=selection)
    rig.set_graph(graph)
    Ks = set_all(rig, W, H, DISTS)
    assert [rig.undistortion_active(c) for c in range(C)] == [False, False, True, True]
    for f in range(2):
        rig.upload(frames(mc, 1, C, W, H, f0=3 + f))
        rig.process(1)
        assert check_images(rig, C, Ks, DISTS) == 2   # the two pass-through cameras keep their points
        assert rig.features_undist(0).tobytes() == rig.features(0)[1].tobytes()
    rig.close()


@pytest.mark.parametrize("W,H", [(752, 480), (1920, 1080)])
def test_other_sizes(mc, W, H):
    C = 2
    dists = [DISTS[2], DISTS[3]]
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=1500)
    Ks = set_all(rig, W, H, dists)
    rig.upload(frames(mc, 1, C, W, H, f0=1))
    rig.process(1)
    assert check_images(rig, C, Ks, dists) == C
    rig.close()


@pytest.mark.parametrize("selection", [2, 1], ids=["gpu", "host"])
def test_batched_multi_frame_multi_slot(mc, selection):
    """8 rig frames per job on 2 slots in flight together (the copy path: device buffer + D2H on the side stream)"""
    C, W, H, F = 4, 1280, 720, 8
    rig = mc.Rig(C, W, H, F, 2, nfeatures=2000, selection=selection)
    Ks = set_all(rig, W, H, DISTS)
    for s in range(2):
        rig.upload(frames(mc, F, C, W, H, f0=10 * s), slot=s)
    for s in range(2):
        rig.process_submit(F, slot=s)
    for s in range(2):
        rig.process_wait(slot=s)
    for s in range(2):
        assert check_images(rig, F * C, Ks, DISTS, slot=s) == F * 2
    rig.close()


@pytest.mark.parametrize("batch", [1, 9])
def test_forced_fallback_to_the_host_stage(mc, monkeypatch, batch):
    """a job whose GPU selection raises its flag (scan cap turned down) is redone by the host stage: the undistorted set follows the
    redone list"""
    from test_gpu_select import _clustered_image
    monkeypatch.setenv("MCORB_SELECT_DEEP_CAP", "8")
    W, H = 800, 600
    rig = mc.Rig(1, W, H, batch, 1, nfeatures=1000, selection=2)
    Ks = set_all(rig, W, H, [DISTS[2]])
    plain = mc.synth_rig_frame(3, 1, 0, W, H)
    rig.upload([_clustered_image(W, H) if m == batch - 1 else plain for m in range(batch)])
    rig.extract(batch)
    assert rig.select_fallbacks() == 1
    assert check_images(rig, batch, Ks * batch, [DISTS[2]] * batch) == batch
    rig.close()


def test_orientation_mode(mc):
    C, W, H = 2, 1280, 720
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=1500, orientation=1)
    dists = [DISTS[3], DISTS[2]]
    Ks = set_all(rig, W, H, dists)
    rig.upload(frames(mc, 1, C, W, H, f0=2))
    rig.process(1)
    assert check_images(rig, C, Ks, dists) == C
    assert np.any(rig.features_undist(0)["angle"] != 0)
    rig.close()


def _processed_rig(mc, C=4, W=1280, H=720, F=1, f0=4, **kw):
    rig = mc.Rig(C, W, H, F, 1, nfeatures=2000, **kw)
    Ks = set_all(rig, W, H, DISTS[:C])
    rig.upload(frames(mc, F, C, W, H, f0=f0))
    rig.process(F)
    und = [rig.features_undist(m) for m in range(F * C)]
    return rig, Ks, und


def _calibration(C):
    K = [kmat(1280, 720, 0.85 + 0.03 * c) for c in range(C)]
    R, t = [], []
    for c in range(C):
        a = 0.05 * c
        R.append(np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]))
        t.append(np.array([0.12 * c, 0.01 * c, 0.0]))
    return K, R, t


def test_bow_tracks_default_to_the_rigs_set(mc):
    """mcorb_rig_match_bow (no y_undist argument) and mcorb_rig_match_bow_frames with NULL read the rig's undistorted rows"""
    C, F = 4, 3
    rig, _, und = _processed_rig(mc, F=F)
    voc = mc.ORBVocabulary().create(**O.make_vocabulary(10, 4, seed=3))
    yu = [np.ascontiguousarray(k["y"], np.float32) for k in und]
    raw = [np.ascontiguousarray(rig.features(m)[1]["y"], np.float32) for m in range(F * C)]
    for f in range(F):
        single = voc.match_rig_frame(rig, f, levelsup=2)
        explicit = voc.match_rig_frames(rig, f, 1, levelsup=2, y_undist=[None] * (f * C) + yu[f * C:(f + 1) * C])[0]
        assert all(np.array_equal(a, b) for a, b in zip(single, explicit)), "frame %d" % f
        assert len(single[0]) > 0
    batched = voc.match_rig_frames(rig, 0, F, levelsup=2)
    explicit = voc.match_rig_frames(rig, 0, F, levelsup=2, y_undist=yu)
    with_raw = voc.match_rig_frames(rig, 0, F, levelsup=2, y_undist=raw)
    for f in range(F):
        assert all(np.array_equal(a, b) for a, b in zip(batched[f], explicit[f])), "frame %d" % f
    assert any(not np.array_equal(batched[f][0], with_raw[f][0]) for f in range(F))   # the gate did see other rows
    rig.close()


def test_epipolar_tracks_and_lf_features_default_to_the_rigs_set(mc):
    C, F = 4, 2
    rig, _, und = _processed_rig(mc, F=F, f0=6)
    K, R, t = _calibration(C)
    Fm = np.stack([mc.fundamental_from_extrinsics(K[i], R[i], t[i], K[j], R[j], t[j]) for i in range(C - 1) for j in range(i + 1, C)])
    for f in range(F):
        a = rig.tracks_epipolar(f, Fm)
        b = rig.tracks_epipolar(f, Fm, kps_undist=und[f * C:(f + 1) * C])
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    tracks = [rig.tracks(f)[0] for f in range(F)]
    for f in range(F):
        got = rig.obtain_lf_features(f, tracks[f], K, R, t)
        want = rig.obtain_lf_features(f, tracks[f], K, R, t, kps_undist=und[f * C:(f + 1) * C])
        assert got[0].tobytes() == want[0].tobytes() and got[1:3] == want[1:3] and got[1] > 0 and got[2] > 0
    got = rig.obtain_lf_features_frames(0, tracks, K, R, t)
    want = rig.obtain_lf_features_frames(0, tracks, K, R, t, kps_undist=und)
    for f in range(F):
        assert got[f][0].tobytes() == want[f][0].tobytes() and got[f][1:3] == want[f][1:3]
    raw = rig.obtain_lf_features(0, tracks[0], K, R, t, kps_undist=[rig.features(c)[1] for c in range(C)])
    assert raw[0].tobytes() != got[0][0].tobytes()   # the default was not the raw set
    rig.close()


def test_python_mirror(mc):
    """MultiCameraFrame.setDistortion once, then every extraction fills image_kps_undist; BruteForceMatch returns those keypoints,
    computeIntraMatches(old=True) reads them; without distortion image_kps_undist stays the very image_kps object"""
    C, W, H = 4, 1280, 720
    frame = mc.MultiCameraFrame(C, W, H, nfeatures=2000)
    frame.setData([mc.synth_rig_frame(5, C, c, W, H) for c in range(C)])
    frame.extractFeaturesParallel()
    assert frame.image_kps_undist is frame.image_kps
    Ks = [kmat(W, H, 0.85 + 0.03 * c) for c in range(C)]
    frame.setDistortion(Ks, DISTS)
    for f in (5, 6):
        frame.setData([mc.synth_rig_frame(f, C, c, W, H) for c in range(C)])
        frame.extractFeaturesParallel()
        with np.errstate(all="ignore"):
            want = [U.undistort_records(frame.image_kps[c], Ks[c], DISTS[c]) for c in range(C)]
        assert all(frame.image_kps_undist[c].tobytes() == want[c].tobytes() for c in range(C))
        i1, i2, k1, k2 = frame.BruteForceMatch(1, 2, 75.0, 0.85)
        assert len(i1) > 0 and k1.tobytes() == want[1][i1].tobytes() and k2.tobytes() == want[2][i2].tobytes()
    K, R, t = _calibration(C)
    frame.setCalibration(K, R, t)
    a = frame.computeIntraMatches(old=True)
    b = frame.rig.tracks_epipolar(0, frame.F_mats, kps_undist=want)[0]
    assert [m.matchIndex for m in a] == b.tolist()
    frame.setUndistorted([k.copy() for k in frame.image_kps])   # still overrides
    assert frame.image_kps_undist[2].tobytes() == frame.image_kps[2].tobytes()
    frame.setDistortion(Ks, [None] * C)
    frame.extractFeaturesParallel()
    assert frame.image_kps_undist is frame.image_kps


def test_cpp_adapter(mc, tmp_path):
    C, W, H, N, f = 4, 1280, 720, 2000, 7
    exe = str(tmp_path / "test_undistort_adapter")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_undistort_adapter.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mc-slam_amd"), "-lmcorb", "-Wl,-rpath," + os.path.join(ROOT, "mc-slam_amd")])
    Ks = [kmat(W, H, 0.85 + 0.03 * c) for c in range(C)]
    cf = tmp_path / "coeffs.bin"
    with open(cf, "wb") as fh:
        for c in range(C):
            d = np.zeros(12)
            d[:len(DISTS[c])] = DISTS[c]
            fh.write(Ks[c].astype("<f8").tobytes() + np.int32(len(DISTS[c])).tobytes() + d.astype("<f8").tobytes())
    out = subprocess.run([exe, str(C), str(W), str(H), str(N), str(f), str(tmp_path), str(cf)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for c in range(C):
        kps = np.fromfile(tmp_path / ("kps_%d.bin" % c), mc.KP_DTYPE)
        und = np.fromfile(tmp_path / ("undist_%d.bin" % c), kps.dtype)
        with np.errstate(all="ignore"):
            want = U.undistort_records(kps, Ks[c], DISTS[c])
        assert len(kps) > 500 and und.tobytes() == want.tobytes(), "camera %d" % c


def test_set_clear_reset_between_jobs(mc):
    """a cleared rig computes what a rig that never had undistortion computes (graph replay included); a re-set one the set again"""
    C, W, H = 4, 1280, 720
    plain = mc.Rig(C, W, H, 1, 1, nfeatures=2000)
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=2000)
    for r in (plain, rig):
        r.set_graph(1)
    Ks = set_all(rig, W, H, DISTS)
    imgs = frames(mc, 1, C, W, H, f0=8)
    rig.upload(imgs)
    rig.process(1)
    check_images(rig, C, Ks, DISTS)
    for c in range(C):
        rig.set_undistortion(c)   # clear
    assert not any(rig.undistortion_active(c) for c in range(C))
    with pytest.raises(mc.McorbError) as e:
        rig.features_undist(0)    # extracted before the set call
    assert e.value.code == mc.E_STATE
    for f in range(2):
        imgs = frames(mc, 1, C, W, H, f0=8 + f)
        for r in (plain, rig):
            r.upload(imgs)
            r.process(1)
        for m in range(C):
            a, b = plain.features(m), rig.features(m)
            assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
            assert rig.features_undist(m).tobytes() == b[1].tobytes() == plain.features_undist(m).tobytes()
        assert np.array_equal(plain.tracks(0)[0], rig.tracks(0)[0])
    Ks = set_all(rig, W, H, DISTS)   # re-set
    rig.upload(imgs)
    rig.process(1)
    assert check_images(rig, C, Ks, DISTS) == 2
    plain.close()
    rig.close()


def test_set_during_a_submitted_job_is_refused(mc):
    C, W, H = 2, 640, 480
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=1000)
    rig.upload(frames(mc, 1, C, W, H))
    rig.process_submit(1)
    with pytest.raises(mc.McorbError) as e:
        rig.set_undistortion(0, kmat(W, H), DISTS[2])
    assert e.value.code == mc.E_STATE
    rig.process_wait()
    rig.set_undistortion(0, kmat(W, H), DISTS[2])
    assert rig.undistortion_active(0)
    rig.close()


def test_argument_checks(mc):
    import ctypes as C
    rig = mc.Rig(2, 640, 480, 1, 1, nfeatures=500)
    L = rig.L
    K = kmat(640, 480)
    for n in (1, 3, 6, 13, 14):
        d = np.full(n, 0.01)
        assert L.mcorb_rig_set_undistortion(rig.h_rig, 0, K.ctypes.data, d.ctypes.data, n) == mc.E_ARG
    d = np.array(DISTS[2])
    for bad in ((0, 0), (1, 1)):
        K2 = K.copy()
        K2[bad] = 0.0
        assert L.mcorb_rig_set_undistortion(rig.h_rig, 0, K2.ctypes.data, d.ctypes.data, 5) == mc.E_ARG
    for v in (np.nan, np.inf, 1e300):   # 1e300 becomes inf through float, as in the reference
        K2 = K.copy()
        K2[1, 1] = v
        assert L.mcorb_rig_set_undistortion(rig.h_rig, 0, K2.ctypes.data, d.ctypes.data, 5) == mc.E_ARG
    assert L.mcorb_rig_set_undistortion(rig.h_rig, 2, K.ctypes.data, d.ctypes.data, 5) == mc.E_ARG
    assert L.mcorb_rig_set_undistortion(rig.h_rig, 0, None, d.ctypes.data, 5) == mc.E_ARG
    assert L.mcorb_rig_undistortion_active(rig.h_rig, 5) == mc.E_ARG
    assert not rig.undistortion_active(0)
    for n in (4, 5, 8, 12):
        dd = np.zeros(n)
        dd[0] = -0.1
        assert L.mcorb_rig_set_undistortion(rig.h_rig, 0, K.ctypes.data, dd.ctypes.data, n) == 0
        assert rig.undistortion_active(0)
    assert L.mcorb_rig_set_undistortion(rig.h_rig, 0, K.ctypes.data, None, 5) == 0 and not rig.undistortion_active(0)
    assert L.mcorb_rig_set_undistortion(rig.h_rig, 1, K.ctypes.data, d.ctypes.data, 0) == 0 and not rig.undistortion_active(1)
    rig.close()
