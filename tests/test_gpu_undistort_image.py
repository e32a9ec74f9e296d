"""cv::undistort at the hand-off (k_remap_u8, behind every upload form of a rig with image undistortion set): level 0 equals the
numpy restatement (tests/undistort_image_ref.py) of the raw plane bit for bit; the whole job on it equals the job of a plain rig
fed the already-remapped planes; a re-run on resident inputs is not undistorted twice; set / clear / re-set between jobs; the
exclusion with keypoint undistortion; the C ABI's argument and state checks; the Python mirror and the C++ adapter."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import undistort_image_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 4, 5, 8 and 12 coefficients; the second is a pincushion strong enough to pull the border's zeros into the corners
DISTS = [
    [-0.2873, 0.0912, 0.00031, -0.00047],
    [0.3841, 0.1422, -0.00112, 0.00083, 0.0213],
    [0.5213, -0.1274, 0.00041, -0.00037, 0.0089, 0.8723, -0.0612, 0.0301],
    [-0.2791, 0.0833, 0.00027, -0.00061, -0.0175, 0.0213, -0.0034, 0.0011, 0.0017, -0.0008, -0.0012, 0.0004],
]


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


def kmat(W, H, f=0.9):
    return np.array([[f * W, 0.0, W / 2 + 3.3], [0.0, f * W * 1.002, H / 2 - 2.1], [0.0, 0.0, 1.0]])


def frames(mc, F, C, W, H, f0=0):
    return [mc.synth_rig_frame(f0 + f, C, c, W, H) for f in range(F) for c in range(C)]


_MAPS = {}


def ref_maps(W, H, c, dist):
    key = (W, H, c, tuple(dist))
    if key not in _MAPS:
        with np.errstate(all="ignore"):
            _MAPS[key] = R.undistort_map(kmat(W, H, 0.85 + 0.03 * c), dist, W, H)
    return _MAPS[key]


def set_all(rig, W, H, dists):
    """dists[c] = None leaves the camera unset"""
    for c, d in enumerate(dists):
        if d is not None:
            rig.set_image_undistortion(c, kmat(W, H, 0.85 + 0.03 * c), d)


def expected_level0(raw, W, H, c, dist):
    if dist is None:
        return raw
    return R.remap(raw, *ref_maps(W, H, c, dist))[0]


def check_planes(rig, raws, W, H, dists, slot=0):
    C = len(dists)
    for m, raw in enumerate(raws):
        c = m % C
        assert np.array_equal(rig.raw_image(m, slot=slot), raw), "raw plane of image %d (slot %d)" % (m, slot)
        got = rig.level(m, 0, slot=slot)
        want = expected_level0(raw, W, H, c, dists[c])
        assert np.array_equal(got, want), "level 0 of image %d (camera %d, slot %d): %d pixels differ" % (m, c, slot, int((got != want).sum()))
        if dists[c] is not None:
            assert not np.array_equal(got, raw)


def upload_form(rig, form, imgs, slot=0):
    """uploads the u8 planes `imgs` through one of the forms; returns the raw planes the rig must then hold"""
    if form == "u8":
        rig.upload(imgs, slot=slot)
        return imgs
    if form == "staged":
        for m, im in enumerate(imgs):
            rig.staging(m, slot=slot)[:] = im
        rig.upload_staged(len(imgs), slot=slot)
        return imgs
    if form == "f32c1":
        rig.upload([im.astype(np.float32) / np.float32(255) for im in imgs], slot=slot)
        return imgs   # cvRound(float(u / 255) * 255) == u for every u8 value
    assert form == "f32c3"
    bgr, gray = [], []
    for i, im in enumerate(imgs):
        b, g, r = im, np.roll(im, 7 + i, axis=1), np.roll(im, 5, axis=0)
        bgr.append(np.stack([b, g, r], axis=2).astype(np.float32) / np.float32(255))
        gray.append(((b.astype(np.int64) * 1868 + g.astype(np.int64) * 9617 + r.astype(np.int64) * 4899 + 8192) >> 14).astype(np.uint8))
    rig.upload(bgr, slot=slot)
    return gray


@pytest.mark.parametrize("form", ["u8", "staged", "f32c1", "f32c3"])
@pytest.mark.parametrize("W,H", [(752, 480), (1280, 720), (1920, 1080)])
def test_one_frame_level0_after_each_upload_form(mc, W, H, form):
    """one rig frame of 5 cameras: four models and one camera left unset (copied through by the same launch)"""
    dists = DISTS + [None]
    C = len(dists)
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=1000)
    set_all(rig, W, H, dists)
    assert [rig.image_undistortion_active(c) for c in range(C)] == [True] * 4 + [False]
    for c in range(4):
        m1, m2 = rig.undistort_map(c)
        r1, r2 = ref_maps(W, H, c, dists[c])
        assert np.array_equal(m1, r1) and np.array_equal(m2, r2), "camera %d's map" % c
    for f in range(2):
        raws = upload_form(rig, form, frames(mc, 1, C, W, H, f0=2 + f))
        check_planes(rig, raws, W, H, dists)
    rig.close()


@pytest.mark.parametrize("form", ["u8", "staged", "f32c1"])
def test_nine_image_batch(mc, form):
    """9 images on a 4-camera rig: two whole frames and one image of a third (camera 0 has one frame more than the others)"""
    C, W, H = 4, 752, 480
    dists = [DISTS[0], None, DISTS[2], DISTS[1]]
    rig = mc.Rig(C, W, H, 3, 1, nfeatures=1000)
    set_all(rig, W, H, dists)
    imgs = frames(mc, 3, C, W, H, f0=1)[:9]
    raws = upload_form(rig, form, imgs)
    check_planes(rig, raws, W, H, dists)
    rig.extract(9)
    assert all(len(rig.features(m)[1]) > 100 for m in range(9))
    rig.close()


@pytest.mark.parametrize("form", ["u8", "staged", "f32c3"])
def test_full_batch_on_two_slots(mc, form):
    C, W, H, F = 4, 1280, 720, 8
    rig = mc.Rig(C, W, H, F, 2, nfeatures=1500)
    set_all(rig, W, H, DISTS)
    raws = [upload_form(rig, form, frames(mc, F, C, W, H, f0=20 * s), slot=s) for s in range(2)]
    for s in range(2):
        rig.process_submit(F, slot=s)
    for s in range(2):
        rig.process_wait(slot=s)
    for s in range(2):
        check_planes(rig, raws[s], W, H, DISTS, slot=s)
    assert not np.array_equal(rig.level(0, 0, slot=0), rig.level(0, 0, slot=1))
    rig.close()


def job_results(rig, F, C, bound, slot=0):
    out = {"features": [(f[0], f[1].tobytes(), f[2].tobytes()) for f in (rig.features(m, slot=slot) for m in range(F * C))]}
    out["undist"] = [rig.features_undist(m, slot=slot).tobytes() for m in range(F * C)]
    out["knn"] = [tuple(a.tobytes() for a in rig.pair_knn2(f, i, j, slot=slot)) for f in range(F) for i in range(C - 1) for j in range(i + 1, C)]
    out["tracks"] = [(t[0].tobytes(), t[1]) for t in (rig.tracks(f, slot=slot) for f in range(F))]
    if bound:
        out["bow_tracks"] = [tuple(np.asarray(a).tobytes() for a in t) for t in rig.bow_tracks(0, F, slot=slot)]
        lf = [rig.lf_features(f, slot=slot) for f in range(F)]
        out["lf"] = [(a[0].tobytes(), a[1], a[2], a[3].tobytes()) for a in lf]
        out["lf_n"] = [len(a[0]) for a in lf]
    return out


def same_results(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], "%s differs %s" % (k, what)


@pytest.mark.parametrize("selection,graph", [(2, 0), (2, 1), (1, 0)], ids=["gpu", "gpu-graph", "host"])
@pytest.mark.parametrize("F", [1, 3])
def test_whole_job_equals_plain_rig_on_remapped_planes(mc, selection, graph, F):
    """keypoints, descriptors, k-NN tables, tracks and, with a vocabulary and the LF cameras bound, BoW tracks and LF features,
    compared with ==; three jobs per rig (a captured graph is replayed); each job is then re-run on the resident inputs"""
    from test_lf_features import _rig_calibration
    C, W, H, levelsup = 4, 1280, 720, 3
    voc = mc.ORBVocabulary().create(**O.make_vocabulary(10, 4, seed=9))
    cal = _rig_calibration(C, fx=0.8 * W, cx=W / 2.0, cy=H / 2.0)
    rigs = [mc.Rig(C, W, H, F, 1, nfeatures=2000, selection=selection) for _ in range(2)]
    rig, plain = rigs
    for r in rigs:
        r.set_graph(graph)
        r.set_vocabulary(voc, levelsup=levelsup)
        r.set_lf(*cal)
    set_all(rig, W, H, DISTS)
    for job in range(3):
        imgs = frames(mc, F, C, W, H, f0=3 + 5 * job)
        rig.upload(imgs)
        plain.upload([expected_level0(im, W, H, m % C, DISTS[m % C]) for m, im in enumerate(imgs)])
        for r in rigs:
            r.process(F)
        a, b = job_results(rig, F, C, True), job_results(plain, F, C, True)
        same_results(a, b, "(job %d)" % job)
        assert a["undist"] == [f[1] for f in a["features"]]   # image_kps_undist is the raw keypoint set (:241-242)
        assert all(len(f[1]) > 0 and len(f[2]) > 500 * 32 for f in a["features"]) and all(n > 0 for n in a["lf_n"])
        level0 = rig.level(1, 0)
        rig.process(F)   # resident inputs: the remap belongs to the upload and does not run again
        same_results(job_results(rig, F, C, True), a, "(job %d re-run)" % job)
        assert np.array_equal(rig.level(1, 0), level0)
    for r in rigs:
        r.close()


def test_set_clear_reset_between_jobs(mc):
    """a cleared rig computes what a rig that never had it computes (graph replay included); a re-set one undistorts again"""
    C, W, H = 4, 1280, 720
    plain = mc.Rig(C, W, H, 1, 1, nfeatures=2000)
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=2000)
    for r in (plain, rig):
        r.set_graph(1)
    set_all(rig, W, H, DISTS)
    imgs = frames(mc, 1, C, W, H, f0=8)
    rig.upload(imgs)
    rig.process(1)
    check_planes(rig, imgs, W, H, DISTS)
    distorted = job_results(rig, 1, C, False)
    for c in (0, 1, 2):
        rig.set_image_undistortion(c)   # clear three: the fourth still goes through the map, the others are copied
    assert [rig.image_undistortion_active(c) for c in range(C)] == [False, False, False, True]
    rig.upload(imgs)
    check_planes(rig, imgs, W, H, [None, None, None, DISTS[3]])
    rig.set_image_undistortion(3)
    assert not any(rig.image_undistortion_active(c) for c in range(C))
    for f in range(2):
        imgs = frames(mc, 1, C, W, H, f0=8 + f)
        for r in (plain, rig):
            r.upload(imgs)
            r.process(1)
        same_results(job_results(rig, 1, C, False), job_results(plain, 1, C, False), "(cleared, job %d)" % f)
        assert np.array_equal(rig.level(2, 0), imgs[2])
    set_all(rig, W, H, DISTS)   # re-set
    imgs = frames(mc, 1, C, W, H, f0=8)
    rig.upload(imgs)
    rig.process(1)
    check_planes(rig, imgs, W, H, DISTS)
    same_results(job_results(rig, 1, C, False), distorted, "(re-set)")
    plain.close()
    rig.close()


def test_excludes_keypoint_undistortion_both_ways(mc):
    C, W, H = 2, 640, 480
    K, d = kmat(W, H), DISTS[0]
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=500)
    rig.set_undistortion(0, K, [-0.2873, 0.0912, 0.00031, -0.00047, -0.0312])
    with pytest.raises(mc.McorbError) as e:
        rig.set_image_undistortion(1, K, d)
    assert e.value.code == mc.E_STATE and not rig.image_undistortion_active(1)
    with pytest.raises(mc.McorbError) as e:
        rig.set_image_undistortion(1)   # clearing is refused alike: the call mirrors the reference's rig-wide switch
    assert e.value.code == mc.E_STATE
    rig.set_undistortion(0)
    rig.set_image_undistortion(1, K, d)
    assert rig.image_undistortion_active(1)
    with pytest.raises(mc.McorbError) as e:
        rig.set_undistortion(0, K, [-0.2873, 0.0912, 0.00031, -0.00047, -0.0312])
    assert e.value.code == mc.E_STATE and not rig.undistortion_active(0)
    rig.set_image_undistortion(1)
    rig.set_undistortion(0, K, [-0.2873, 0.0912, 0.00031, -0.00047, -0.0312])
    assert rig.undistortion_active(0)
    rig.close()


def test_set_during_a_submitted_job_is_refused(mc):
    C, W, H = 2, 640, 480
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=1000)
    rig.upload(frames(mc, 1, C, W, H))
    rig.process_submit(1)
    with pytest.raises(mc.McorbError) as e:
        rig.set_image_undistortion(0, kmat(W, H), DISTS[1])
    assert e.value.code == mc.E_STATE
    rig.process_wait()
    rig.set_image_undistortion(0, kmat(W, H), DISTS[1])
    assert rig.image_undistortion_active(0)
    rig.close()


def test_argument_checks_and_hooks(mc):
    rig = mc.Rig(2, 640, 480, 1, 1, nfeatures=500)
    L = rig.L
    K = kmat(640, 480)
    out = np.zeros((480, 640), np.uint8)
    m1 = np.zeros((480, 640, 2), np.int16)
    m2 = np.zeros((480, 640), np.uint16)
    # nothing set yet: no raw planes, no map
    assert L.mcorb_rig_get_raw_image(rig.h_rig, 0, 0, out.ctypes.data, 640) == mc.E_STATE
    assert L.mcorb_rig_get_undistort_map(rig.h_rig, 0, m1.ctypes.data, m2.ctypes.data, 640 * 480) == mc.E_STATE
    for n in (1, 3, 6, 13, 14):
        d = np.full(n, 0.01)
        assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 0, K.ctypes.data, d.ctypes.data, n) == mc.E_ARG
    d = np.array(DISTS[1])
    for bad in ((0, 0), (1, 1)):
        K2 = K.copy()
        K2[bad] = 0.0
        assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 0, K2.ctypes.data, d.ctypes.data, 5) == mc.E_ARG
    for v in (np.nan, np.inf, -np.inf):
        K2 = K.copy()
        K2[0, 2] = v
        assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 0, K2.ctypes.data, d.ctypes.data, 5) == mc.E_ARG
        d2 = d.copy()
        d2[3] = v
        assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 0, K.ctypes.data, d2.ctypes.data, 5) == mc.E_ARG
    assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 2, K.ctypes.data, d.ctypes.data, 5) == mc.E_ARG
    assert L.mcorb_rig_set_image_undistortion(rig.h_rig, -1, K.ctypes.data, d.ctypes.data, 5) == mc.E_ARG
    assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 0, None, d.ctypes.data, 5) == mc.E_ARG
    assert L.mcorb_rig_image_undistortion_active(rig.h_rig, 5) == mc.E_ARG
    assert not rig.image_undistortion_active(0)
    for n in (4, 5, 8, 12):   # all-zero coefficients included: there is no zero test on this path
        dd = np.zeros(n)
        assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 0, K.ctypes.data, dd.ctypes.data, n) == 0
        assert rig.image_undistortion_active(0)
    a1, a2 = rig.undistort_map(0)
    yy, xx = np.mgrid[0:480, 0:640]
    assert np.array_equal(a1[..., 0], xx) and np.array_equal(a1[..., 1], yy) and not a2.any()
    imgs = frames(mc, 1, 2, 640, 480)
    rig.upload(imgs)
    assert np.array_equal(rig.level(0, 0), imgs[0]) and np.array_equal(rig.raw_image(1), imgs[1])
    assert L.mcorb_rig_get_undistort_map(rig.h_rig, 0, m1.ctypes.data, m2.ctypes.data, 640 * 480 - 1) == mc.E_CAP
    assert L.mcorb_rig_get_undistort_map(rig.h_rig, 1, m1.ctypes.data, m2.ctypes.data, 640 * 480) == mc.E_STATE
    assert L.mcorb_rig_get_undistort_map(rig.h_rig, 2, m1.ctypes.data, m2.ctypes.data, 640 * 480) == mc.E_ARG
    assert L.mcorb_rig_get_raw_image(rig.h_rig, 0, 2, out.ctypes.data, 640) == mc.E_ARG
    assert L.mcorb_rig_get_raw_image(rig.h_rig, 1, 0, out.ctypes.data, 640) == mc.E_ARG
    assert L.mcorb_rig_get_raw_image(rig.h_rig, 0, 0, out.ctypes.data, 639) == mc.E_ARG
    assert L.mcorb_rig_get_raw_image(rig.h_rig, 0, 0, None, 640) == mc.E_ARG
    assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 0, K.ctypes.data, None, 5) == 0 and not rig.image_undistortion_active(0)
    assert L.mcorb_rig_set_image_undistortion(rig.h_rig, 1, K.ctypes.data, d.ctypes.data, 0) == 0 and not rig.image_undistortion_active(1)
    rig.close()


def test_python_mirror(mc):
    """MultiCameraFrame.setRectify once, then setData undistorts every frame and image_kps_undist stays the image_kps object"""
    C, W, H = 4, 1280, 720
    frame = mc.MultiCameraFrame(C, W, H, nfeatures=2000)
    plain = mc.MultiCameraFrame(C, W, H, nfeatures=2000)
    Ks = [kmat(W, H, 0.85 + 0.03 * c) for c in range(C)]
    frame.setRectify(Ks, DISTS)
    for f in (5, 6):
        imgs = [mc.synth_rig_frame(f, C, c, W, H) for c in range(C)]
        frame.setData(imgs if f == 5 else [im.astype(np.float32) / np.float32(255) for im in imgs])
        plain.setData([expected_level0(im, W, H, c, DISTS[c]) for c, im in enumerate(imgs)])
        for fr in (frame, plain):
            fr.extractFeaturesParallel()
        assert frame.image_kps_undist is frame.image_kps
        for c in range(C):
            assert np.array_equal(frame.rig.level(c, 0), expected_level0(imgs[c], W, H, c, DISTS[c]))
            assert len(frame.image_kps[c]) > 500 and frame.image_kps[c].tobytes() == plain.image_kps[c].tobytes()
            assert frame.image_descriptors[c].tobytes() == plain.image_descriptors[c].tobytes()
        a, b = frame.BruteForceMatch(1, 2, 75.0, 0.85), plain.BruteForceMatch(1, 2, 75.0, 0.85)
        assert len(a[0]) > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert [m.matchIndex for m in frame.computeIntraMatches()] == [m.matchIndex for m in plain.computeIntraMatches()]
    with pytest.raises(mc.McorbError) as e:
        frame.setDistortion(Ks, DISTS)
    assert e.value.code == mc.E_STATE
    frame.setRectify(Ks, [None] * C)
    imgs = [mc.synth_rig_frame(7, C, c, W, H) for c in range(C)]
    frame.setData(imgs)
    assert np.array_equal(frame.rig.level(3, 0), imgs[3])
    with pytest.raises(ValueError):
        frame.setRectify(Ks[:2], DISTS[:2])


@pytest.mark.parametrize("f32", [0, 1], ids=["setData", "setDataF32"])
def test_cpp_adapter(mc, tmp_path, f32):
    C, W, H, N, f = 4, 1280, 720, 2000, 7
    exe = str(tmp_path / "test_undistort_image_adapter")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_undistort_image_adapter.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mc-slam_amd"), "-lmcorb", "-Wl,-rpath," + os.path.join(ROOT, "mc-slam_amd")])
    dists = DISTS[:3] + [None]
    cf = tmp_path / "coeffs.bin"
    with open(cf, "wb") as fh:
        for c in range(C):
            d = np.zeros(12)
            n = 0 if dists[c] is None else len(dists[c])
            d[:n] = dists[c] if n else []
            fh.write(kmat(W, H, 0.85 + 0.03 * c).astype("<f8").tobytes() + np.int32(n).tobytes() + d.astype("<f8").tobytes())
    out = subprocess.run([exe, str(C), str(W), str(H), str(N), str(f), str(tmp_path), str(cf), str(f32)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    imgs = frames(mc, 1, C, W, H, f0=f)
    want = [expected_level0(imgs[c], W, H, c, dists[c]) for c in range(C)]
    plain = mc.Rig(C, W, H, 1, 1, nfeatures=N)
    plain.upload(want)
    plain.extract(C)
    for c in range(C):
        assert np.array_equal(np.fromfile(tmp_path / ("raw_%d.bin" % c), np.uint8).reshape(H, W), imgs[c])
        assert np.array_equal(np.fromfile(tmp_path / ("level0_%d.bin" % c), np.uint8).reshape(H, W), want[c]), "camera %d" % c
        _, k, d = plain.features(c)
        assert len(k) > 500 and np.fromfile(tmp_path / ("kps_%d.bin" % c), np.uint8).tobytes() == k.tobytes()
        assert np.fromfile(tmp_path / ("desc_%d.bin" % c), np.uint8).tobytes() == d.tobytes()
    plain.close()
