"""A vocabulary bound to the rig (mcorb_rig_set_vocabulary): every extraction job also runs transform() of every image and the
BoW-guided computeIntraMatches(matches, words_) of every frame on the device, in the same submission (k_bow_descend, k_bow_fold,
k_bow_tables, k_bow_best2).  The results equal the oracle's and the explicit calls' (mcorb_rig_transform_images,
mcorb_rig_match_bow_frames) bit for bit, doubles included, on every path a job takes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the cases of test_bow.py::test_transform_matches_oracle: (k, L, weighting, scoring, levelsup), L2 and DOT_PRODUCT included
CASES = [(10, 3, 0, 0, 2), (10, 4, 0, 0, 4), (5, 5, 1, 1, 3), (3, 6, 2, 0, 4), (10, 3, 3, 5, 1), (7, 2, 0, 0, 4)]
DIST = [-0.2873, 0.0912, 0.00031, -0.00047, -0.0312]   # 5 coefficients, far from a pass-through


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


def frames(mc, F, C, W, H, f0=0):
    return [mc.synth_rig_frame(f0 + f, C, c, W, H) for f in range(F) for c in range(C)]


def same_transform(a, b, what=""):
    (ia, va), fa = a
    (ib, vb), fb = b
    assert np.array_equal(ia, ib), what
    assert va.dtype == vb.dtype == np.float64 and np.array_equal(va, vb), "BowVector values differ %s" % what
    assert list(fa) == list(fb), what
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), what


def same_tracks(a, b, what=""):
    assert len(a) == len(b)
    for f, (x, y) in enumerate(zip(a, b)):
        for u, v in zip(x, y):
            assert u.shape == v.shape and np.array_equal(u, v), "%s frame %d" % (what, f)


def oracle_tracks(v, feats, levelsup, C, rows=None):
    out = []
    for f in range(len(feats) // C):
        sl = slice(f * C, (f + 1) * C)
        fvs = [O.bow_transform(v, x[2], levelsup)[1] for x in feats[sl]]
        ys = [x[1]["y"] for x in feats[sl]] if rows is None else rows[sl]
        out.append(O.intra_matches_bow([x[2] for x in feats[sl]], ys, fvs))
    return out


@pytest.mark.parametrize("case", range(len(CASES)))
def test_bound_transform_equals_oracle(mc, case):
    """every image's BowVector / FeatureVector from the job equals O.bow_transform of its descriptors and the explicit call's;
    one frame (small batch) and three frames (copy path); C = 2, 4 and 5 across the cases"""
    k, L, weighting, scoring, levelsup = CASES[case]
    C = (2, 4, 5)[case % 3]
    W, H = 640, 480
    v = O.make_vocabulary(k, L, seed=k * 10 + L, scoring=scoring, weighting=weighting)
    voc = mc.ORBVocabulary().create(**v)
    for F in (1, 3):
        rig = mc.Rig(C, W, H, F, 1, nfeatures=1000)
        rig.set_vocabulary(voc, levelsup=levelsup, match=False)
        rig.upload(frames(mc, F, C, W, H, f0=case))
        rig.extract(F * C)
        got = rig.bow_transforms(0, F * C)
        feats = [rig.features(m) for m in range(F * C)]
        explicit = voc.transform_rig_images(rig, 0, F * C, levelsup=levelsup)
        for m in range(F * C):
            assert len(feats[m][2]) > 100
            same_transform(O.bow_transform(v, feats[m][2], levelsup), got[m], "image %d F %d" % (m, F))
            same_transform(explicit[m], got[m], "explicit image %d" % m)
        rig.close()


@pytest.mark.parametrize("F", [1, 3])
def test_bound_match_raw_and_undistorted_rows(mc, F):
    """tracks, n_rays and words_ of every frame equal O.intra_matches_bow and mcorb_rig_match_bow_frames, first on the raw rows,
    then with undistortion set, whose bent rows the |dy| < 50 gate must see"""
    C, W, H, levelsup = 4, 640, 480, 2
    v = O.make_vocabulary(10, 4, seed=3)
    voc = mc.ORBVocabulary().create(**v)
    rig = mc.Rig(C, W, H, F, 1, nfeatures=900)
    rig.set_vocabulary(voc, levelsup=levelsup)
    imgs = frames(mc, F, C, W, H, f0=5)
    rig.upload(imgs)
    rig.extract(F * C)
    feats = [rig.features(m) for m in range(F * C)]
    raw = rig.bow_tracks(0, F)
    want = oracle_tracks(v, feats, levelsup, C)
    same_tracks(raw, want, "raw vs oracle")
    assert all(len(t[0]) > 30 for t in raw)
    same_tracks(raw, voc.match_rig_frames(rig, 0, F, levelsup=levelsup), "raw vs explicit")

    K = np.array([[0.9 * W, 0.0, W / 2 + 3.3], [0.0, 0.9 * W, H / 2 - 2.1], [0.0, 0.0, 1.0]])
    for c in range(C):
        rig.set_undistortion(c, K, DIST)
    rig.upload(imgs)
    rig.extract(F * C)
    got = rig.bow_tracks(0, F)
    rows = [rig.features_undist(m)["y"] for m in range(F * C)]
    same_tracks(got, oracle_tracks(v, feats, levelsup, C, rows), "undistorted vs oracle")
    same_tracks(got, voc.match_rig_frames(rig, 0, F, levelsup=levelsup), "undistorted vs explicit")
    assert any(not (g[0].shape == r[0].shape and np.array_equal(g[0], r[0])) for g, r in zip(got, raw)), \
        "the bent rows should change at least one frame's tracks"
    rig.close()


def test_camera_without_features_gives_no_matches(mc):
    C, W, H = 3, 640, 480
    v = O.make_vocabulary(10, 4, seed=3)
    voc = mc.ORBVocabulary().create(**v)
    rig = mc.Rig(C, W, H, 2, 1, nfeatures=900)
    rig.set_vocabulary(voc, levelsup=2)
    imgs = frames(mc, 2, C, W, H, f0=2)
    imgs[1] = np.full((H, W), 117, np.uint8)   # frame 0, camera 1: uniform, no keypoint
    rig.upload(imgs)
    rig.extract(2 * C)
    assert len(rig.features(1)[1]) == 0
    got = rig.bow_tracks(0, 2)
    assert len(got[0][0]) == 0 and len(got[0][2]) == 0   # the reference returns no matches (:602-603)
    assert len(got[1][0]) > 30
    (ids, vals), fv = rig.bow_transforms(1, 1)[0]
    assert len(ids) == 0 and fv == {}
    same_tracks(got, voc.match_rig_frames(rig, 0, 2, levelsup=2))
    rig.close()


def _explicit(rig, voc, nimg, C, levelsup, slot=0):
    return (voc.transform_rig_images(rig, 0, nimg, slot=slot, levelsup=levelsup),
            voc.match_rig_frames(rig, 0, nimg // C, slot=slot, levelsup=levelsup))


def _check_job(rig, voc, nimg, C, levelsup, slot=0):
    tf, tr = rig.bow_transforms(0, nimg, slot=slot), rig.bow_tracks(0, nimg // C, slot=slot)
    etf, etr = _explicit(rig, voc, nimg, C, levelsup, slot)
    for m in range(nimg):
        same_transform(etf[m], tf[m], "slot %d image %d" % (slot, m))
    same_tracks(tr, etr, "slot %d" % slot)
    return tr


@pytest.mark.parametrize("selection,graph", [(2, 0), (2, 1), (1, 0)], ids=["gpu", "gpu-graph", "host"])
@pytest.mark.parametrize("undist", [False, True], ids=["raw", "undist"])
def test_every_path_one_slot(mc, selection, graph, undist):
    """one rig frame per job (host-mapped results), three jobs per rig so that a captured graph is replayed"""
    C, W, H, levelsup = 4, 1280, 720, 3
    v = O.make_vocabulary(10, 4, seed=9)
    voc = mc.ORBVocabulary().create(**v)
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=2000, selection=selection)
    rig.set_graph(graph)
    if undist:
        K = np.array([[0.9 * W, 0.0, W / 2], [0.0, 0.9 * W, H / 2], [0.0, 0.0, 1.0]])
        for c in range(C):
            rig.set_undistortion(c, K, DIST)
    rig.set_vocabulary(voc, levelsup=levelsup)
    for f in range(3):
        rig.upload(frames(mc, 1, C, W, H, f0=3 + f))
        rig.extract(C) if f != 1 else rig.process(1)
        assert len(_check_job(rig, voc, C, C, levelsup)[0][0]) > 50
    rig.close()


@pytest.mark.parametrize("selection", [2, 1], ids=["gpu", "host"])
def test_two_slots_in_flight(mc, selection):
    """four rig frames per job (device buffers, copies on the side stream) on two slots submitted before either is waited for"""
    C, W, H, F, levelsup = 4, 1280, 720, 4, 2
    v = O.make_vocabulary(10, 4, seed=13)
    voc = mc.ORBVocabulary().create(**v)
    rig = mc.Rig(C, W, H, F, 2, nfeatures=2000, selection=selection)
    rig.set_vocabulary(voc, levelsup=levelsup)
    for s in range(2):
        rig.upload(frames(mc, F, C, W, H, f0=10 * s), slot=s)
    for s in range(2):
        rig.extract_submit(F * C, slot=s)
    for s in range(2):
        rig.extract_wait(slot=s)
    job = [(rig.bow_transforms(0, F * C, slot=s), rig.bow_tracks(0, F, slot=s)) for s in range(2)]
    for s in range(2):
        etf, etr = _explicit(rig, voc, F * C, C, levelsup, slot=s)
        for m in range(F * C):
            same_transform(etf[m], job[s][0][m], "slot %d image %d" % (s, m))
        same_tracks(job[s][1], etr, "slot %d" % s)
    assert len(job[0][1][0][0]) > 50 and not np.array_equal(job[0][1][0][0], job[1][1][0][0])
    rig.close()


@pytest.mark.parametrize("frames_per_job", [1, 5])   # 2 images: host-mapped results; 10: copies
def test_forced_fallback_to_the_host_stage(mc, monkeypatch, frames_per_job):
    """a job whose GPU selection raises its flag is redone by the host stage: the BoW results follow the redone lists"""
    from test_gpu_select import _clustered_image
    monkeypatch.setenv("MCORB_SELECT_DEEP_CAP", "8")
    C, W, H = 2, 800, 600
    v = O.make_vocabulary(10, 3, seed=21)
    voc = mc.ORBVocabulary().create(**v)
    rig = mc.Rig(C, W, H, frames_per_job, 1, nfeatures=1000, selection=2)
    rig.set_vocabulary(voc, levelsup=2)
    imgs = frames(mc, frames_per_job, C, W, H, f0=3)
    imgs[-1] = _clustered_image(W, H)
    rig.upload(imgs)
    rig.extract(frames_per_job * C)
    assert rig.select_fallbacks() == 1
    _check_job(rig, voc, frames_per_job * C, C, 2)
    rig.close()


def test_binding_lifecycle(mc):
    from importlib import import_module
    lib = import_module("mc-slam_amd")._lib
    C, W, H = 2, 640, 480
    v = O.make_vocabulary(10, 4, seed=3)
    voc = mc.ORBVocabulary().create(**v)
    rig = mc.Rig(C, W, H, 2, 1, nfeatures=1000)
    imgs = frames(mc, 2, C, W, H, f0=1)
    rig.upload(imgs)
    # refused while a job is submitted
    rig.extract_submit(2 * C)
    with pytest.raises(mc.McorbError) as e:
        rig.set_vocabulary(voc, levelsup=2)
    assert e.value.code == mc.E_STATE
    rig.extract_wait()
    # argument checks
    with pytest.raises(mc.McorbError) as e:
        rig.set_vocabulary(voc, levelsup=-1)
    assert e.value.code == mc.E_ARG
    rig.set_vocabulary(voc, levelsup=2)
    with pytest.raises(mc.McorbError) as e:   # not a whole number of frames
        rig.extract(3)
    assert e.value.code == mc.E_ARG
    rig.set_vocabulary(voc, levelsup=2, match=False)
    rig.extract(3)                             # (the transform alone takes any image count)
    assert len(rig.bow_transforms(0, 3)) == 3
    # rebinding with another levelsup changes the next job's results
    rig.set_vocabulary(voc, levelsup=2)
    rig.extract(2 * C)
    a = rig.bow_transforms(0, 1)[0][1]
    rig.set_vocabulary(voc, levelsup=1)
    rig.extract(2 * C)
    b = rig.bow_transforms(0, 1)[0][1]
    feats0 = rig.features(0)[2]
    assert list(a) != list(b)
    same_transform(O.bow_transform(v, feats0, 1), rig.bow_transforms(0, 1)[0])
    same_tracks(rig.bow_tracks(0, 2), oracle_tracks(v, [rig.features(m) for m in range(2 * C)], 1, C))
    # unbinding: the getters answer E_STATE after the next extraction, as without the feature
    rig.set_vocabulary(None)
    rig.extract(2 * C)
    with pytest.raises(mc.McorbError) as e:
        rig.bow_tracks(0, 1)
    assert e.value.code == lib.E_STATE
    with pytest.raises(mc.McorbError) as e:
        rig.bow_transforms(0, 1)
    assert e.value.code == lib.E_STATE
    rig.close()


def test_kcap_beyond_the_lds_bound_is_refused(mc):
    v = O.make_vocabulary(5, 2, seed=1)
    voc = mc.ORBVocabulary().create(**v)
    rig = mc.Rig(1, 1280, 720, 1, 1, nfeatures=5000)
    with pytest.raises(mc.McorbError) as e:
        rig.set_vocabulary(voc)
    assert e.value.code == mc.E_ARG
    rig.close()
    rig = mc.Rig(1, 1280, 720, 1, 1, nfeatures=4000)   # nfeatures = 4000 at 8 levels fits
    rig.set_vocabulary(voc)
    rig.close()


def test_full_size_vocabulary(mc):
    """4 cameras at 1280x720, 2000 features, a k = 10, L = 6 vocabulary (1 111 110 nodes), one batch of two frames"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from bow_rate import full_vocabulary
    C, W, H, N, F = 4, 1280, 720, 2000, 2
    v = full_vocabulary(10, 6, seed=1)
    voc = mc.ORBVocabulary().create(**v)
    rig = mc.Rig(C, W, H, F, 1, nfeatures=N)
    rig.set_vocabulary(voc, levelsup=4)
    rig.upload(frames(mc, F, C, W, H, f0=3))
    rig.extract(F * C)
    feats = [rig.features(m) for m in range(F * C)]
    got_t = rig.bow_transforms(0, F * C)
    for m in range(F * C):
        same_transform(O.bow_transform(v, feats[m][2], 4), got_t[m], "image %d" % m)
        assert len(got_t[m][0][0]) > 1500
    got = rig.bow_tracks(0, F)
    same_tracks(got, oracle_tracks(v, feats, 4, C), "full size")
    assert all(len(t[0]) > 200 for t in got)
    rig.close()


def test_multicameraframe_set_vocabulary(mc):
    """setVocabulary: extractFeaturesParallel() fills BoW_vecs / BoW_feats (MultiCameraFrame.cpp:252-261), and
    computeIntraMatchesBoW reads the job's tracks, equal to the unbound frame's"""
    C, W, H = 4, 1280, 720
    v = O.make_vocabulary(6, 6, seed=17)   # levelsup 4 of L 6: FeatureVectors keyed two levels below the root
    voc = mc.ORBVocabulary().create(**v)
    imgs = frames(mc, 1, C, W, H, f0=6)
    plain = mc.MultiCameraFrame(C, W, H, nfeatures=2000)
    plain.setData(imgs)
    plain.extractFeaturesParallel()
    assert plain.BoW_vecs == [] and plain.BoW_feats == []
    w0 = []
    m0 = plain.computeIntraMatchesBoW(voc, w0, levelsup=4)
    bound = mc.MultiCameraFrame(C, W, H, nfeatures=2000)
    bound.setVocabulary(voc, levelsup=4)
    bound.setData(imgs)
    bound.extractFeaturesParallel()
    assert len(bound.BoW_vecs) == C and len(bound.BoW_feats) == C
    for c in range(C):
        same_transform(O.bow_transform(v, bound.image_descriptors[c], 4), (bound.BoW_vecs[c], bound.BoW_feats[c]), "camera %d" % c)
    w1 = []
    m1 = bound.computeIntraMatchesBoW(voc, w1, levelsup=4)
    assert len(m0) > 50 and w0 == w1
    assert [m.matchIndex for m in m0] == [m.matchIndex for m in m1] and [m.n_rays for m in m0] == [m.n_rays for m in m1]
    plain.rig.close()
    bound.rig.close()


def test_cpp_adapter(mc, tmp_path):
    """the adapter's setVocabulary: BoW_vecs / BoW_feats and the BoW-guided tracks equal the explicit path's"""
    C, W, H, N, f = 4, 1280, 720, 2000, 7
    v = O.make_vocabulary(6, 6, seed=19)   # the adapter's default levelsup is 4
    vpath = str(tmp_path / "voc.txt")
    O.write_vocabulary_text(v, vpath)
    exe = str(tmp_path / "test_live_bow_adapter")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_live_bow_adapter.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mc-slam_amd"), "-lmcorb", "-Wl,-rpath," + os.path.join(ROOT, "mc-slam_amd")])
    out = subprocess.run([exe, str(C), str(W), str(H), str(N), str(f), vpath], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tracks" in out.stdout
