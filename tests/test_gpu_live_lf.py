"""obtainLfFeatures and the LF set's transform inside the extraction job (mcorb_rig_set_lf): every job of a vocabulary bound with
MCORB_BOW_MATCH also gives, per frame, what FrontEnd::processFrame's obtainLfFeatures (FrontEnd.cpp:1009-1024) and its
orb_vocabulary->transform of the LF set (:525) leave.  The triangulations run in k_lf_tracks on the device.  The results equal
the explicit calls on the job's own tracks bit for bit (mcorb_rig_obtain_lf_features with words_ all 1, no masks, the rig's
undistorted set; mcorb_vocab_transform of its descriptors), on every path a job takes; the device triangulation equals the
host's bit for bit; and the oracle within the existing tolerances."""
import os
import subprocess

import numpy as np
import pytest

import lf_problems
import oracle_lib as O
from test_lf_features import _rig_calibration

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST = [-0.2873, 0.0912, 0.00031, -0.00047, -0.0312]
TOL = 1e-9


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


def frames(mc, F, C, W, H, f0=0):
    return [mc.synth_rig_frame(f0 + f, C, c, W, H) for f in range(F) for c in range(C)]


def calib(C, W, H):
    # disparity fx * baseline / Z per camera: the synthetic rig's 24 px at Z = fx * 0.5 / 24, inside the 0.5 < z < 40 gate
    return _rig_calibration(C, fx=0.8 * W, cx=W / 2.0, cy=H / 2.0)


def explicit(rig, voc, frame, levelsup, cal, total_feats, slot=0):
    tr = rig.bow_tracks(frame, 1, slot=slot)[0][0]
    lf = rig.obtain_lf_features(frame, tr, *cal, words=np.ones(len(tr), np.uint32), total_feats=total_feats, slot=slot)
    return lf, voc.transform(lf[0]["desc"], levelsup)


def same_lf(a, b, what=""):
    (fa, ia, ma, wa), (fb, ib, mb, wb) = a, b
    assert (ia, ma) == (ib, mb) and len(fa) == len(fb), what
    assert fa.tobytes() == fb.tobytes(), "features differ %s" % what
    assert wa.tolist() == wb.tolist(), what


def same_bow(a, b, what=""):
    (ia, va), fa = a
    (ib, vb), fb = b
    assert np.array_equal(ia, ib) and va.tobytes() == vb.tobytes(), "lfBoW differs %s" % what
    assert list(fa) == list(fb) and all(np.array_equal(fa[k], fb[k]) for k in fa), "lfFeatVec differs %s" % what


def check_job(rig, voc, nframes, levelsup, cal, total_feats, slot=0):
    got = [(rig.lf_features(f, slot=slot), rig.lf_bow(f, slot=slot)) for f in range(nframes)]
    for f in range(nframes):
        lf, bow = explicit(rig, voc, f, levelsup, cal, total_feats, slot)
        same_lf(got[f][0], lf, "slot %d frame %d" % (slot, f))
        same_bow(got[f][1], bow, "slot %d frame %d" % (slot, f))
    return got


def test_device_triangulation_equals_host():
    """10^5 problems of 2 .. MCORB_MAX_CAMS views of every kind through k_lf_tracks' solver: bit-equal to mcorb_host_triangulate,
    and every exit of the solver is taken"""
    from importlib import import_module
    lib = import_module("mc-slam_amd")._lib
    L = lib.load()
    nv, x, P, kinds = lf_problems.problems(100_000, lib.MAX_CAMS, seed=7)
    n = len(nv)
    X, br = np.zeros((n, 3)), np.zeros(n, np.int32)
    assert L.mcorb_dev_triangulate_selftest(0, x.ctypes.data, P.ctypes.data, nv.ctypes.data, n, X.ctypes.data, br.ctypes.data) == 0
    Xh, bh = np.zeros(3), np.zeros(1, np.int32)
    xo = po = 0
    bad = []
    for i, k in enumerate(nv):
        xi, Pi = np.ascontiguousarray(x[xo:xo + 2 * k]), np.ascontiguousarray(P[po:po + 12 * k])
        assert L.mcorb_host_triangulate_branch(xi.ctypes.data, Pi.ctypes.data, int(k), Xh.ctypes.data, bh.ctypes.data) == 0
        if Xh.tobytes() != X[i].tobytes() or bh[0] != br[i]:
            bad.append((i, kinds[i], int(k)))
        xo += 2 * k
        po += 12 * k
    assert not bad, "%d problems differ, first %s" % (len(bad), bad[:5])
    counts = np.bincount(br, minlength=4)
    assert np.all(counts > 0), counts   # zero trace, unshifted only, Rayleigh, Sylvester re-run


@pytest.mark.parametrize("selection,graph", [(2, 0), (2, 1), (1, 0)], ids=["gpu", "gpu-graph", "host"])
@pytest.mark.parametrize("undist", [False, True], ids=["raw", "undist"])
def test_every_path_one_slot(mc, selection, graph, undist):
    """one rig frame per job, three jobs per rig (a captured graph is replayed), extract and process"""
    C, W, H, levelsup = 4, 1280, 720, 3
    v = O.make_vocabulary(10, 4, seed=9)
    voc = mc.ORBVocabulary().create(**v)
    cal = calib(C, W, H)
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=2000, selection=selection)
    rig.set_graph(graph)
    if undist:
        for c in range(C):
            rig.set_undistortion(c, cal[0][c], DIST)
    rig.set_vocabulary(voc, levelsup=levelsup)
    rig.set_lf(*cal)
    for f in range(3):
        rig.upload(frames(mc, 1, C, W, H, f0=3 + f))
        rig.extract(C) if f != 1 else rig.process(1)
        got = check_job(rig, voc, 1, levelsup, cal, 3000)
        assert got[0][0][1] > 50 and got[0][0][2] > 0
    rig.close()


@pytest.mark.parametrize("F", [1, 3, 32])
@pytest.mark.parametrize("short_fill", [False, True], ids=["total3000", "total-below-tracks"])
def test_batches_and_total_feats(mc, F, short_fill):
    """batches of 1, 3 and 32 frames; total_feats = 3000, and one below the accepted track count (the mono fill is empty)"""
    C, W, H, levelsup = 4, 640, 480, 2
    v = O.make_vocabulary(10, 4, seed=3)
    voc = mc.ORBVocabulary().create(**v)
    cal = calib(C, W, H)
    rig = mc.Rig(C, W, H, F, 1, nfeatures=1000)
    rig.set_vocabulary(voc, levelsup=levelsup)
    rig.set_lf(*cal)
    rig.upload(frames(mc, F, C, W, H, f0=11))
    rig.extract(F * C)
    total = 3000
    if short_fill:
        total = rig.lf_features(0)[1] - 1
        assert total > 10
        rig.set_lf(*cal, total_feats=total)
        rig.extract(F * C)
    got = check_job(rig, voc, F, levelsup, cal, total)
    if short_fill:
        assert got[0][0][2] == 0
    rig.close()


@pytest.mark.parametrize("selection", [2, 1], ids=["gpu", "host"])
def test_two_slots_in_flight(mc, selection):
    C, W, H, F, levelsup = 4, 1280, 720, 4, 2
    v = O.make_vocabulary(10, 4, seed=13)
    voc = mc.ORBVocabulary().create(**v)
    cal = calib(C, W, H)
    rig = mc.Rig(C, W, H, F, 2, nfeatures=2000, selection=selection)
    rig.set_vocabulary(voc, levelsup=levelsup)
    rig.set_lf(*cal)
    for s in range(2):
        rig.upload(frames(mc, F, C, W, H, f0=10 * s), slot=s)
    for s in range(2):
        rig.extract_submit(F * C, slot=s)
    for s in range(2):
        rig.extract_wait(slot=s)
    for s in range(2):
        check_job(rig, voc, F, levelsup, cal, 3000, slot=s)
    assert rig.lf_features(0, slot=0)[0].tobytes() != rig.lf_features(0, slot=1)[0].tobytes()
    rig.close()


@pytest.mark.parametrize("frames_per_job", [1, 5])
def test_forced_fallback_to_the_host_stage(mc, monkeypatch, frames_per_job):
    from test_gpu_select import _clustered_image
    monkeypatch.setenv("MCORB_SELECT_DEEP_CAP", "8")
    C, W, H = 2, 800, 600
    v = O.make_vocabulary(10, 3, seed=21)
    voc = mc.ORBVocabulary().create(**v)
    cal = calib(C, W, H)
    rig = mc.Rig(C, W, H, frames_per_job, 1, nfeatures=1000, selection=2)
    rig.set_vocabulary(voc, levelsup=2)
    rig.set_lf(*cal)
    imgs = frames(mc, frames_per_job, C, W, H, f0=3)
    imgs[-1] = _clustered_image(W, H)
    rig.upload(imgs)
    rig.extract(frames_per_job * C)
    assert rig.select_fallbacks() == 1
    check_job(rig, voc, frames_per_job, 2, cal, 3000)
    rig.close()


@pytest.mark.parametrize("C", [4, 5])
def test_bound_equals_oracle(mc, C):
    """the job's output on its own tracks against the oracle's statement-by-statement restatement (LAPACK SVD): integers and
    order exact, point3d / uv_ref within 1e-9 relative; five cameras take k_lf_tracks' run-time-shaped instance"""
    W, H, levelsup = 1280, 720, 2
    v = O.make_vocabulary(10, 4, seed=5)
    voc = mc.ORBVocabulary().create(**v)
    cal = calib(C, W, H)
    rig = mc.Rig(C, W, H, 1, 1, nfeatures=1500)
    rig.set_vocabulary(voc, levelsup=levelsup)
    rig.set_lf(*cal)
    rig.upload(frames(mc, 1, C, W, H, f0=6))
    rig.extract(C)
    got, ni, nm, wf = rig.lf_features(0)
    tr = rig.bow_tracks(0, 1)[0][0]
    feats = [rig.features(c) for c in range(C)]
    ora, oni, onm, owf = O.obtain_lf_features([f[1] for f in feats], [f[2] for f in feats], tr, *cal,
                                              words=np.ones(len(tr), np.uint32), total_feats=3000)
    assert (ni, nm) == (oni, onm) and wf.tolist() == owf == [1] and len(got) == len(ora)
    assert ni > 50
    for g, o in zip(got, ora):
        assert g["match_index"][:C].tolist() == o["match_index"] and g["mono"] == o["mono"] and g["n_rays"] == o["n_rays"]
        assert np.array_equal(g["desc"], o["desc"])
        if g["mono"]:
            assert g["uv_ref"][0] == o["uv_ref"][0] and g["uv_ref"][1] == o["uv_ref"][1]
        else:
            assert np.allclose(g["point3d"], o["point3d"], rtol=TOL, atol=TOL)
            assert np.allclose(g["uv_ref"], np.array(o["uv_ref"], np.float32), rtol=1e-6, atol=1e-4)
    same_bow(rig.lf_bow(0), O.bow_transform(v, got["desc"], levelsup), "vs oracle transform")
    rig.close()


def test_lifecycle(mc):
    C, W, H, levelsup = 2, 640, 480, 2
    v = O.make_vocabulary(10, 4, seed=3)
    voc = mc.ORBVocabulary().create(**v)
    cal = calib(C, W, H)
    imgs = frames(mc, 2, C, W, H, f0=1)
    plain = mc.Rig(C, W, H, 2, 1, nfeatures=1000)
    plain.set_vocabulary(voc, levelsup=levelsup)
    plain.upload(imgs)
    plain.extract(2 * C)
    rig = mc.Rig(C, W, H, 2, 1, nfeatures=1000)
    rig.set_vocabulary(voc, levelsup=levelsup)
    rig.upload(imgs)
    # bad arguments, and refused while a job is submitted
    with pytest.raises(mc.McorbError) as e:
        rig.set_lf(*cal, total_feats=-1)
    assert e.value.code == mc.E_ARG
    rig.extract_submit(2 * C)
    with pytest.raises(mc.McorbError) as e:
        rig.set_lf(*cal)
    assert e.value.code == mc.E_STATE
    rig.extract_wait()
    with pytest.raises(mc.McorbError) as e:   # the job ran without the stage
        rig.lf_features(0)
    assert e.value.code == mc.E_STATE
    rig.set_lf(*cal)
    rig.extract(2 * C)
    a = check_job(rig, voc, 2, levelsup, cal, 3000)
    with pytest.raises(mc.McorbError) as e:
        rig.lf_features(2)
    assert e.value.code in (mc.E_STATE, mc.E_ARG)
    # rebinding with other cameras takes effect on the next job
    K, R, t = cal
    cal2 = ([k * np.array([[1.1, 1, 1.05], [1, 1.1, 0.95], [1, 1, 1]]) for k in K], R, [tt * 0.5 for tt in t])
    rig.set_lf(*cal2)
    rig.extract(2 * C)
    b = check_job(rig, voc, 2, levelsup, cal2, 3000)
    assert a[0][0][0].tobytes() != b[0][0][0].tobytes()
    # the vocabulary without MCORB_BOW_MATCH: the stage does not run
    rig.set_vocabulary(voc, levelsup=levelsup, match=False)
    rig.extract(2 * C)
    with pytest.raises(mc.McorbError) as e:
        rig.lf_features(0)
    assert e.value.code == mc.E_STATE
    # unbinding: outputs and getter states equal a never-bound rig's
    rig.set_vocabulary(voc, levelsup=levelsup)
    rig.set_lf(None, None, None)
    rig.extract(2 * C)
    for m in range(2 * C):
        x, y = rig.features(m), plain.features(m)
        assert x[1].tobytes() == y[1].tobytes() and np.array_equal(x[2], y[2])
    for f in range(2):
        for r in (rig, plain):
            with pytest.raises(mc.McorbError) as e:
                r.lf_features(f)
            assert e.value.code == mc.E_STATE
            with pytest.raises(mc.McorbError) as e:
                r.lf_bow(f)
            assert e.value.code == mc.E_STATE
        for u, w in zip(rig.bow_tracks(f, 1)[0], plain.bow_tracks(f, 1)[0]):
            assert np.array_equal(u, w)
    rig.close()
    plain.close()


def test_multicameraframe_set_lf_config(mc):
    C, W, H = 4, 1280, 720
    v = O.make_vocabulary(6, 6, seed=17)
    voc = mc.ORBVocabulary().create(**v)
    cal = calib(C, W, H)
    fr = mc.MultiCameraFrame(C, W, H, nfeatures=2000)
    fr.setVocabulary(voc, levelsup=4)
    fr.setLfConfig(*cal)
    fr.setData(frames(mc, 1, C, W, H, f0=6))
    fr.extractFeaturesParallel()
    (feats, ni, nm, wf), bow = explicit(fr.rig, voc, 0, 4, cal, 3000)
    assert fr.intramatch_size == ni > 50 and fr.mono_size == nm and len(fr.intraMatches) == len(feats)
    for m, g in zip(fr.intraMatches, feats):
        assert m.matchIndex == g["match_index"].tolist() and m.mono == bool(g["mono"]) and m.n_rays == g["n_rays"]
        assert np.array_equal(m.matchDesc, g["desc"]) and m.point3D.tobytes() == g["point3d"].tobytes()
        assert m.uv_ref == (float(g["uv_ref"][0]), float(g["uv_ref"][1]))
    same_bow((fr.lfBoW, fr.lfFeatVec), bow)
    fr.rig.close()


def test_cpp_adapter(mc, tmp_path):
    C, W, H, N, f = 4, 1280, 720, 2000, 7
    v = O.make_vocabulary(6, 6, seed=19)
    vpath = str(tmp_path / "voc.txt")
    O.write_vocabulary_text(v, vpath)
    exe = str(tmp_path / "test_live_lf_adapter")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_live_lf_adapter.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mc-slam_amd"), "-lmcorb", "-Wl,-rpath," + os.path.join(ROOT, "mc-slam_amd")])
    out = subprocess.run([exe, str(C), str(W), str(H), str(N), str(f), vpath], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lf features" in out.stdout
