"""The local bundle adjustment on the host-only store (device -1): mcorb_lmap_bundle_adjust against the plain-Python restatement
(ba_ref.py) and against answers written out by hand.  Bit for bit, floats as raw bytes, unless a test says otherwise.  No GPU.

On the commit before this call existed every test of this file fails (`python -m pytest tests/test_ba_cpu.py`): LocalMap has no
bundle_adjust."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ba_cases as BC
import ba_ref as B
import kfdb_cases as K
import pose_cases as PC
import pose_ref as P
import track_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture()
def lm(mc, voc):
    assert hasattr(mc.LocalMap, "bundle_adjust")
    return mc.LocalMap(voc, device=-1, max_landmarks=4096, max_candidates=1024)


@pytest.fixture(scope="module")
def seeded():
    """the seeded scene and its restatement, computed once"""
    sc = BC.scene()
    return sc, BC.ref(sc)


def both(mc, lm, sc, what, max_iterations=25, forms=("pts", "lids")):
    ref = BC.ref(sc, max_iterations)
    for form in forms:
        BC.same(BC.as_ref(BC.run(mc, lm, sc, max_iterations, form)), ref, "%s, %s" % (what, form))
    return ref


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the Jacobians (a comparison with a tolerance)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncams", [1, 4])
@pytest.mark.parametrize("sigma", [1.0, 0.694])
def test_jacobians_central_differences(mc, lm, ncams, sigma):
    """mcorb_ba_eval's J and JX against central differences of its whitened r through the Cayley retraction of the restatement
    and through point addition: h = 1e-6, pass at 1e-5 * max(1, |J_ij|), section 9g's rule (the difference quotient of a 1e3 px
    value carries about 1e-16 * 1e3 / 1e-6 = 1e-7).  Rigs with skew.  The library's r, J, JX and w equal the restatement's on the
    bits"""
    assert hasattr(mc, "ba_eval")
    sc = BC.scene(ncams=ncams, nlm=12, skew=0.3, seed=3)
    cams, pose = sc["cams"], sc["poses"][2]
    obs = [o for o in sc["obs"] if o[0] == 2]
    cam = np.array([o[1] for o in obs], np.int32)
    uv = np.array([[o[3], o[4]] for o in obs], np.float32)
    pts = np.array([sc["pts"][o[2]] for o in obs])
    cc = PC.to_cams(mc, cams)
    r0, J, JX, w = mc.ba_eval(cc, pose[0], pose[1], cam, uv, pts, sigma)
    assert len(obs) >= 5 and set(cam.tolist()) == set(range(ncams))
    for i, o in enumerate(obs):
        r, Jr, JXr, wr, _ = B.observation(cams[o[1]], pose, sc["pts"][o[2]], o[3], o[4], 1.0 / sigma)
        assert np.array(BC.flat([r, Jr, JXr, wr])).tobytes() == np.array(BC.flat([r0[i].tolist(), J[i].tolist(), JX[i].tolist(), w[i]])).tobytes()
    h = 1e-6
    worst = 0.0
    for k in range(9):
        d = [0.0] * 9
        d[k] = h
        plus = mc.ba_eval(cc, *P.retract(pose, d[:6]), cam, uv, pts + np.array(d[6:]), sigma)[0]
        d[k] = -h
        minus = mc.ba_eval(cc, *P.retract(pose, d[:6]), cam, uv, pts + np.array(d[6:]), sigma)[0]
        num = (plus - minus) / (2 * h)
        ana = J[:, :, k] if k < 6 else JX[:, :, k - 6]
        err = np.abs(num - ana) / np.maximum(1.0, np.abs(ana))
        worst = max(worst, float(err.max()))
    print("worst relative difference %.3g" % worst)
    assert worst < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------
# 2. one step (the other comparison with a tolerance)
# ---------------------------------------------------------------------------------------------------------------------------
def full_step(sc, lam):
    """numpy.linalg.solve on the full damped normal equations of the restatement's linearization: the unknowns are the system's
    keyframes (6 each), then the landmarks (3 each)"""
    nkf, nlm = len(sc["poses"]), len(sc["pts"])
    inv_s = [1.0 / s for s in sc["sigma"]]
    _, per_lm, sys_of_kf, kf_of_sys = B.plan(nkf, nlm, sc["fixed"], sc["obs"])
    nsys = len(kf_of_sys)
    n = 6 * nsys + 3 * nlm
    H, g = np.zeros((n, n)), np.zeros(n)
    for kf, cam, j, kx, ky, octave in sc["obs"]:
        r, J, JX, w, _ = B.observation(sc["cams"][cam], sc["poses"][kf], sc["pts"][j], kx, ky, inv_s[octave])
        A = np.zeros((2, n))
        if sys_of_kf[kf] >= 0:
            A[:, 6 * sys_of_kf[kf]:6 * sys_of_kf[kf] + 6] = J
        A[:, 6 * nsys + 3 * j:6 * nsys + 3 * j + 3] = JX
        H += w * A.T @ A
        g += w * A.T @ np.array(r)
    H[np.diag_indices(n)] *= 1.0 + lam
    return np.linalg.solve(H, -g), nsys, kf_of_sys


def test_one_step_against_the_full_normal_equations(mc, lm, seeded):
    """The Schur step of the first solve (lambda = 1e-4) of the seeded scene against numpy.linalg.solve on the full damped normal
    equations of the same linearization, as the relative 2-norm difference of the whole step (12 pose and 600 point unknowns).
    The restatement's own figure is 1.43e-12 (seeds 12 and 13: 8.2e-13, 1.2e-12); the pass mark is ten times that, 1.5e-11.
    The library's step is read off a call with max_iterations = 1, whose trial is accepted: the returned state minus the
    initial one, the poses through the retraction of the numpy step"""
    sc, _ = seeded
    x, nsys, kf_of_sys = full_step(sc, 1e-4)
    got = BC.run(mc, lm, sc, max_iterations=1)
    assert got.status == B.MAX_ITER and got.iterations == 1 and got.cost_final < got.cost_initial
    dX = (got.pts - np.array(sc["pts"])).reshape(-1)
    rel = np.linalg.norm(dX - x[6 * nsys:]) / np.linalg.norm(x[6 * nsys:])
    print("points: relative difference %.3g" % rel)
    assert rel < 1.5e-11
    for a, k in enumerate(kf_of_sys):
        Rn, tn = P.retract(sc["poses"][k], [float(v) for v in x[6 * a:6 * a + 6]])
        dR, dt = np.abs(got.R[k] - np.array(Rn)).max(), np.abs(got.t[k] - np.array(tn)).max()
        print("keyframe %d: |dR| %.3g, |dt| %.3g" % (k, dR, dt))
        assert dR < 1.5e-11 * np.linalg.norm(x[:6 * nsys]) and dt < 1.5e-11 * np.linalg.norm(x[:6 * nsys])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. rows written out by hand
# ---------------------------------------------------------------------------------------------------------------------------
def test_z_rows(mc, lm):
    """q.z of 0.0, -0.0, 1e-300, -1e-300 and NaN among ordinary rows: 0.0, -0.0 and -1e-300 are behind (zero Jacobians, the
    whitened (2 fx, 2 fx)), 1e-300 is in front and overflows, NaN is not behind and poisons the cost"""
    for with_nan in (True, False):
        for extra in ((), (1,)):
            sc = BC.hand_scene(PC.z_rows(with_nan) + BC.huber_rows(1.0), fixed=not extra, extra_kf=extra)
            ref = both(mc, lm, sc, "z rows, NaN %s, %d keyframes" % (with_nan, 1 + len(extra)))
            if with_nan:
                assert ref["status"] == B.NO_STEP and ref["cost_initial"] != ref["cost_initial"]
    rig, one = PC.flat_rig(), PC.to_cams(mc, PC.flat_rig())
    rows = PC.z_rows(True)[6:]
    r, J, JX, w = mc.ba_eval(one, T.EYE, [0.0] * 3, [0] * 5, [[1.0, 2.0]] * 5, [row[4] for row in rows], 0.5)
    for i in (0, 1, 3):      # behind: 2 fx / sigma = 4
        assert r[i].tolist() == [4.0, 4.0] and not J[i].any() and not JX[i].any()
    assert r[2, 0] > 1e299 and np.isnan(r[4]).all()


@pytest.mark.parametrize("sigma", [1.0, 0.25])
def test_huber_rows(mc, lm, sigma):
    """the whitened e exactly k and one ulp either side: w is 1 at and under k, k / e above"""
    rows = BC.huber_rows(sigma)
    k = P.HUBER_K
    one = PC.to_cams(mc, PC.flat_rig())
    r, J, JX, w = mc.ba_eval(one, T.EYE, [0.0] * 3, [0] * 3, [[0.0, 0.0]] * 3, [row[4] for row in rows], sigma)
    assert r[:, 0].tolist() == [np.nextafter(k, 0.0), k, np.nextafter(k, 10.0)]
    assert w.tolist() == [1.0, 1.0, k / np.nextafter(k, 10.0)] and w[2] < 1.0
    ref = both(mc, lm, BC.hand_scene(rows, sigma=(sigma,)), "Huber rows")
    assert ref["status"] == B.CONVERGED


def test_chi2_rows(mc, lm):
    """the whitened r.r exactly 5.991 (in) and the next double above (out), under sigma 1 and 4"""
    rows, sigma, flags = BC.chi2_rows()
    ref = both(mc, lm, BC.hand_scene(rows, sigma=sigma), "chi2 rows")
    assert ref["status"] == B.NO_STEP and ref["inliers"] == flags and ref["n_inliers"] == 3


# ---------------------------------------------------------------------------------------------------------------------------
# 4. degenerate shapes
# ---------------------------------------------------------------------------------------------------------------------------
def test_no_observations(mc, lm, seeded):
    sc, _ = seeded
    sc = dict(sc, obs=[])
    ref = both(mc, lm, sc, "no observations")
    assert ref["status"] == B.NO_OBS and ref["iterations"] == 0 and ref["pts"] == sc["pts"]
    ref = both(mc, lm, dict(sc, pts=[]), "no observations, no landmarks", forms=("pts",))
    assert ref["status"] == B.NO_OBS


@pytest.mark.parametrize("case", range(7))
def test_degenerate(mc, lm, case):
    name, sc, check = BC.degenerate()[case]
    check(sc, both(mc, lm, sc, name))


@pytest.mark.parametrize("its", [1, 100])
def test_max_iterations(mc, lm, its):
    sc = BC.scene(nlm=30, seed=21)
    ref = both(mc, lm, sc, "max_iterations %d" % its, max_iterations=its)
    assert ref["status"] == (B.MAX_ITER if its == 1 else B.CONVERGED) and (its != 1 or ref["iterations"] == 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the seeded scenes
# ---------------------------------------------------------------------------------------------------------------------------
def test_seeded_scene(mc, lm, seeded):
    """4 keyframes 0.3 m apart, the first two fixed; a 4-camera ring rig on 0.1 m lever arms, fx = fy = 160, 320 x 240; 200
    landmarks, 782 observations with 0.3 px noise; the free poses off by 0.02 rad and 0.1 m, the points by 0.1 m.  The
    restatement: CONVERGED in 4 solves, cost 16381.6 -> 139.80, the free poses 0.44 mrad and 1.74 mm from the truth; the pass
    marks are ten times those errors"""
    sc, ref = seeded
    assert len(sc["obs"]) == 782 and len(sc["pts"]) == 200
    assert ref["status"] == B.CONVERGED and ref["iterations"] == 4 and ref["cost_final"] < 0.01 * ref["cost_initial"]
    for form in ("pts", "lids"):
        got = BC.run(mc, lm, sc, form=form)
        BC.same(BC.as_ref(got), ref, "seeded scene, " + form)
        ang, dist = BC.errors(sc, list(zip(got.R.tolist(), got.t.tolist())))
        print("pose error %.3g rad, %.3g m; cost %.6g -> %.6g" % (ang, dist, got.cost_initial, got.cost_final))
        assert ang < 4.4e-3 and dist < 17.4e-3
        assert got.n_inliers == got.inliers.sum() == ref["n_inliers"]


def test_two_calls_around_moved_observations(mc, lm):
    """the seeded scene with 5 % of the observations moved by 30 px.  The restatement: the first call ends in MAX_ITER after 25
    solves (Huber alone leaves a linear tail) and flags 57 observations, all 33 moved ones among them; the second call, from the
    initial estimate without the flagged observations and without the landmarks left with fewer than two, converges in 5 solves
    to 0.81 mrad and 2.70 mm; the pass marks are ten times those.  Asserted on the poses and the flags only"""
    sc = BC.scene(moved=0.05)
    ref = BC.ref(sc)
    first = BC.run(mc, lm, sc)
    BC.same(BC.as_ref(first), ref, "first call")
    flagged = ~first.inliers
    assert first.status == B.MAX_ITER and first.iterations == 25
    assert sum(sc["moved"]) == 33 and all(f for f, m in zip(flagged, sc["moved"]) if m) and flagged.sum() <= 2 * 33
    sc2, keep = BC.without(sc, flagged.tolist())
    second = BC.run(mc, lm, sc2)
    BC.same(BC.as_ref(second), BC.ref(sc2), "second call")
    ang, dist = BC.errors(sc2, list(zip(second.R.tolist(), second.t.tolist())))
    print("second call: %d solves, pose error %.3g rad, %.3g m" % (second.iterations, ang, dist))
    assert second.status == B.CONVERGED and ang < 8.1e-3 and dist < 27e-3


# ---------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def read_back(lm, lids):
    return [(p.tobytes(), q.tobytes()) for p, q, _, _ in (lm.get(int(l)) for l in lids)]


def check_refusals(mc, lm):
    sc = BC.scene(nlm=20, seed=21)
    lids = BC.fill_points(lm, sc["pts"])
    before = read_back(lm, lids)
    kf, cam, olm, uv, octave = BC.arrays(sc["obs"])
    cc = PC.to_cams(mc, sc["cams"])
    pts = np.array(sc["pts"])

    def refused(code, pending=False, **kw):
        a = dict(cams=cc, kf_R=[p[0] for p in sc["poses"]], kf_t=[p[1] for p in sc["poses"]], fixed=sc["fixed"], obs_kf=kf, obs_cam=cam,
                 obs_lm=olm, uv=uv, octave=octave, sigma=sc["sigma"], lids=lids)
        a.update(kw)
        with pytest.raises(mc.McorbError) as e:
            lm.bundle_adjust(**a)
        assert e.value.code == code, (kw.keys(), e.value)
        assert pending or read_back(lm, lids) == before

    for name, arr, top in (("obs_kf", kf, 4), ("obs_cam", cam, 4), ("obs_lm", olm, 20), ("octave", octave, 4)):
        for v in (top, -1):
            bad = arr.copy()
            bad[7] = v
            refused(mc.E_ARG, **{name: bad})
    for v in (4096, -1):
        bad = lids.copy()
        bad[5] = v
        refused(mc.E_ARG, lids=bad)
    refused(mc.E_ARG, pts=pts)                      # both
    refused(mc.E_ARG, lids=None)                    # neither
    refused(mc.E_ARG, max_iterations=0)
    refused(mc.E_ARG, max_iterations=101)
    refused(mc.E_ARG, sigma=[])
    refused(mc.E_ARG, sigma=[1.0] * 17)
    for v in (0.0, -1.0, float("nan")):
        refused(mc.E_ARG, sigma=[1.0, v, 1.0, 1.0])
    bad = lids.copy()
    bad[5] = 3000                                   # a slot that was never set
    refused(mc.E_STATE, lids=bad)
    # counts and NULL arrays, through the C entry
    res, par = mc._lib.BAResultC(), mc.ba_params(sc["sigma"])
    R_ = np.array([p[0] for p in sc["poses"]], np.float64).reshape(-1)
    t_ = np.array([p[1] for p in sc["poses"]], np.float64).reshape(-1)
    fx = np.array(sc["fixed"], np.uint8)
    Ro, to, po, fl = np.zeros(17 * 9), np.zeros(17 * 3), np.zeros((20, 3)), np.zeros(len(kf), np.uint8)

    def entry(nkf=4, ncams=4, nlm=20, nobs=len(kf), R=R_.ctypes.data, fixed=fx.ctypes.data, okf=kf.ctypes.data, out=Ro.ctypes.data,
              pout=po.ctypes.data, params=C.byref(par)):
        return lm.L.mcorb_lmap_bundle_adjust(lm.h, nkf, R, t_.ctypes.data, fixed, ncams, C.addressof(cc.cams), nlm, lids.ctypes.data, None,
                                             nobs, okf, cam.ctypes.data, olm.ctypes.data, uv.ctypes.data, octave.ctypes.data, params, out,
                                             to.ctypes.data, pout, C.byref(res), fl.ctypes.data)

    for kw in (dict(nkf=0), dict(nkf=17), dict(ncams=0), dict(ncams=17), dict(nlm=-1), dict(nlm=65537), dict(nobs=-1), dict(nobs=(1 << 20) + 1),
               dict(R=None), dict(fixed=None), dict(okf=None), dict(out=None), dict(pout=None), dict(params=None)):
        assert entry(**kw) == mc.E_ARG, kw
    assert read_back(lm, lids) == before
    # while a tracking call is pending
    v = T.to_view(mc, T.flat_view())
    lm.track_submit(v, [np.zeros((0, 2), np.float32)], [np.zeros((0, 32), np.uint8)], [])
    refused(mc.E_STATE, pending=True)
    lm.track_wait()
    assert read_back(lm, lids) == before
    # and it runs after all that
    got = lm.bundle_adjust(cc, [p[0] for p in sc["poses"]], [p[1] for p in sc["poses"]], sc["fixed"], kf, cam, olm, uv, octave, sc["sigma"],
                           lids=lids)
    BC.same(BC.as_ref(got), BC.ref(sc), "after the refusals")
    assert read_back(lm, lids) == before


def test_refusals(mc, lm):
    check_refusals(mc, lm)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the header under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_under_asan_ubsan(mc, lm, seeded, tmp_path):
    """tests/cpp/test_ba_sanitize.cpp (its own main, -fsanitize=address,undefined) runs ba_plan and ba_run_serial on the seeded
    scene: no report, and its records -- the result, the poses, the points and the flags -- equal the library's"""
    sc, ref = seeded
    exe = str(tmp_path / "test_ba_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_ba_sanitize.cpp"),
                           "-o", exe])
    kf, cam, olm, uv, octave = BC.arrays(sc["obs"])
    cc = PC.to_cams(mc, sc["cams"])
    nkf, ncams, nlm, nobs, nlev = len(sc["poses"]), len(sc["cams"]), len(sc["pts"]), len(kf), len(sc["sigma"])
    blob = struct.pack("<6i", nkf, ncams, nlm, nobs, nlev, 25)
    blob += np.array(sc["sigma"], np.float64).tobytes()
    blob += bytes(C.string_at(C.addressof(cc.cams), ncams * C.sizeof(mc._lib.TrackCam)))
    blob += np.array([p[0] for p in sc["poses"]], np.float64).tobytes() + np.array([p[1] for p in sc["poses"]], np.float64).tobytes()
    blob += np.array(sc["fixed"], np.uint8).tobytes() + np.array(sc["pts"], np.float64).tobytes()
    blob += kf.tobytes() + cam.tobytes() + olm.tobytes() + uv.tobytes() + octave.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bad=0" in out.stdout and not out.stderr, out.stdout + out.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    got = BC.run(mc, lm, sc)
    want = struct.pack("<2d4i", got.cost_initial, got.cost_final, got.status, got.iterations, got.n_inliers, got.n_obs)
    want += got.R.tobytes() + got.t.tobytes() + got.pts.tobytes() + got.inliers.astype(np.uint8).tobytes()
    assert raw == want
