"""The local bundle adjustment on a device store (LocalMap.bundle_adjust: the chain of k_ba_* kernels in one submission): the
device store == the host-only store == the plain-Python restatement (ba_ref.py), floats as raw bytes, no tolerance, no excluded
case.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_ba.py`): LocalMap
has no bundle_adjust."""
import numpy as np
import pytest

import ba_cases as BC
import ba_ref as B
import kfdb_cases as K
import pose_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    assert hasattr(mc.LocalMap, "bundle_adjust")
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


def three_ways(mc, lms, sc, what, max_iterations=25, forms=("pts", "lids")):
    """the device store and the host-only store, both forms, against the restatement -> the restatement"""
    ref = BC.ref(sc, max_iterations)
    for lm, who in zip(lms, ("device store", "host-only store")):
        for form in forms:
            got = BC.run(mc, lm, sc, max_iterations, form)
            BC.same(BC.as_ref(got), ref, "%s: %s, %s" % (what, who, form))
            assert got.n_obs == len(sc["obs"])
    return ref


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_landmark_counts(mc, lms, n):
    """either side of a wave, of the fold's workgroup and of four trips of its lanes; at most 3 observations per landmark keep
    the restatement short, and 1025 landmarks run 3 solves"""
    sc = BC.scene(nlm=n, seed=30 + n % 7, max_views=3)
    ref = three_ways(mc, lms, sc, "%d landmarks" % n, max_iterations=3 if n == 1025 else 25)
    assert ref["status"] == (B.NO_OBS if n == 0 else ref["status"])
    if 63 <= n < 1025:
        assert ref["status"] == B.CONVERGED


@pytest.mark.parametrize("nkf", [1, 2, 3, 16])
def test_keyframe_counts(mc, lms, nkf):
    """one free keyframe alone, one and two free beside a fixed one, and the full window: 14 free keyframes, 84 unknowns, 105
    pairs"""
    sc = BC.scene(nkf=nkf, nlm=40, nfixed={1: 0, 2: 1, 3: 1, 16: 2}[nkf], seed=40 + nkf, spacing=0.3 if nkf < 16 else 0.1)
    assert set(o[0] for o in sc["obs"]) == set(range(nkf))
    ref = three_ways(mc, lms, sc, "%d keyframes" % nkf, max_iterations=4 if nkf == 16 else 25, forms=("pts",))
    assert ref["status"] in (B.CONVERGED, B.MAX_ITER) and ref["cost_final"] < ref["cost_initial"]


@pytest.mark.parametrize("ncams", [1, 4, 16])
def test_rigs(mc, lms, ncams):
    sc = BC.scene(ncams=ncams, nlm=60, seed=50 + ncams, skew=0.2)
    assert set(o[1] for o in sc["obs"]) == set(range(ncams))
    ref = three_ways(mc, lms, sc, "%d cameras" % ncams, forms=("pts",))
    assert ref["status"] in (B.CONVERGED, B.MAX_ITER) and ref["cost_final"] < ref["cost_initial"]


def test_hand_written_rows_in_one_launch(mc, lms):
    """the rows of test_ba_cpu.py: q.z of 0.0, -0.0, 1e-300, -1e-300 and NaN; whitened e one ulp under k, exactly k and one ulp
    above, under two sigmas; the whitened chi2 exactly 5.991 and the next double above, under two sigmas"""
    for with_nan in (True, False):
        for extra in ((), (1,)):
            sc = BC.hand_scene(PC.z_rows(with_nan) + BC.huber_rows(1.0), fixed=not extra, extra_kf=extra)
            three_ways(mc, lms, sc, "z and Huber rows, NaN %s, keyframes %d" % (with_nan, 1 + len(extra)))
    for s in (1.0, 0.25):
        ref = three_ways(mc, lms, BC.hand_scene(BC.huber_rows(s), sigma=(s,)), "Huber rows, sigma %g" % s)
        assert ref["status"] == B.CONVERGED
    rows, sigma, flags = BC.chi2_rows()
    ref = three_ways(mc, lms, BC.hand_scene(rows, sigma=sigma), "chi2 rows")
    assert ref["status"] == B.NO_STEP and ref["inliers"] == flags


@pytest.mark.parametrize("case", range(7))
def test_degenerate(mc, lms, case):
    name, sc, check = BC.degenerate()[case]
    check(sc, three_ways(mc, lms, sc, name))


@pytest.mark.parametrize("its", [1, 100])
def test_max_iterations(mc, lms, its):
    sc = BC.scene(nlm=30, seed=21)
    ref = three_ways(mc, lms, sc, "max_iterations %d" % its, max_iterations=its)
    assert ref["status"] == (B.MAX_ITER if its == 1 else B.CONVERGED) and (its != 1 or ref["iterations"] == 1)
    us, idle = lms[0].last_ba_timing()
    assert idle == 5 * (its - ref["iterations"])


def test_points_moved_just_before_the_call(mc, lms):
    """the chain gathers the points from the store's HBM state, not from a host copy: update_points, then bundle_adjust by lids"""
    sc = BC.scene(nlm=50, seed=23)
    new = np.array(sc["pts"]) + np.random.default_rng(3).normal(scale=0.02, size=(len(sc["pts"]), 3))
    sc_new = dict(sc, pts=new.tolist())
    ref_old, ref_new = BC.ref(sc), BC.ref(sc_new)
    assert BC.flat([ref_old["t"]]) != BC.flat([ref_new["t"]])
    for lm, who in zip(lms, ("device store", "host-only store")):
        BC.same(BC.as_ref(BC.run(mc, lm, sc, form="lids", first_lid=1500)), ref_old, who + ", before")
        lids = np.arange(1500, 1500 + len(new), dtype=np.int32)
        upd, _ = lm.update_points(lids, new, max_diff=5.0)
        assert upd.all()
        kf, cam, olm, uv, octave = BC.arrays(sc["obs"])
        got = lm.bundle_adjust(PC.to_cams(mc, sc["cams"]), [p[0] for p in sc["poses"]], [p[1] for p in sc["poses"]], sc["fixed"], kf, cam,
                               olm, uv, octave, sc["sigma"], lids=lids)
        BC.same(BC.as_ref(got), ref_new, who + ", after")
        assert np.array_equal(np.array([lm.get(int(l))[0] for l in lids]), new)      # the store is not written


def test_timing(mc, lms):
    """positive after a launch, unchanged by a call without observations (which launches nothing)"""
    sc = BC.scene(nlm=100, seed=24)
    BC.run(mc, lms[0], sc)
    us, idle = lms[0].last_ba_timing()
    assert all(u > 0 for u in us) and idle > 0
    BC.run(mc, lms[0], dict(sc, obs=[]))
    assert lms[0].last_ba_timing() == (us, idle)
    assert lms[1].last_ba_timing() == ((0.0,) * 7, 0)
    print("bundle_adjust, 100 landmarks, spans in us: %s, idle launches %d" % (", ".join("%.1f" % u for u in us), idle))


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_ba_cpu.py, the store read back unchanged"""
    from test_ba_cpu import check_refusals
    check_refusals(mc, lms[0])
