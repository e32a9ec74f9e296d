"""The rig pose refinement on a device store (LocalMap.refine_pose: k_pose_refine, one workgroup for both rounds): the device
store == the host-only store == the plain-Python restatement (pose_ref.py), floats as raw bytes, no tolerance, no excluded case.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_pose.py`):
LocalMap has no refine_pose."""
import numpy as np
import pytest

import kfdb_cases as K
import pose_cases as PC
import pose_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    assert hasattr(mc.LocalMap, "refine_pose")
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.fixture(scope="module")
def big():
    """a 4-camera scene of more than 1025 observations, a fifth of them moved"""
    cams, truth, init, obs, moved = PC.scene(4, nlm=280, seed=9)
    assert len(obs) >= 1025
    return cams, truth, init, obs, moved


def three_ways(mc, lms, cams, init, obs, what, inv_sigma2=PC.INV_SIGMA2, max_iterations=25, forms=("pts", "lids")):
    """the device store and the host-only store, both forms, against the restatement -> the restatement"""
    ref = P.refine(cams, init, obs, inv_sigma2, max_iterations)
    for lm, who in zip(lms, ("device store", "host-only store")):
        for form in forms:
            got = PC.refine(mc, lm, cams, init, obs, inv_sigma2, max_iterations, form)
            PC.same(PC.as_ref(got), ref, "%s: %s, %s" % (what, who, form))
            assert got.n_obs == len(obs)
    return ref


@pytest.mark.parametrize("n", [0, 1, 5, 6, 63, 64, 65, 255, 256, 257, 1025])
def test_observation_counts(mc, lms, big, n):
    """below and above the 6 unknowns, either side of a wave, of the workgroup and of four trips of its lanes"""
    cams, truth, init, obs, moved = big
    ref = three_ways(mc, lms, cams, init, obs[:n], "%d observations" % n)
    assert ref["status"] == (P.NO_OBS if n == 0 else ref["status"])
    if n >= 63:
        assert ref["status"] == P.CONVERGED and [ref["inliers"][i] for i in range(n)] == [not m for m in moved[:n]]


@pytest.mark.parametrize("ncams", [1, 4, 16])
def test_rigs(mc, lms, ncams):
    cams, truth, init, obs, moved = PC.scene(ncams, nlm=max(20, 160 // ncams), seed=20 + ncams)
    assert set(o[0] for o in obs) == set(range(ncams))
    ref = three_ways(mc, lms, cams, init, obs, "%d cameras" % ncams)
    assert ref["status"] == P.CONVERGED and ref["inliers"] == [not m for m in moved]


def test_hand_written_rows_in_one_launch(mc, lms):
    """the rows of test_pose_cpu.py: q.z of 0.0, -0.0, 1e-300, -1e-300 and NaN; e one ulp under k, exactly k and one ulp above --
    one problem with the NaN row (every cost is NaN: nothing is accepted) and one without (the loop runs); then the chi2 rows:
    exactly 5.991, the next double above, octaves with different inv_sigma2"""
    rig = PC.flat_rig()
    for with_nan in (True, False):
        obs = PC.z_rows(with_nan) + PC.huber_rows()
        ref = three_ways(mc, lms, rig, PC.IDENT, obs, "z and Huber rows, NaN %s" % with_nan)
        assert (ref["status"] == P.NO_STEP) == with_nan
        assert [ref["inliers"][i] for i in range(6, 10)] == [False] * 4
    ref = three_ways(mc, lms, rig, PC.IDENT, PC.huber_rows(), "Huber rows")
    assert ref["status"] == P.CONVERGED
    obs, inv, flags = PC.chi2_rows()
    ref = three_ways(mc, lms, rig, PC.IDENT, obs, "chi2 rows", inv_sigma2=inv)
    assert ref["status"] == P.NO_STEP and ref["inliers"] == flags


def test_degenerate(mc, lms, big):
    cams, truth, init, obs, moved = big
    for n in (2, 3):
        three_ways(mc, lms, cams, init, obs[:n], "%d observations" % n)
    ref = three_ways(mc, lms, PC.flat_rig(), PC.IDENT, [(0, 3.0, 4.0, 0, [3.0, 4.0, 1.0])], "an exact observation")
    assert ref["status"] == P.NO_STEP
    behind = [(c, kx, ky, o, [-v for v in X]) for c, kx, ky, o, X in PC.z_rows(False)[:6]]
    ref = three_ways(mc, lms, PC.flat_rig(), PC.IDENT, behind, "all behind the rig")
    assert ref["status"] == P.NO_STEP and ref["n_inliers"] == 0
    bad = ([row[:] for row in init[0]], init[1][:])
    bad[0][1][2] = float("nan")
    ref = three_ways(mc, lms, cams, bad, obs[:70], "a NaN initial pose")
    assert ref["status"] == P.NO_STEP and P.same_bits(ref["R"], bad[0])


@pytest.mark.parametrize("its", [1, 100])
def test_max_iterations(mc, lms, big, its):
    cams, truth, init, obs, moved = big
    ref = three_ways(mc, lms, cams, init, obs[:130], "max_iterations %d" % its, max_iterations=its)
    assert ref["status"] == (P.MAX_ITER if its == 1 else P.CONVERGED) and ref["iterations"] == ((1, 1) if its == 1 else ref["iterations"])


def test_points_moved_just_before_the_call(mc, lms, big):
    """the kernel gathers the points from the store's HBM state, not from a host copy: update_points, then refine_pose by lids"""
    cams, truth, init, obs, moved = big
    obs = obs[:200]
    cam, uv, octave, pts = PC.arrays(obs)
    new = pts + np.random.default_rng(3).normal(scale=0.02, size=pts.shape)
    ref_old = P.refine(cams, init, obs, PC.INV_SIGMA2)
    ref_new = P.refine(cams, init, [(o[0], o[1], o[2], o[3], new[i].tolist()) for i, o in enumerate(obs)], PC.INV_SIGMA2)
    assert not P.same_bits(ref_old["t"], ref_new["t"])
    for lm, who in zip(lms, ("device store", "host-only store")):
        lids = PC.fill_points(lm, obs, first_lid=1500)
        cc = PC.to_cams(mc, cams)
        PC.same(PC.as_ref(lm.refine_pose(cc, init[0], init[1], cam, uv, octave, PC.INV_SIGMA2, lids=lids)), ref_old, who + ", before")
        upd, _ = lm.update_points(lids, new, max_diff=5.0)
        assert upd.all()
        PC.same(PC.as_ref(lm.refine_pose(cc, init[0], init[1], cam, uv, octave, PC.INV_SIGMA2, lids=lids)), ref_new, who + ", after")


def test_timing(mc, lms, big):
    """positive after a launch, unchanged by a call without observations (which launches nothing)"""
    cams, truth, init, obs, moved = big
    PC.refine(mc, lms[0], cams, init, obs[:300])
    us = lms[0].last_pose_timing()
    assert us > 0
    PC.refine(mc, lms[0], cams, init, [])
    assert lms[0].last_pose_timing() == us
    assert lms[1].last_pose_timing() == 0
    print("k_pose_refine, 300 observations: %.1f us" % us)


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_pose_cpu.py, the store read back unchanged"""
    from test_pose_cpu import check_refusals
    cams, truth, init, obs, moved = PC.scene()
    check_refusals(mc, lms[0], (cams, truth, init, obs, moved, None))
