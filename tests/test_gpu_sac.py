"""The absolute rig pose by RANSAC on a device store (LocalMap.ransac_pose: k_sac_hypotheses, k_sac_score, k_sac_pick and, with a
refinement, k_pose_refine in one submission): the device store == the host-only store == the plain-Python restatement
(sac_ref.py, the solver's poses through the mcorb_sac_solve hook), floats as raw bytes, no tolerance, no excluded case.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_sac.py`):
LocalMap has no ransac_pose."""
import math

import numpy as np
import pytest

import kfdb_cases as K
import pose_cases as PC
import pose_ref as P
import sac_cases as SC
import sac_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    assert hasattr(mc.LocalMap, "ransac_pose")
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.fixture(scope="module")
def big():
    """a 4-camera scene of more than 1 025 matches, 40 % of them moved"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=1040, seed=13)
    assert match[-1] + 1 >= 1025
    return cams, truth, obs, match, moved


def prefix(obs, match, n_matches):
    """the observations of the first n_matches matches"""
    n = next((i for i, k in enumerate(match) if k >= n_matches), len(obs))
    return obs[:n], match[:n]


def three_ways(mc, lms, cams, obs, what, threshold=SC.THRESHOLD, match=None, max_iterations=100, seed=0, forms=("pts", "lids"), ref=None):
    """the device store and the host-only store, both forms, against the restatement: the model, sample[4], the flags, the status
    and -- through the debug read-back -- the counts of all hypotheses -> the restatement"""
    if ref is None:
        ref = S.ransac(cams, obs, threshold, SC.solver_of(mc, cams), match, max_iterations, seed)
    for lm, who in zip(lms, ("device store", "host-only store")):
        for form in forms:
            got = SC.run(mc, lm, cams, obs, threshold, match, max_iterations, seed, form=form)
            SC.same_plain(got, ref, "%s: %s, %s" % (what, who, form))
            if ref["status"] != S.NO_OBS:
                count, valid = lm.last_ransac_counts()
                assert valid.tolist() == [m is not None for m in ref["models"]], (what, who, form, "models")
                assert count.tolist() == [c or 0 for c in ref["counts"]], (what, who, form, "counts")
    return ref


@pytest.mark.parametrize("size", [0, 3, 4, 63, 64, 65, 255, 256, 257, 1025])
def test_consensus_sizes(mc, lms, big, size):
    """below a sample, either side of a wave, of a workgroup's tile and of four tiles"""
    cams, truth, obs, match, moved = big
    o, m = prefix(obs, match, size)
    ref = three_ways(mc, lms, cams, o, "%d matches" % size, match=m, forms=("pts",) if size == 0 else ("pts", "lids"))
    assert ref["n_consensus"] == size
    # (four matches of this 4-camera scene: no camera has four consensus observations)
    assert ref["status"] == (S.NO_OBS if size == 0 else S.NO_MODEL if size in (3, 4) else S.OK)
    if size >= 63:
        cons = S.consensus(o, m)[0]
        assert all(ref["flags"][i] == (not moved[i]) for i in cons)


@pytest.mark.parametrize("its", [1, 63, 64, 65, 100, 1024])
def test_max_iterations(mc, lms, big, its):
    """either side of a wave of hypotheses and of k_sac_score's blocks of them; the arg-max over four trips of k_sac_pick's lanes"""
    cams, truth, obs, match, moved = big
    o, m = prefix(obs, match, 130)
    ref = three_ways(mc, lms, cams, o, "%d hypotheses" % its, match=m, max_iterations=its, forms=("lids",))
    assert len(ref["counts"]) == its and (its == 1 or ref["status"] == S.OK)


@pytest.mark.parametrize("ncams", [1, 4, 16])
def test_rigs(mc, lms, ncams):
    cams, truth, obs, match, moved = SC.scene(ncams, nlm=200, seed=20 + ncams)
    assert set(o[0] for o in obs) == set(range(ncams))
    ref = three_ways(mc, lms, cams, obs, "%d cameras" % ncams, match=match)
    cons = S.consensus(obs, match)[0]
    assert ref["status"] == S.OK and all(ref["flags"][i] == (not moved[i]) for i in cons)


@pytest.mark.parametrize("per_match", [1, 2, 16])
def test_match_forms(mc, lms, per_match):
    cams, truth, obs, match, moved = SC.scene(4, nlm=40, seed=7, per_match=per_match)
    ref = three_ways(mc, lms, cams, obs, "%d per match" % per_match, match=match)
    assert ref["n_consensus"] == match[-1] + 1 and ref["status"] == S.OK
    if per_match == 1:
        three_ways(mc, lms, cams, obs, "no match array", match=None)


def test_points_moved_just_before_the_call(mc, lms):
    """the kernels gather the points from the store's HBM state, not from a host copy: update_points, then ransac_pose by lids"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=120, seed=31)
    cam, uv, octave, pts = PC.arrays(obs)
    new = pts + np.random.default_rng(3).normal(scale=0.002, size=pts.shape)
    moved_obs = [(o[0], o[1], o[2], o[3], new[i].tolist()) for i, o in enumerate(obs)]
    ref_old = S.ransac(cams, obs, SC.THRESHOLD, SC.solver_of(mc, cams), match, 100, 0)
    ref_new = S.ransac(cams, moved_obs, SC.THRESHOLD, SC.solver_of(mc, cams), match, 100, 0)
    assert ref_old["status"] == ref_new["status"] == S.OK and not P.same_bits(ref_old["t"], ref_new["t"])
    for lm, who in zip(lms, ("device store", "host-only store")):
        lids = PC.fill_points(lm, obs, first_lid=1500)
        cc = PC.to_cams(mc, cams)
        SC.same_plain(lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match), ref_old, who + ", before")
        upd, _ = lm.update_points(lids, new, max_diff=5.0)
        assert upd.all()
        SC.same_plain(lm.ransac_pose(cc, cam, uv, octave, SC.THRESHOLD, lids=lids, match=match), ref_new, who + ", after")


def test_hand_built_rows_in_one_launch(mc, lms):
    """the rows of test_sac_cpu.py: a threshold equal to an observation's score (no inlier), the next double above (an inlier), a
    NaN score from a point at the camera centre, in one launch each; and S = 4, where all counts tie and the lowest hypothesis
    with a model wins"""
    from test_sac_cpu import threshold_rows
    rig, obs, seed, sc, model = threshold_rows(mc)
    at = three_ways(mc, lms, rig, obs, "threshold = the score", threshold=sc, max_iterations=1, seed=seed)
    above = three_ways(mc, lms, rig, obs, "the next double", threshold=S.next_up(sc), max_iterations=1, seed=seed)
    assert at["flags"] == [True] * 4 + [False, False] and above["flags"] == [True] * 5 + [False]
    many = three_ways(mc, lms, rig, obs, "64 hypotheses on the rows", threshold=S.next_up(sc), max_iterations=64, seed=seed)
    # (hypotheses that draw the point at the camera centre, some as one of the solver's three, are among them)
    assert many["status"] == S.OK and sum(1 for smp in many["samples"] if 5 in smp[:3]) >= 3
    ref = three_ways(mc, lms, PC.flat_rig(), SC.square(), "S = 4", threshold=1e-9)
    with_model = [h for h, c in enumerate(ref["counts"]) if c is not None]
    assert len(with_model) >= 2 and all(ref["counts"][h] == 4 for h in with_model) and ref["best"] == with_model[0]


def test_no_model_no_obs_and_timing(mc, lms, big):
    """the three timings are positive after a launch; NO_OBS launches nothing and leaves them; NO_MODEL is a launch"""
    cams, truth, obs, match, moved = big
    o, m = prefix(obs, match, 300)
    SC.run(mc, lms[0], cams, o, match=m)
    us, nh = lms[0].last_ransac_timing()
    assert all(v > 0 for v in us) and nh == 100
    print("k_sac_hypotheses %.1f us, k_sac_score %.1f us, k_sac_pick %.1f us: 300 matches, 100 hypotheses" % us)
    got = SC.run(mc, lms[0], cams, [], max_iterations=7)
    assert got.status == S.NO_OBS and lms[0].last_ransac_timing() == (us, nh)
    three = SC.square()[:3]
    ref = three_ways(mc, lms, PC.flat_rig(), three, "S = 3", max_iterations=5)
    assert ref["status"] == S.NO_MODEL
    us2, nh2 = lms[0].last_ransac_timing()
    assert nh2 == 5 and all(v > 0 for v in us2)
    got = SC.run(mc, lms[0], PC.flat_rig(), three, max_iterations=5)
    assert P.same_bits(got.R.tolist(), S.IDENT[0]) and got.t.tolist() == [0.0] * 3 and not got.inliers.any()
    assert lms[1].last_ransac_timing()[0] == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("ncams", [1, 4])
def test_with_refinement(mc, lms, ncams):
    """used = 1; the refinement part equals refine_pose on the device store from the returned RANSAC pose; both stores and the
    restatement agree on everything"""
    cams, truth, obs, match, moved = SC.scene(ncams, nlm=300, seed=40 + ncams, per_match=2)
    sac, ref, final = S.ransac_refine(cams, obs, SC.THRESHOLD, SC.solver_of(mc, cams), PC.INV_SIGMA2, match, 100, 0)
    assert final["used"] == 1
    for lm, who in zip(lms, ("device store", "host-only store")):
        for form in ("pts", "lids"):
            got = SC.run(mc, lm, cams, obs, match=match, refine=(PC.INV_SIGMA2,), form=form)
            SC.same(got, sac, who)
            SC.same_final(got, final, who)
            explicit = PC.refine(mc, lm, cams, (got.sac_R.tolist(), got.sac_t.tolist()), obs, form=form)
            PC.same(dict(PC.as_ref(explicit), inliers=ref["inliers"]), ref, who + ": explicit refine_pose")
            for f in ("R", "t", "cost_initial", "cost_final"):
                assert P.same_bits(np.asarray(getattr(got.refine, f)).tolist(), np.asarray(getattr(explicit, f)).tolist()), (who, f)
            assert (got.refine.status, got.refine.iterations, got.refine.n_inliers, got.refine.n_obs) == \
                (explicit.status, explicit.iterations, explicit.n_inliers, explicit.n_obs)
            assert explicit.inliers.tolist() == [bool(v) for v in ref["inliers"]]


def test_refinement_culls_a_match_the_ransac_kept(mc, lms):
    """the rule of FrontEnd.cpp:4786 on both stores: used = 0 (the case of test_sac_cpu.py)"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=60, seed=9, moved=0.0)
    obs = [(c, PC.f32(kx + 5.0) if i % 9 == 4 and i < 72 else kx, ky, 0, X) for i, (c, kx, ky, o, X) in enumerate(obs)]
    thr = 1.0 - math.cos(16.0 / 500.0)
    sac, ref, final = S.ransac_refine(cams, obs, thr, SC.solver_of(mc, cams), PC.INV_SIGMA2, match, 100, 0)
    assert final["used"] == 0
    for lm, who in zip(lms, ("device store", "host-only store")):
        got = SC.run(mc, lm, cams, obs, thr, match=match, refine=(PC.INV_SIGMA2,))
        SC.same(got, sac, who)
        SC.same_final(got, final, who)
        assert got.used == 0 and got.refine.n_inliers == ref["n_inliers"] < len(obs)


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_sac_cpu.py, a pending tracking call among them, the store read back unchanged"""
    from test_sac_cpu import check_refusals
    check_refusals(mc, lms[0])
