"""The RANSAC with the rig solver on a device store (LocalMap.ransac_pose(..., solver="rig"): k_sac_hypotheses_rig, four lanes per
hypothesis, in k_sac_hypotheses' place; k_sac_score, k_sac_pick and, with a refinement, k_pose_refine as they were, in one
submission): the device store == the host-only store == the plain-Python restatement (sac_rig_ref.py, the solver's poses through
the mcorb_sac_solve_rig hook), floats as raw bytes, no tolerance, no excluded case.

On the commit before the solver existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_sac_rig.py`):
ransac_pose has no `solver`."""
import inspect

import numpy as np
import pytest

import kfdb_cases as K
import pose_cases as PC
import pose_ref as P
import sac_cases as SC
import sac_ref as S
import sac_rig_cases as RC
import sac_rig_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    assert "solver" in inspect.signature(mc.LocalMap.ransac_pose).parameters
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.fixture(scope="module")
def big():
    """a 4-camera scene of more than 257 matches, 40 % of them moved"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=280, seed=13)
    assert match[-1] + 1 >= 257
    return cams, truth, obs, match, moved


def prefix(obs, match, n_matches):
    """the observations of the first n_matches matches"""
    n = next((i for i, k in enumerate(match) if k >= n_matches), len(obs))
    return obs[:n], match[:n]


def three_ways(mc, lms, cams, obs, what, threshold=SC.THRESHOLD, match=None, max_iterations=100, seed=0, forms=("pts", "lids")):
    """the device store and the host-only store, both forms, against the restatement: the model, sample[4], the flags, the status
    and -- through the debug read-back -- the counts of all hypotheses -> the restatement"""
    ref = R.ransac(cams, obs, threshold, RC.solver_of(mc, cams), match, max_iterations, seed)
    for lm, who in zip(lms, ("device store", "host-only store")):
        for form in forms:
            got = RC.run(mc, lm, cams, obs, "rig", threshold, match, max_iterations, seed, form=form)
            SC.same_plain(got, ref, "%s: %s, %s" % (what, who, form))
            if ref["status"] != S.NO_OBS:
                count, valid = lm.last_ransac_counts()
                assert valid.tolist() == [m is not None for m in ref["models"]], (what, who, form, "models")
                assert count.tolist() == [c or 0 for c in ref["counts"]], (what, who, form, "counts")
    return ref


@pytest.mark.parametrize("size", [0, 3, 4, 5, 63, 64, 65, 257])
def test_consensus_sizes(mc, lms, big, size):
    """below a sample, a sample, either side of a wave and of k_sac_score's tile"""
    cams, truth, obs, match, moved = big
    o, m = prefix(obs, match, size)
    ref = three_ways(mc, lms, cams, o, "%d matches" % size, match=m, forms=("pts",) if size == 0 else ("pts", "lids"))
    assert ref["n_consensus"] == size
    assert ref["status"] == (S.NO_OBS if size == 0 else S.NO_MODEL if size == 3 else S.OK)
    if size >= 63:
        cons = S.consensus(o, m)[0]
        assert all(ref["flags"][i] == (not moved[i]) for i in cons)


@pytest.mark.parametrize("its", [1, 15, 16, 17, 64, 100, 1024])
def test_max_iterations(mc, lms, big, its):
    """either side of a wave of 16 quads, a quad alone, four waves exactly, a last wave with four quads, 64 full waves"""
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


def test_thin_scene(mc, lms):
    """16 x 3 observations (test_sac_rig_cpu.py's): the central solver has no model on either store, the rig solver's winner has
    exactly the unmoved observations as inliers; and the four observations spread one per camera"""
    cams, truth, obs, match, moved = RC.thin_scene(16)
    for lm in lms:
        got = RC.run(mc, lm, cams, obs, "central", match=match)
        assert got.status == S.NO_MODEL and got.n_models == 0
    ref = three_ways(mc, lms, cams, obs, "16 x 3", match=match)
    assert ref["status"] == S.OK and ref["flags"] == [not v for v in moved]
    cams, truth, obs, match, moved = RC.thin_scene(4, per_cam=1, moved=0.0, noise=0.0)
    ref = three_ways(mc, lms, cams, obs, "one per camera")
    assert ref["status"] == S.OK and ref["n_inliers"] == 4
    assert any(m is None for m in ref["models"]) or ref["n_models"] == 100      # (hypotheses whose draws ran out are among them, or none)


@pytest.mark.parametrize("per_match", [1, 2, 16])
def test_match_forms(mc, lms, per_match):
    cams, truth, obs, match, moved = SC.scene(4, nlm=40, seed=7, per_match=per_match)
    ref = three_ways(mc, lms, cams, obs, "%d per match" % per_match, match=match)
    assert ref["n_consensus"] == match[-1] + 1 and ref["status"] == S.OK
    if per_match == 1:
        three_ways(mc, lms, cams, obs, "no match array", match=None)


def test_more_than_one_root_and_ties(mc, lms, big):
    """the quad's pick: hypotheses with two or more surviving roots are among those compared above, the pick being a later root in
    some; and S = 4 in one camera, exact, where every model has all four as inliers and the lowest hypothesis with a model wins"""
    cams, truth, obs, match, moved = big
    o, m = prefix(obs, match, 130)
    ref = three_ways(mc, lms, cams, o, "roots", match=m, forms=("pts",))
    solve = RC.solver_of(mc, cams)
    cand = [R.candidates(cams, o, s, solve) for s in ref["samples"]]
    many = [c for c in cand if len(c) >= 2]
    later = [c for c in many if min(range(len(c)), key=lambda k: (c[k][1], k)) > 0]
    assert len(many) >= 1 and len(later) >= 1, (len(many), len(later))
    ref = three_ways(mc, lms, PC.flat_rig(), SC.square(), "S = 4", threshold=1e-9)
    with_model = [h for h, c in enumerate(ref["counts"]) if c is not None]
    assert len(with_model) >= 2 and all(ref["counts"][h] == 4 for h in with_model) and ref["best"] == with_model[0]


def test_no_model_no_obs_and_timing(mc, lms, big):
    """the three timings are positive after a launch; NO_OBS launches nothing and leaves them; NO_MODEL is a launch"""
    cams, truth, obs, match, moved = big
    o, m = prefix(obs, match, 257)
    RC.run(mc, lms[0], cams, o, match=m)
    us, nh = lms[0].last_ransac_timing()
    assert all(v > 0 for v in us) and nh == 100
    print("k_sac_hypotheses_rig %.1f us, k_sac_score %.1f us, k_sac_pick %.1f us: 257 matches, 100 hypotheses" % us)
    got = RC.run(mc, lms[0], cams, [], max_iterations=7)
    assert got.status == S.NO_OBS and lms[0].last_ransac_timing() == (us, nh)
    ref = three_ways(mc, lms, cams, o[:3], "S = 3", max_iterations=5)
    assert ref["status"] == S.NO_MODEL
    us2, nh2 = lms[0].last_ransac_timing()
    assert nh2 == 5 and all(v > 0 for v in us2)
    got = RC.run(mc, lms[0], cams, o[:3], max_iterations=5)
    assert P.same_bits(got.R.tolist(), S.IDENT[0]) and got.t.tolist() == [0.0] * 3 and not got.inliers.any()
    assert lms[1].last_ransac_timing()[0] == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("ncams", [4, 16])
def test_with_refinement(mc, lms, ncams):
    """the refinement part equals refine_pose on the device store from the returned RANSAC pose; both stores and the restatement
    agree on everything.  4 cameras: 300 landmarks, two observations per match, used = 1; 16 cameras: the thin scene"""
    cams, truth, obs, match, moved = SC.scene(4, nlm=300, seed=44, per_match=2) if ncams == 4 else RC.thin_scene(16)
    sac, ref, final = R.ransac_refine(cams, obs, SC.THRESHOLD, RC.solver_of(mc, cams), PC.INV_SIGMA2, match, 100, 0)
    assert sac["status"] == S.OK and (ncams == 16 or final["used"] == 1)
    for lm, who in zip(lms, ("device store", "host-only store")):
        for form in ("pts", "lids"):
            got = RC.run(mc, lm, cams, obs, match=match, refine=(PC.INV_SIGMA2,), form=form)
            SC.same(got, sac, who)
            SC.same_final(got, final, who)
            explicit = PC.refine(mc, lm, cams, (got.sac_R.tolist(), got.sac_t.tolist()), obs, form=form)
            PC.same(dict(PC.as_ref(explicit), inliers=ref["inliers"]), ref, who + ": explicit refine_pose")
            for f in ("R", "t", "cost_initial", "cost_final"):
                assert P.same_bits(np.asarray(getattr(got.refine, f)).tolist(), np.asarray(getattr(explicit, f)).tolist()), (who, f)
            assert (got.refine.status, got.refine.iterations, got.refine.n_inliers, got.refine.n_obs) == \
                (explicit.status, explicit.iterations, explicit.n_inliers, explicit.n_obs)
            assert explicit.inliers.tolist() == [bool(v) for v in ref["inliers"]]


def test_refusals_on_a_device_store(mc, lms):
    """the refusals of test_sac_rig_cpu.py, a pending tracking call among them, the store read back unchanged"""
    from test_sac_rig_cpu import check_refusals
    check_refusals(mc, lms[0])
