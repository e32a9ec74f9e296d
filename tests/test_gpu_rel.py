"""The relative rig pose between two frames by RANSAC on a device store (LocalMap.relative_pose: k_rel_hypotheses, k_rel_score and
k_rel_pick in one submission): the device store == the host-only store == the plain-Python restatement (rel_ref.py, the solver's
pose through the mcorb_rel_solve hook), floats as raw bytes, no tolerance, no excluded case.  Compared: the model, sample[17], the
flags, the status and -- through the read-back -- the counts of all hypotheses.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_rel.py`):
LocalMap has no relative_pose."""
import pytest

import kfdb_cases as K
import pose_ref as P
import rel_cases as RC
import rel_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb.LocalMap, "relative_pose")
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.fixture(scope="module")
def big():
    """an 8-camera scene of 1 025 matches with N(0, 0.1 px), 10 % of them moved"""
    return RC.scene(8, 1025, 21, moved=0.1)


def three_ways(mc, lms, cams, matches, what, threshold=RC.THRESHOLD, max_iterations=100, seed=0):
    """the device store and the host-only store against the restatement -> the restatement"""
    ref = RR.ransac(cams, matches, threshold, RC.solver_of(mc, cams), max_iterations, seed)
    for lm, who in zip(lms, ("device store", "host-only store")):
        got = RC.run(mc, lm, cams, matches, threshold, max_iterations, seed)
        RC.same(got, ref, "%s: %s" % (what, who))
        if ref["status"] != RR.NO_OBS:
            RC.same_counts(lm, ref, "%s: %s" % (what, who))
    return ref


@pytest.mark.parametrize("size", [0, 16, 17, 18, 63, 64, 65, 255, 256, 257, 1025])
def test_match_counts(mc, lms, big, size):
    """below a sample, a sample, either side of a wave, of a workgroup's tile and of four tiles"""
    cams, truth, matches, moved = big
    ref = three_ways(mc, lms, cams, matches[:size], "%d matches" % size)
    assert ref["status"] == (RR.NO_OBS if size == 0 else RR.NO_MODEL if size == 16 else RR.OK)
    assert len(ref["inliers"]) == size


@pytest.mark.parametrize("its", [1, 63, 64, 65, 100, 1025])
def test_max_iterations(mc, lms, big, its):
    """either side of a wave of hypotheses and of k_rel_score's blocks of them; the arg-max over five trips of k_rel_pick's lanes"""
    cams, truth, matches, moved = big
    ref = three_ways(mc, lms, cams, matches[:130], "%d hypotheses" % its, max_iterations=its)
    assert len(ref["counts"]) == its and ref["n_models"] == its and ref["status"] == RR.OK


def test_the_most_hypotheses(mc, lms, big):
    """MCORB_REL_MAX_ITERATIONS hypotheses on 64 matches: the 14 bits of the key, 64 trips of the pick"""
    cams, truth, matches, moved = big
    ref = three_ways(mc, lms, cams, matches[:64], "16 384 hypotheses", max_iterations=mc.REL_MAX_ITERATIONS)
    assert len(ref["counts"]) == 16384 and ref["status"] == RR.OK
    assert ref["best"] == ref["counts"].index(max(ref["counts"]))


@pytest.mark.parametrize("ncams", [1, 4, 16])
def test_rigs(mc, lms, ncams):
    cams, truth, matches, moved = RC.scene(ncams, 200, 30 + ncams, moved=0.1)
    assert set(m[0] for m in matches) == set(range(ncams))
    ref = three_ways(mc, lms, cams, matches, "%d cameras" % ncams)
    if ncams == 1:      # a central rig: the scale is not observable
        assert ref["status"] == RR.NO_MODEL and ref["n_models"] == 0
    else:
        assert ref["status"] == RR.OK and ref["n_models"] == 100


def test_hand_built_rows_in_one_launch(mc, lms):
    """the rows of test_rel_cpu.py: a threshold equal to a match's score (no inlier), the next double above (an inlier), a NaN
    row, in one launch each; and S = 17, where all counts tie and hypothesis 0 wins"""
    from test_rel_cpu import nan_rows, threshold_rows
    cams, matches, k, sc, model = threshold_rows(mc)
    at = three_ways(mc, lms, cams, matches, "threshold = the score", threshold=sc, max_iterations=1)
    above = three_ways(mc, lms, cams, matches, "the next double", threshold=RR.next_up(sc), max_iterations=1)
    assert not at["inliers"][k] and above["inliers"][k]
    cams, matches = nan_rows()
    wide = three_ways(mc, lms, cams, matches, "a NaN row", threshold=1.5, max_iterations=60)
    assert wide["status"] == RR.OK and not wide["inliers"][7] and any(7 in s for s in wide["samples"])
    cams, truth, matches, moved = RC.scene(8, 17, 3, moved=0.0, noise=0.0)
    tie = three_ways(mc, lms, cams, matches, "S = 17", threshold=1e-9, max_iterations=40)
    assert all(c == 17 for c in tie["counts"]) and tie["best"] == 0


def test_no_obs_no_model_and_timing(mc, lms, big):
    """the three timings are positive after a launch; NO_OBS launches nothing and leaves them; NO_MODEL is a launch"""
    cams, truth, matches, moved = big
    RC.run(mc, lms[0], cams, matches[:300])
    us, nh = lms[0].last_relative_timing()
    assert all(v > 0 for v in us) and nh == 100
    print("k_rel_hypotheses %.1f us, k_rel_score %.1f us, k_rel_pick %.1f us: 300 matches, 100 hypotheses" % us)
    got = RC.run(mc, lms[0], cams, [], max_iterations=7)
    assert got.status == RR.NO_OBS and lms[0].last_relative_timing() == (us, nh)
    ref = three_ways(mc, lms, cams, matches[:16], "S = 16", max_iterations=5)
    assert ref["status"] == RR.NO_MODEL
    us2, nh2 = lms[0].last_relative_timing()
    assert nh2 == 5 and all(v > 0 for v in us2)
    got = RC.run(mc, lms[0], cams, matches[:16], max_iterations=5)
    assert P.same_bits(got.R.tolist(), RR.IDENT[0]) and got.t.tolist() == [0.0] * 3 and not got.inliers.any()
    assert lms[1].last_relative_timing()[0] == (0.0, 0.0, 0.0)


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_rel_cpu.py, a pending tracking call among them, the store read back unchanged"""
    from test_rel_cpu import check_refusals
    check_refusals(mc, lms[0])
