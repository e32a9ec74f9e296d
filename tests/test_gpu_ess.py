"""The pose of one camera between two frames by five-point RANSAC on a device store (LocalMap.essential_pose: k_ess_hypotheses,
k_ess_score, k_ess_pick and k_ess_finish in one submission): the device store == the host-only store == the restatement
(ess_ref.py, the solver's models through the mcorb_ess_solve hook), doubles as raw bytes, no tolerance, no excluded case.
Compared: every slot's count, valid flag and model, E, R, t, the four cheirality counts, both inlier counts, the flags, sample[5],
best_hypothesis, best_root and the status.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_ess.py`):
LocalMap has no essential_pose."""
import math

import numpy as np
import pytest

import ess_cases as EC
import ess_ref as ER
import kfdb_cases as K
import rel_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb.LocalMap, "essential_pose")
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.fixture(scope="module")
def big():
    """a general scene of 1 025 matches with N(0, 0.1 px), 10 % of them moved"""
    return EC.scene("general", n=1025, seed=21, noise=0.1)


def three_ways(mc, lms, matches, what, **kw):
    """the device store and the host-only store against the restatement -> the restatement"""
    ref = ER.ransac(EC.CAM, matches, EC.solver_of(mc), **kw)
    got = []
    for lm, who in zip(lms, ("device store", "host-only store")):
        got.append(EC.run(mc, lm, matches, **kw))
        EC.same(got[-1], ref, "%s: %s" % (what, who))
        if ref["status"] != ER.NO_OBS:
            EC.same_counts(lm, ref, "%s: %s" % (what, who))
    EC.same_stores(got[0], got[1], what)
    return ref


@pytest.mark.parametrize("size", [0, 4, 5, 6, 63, 64, 65, 255, 256, 257, 1025])
def test_match_counts(mc, lms, big, size):
    """below a sample, a sample, either side of a wave, of a workgroup's tile and of four tiles"""
    truth, matches, moved = big
    ref = three_ways(mc, lms, matches[:size], "%d matches" % size)
    assert ref["status"] == (ER.NO_OBS if size == 0 else ER.NO_MODEL if size == 4 else ER.OK)
    assert len(ref["inliers"]) == size


@pytest.mark.parametrize("its", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1025])
def test_max_iterations(mc, lms, big, its):
    """either side of k_ess_hypotheses' four hypotheses per wave, of k_ess_score's blocks of 40 slots, of a wave and of several
    trips of k_ess_pick's lanes over the slots"""
    truth, matches, moved = big
    ref = three_ways(mc, lms, matches[:64], "%d hypotheses" % its, max_iterations=its)
    assert len(ref["counts"]) == 10 * its and ref["status"] == ER.OK


def test_the_most_hypotheses(mc, lms, big):
    """MCORB_ESS_MAX_ITERATIONS hypotheses on 64 matches: the 14 + 4 bits of the key, 640 trips of the pick, 4 096 blocks of slots.
    Among them are hypotheses with 10 real roots and hypotheses with none (read on the restatement: 55 and 5)"""
    truth, matches, moved = big
    ref = three_ways(mc, lms, matches[:64], "16 384 hypotheses", max_iterations=mc.ESS_MAX_ITERATIONS)
    assert len(ref["counts"]) == 163840 and ref["status"] == ER.OK
    assert 10 * ref["best"] + ref["root"] == ref["counts"].index(max(ref["counts"]))
    assert max(ref["roots"]) == 10 and min(ref["roots"]) == 0 and all(s[0] >= 0 for s in ref["samples"])


@pytest.mark.parametrize("kind", EC.KINDS)
def test_scene_kinds(mc, lms, kind):
    truth, matches, moved = EC.scene(kind, seed=0, noise=0.1)
    ref = three_ways(mc, lms, matches, kind, max_iterations=200)
    assert ref["status"] == ER.OK


def test_hand_built_rows_in_one_launch(mc, lms):
    """the rows of test_ess_cpu.py, one launch each: a threshold equal to a match's Sampson value (no inlier) and the next double
    (an inlier); a NaN row; a distance equal to an inlier's depth and the next double; the tie of four zero votes; S = 5, where all
    counts tie and hypothesis 0's root 0 wins"""
    from test_ess_cpu import gate_rows
    matches, E, k, s, px = gate_rows(mc)
    at = three_ways(mc, lms, matches, "threshold = the value", threshold_px=px, max_iterations=1)
    above = three_ways(mc, lms, matches, "the next double", threshold_px=math.nextafter(px, math.inf), max_iterations=1)
    assert not at["ransac_inliers"][k] and above["ransac_inliers"][k]
    matches[7] = (matches[7][0], float("nan"), matches[7][2], matches[7][3])
    wide = three_ways(mc, lms, matches, "a NaN row", threshold_px=1e4, max_iterations=60)
    assert wide["status"] == ER.OK and not wide["ransac_inliers"][7] and any(7 in smp for smp in wide["samples"])
    truth, matches, moved = EC.scene("general", seed=1, noise=0.1)
    ref = three_ways(mc, lms, matches, "the scene", max_iterations=200)
    R, t = ER.candidate(ref["cands"], ref["winner"])
    z = [ER.depths(R, t, ER.point(EC.CAM, m)) for m in matches]
    for cam in (0, 1):
        k = max((i for i in range(len(matches)) if ref["inliers"][i] and z[i][cam] > z[i][1 - cam]), key=lambda i: z[i][cam])
        at = three_ways(mc, lms, matches, "distance = the depth", distance=z[k][cam], max_iterations=200)
        above = three_ways(mc, lms, matches, "the next double", distance=math.nextafter(z[k][cam], math.inf), max_iterations=200)
        assert not at["inliers"][k] and above["inliers"][k] and above["n_inliers"] == at["n_inliers"] + 1
    tie = three_ways(mc, lms, matches, "four zero votes", distance=1e-3, max_iterations=200)
    assert tie["status"] == ER.OK and tie["cheirality"] == [0, 0, 0, 0] and tie["winner"] == 0 and not any(tie["inliers"])
    truth, matches, moved = EC.scene("general", n=5, seed=3, moved=0.0)
    five = three_ways(mc, lms, matches, "S = 5", max_iterations=40)
    assert (five["best"], five["root"]) == (0, 0) and all(c == 5 for c, v in zip(five["counts"], five["valid"]) if v)


def test_no_obs_no_model_and_timing(mc, lms, big):
    """the four timings are positive after a launch; NO_OBS launches nothing and leaves them; NO_MODEL is a launch"""
    truth, matches, moved = big
    EC.run(mc, lms[0], matches[:300])
    us, nh = lms[0].last_essential_timing()
    assert all(v > 0 for v in us) and nh == 100
    print("k_ess_hypotheses %.1f us, k_ess_score %.1f us, k_ess_pick %.1f us, k_ess_finish %.1f us: 300 matches, 100 hypotheses" % us)
    got = EC.run(mc, lms[0], [], max_iterations=7)
    assert got.status == ER.NO_OBS and lms[0].last_essential_timing() == (us, nh)
    ref = three_ways(mc, lms, matches[:4], "S = 4", max_iterations=5)
    assert ref["status"] == ER.NO_MODEL
    us2, nh2 = lms[0].last_essential_timing()
    assert nh2 == 5 and all(v > 0 for v in us2)
    got = EC.run(mc, lms[0], matches[:4], max_iterations=5)
    assert got.R.tolist() == ER.IDENT and got.t.tolist() == [0.0] * 3 and not got.inliers.any() and got.best_hypothesis == -1
    assert lms[1].last_essential_timing()[0] == (0.0, 0.0, 0.0, 0.0)


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_ess_cpu.py, a pending tracking call among them, the store read back unchanged"""
    from test_ess_cpu import check_refusals
    check_refusals(mc, lms[0])


def test_bootstrap_and_the_neighbours_scratch(mc, lms, big):
    """the bootstrap of a one-camera rig on the device store: essential_pose, then initialize with its (R, t) and flags -- DONE,
    scaled, median depth 1 --, equal to the host-only store's on the bytes.  Then relative_pose and essential_pose again on the
    same stores: the scratch owners do not overlap"""
    from test_ess_cpu import bootstrap
    runs = [bootstrap(mc, lm) for lm in lms]
    EC.same_stores(runs[0][0], runs[1][0], "bootstrap")
    for k in ("pt3d", "normal", "new_lid", "t_out"):
        assert np.asarray(getattr(runs[0][1], k)).tobytes() == np.asarray(getattr(runs[1][1], k)).tobytes(), k
    truth, matches, moved = big
    first = [EC.run(mc, lm, matches[:300]) for lm in lms]
    cams, _, rel_matches, _ = RC.scene(8, 200, 21, moved=0.1)
    rel = [RC.run(mc, lm, cams, rel_matches, RC.THRESHOLD, 100, 0) for lm in lms]
    assert rel[0].status == 0 and rel[0].R.tobytes() == rel[1].R.tobytes() and rel[0].inliers.tolist() == rel[1].inliers.tolist()
    again = [EC.run(mc, lm, matches[:300]) for lm in lms]
    for a, b in zip(first, again):
        EC.same_stores(a, b, "after relative_pose")
    EC.same_stores(again[0], again[1], "device store == host-only store")
