"""The rig pose between two frames from 3D-3D pairs on a device store (LocalMap.align_pose: k_align_hypotheses, k_align_score,
k_align_pick and k_align_fit in one submission; mode "all": k_align_fit alone): the device store == the host-only store == the
numpy restatement (align_ref.py, the solver's poses through the mcorb_align_solve hook), floats as raw bytes, no tolerance, no
excluded case.  Compared: both poses, mean_error, sample[3], the flags, the status and -- through the read-back -- the counts of
all hypotheses.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_align.py`):
LocalMap has no align_pose."""
import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
import kfdb_cases as K
import pose_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb.LocalMap, "align_pose")
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.fixture(scope="module")
def big():
    """1 025 pairs, 100 of them moved by 1 m, N(0, 0.02 m) on the others"""
    return AC.scene(n=1025, seed=21, moved=100)


def three_ways(mc, lms, p1, p2, what, **kw):
    """the device store and the host-only store against the restatement -> the restatement"""
    want = AC.ref(mc, p1, p2, **kw)
    for lm, who in zip(lms, ("device store", "host-only store")):
        AC.same(AC.run(mc, lm, p1, p2, **kw), want, "%s: %s" % (what, who))
        if kw.get("mode", AR.SAC) == AR.SAC and want["status"] != AR.NO_OBS:
            AC.same_counts(lm, want, "%s: %s" % (what, who))
    return want


@pytest.mark.parametrize("mode", [AR.ALL, AR.SAC])
@pytest.mark.parametrize("size", [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1025])
def test_pair_counts(mc, lms, big, size, mode):
    """below a sample, a sample, either side of a wave, of a workgroup's tile and of four tiles; mode 0 fills the fold's lanes to
    every one of these occupancies, mode 1's refit does with the winner's members"""
    truth, p1, p2, moved = big
    want = three_ways(mc, lms, p1[:size], p2[:size], "%d pairs" % size, mode=mode)
    assert want["status"] == (AR.NO_OBS if size == 0 else AR.NO_MODEL if size < 3 else AR.OK)
    assert len(want["inliers"]) == size and (size < 3 or want["used"] == AR.USED_FIT)


@pytest.mark.parametrize("refit", [False, True])
@pytest.mark.parametrize("its", [1, 63, 64, 65, 100, 1025])
def test_max_iterations(mc, lms, big, its, refit):
    """either side of a wave of hypotheses and of k_align_score's blocks of them; the arg-max over five trips of k_align_pick's
    lanes; with the refit and without"""
    truth, p1, p2, moved = big
    want = three_ways(mc, lms, p1[:64], p2[:64], "%d hypotheses" % its, max_iterations=its, refit=refit)
    assert len(want["counts"]) == its and want["n_models"] == its and want["status"] == AR.OK
    assert want["used"] == (AR.USED_FIT if refit else AR.USED_SAC)


def test_the_most_hypotheses(mc, lms, big):
    """MCORB_ALIGN_MAX_ITERATIONS hypotheses on 64 pairs: the 14 bits of the key, 64 trips of the pick"""
    truth, p1, p2, moved = big
    want = three_ways(mc, lms, p1[:64], p2[:64], "16 384 hypotheses", max_iterations=mc.ALIGN_MAX_ITERATIONS)
    assert len(want["counts"]) == 16384 and want["status"] == AR.OK
    assert want["best"] == want["counts"].index(max(want["counts"]))


def test_lids_against_points(mc, lms, big):
    """frame 1's points read from the store's landmark array on the device: the bytes of the pts1 call, the store unchanged"""
    from test_align_cpu import MODES, read_back
    truth, p1, p2, moved = big
    p1, p2 = p1[:300], p2[:300]
    lids = np.arange(300, 1200, 3, dtype=np.int32)
    for lm in lms:
        lm.set(lids, p1, np.zeros_like(p1))
    before = [read_back(lm, lids) for lm in lms]
    for kw in MODES:
        want = AC.ref(mc, p1, p2, **kw)
        for lm in lms:
            by_lid = AC.run(mc, lm, None, p2, lids1=lids, **kw)
            AC.same(by_lid, want, "lids1")
            AC.same_results(by_lid, AC.run(mc, lm, p1, p2, **kw), "lids1 against pts1")
    assert [read_back(lm, lids) for lm in lms] == before


def test_hand_built_rows_in_one_launch(mc, lms):
    """the rows of test_align_cpu.py, one launch each: the degenerate sets in both modes, the half turn, n = 3, a limit equal to
    a pair's distance and the next double above for both limits, a NaN row"""
    from test_align_cpu import nan_rows, threshold_rows
    for name, (p1, p2) in (("collinear", AC.collinear()), ("collinear as float", AC.collinear(True)), ("coincident", AC.coincident())):
        for mode in (AR.ALL, AR.SAC):
            assert three_ways(mc, lms, p1, p2, name, mode=mode, max_iterations=20)["status"] == AR.NO_MODEL
    truth, p1, p2 = AC.half_turn()
    assert three_ways(mc, lms, p1, p2, "half turn", mode=AR.ALL)["n_inliers"] == 40
    assert three_ways(mc, lms, p1, p2, "half turn", max_iterations=10)["n_inliers"] == 40
    truth, p1, p2, moved = AC.scene(n=3, moved=0, noise=0.0)
    tie = three_ways(mc, lms, p1, p2, "n = 3", max_iterations=40)
    assert all(c == 3 for c in tie["counts"]) and tie["best"] == 0
    p1, p2, k, d, model = threshold_rows(mc)
    at = three_ways(mc, lms, p1, p2, "threshold = the distance", threshold=d, inlier_dist=10.0, max_iterations=1, refit=False)
    above = three_ways(mc, lms, p1, p2, "the next double", threshold=AR.next_up(d), inlier_dist=10.0, max_iterations=1, refit=False)
    assert above["sac_n_inliers"] == at["sac_n_inliers"] + 1
    at = three_ways(mc, lms, p1, p2, "inlier_dist = the distance", threshold=10.0, inlier_dist=d, max_iterations=1, refit=False)
    above = three_ways(mc, lms, p1, p2, "the next double", threshold=10.0, inlier_dist=AR.next_up(d), max_iterations=1, refit=False)
    assert not at["inliers"][k] and above["inliers"][k]
    p1, p2 = nan_rows()
    wide = three_ways(mc, lms, p1, p2, "a NaN row", threshold=1e9, inlier_dist=1e9, max_iterations=60)
    assert wide["status"] == AR.OK and not wide["inliers"][7] and any(7 in s for s in wide["samples"])
    assert three_ways(mc, lms, p1, p2, "a NaN row, all", mode=AR.ALL)["status"] == AR.NO_MODEL


def test_no_obs_no_model_and_timing(mc, lms, big):
    """the four timings are positive after a mode-1 launch; NO_OBS launches nothing and leaves them; mode 0 leaves the first
    three and the hypotheses and sets the fourth; NO_MODEL is a launch; a host-only store has no timings"""
    truth, p1, p2, moved = big
    AC.run(mc, lms[0], p1[:300], p2[:300])
    us, nh = lms[0].last_align_timing()
    assert all(v > 0 for v in us) and nh == 100
    print("k_align_hypotheses %.1f us, k_align_score %.1f us, k_align_pick %.1f us, k_align_fit %.1f us: 300 pairs, 100 hypotheses" % us)
    got = AC.run(mc, lms[0], p1[:0], p2[:0], max_iterations=7)
    assert got.status == AR.NO_OBS and lms[0].last_align_timing() == (us, nh)
    AC.run(mc, lms[0], p1[:300], p2[:300], mode=AR.ALL)
    us0, nh0 = lms[0].last_align_timing()
    assert us0[:3] == us[:3] and us0[3] > 0 and nh0 == 100
    print("k_align_fit alone %.1f us: 300 pairs" % us0[3])
    want = three_ways(mc, lms, p1[:2], p2[:2], "n = 2", max_iterations=5)
    assert want["status"] == AR.NO_MODEL
    us2, nh2 = lms[0].last_align_timing()
    assert nh2 == 5 and all(v > 0 for v in us2)
    got = AC.run(mc, lms[0], p1[:2], p2[:2], max_iterations=5)
    assert P.same_bits(got.R.tolist(), AR.IDENT[0]) and got.t.tolist() == [0.0] * 3 and not got.inliers.any()
    assert lms[1].last_align_timing()[0] == (0.0, 0.0, 0.0, 0.0)


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_align_cpu.py, a pending tracking call among them, the store read back unchanged"""
    from test_align_cpu import check_refusals
    check_refusals(mc, lms[0])
