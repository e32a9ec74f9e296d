"""The polish of the essential pose's RANSAC winner on a device store (LocalMap.essential_pose_polished: k_ess_hypotheses,
k_ess_score, k_ess_pick, k_ess_finish and k_ess_fit in one submission): the device store == the host-only store == the
plain-Python restatement (ess_polish_ref.py), floats as raw bytes, no tolerance, no excluded case.  Compared: the accepted pose, E,
flags and both counts, the winner's record, and per round the members, iterations, status, both costs, both counts and the verdict.

On the commit before the polish existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_ess_polish.py`):
LocalMap has no essential_pose_polished."""
import numpy as np
import pytest

import ess_cases as EC
import ess_polish_cases as EPC
import ess_polish_ref as EP
import ess_ref as ER
import kfdb_cases as K
import rel_cases as RC
import track_cases as T

pytestmark = pytest.mark.gpu
HYP = 64


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb.LocalMap, "essential_pose_polished")
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.fixture(scope="module")
def big():
    """per kind a scene of 1 025 matches with N(0, 0.1 px), 10 % of them moved"""
    return {kind: EC.scene(kind, n=1025, seed=21, noise=0.1)[1] for kind in EC.KINDS}


def three_ways(mc, lms, matches, what, **kw):
    """the device store and the host-only store against the restatement -> the restatement's two dicts"""
    ref, rp = EPC.reference(mc, matches, **kw)
    got = []
    for lm, who in zip(lms, ("device store", "host-only store")):
        got.append(EPC.run(mc, lm, matches, **kw))
        EPC.same(*got[-1], ref, rp, "%s: %s" % (what, who))
        if ref["status"] != ER.NO_OBS:
            EC.same_counts(lm, ref, "%s: %s" % (what, who))
    EC.same_stores(got[0][0], got[1][0], what)
    EPC.same_polish(got[0][1], got[1][1], what)
    return ref, rp


@pytest.mark.parametrize("kind", EC.KINDS)
@pytest.mark.parametrize("size", [5, 6, 63, 64, 65, 255, 256, 257, 1025])
def test_match_counts_rounds_and_iterations(mc, lms, big, kind, size):
    """a sample, either side of a wave, of the 256 lanes of the fold and of four trips of them, at 64 hypotheses with one and two
    rounds of 1, 10 and 100 solves"""
    for rounds in (1, 2):
        for its in (1, 10, 100):
            ref, rp = three_ways(mc, lms, big[kind][:size], "%s, %d matches, %d rounds, %d solves" % (kind, size, rounds, its),
                                 max_iterations=HYP, rounds=rounds, polish_iterations=its)
            assert len(ref["counts"]) == 10 * HYP and len(rp["inliers"]) == size
            assert ref["status"] == ER.OK and 1 <= len(rp["rounds"]) <= rounds and all(q["iterations"] <= its for q in rp["rounds"])


def test_pass_through_and_timing(mc, lms, big):
    """the five timings are positive after a polished launch; NO_OBS launches nothing and leaves all five; NO_MODEL is a launch
    whose k_ess_fit passes k_ess_finish's record through"""
    matches = big["general"]
    EPC.run(mc, lms[0], matches[:300])
    us, nh = lms[0].last_essential_timing5()
    assert len(us) == 5 and all(v > 0 for v in us) and nh == 100
    assert lms[0].last_essential_timing() == (us[:4], nh)
    print("k_ess_hypotheses %.1f us, k_ess_score %.1f us, k_ess_pick %.1f us, k_ess_finish %.1f us, k_ess_fit %.1f us: 300 matches, 100 "
          "hypotheses" % us)
    ref, rp = EPC.reference(mc, [], max_iterations=7)
    for lm in lms:
        EPC.same(*EPC.run(mc, lm, [], max_iterations=7), ref, rp, "S = 0")
    assert ref["status"] == ER.NO_OBS and lms[0].last_essential_timing5() == (us, nh)
    ref, rp = three_ways(mc, lms, matches[:4], "S = 4", max_iterations=5)
    assert ref["status"] == ER.NO_MODEL and not rp["rounds"]
    us2, nh2 = lms[0].last_essential_timing5()
    assert nh2 == 5 and all(v > 0 for v in us2)
    got, pol = EPC.run(mc, lms[0], matches[:4], max_iterations=5)
    assert got.R.tolist() == ER.IDENT and got.t.tolist() == [0.0] * 3 and not got.inliers.any() and pol.rounds_run == 0
    assert lms[1].last_essential_timing5()[0] == (0.0, 0.0, 0.0, 0.0, 0.0)


def test_a_winner_without_flags(mc, lms, big):
    """distance_thresh below every depth: an OK winner with no flag runs a round without a member that ends in NO_STEP"""
    ref, rp = three_ways(mc, lms, big["general"][:300], "no flags", distance=1e-3, max_iterations=HYP, polish_iterations=5)
    assert ref["status"] == ER.OK and ref["n_inliers"] == 0 and rp["rounds"][0]["status"] == EP.NO_STEP


def test_hostile_keypoints(mc, lms):
    """+-inf, NaN and FLT_MAX keypoints and a match at the epipole among 120 matches: the device agrees with the host-only store
    and the restatement, returns, and the next call on the same store is correct"""
    rows = EPC.hostile_matches()
    for its in (10, 100):
        three_ways(mc, lms, rows, "hostile keypoints, %d solves" % its, polish_iterations=its)
    _, matches, _ = EC.scene("general", n=60, seed=5, noise=0.1)
    three_ways(mc, lms, matches, "the next call")


def test_the_neighbours_are_what_they_were(mc, lms, big):
    """essential_pose, relative_pose and the bootstrap's initialize on the device store before and after polished calls: the same
    bytes, the host-only store's"""
    from test_ess_cpu import bootstrap
    matches = big["general"][:300]
    cams, _, rel_matches, _ = RC.scene(8, 200, 21, moved=0.1)
    ref = ER.ransac(EC.CAM, matches, EC.solver_of(mc))

    def neighbours(lm):
        ess = EC.run(mc, lm, matches)
        EC.same(ess, ref, "essential_pose")
        EC.same_counts(lm, ref, "essential_pose")
        return ess, RC.run(mc, lm, cams, rel_matches, RC.THRESHOLD, 100, 0), bootstrap(mc, lm)

    before = neighbours(lms[0])
    three_ways(mc, lms, matches, "polished")
    three_ways(mc, lms, big["forward"][:1025], "polished, more matches")
    for after in (neighbours(lms[0]), neighbours(lms[1])):
        EC.same_stores(before[0], after[0], "essential_pose")
        assert before[1].status == 0 and before[1].R.tobytes() == after[1].R.tobytes() and before[1].t.tobytes() == after[1].t.tobytes()
        assert before[1].inliers.tolist() == after[1].inliers.tolist()
        EC.same_stores(before[2][0], after[2][0], "bootstrap")
        for k in ("pt3d", "normal", "new_lid", "t_out"):
            assert np.asarray(getattr(before[2][1], k)).tobytes() == np.asarray(getattr(after[2][1], k)).tobytes(), k


def test_bootstrap_on_the_device_store(mc, lms):
    """essential_pose_polished's (R, t) and flags into initialize on the device store: DONE, scaled"""
    from test_ess_polish_cpu import test_bootstrap_end_to_end
    test_bootstrap_end_to_end(mc, lms[0])


def test_polished_first_on_fresh_stores(mc, big):
    """a device store and a host-only store that never ran a plain call: polished, plain, polished, plain at 5, 65, 257 and 6
    matches, so the polish's buffers are allocated before any plain call and every buffer grows between calls of the other kind.
    After every call the two stores hold the same bytes: result, flags, polish record, counts and models; a plain call leaves
    k_ess_fit's timing as the polished call before it left it"""
    matches = big["general"]
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    dev, host = [mc.LocalMap(voc, device=d, max_landmarks=4096, max_candidates=1024) for voc, d in zip(vocs, (0, -1))]
    fit_us = None
    for size, polished in ((5, True), (65, False), (257, True), (6, False)):
        what = "%d matches, %s" % (size, "polished" if polished else "plain")
        if polished:
            (a, pa), (b, pb) = [EPC.run(mc, lm, matches[:size], max_iterations=HYP, rounds=2, polish_iterations=10) for lm in (dev, host)]
            EPC.same_polish(pa, pb, what)
            fit_us = dev.last_essential_timing5()[0][4]
            assert fit_us > 0, what
        else:
            a, b = [EC.run(mc, lm, matches[:size], max_iterations=HYP) for lm in (dev, host)]
            assert dev.last_essential_timing5()[0][4] == fit_us, what
        EC.same_stores(a, b, what)
        assert a.n_matches == size and dev.last_essential_timing5()[1] == HYP, what
        ca, cb = dev.last_essential_counts(), host.last_essential_counts()
        assert len(ca[0]) == 10 * HYP and all(x.tobytes() == y.tobytes() for x, y in zip(ca, cb)), (what, "counts")


def test_between_two_tracking_submissions(mc, big):
    """a store with landmarks: a tracking submission, refused while it is pending, the polished call, a second submission -- both
    tracking results are the synchronous call's and the polished call is the restatement's"""
    matches = big["general"][:200]
    ref, rp = EPC.reference(mc, matches)
    v, store, kps, descs, lids = T.scene(4)
    view = T.to_view(mc, v)
    lm = mc.LocalMap(mc.ORBVocabulary().create(**K.vocabulary()), device=0, max_landmarks=4096, max_candidates=1024)
    T.fill(lm, store)
    sync = T.as_lists(lm.track(view, kps, descs, lids))
    lm.track_submit(view, kps, descs, lids)
    with pytest.raises(mc.McorbError) as e:
        EPC.run(mc, lm, matches)
    assert e.value.code == mc.E_STATE
    T.same(T.as_lists(lm.track_wait()), sync, "the first submission")
    EPC.same(*EPC.run(mc, lm, matches), ref, rp, "between the submissions")
    lm.track_submit(view, kps, descs, lids)
    T.same(T.as_lists(lm.track_wait()), sync, "the second submission")
    EPC.same(*EPC.run(mc, lm, matches), ref, rp, "after the submissions")


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_ess_polish_cpu.py, a pending tracking call among them, the store read back unchanged"""
    from test_ess_polish_cpu import check_refusals
    check_refusals(mc, lms[0])
