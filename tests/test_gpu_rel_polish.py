"""The polish of the relative pose's RANSAC winner on a device store (LocalMap.relative_pose_polished: k_rel_hypotheses,
k_rel_score, k_rel_pick and k_rel_fit in one submission): the device store == the host-only store == the plain-Python restatement
(rel_polish_ref.py), floats as raw bytes, no tolerance, no excluded case.  Compared: the accepted pose, flags and count, the
winner's record, and per round the members, iterations, status, both costs, the count and the verdict.

On the commit before the polish existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_rel_polish.py`):
LocalMap has no relative_pose_polished."""
import pytest

import kfdb_cases as K
import pose_ref as P
import rel_cases as RC
import rel_polish_cases as RPC
import rel_ref as RR
import track_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb.LocalMap, "relative_pose_polished")
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.fixture(scope="module")
def big():
    """an 8-camera scene of 1 025 matches with N(0, 0.1 px), 10 % of them moved"""
    return RC.scene(8, 1025, 21, moved=0.1)


def three_ways(mc, lms, cams, matches, what, **kw):
    """the device store and the host-only store against the restatement -> the restatement's two dicts"""
    ref, rp = RPC.reference(mc, cams, matches, **kw)
    for lm, who in zip(lms, ("device store", "host-only store")):
        got, pol = RPC.run(mc, lm, cams, matches, **kw)
        RPC.same(got, pol, ref, rp, "%s: %s" % (what, who))
        if ref["status"] != RR.NO_OBS:
            RC.same_counts(lm, ref, "%s: %s" % (what, who))
    return ref, rp


@pytest.mark.parametrize("size", [17, 18, 63, 64, 65, 255, 256, 257, 1025])
def test_match_counts(mc, lms, big, size):
    """a sample, either side of a wave, of the 256 lanes of the fold and of four trips of them"""
    cams, truth, matches, moved = big
    ref, rp = three_ways(mc, lms, cams, matches[:size], "%d matches" % size)
    assert ref["status"] == RR.OK and len(rp["rounds"]) >= 1 and len(rp["inliers"]) == size


@pytest.mark.parametrize("hyp", [64, 100])
@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("its", [1, 10, 100])
def test_hypotheses_rounds_and_iterations(mc, lms, big, hyp, rounds, its):
    cams, truth, matches, moved = big
    ref, rp = three_ways(mc, lms, cams, matches[:300], "%d hypotheses, %d rounds, %d solves" % (hyp, rounds, its), max_iterations=hyp,
                         rounds=rounds, polish_iterations=its)
    assert len(ref["counts"]) == hyp and 1 <= len(rp["rounds"]) <= rounds and all(q["iterations"] <= its for q in rp["rounds"])


def test_pass_through_and_timing(mc, lms, big):
    """the four timings are positive after a polished launch; NO_OBS launches nothing and leaves them; NO_MODEL is a launch whose
    k_rel_fit passes the pick's record through"""
    cams, truth, matches, moved = big
    RPC.run(mc, lms[0], cams, matches[:300])
    us, nh = lms[0].last_relative_timing4()
    assert len(us) == 4 and all(v > 0 for v in us) and nh == 100
    assert lms[0].last_relative_timing() == (us[:3], nh)
    print("k_rel_hypotheses %.1f us, k_rel_score %.1f us, k_rel_pick %.1f us, k_rel_fit %.1f us: 300 matches, 100 hypotheses" % us)
    ref, rp = RPC.reference(mc, cams, [], max_iterations=7)
    for lm in lms:
        RPC.same(*RPC.run(mc, lm, cams, [], max_iterations=7), ref, rp, "S = 0")
    assert ref["status"] == RR.NO_OBS and lms[0].last_relative_timing4() == (us, nh)
    ref, rp = three_ways(mc, lms, cams, matches[:16], "S = 16", max_iterations=5)
    assert ref["status"] == RR.NO_MODEL and not rp["rounds"]
    us2, nh2 = lms[0].last_relative_timing4()
    assert nh2 == 5 and all(v > 0 for v in us2)
    got, pol = RPC.run(mc, lms[0], cams, matches[:16], max_iterations=5)
    assert P.same_bits(got.R.tolist(), RR.IDENT[0]) and got.t.tolist() == [0.0] * 3 and not got.inliers.any() and pol.rounds_run == 0
    assert lms[1].last_relative_timing4()[0] == (0.0, 0.0, 0.0, 0.0)


def test_hostile_keypoints(mc, lms):
    """+-inf, NaN and FLT_MAX keypoints and a match whose rays coincide among 120 matches: the device agrees with the host-only
    store and the restatement, returns, and the next call on the same store is correct"""
    cams, rows = RPC.hostile_matches()
    for its in (10, 100):
        three_ways(mc, lms, cams, rows, "hostile keypoints, %d solves" % its, polish_iterations=its)
    cams, _, matches, _ = RC.scene(8, 60, 5, 0.1, 0.1)
    three_ways(mc, lms, cams, matches, "the next call")


def test_relative_pose_is_what_it_was(mc, lms, big):
    """relative_pose before and after a polished call on the device store: the restatement's result and counts"""
    cams, truth, matches, moved = big
    ref, rp = RPC.reference(mc, cams, matches[:200])
    RC.same(RC.run(mc, lms[0], cams, matches[:200]), ref, "before")
    RPC.same(*RPC.run(mc, lms[0], cams, matches[:200]), ref, rp, "polished")
    RC.same(RC.run(mc, lms[0], cams, matches[:200]), ref, "after")
    RC.same_counts(lms[0], ref, "after")


def test_polished_first_on_fresh_stores(mc, big):
    """a device store and a host-only store that never ran a plain call: polished, plain, polished, plain at 17, 65, 257 and 18
    matches, so the polish's buffers are allocated before any plain call and every buffer grows between calls of the other kind.
    After every call the two stores hold the same bytes: result, flags, polish record, counts; a plain call leaves k_rel_fit's
    timing as the polished call before it left it"""
    cams, truth, matches, moved = big
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    dev, host = [mc.LocalMap(voc, device=d, max_landmarks=4096, max_candidates=1024) for voc, d in zip(vocs, (0, -1))]
    fit_us = None
    for size, polished in ((17, True), (65, False), (257, True), (18, False)):
        what = "%d matches, %s" % (size, "polished" if polished else "plain")
        if polished:
            (a, pa), (b, pb) = [RPC.run(mc, lm, cams, matches[:size], max_iterations=64, rounds=2, polish_iterations=10) for lm in (dev, host)]
            RPC.same_polish(pa, pb, what)
            fit_us = dev.last_relative_timing4()[0][3]
            assert fit_us > 0, what
        else:
            a, b = [RC.run(mc, lm, cams, matches[:size], max_iterations=64) for lm in (dev, host)]
            assert dev.last_relative_timing4()[0][3] == fit_us, what
        RC.same_stores(a, b, what)
        assert a.n_matches == size and dev.last_relative_timing4()[1] == 64, what
        (ca, va), (cb, vb) = dev.last_relative_counts(), host.last_relative_counts()
        assert len(ca) == 64 and ca.tolist() == cb.tolist() and va.tolist() == vb.tolist(), (what, "counts")


def test_between_two_tracking_submissions(mc, big):
    """a store with landmarks: a tracking submission, refused while it is pending, the polished call, a second submission -- both
    tracking results are the synchronous call's and the polished call is the restatement's"""
    cams, truth, matches, moved = big
    ref, rp = RPC.reference(mc, cams, matches[:200])
    v, store, kps, descs, lids = T.scene(4)
    view = T.to_view(mc, v)
    lm = mc.LocalMap(mc.ORBVocabulary().create(**K.vocabulary()), device=0, max_landmarks=4096, max_candidates=1024)
    T.fill(lm, store)
    sync = T.as_lists(lm.track(view, kps, descs, lids))
    lm.track_submit(view, kps, descs, lids)
    with pytest.raises(mc.McorbError) as e:
        RPC.run(mc, lm, cams, matches[:200])
    assert e.value.code == mc.E_STATE
    T.same(T.as_lists(lm.track_wait()), sync, "the first submission")
    RPC.same(*RPC.run(mc, lm, cams, matches[:200]), ref, rp, "between the submissions")
    lm.track_submit(view, kps, descs, lids)
    T.same(T.as_lists(lm.track_wait()), sync, "the second submission")
    RPC.same(*RPC.run(mc, lm, cams, matches[:200]), ref, rp, "after the submissions")


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_rel_polish_cpu.py, a pending tracking call among them, the store read back unchanged"""
    from test_rel_polish_cpu import check_refusals
    check_refusals(mc, lms[0])
