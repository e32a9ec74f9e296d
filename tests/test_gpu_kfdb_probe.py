"""The keyframe database's probe slots on the device (device >= 0: the probe store in HBM, k_kfdb_score with probes as queries,
k_kfdb_best2's many-probe launch, findInterMatches' knnMatch through the k-NN kernel) against the host-only database (device -1),
bit for bit, on the inputs of test_kfdb_probe_cpu.py."""
import numpy as np
import pytest

import kfdb_cases as K
import kfdb_probe_cases as P
import oracle_lib as O
from test_gpu_live_lf import calib, frames
from test_kfdb_probe_cpu import best2_paths, same_frame, same_matches, same_bf, snapshot, same_snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary().create(**K.vocabulary())


def pair(mc, voc, kfs, probes=(), nprobes=8, **caps):
    """the same entries and probes in a device and a host-only database"""
    caps = dict(dict(max_entries=len(kfs) + 2, max_words=P.MAX_WORDS, max_feats=P.MAX_FEATS), **caps)
    dev, host = mc.ORBDatabase(voc, device=0, **caps), mc.ORBDatabase(voc, device=-1, **caps)
    for i, kf in enumerate(kfs):
        assert dev.add(*kf) == i == host.add(*kf)
    for db in (dev, host):
        db.reserve_probes(nprobes)
        for p, fr in enumerate(probes):
            db.set_probe(p, *fr)
    return dev, host


def same(a, b, what=""):
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), what


def test_probes_round_trip_and_leave_the_entries_alone(mc, voc):
    """entries added before the probe slots exist (the descriptor allocation moves) and after; probe traffic in between"""
    kfs = K.query_keyframes()
    caps = dict(max_entries=len(kfs) + 2, max_words=K.MAX_WORDS, max_feats=K.MAX_FEATS - 3)      # 253: not a multiple of 64
    dev, host = mc.ORBDatabase(voc, device=0, **caps), mc.ORBDatabase(voc, device=-1, **caps)
    for db in (dev, host):
        for kf in kfs[:6]:
            db.add(*kf)
    before = snapshot(dev, kfs[:6])
    probes = [kfs[4], K.keyframe(100, 99), kfs[8], P.EMPTY, K.match_pair()[1], kfs[6]]
    for db in (dev, host):
        db.reserve_probes(len(probes))
        for p, fr in enumerate(probes):
            db.set_probe(p, *fr)
    same_snapshot(snapshot(dev, kfs[:6]), before)
    for p, fr in enumerate(probes):
        same_frame(dev.get_probe(p), fr, "probe %d" % p)
    for db in (dev, host):
        for kf in kfs[6:]:
            db.add(*kf)
    n = dev.size()
    for max_id, max_results in ((-1, -1), (-1, 3), (0, -1), (1, 2), (n - 1, -1), (n + 5, 4)):
        got = dev.query_probes(list(range(len(probes))), [max_id] * len(probes), max_results)
        want = host.query_probes(list(range(len(probes))), [max_id] * len(probes), max_results)
        for p, fr in enumerate(probes):
            same(got[p], want[p], (p, max_id, max_results))
            same(got[p], dev.query(fr[0], max_results, max_id), (p, max_id, max_results))
    for e in range(n):
        for p in range(len(probes)):
            assert dev.score_probe(e, p) == host.score_probe(e, p), (e, p)
    dev.set_probe(0, *probes[4])                                  # overwritten by a shorter frame, then read back
    same_frame(dev.get_probe(0), probes[4])
    same_frame(dev.get_probe(5), probes[5])
    same_snapshot(snapshot(dev, kfs), snapshot(host, kfs))
    for i, kf in enumerate(kfs):
        same_frame(dev.entry(i), kf, "entry %d" % i)


def test_probe_feature_matches_equal_host_only(mc, voc):
    a1, b1 = K.match_pair()
    a2, b2 = P.size_pair()
    a3, b3 = K.ragged_pair()
    dev, host = pair(mc, voc, [a1, a2, a3], [b1, P.EMPTY, b2, b3])
    for ratio in (0.85, 1.0):
        for e in range(3):
            for probes in ([0], [1], [2], [3], [0, 1, 2], [2, 1, 3], [3, 3, 0]):
                got, want = dev.probe_feature_matches(e, probes, ratio), host.probe_feature_matches(e, probes, ratio)
                for g, w in zip(got, want):
                    same_matches(g, w, (e, probes, ratio))
            for p in range(4):
                assert dev.score_probe(e, p) == host.score_probe(e, p)
    assert len(dev.probe_feature_matches(0, [0])[0][0]) > 20 and len(dev.probe_feature_matches(1, [2])[0][0]) > 100


@pytest.fixture(scope="module")
def lfdbs(mc, voc):
    """one entry of 257 LF features and 33 probe slots with LF sets of 1, 63, 64, 65 and 257 features"""
    probes = [P.lf_frame(P.LF_SIZES[i % 5], i) for i in range(33)]
    entries = [P.lf_frame(257, -1), P.lf_frame(65, 77), P.lf_frame(1, 78)]
    return pair(mc, voc, entries, probes, nprobes=33, max_words=260, max_feats=257), probes


@pytest.mark.parametrize("nprobes", [1, 3, 33])
def test_probes_per_launch(lfdbs, nprobes):
    """1, 3 and 33 probes in one launch (33 x ~250 items cross the 256-lane workgroups of the item list many times) equal the
    host-only database, and a batch equals its probes one at a time"""
    (dev, host), probes = lfdbs
    for e in range(3):
        for first in ((0, 1, 2, 3, 4) if nprobes == 1 else (0, 2) if nprobes == 3 else (0,)):
            sel = list(range(first, first + nprobes))
            got, want = dev.probe_feature_matches(e, sel), host.probe_feature_matches(e, sel)
            for p, g, w in zip(sel, got, want):
                same_matches(g, w, (e, p))
                if nprobes > 1 and p % 7 == 0:
                    same_matches(g, dev.probe_feature_matches(e, [p])[0], (e, p))
            if e == 0:
                assert all(len(g[0]) > 0.5 * len(probes[p][2]) for p, g in zip(sel, got))       # near copies: most features match


@pytest.fixture(scope="module")
def b2dbs(mc, voc):
    """P.best2_frames(): A as entry 0, B0 .. B4 as entries 1 .. 5 and as probes 0 .. 4, in a device and a host-only database"""
    A, Bs, _, _ = P.best2_frames()
    return pair(mc, voc, [A] + Bs, Bs, nprobes=len(Bs))


@pytest.mark.parametrize("ratio", [0.85, 1.0])
def test_best2_search_paths_agree(b2dbs, ratio):
    """the one k_kfdb_best2 search through its call paths -- a single pair of entries, one probe, many probes in any order -- on
    1, 255, 256, 257 and 0 items gives the lists of the host-only database (test_kfdb_probe_cpu.py holds those against the
    restatement and counts the edge cases of the frames)"""
    dev, host = b2dbs
    for p, (g, w) in enumerate(zip(best2_paths(dev, ratio), best2_paths(host, ratio))):
        same_matches(g, w, (p, ratio))


def bf_args(rng, nq, nt):
    lids = np.where(rng.random(nq) < 0.3, rng.integers(0, 99, nq), -1).astype(np.int32)
    m1, m2 = (rng.random(nq) < 0.3).astype(np.uint8), (rng.random(nt) < 0.3).astype(np.uint8)
    p2 = rng.normal(0, 3, (nt, 3))
    p1 = p2[rng.integers(0, nt, nq)] + rng.normal(0, 1.1, (nq, 3))
    return lids, m1, p1, m2, p2


def test_inter_matches_bf_equal_host_only(mc, voc, lfdbs):
    (dev, host), probes = lfdbs
    rng = np.random.default_rng(4)
    for e, p in ((1, 4), (2, 0), (0, 1), (0, 4), (1, 0)):      # 65 x 257, 1 x 1, 257 x 63, 257 x 257, 65 x 1
        nq, nt = len(dev.entry(e)[2]), len(probes[p][2])
        args = bf_args(rng, nq, nt)
        got, want = dev.probe_inter_matches_bf(e, p, *args), host.probe_inter_matches_bf(e, p, *args)
        same_bf(got, want, (e, p))
        if min(nq, nt) > 60:
            assert len(got[0]) > 10
    # 2 x 1, the gates of the CPU test, and an empty probe
    c = P.bf_case()
    (dq, lids, m1, p1), (dt, m2, p2) = c["prev"], c["cur"]
    two = np.stack([dq[0], dq[0] ^ 1])
    d2, h2 = pair(mc, voc, [(P.ONE_WORD, {}, two), (P.ONE_WORD, {}, dq)], [(P.ONE_WORD, {}, dt[:1]), (P.ONE_WORD, {}, dt), P.EMPTY], max_feats=40)
    for lid in ([-1, -1], [4, -1], [4, 4]):
        a = (np.array(lid, np.int32), np.zeros(2, np.uint8), np.zeros((2, 3)), np.zeros(1, np.uint8), np.zeros((1, 3)))
        same_bf(d2.probe_inter_matches_bf(0, 0, *a), h2.probe_inter_matches_bf(0, 0, *a), lid)
    assert d2.probe_inter_matches_bf(0, 0, *a)[0].tolist() == [0]                     # two landmarks on one train: the first holds it
    same_bf(d2.probe_inter_matches_bf(1, 1, lids, m1, p1, m2, p2), h2.probe_inter_matches_bf(1, 1, lids, m1, p1, m2, p2))
    assert d2.probe_inter_matches_bf(1, 1, lids, m1, p1, m2, p2)[0].tolist() == [0, 2, 4, 6, 7, 8, 9, 13, 16]
    assert len(d2.probe_inter_matches_bf(1, 2, lids, m1, p1, np.zeros(0, np.uint8), np.zeros((0, 3)))[0]) == 0


def test_query_probes_full_width(mc):
    """max_words = 4096, the LDS staging limit, with a probe of 4096 words"""
    voc4 = mc.ORBVocabulary().create(**K.vocabulary(10, 4))
    none = ({}, np.zeros((0, 32), np.uint8))
    kfs = [(K.keyframe(n, 40 + i, k=10, L=4, pool=60000, extra=0)[0],) + none for i, n in enumerate((4096, 3000, 64))]
    assert len(kfs[0][0][0]) == 4096
    dev, host = pair(mc, voc4, kfs[1:], [kfs[0], kfs[2]], nprobes=2, max_words=4096, max_feats=8)
    for g, h, fr in zip(dev.query_probes([0, 1], [-1, -1], -1), host.query_probes([0, 1], [-1, -1], -1), (kfs[0], kfs[2])):
        same(g, h)
        same(g, dev.query(fr[0], -1))
        assert len(g[0]) == 2
    assert dev.score_probe(0, 0) == host.score_probe(0, 0) != 0.0


def test_set_probe_rig_frame(mc):
    """lfBoW, lfFeatVec and the LF descriptors of a job's frame straight into a probe slot == set_probe of what get_lf_* return"""
    C, W, H, F, levelsup = 4, 320, 240, 3, 2
    voc4 = mc.ORBVocabulary().create(**O.make_vocabulary(10, 4, seed=3))
    rig = mc.Rig(C, W, H, F, 1, nfeatures=300)
    rig.set_vocabulary(voc4, levelsup=levelsup)
    rig.set_lf(*calib(C, W, H))
    caps = dict(max_entries=2, max_words=2048, max_feats=2048)
    dev, host, hostrig = (mc.ORBDatabase(voc4, device=d, **caps) for d in (0, -1, -1))
    for db in (dev, host, hostrig):
        db.reserve_probes(F)
    rig.upload(frames(mc, F, C, W, H, f0=11))
    rig.extract(2 * C)
    with pytest.raises(mc.McorbError) as ei:          # the job ran the LF stage on frames 0 and 1 only
        dev.set_probe_rig_frame(0, rig, 2)
    assert ei.value.code == mc.E_STATE
    with pytest.raises(mc.McorbError) as ei:          # ... and slot 0 is still unset
        dev.get_probe(0)
    assert ei.value.code == mc.E_STATE
    rig.extract(F * C)
    assert dev.add_rig_frame(rig, 0) == 0 == host.add_rig_frame(rig, 0) == hostrig.add_rig_frame(rig, 0)
    for f in range(F):
        dev.set_probe_rig_frame(f, rig, f)
        hostrig.set_probe_rig_frame(f, rig, f)
        bow, fv = rig.lf_bow(f)
        desc = rig.lf_features(f)[0]["desc"]
        assert len(desc) > 0 and len(bow[0]) > 0
        host.set_probe(f, bow, fv, desc)
        same_frame(dev.get_probe(f), (bow, fv, desc), f)
        same_frame(hostrig.get_probe(f), (bow, fv, desc), f)
    assert dev.size() == 1
    want = host.probe_feature_matches(0, [0, 1, 2])
    for g, o, w in zip(dev.probe_feature_matches(0, [0, 1, 2]), hostrig.probe_feature_matches(0, [0, 1, 2]), want):
        same_matches(g, w)
        same_matches(o, w)
    assert len(want[0][0]) > 0 and len(want[2][0]) > 0
    for g, w in zip(dev.query_probes([0, 1, 2], [-1] * 3, -1), host.query_probes([0, 1, 2], [-1] * 3, -1)):
        same(g, w)
    rng = np.random.default_rng(2)
    args = bf_args(rng, len(dev.entry(0)[2]), len(dev.get_probe(2)[2]))
    same_bf(dev.probe_inter_matches_bf(0, 2, *args), host.probe_inter_matches_bf(0, 2, *args))
    rig.close()
