"""The keyframe database on the device (mcorb_kfdb, device >= 0: k_kfdb_score, k_kfdb_best2, k_kfdb_gather) against the host-only
database (device -1), bit for bit -- ids, scores (== on float64), the order among equal scores, score, featureMatchesBow -- and
against the plain-Python restatement of tests/kfdb_ref.py."""
import itertools

import numpy as np
import pytest

import kfdb_cases as K
import kfdb_ref
import oracle_lib as O
from kfdb_ref import same_query
from test_gpu_live_lf import calib, frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary().create(**K.vocabulary())


def pair(mc, voc, kfs, **caps):
    """the same keyframes in a device and a host-only database"""
    caps = dict(dict(max_entries=len(kfs) + 2, max_words=K.MAX_WORDS, max_feats=K.MAX_FEATS), **caps)
    dev, host = mc.ORBDatabase(voc, device=0, **caps), mc.ORBDatabase(voc, device=-1, **caps)
    for i, kf in enumerate(kfs):
        assert dev.add(*kf) == i == host.add(*kf)
    return dev, host


def same(a, b, what=""):
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), what


@pytest.fixture(scope="module")
def qdbs(mc, voc):
    return pair(mc, voc, K.query_keyframes())


def test_entries_round_trip_through_hbm(qdbs):
    dev, host = qdbs
    for i, (bow, fv, desc) in enumerate(K.query_keyframes()):
        (ids, vals), gfv, gdesc = dev.entry(i)
        assert np.array_equal(ids, bow[0]) and vals.tobytes() == np.asarray(bow[1], np.float64).tobytes(), i
        assert sorted(gfv) == sorted(fv) and all(np.array_equal(gfv[k], fv[k]) for k in fv), i
        assert np.array_equal(gdesc, desc), i


def test_query_equals_host_only(qdbs):
    dev, host = qdbs
    n = dev.size()
    queries = [kf[0] for kf in K.query_keyframes()] + K.hand_queries()
    ref = kfdb_ref.RefDatabase()
    for kf in K.query_keyframes():
        ref.add(*kf)
    for max_id, max_results in itertools.product((-1, 0, 1, n - 1, n, n + 5), (-1, 0, 1, 3, n + 5)):
        for qi, q in enumerate(queries):
            what = "query %d max_id %d max_results %d" % (qi, max_id, max_results)
            got = dev.query(q, max_results, max_id)
            same(got, host.query(q, max_results, max_id), what)
            same_query(got, ref.query_full(q, max_id), max_results, what)
    ents = list(range(n))
    max_ids = [(-1, 0, 1, n - 1, n, n + 5)[e % 6] for e in ents]
    for g, h in zip(dev.query_entries(ents, max_ids, 3), host.query_entries(ents, max_ids, 3)):
        same(g, h)


def test_entries_without_words_or_descriptors(mc, voc):
    """add with nbow = 0 beside descriptors, with ndesc = 0 beside words, and with neither: the copies of 0 bytes are not queued,
    the counts are; entries, queries and scores equal the host-only database's"""
    full = K.keyframe(65, 14)
    w = full[0][0][:1]
    kfs = [((np.zeros(0, np.uint32), np.zeros(0)), {}, full[2][:5]),             # no word, five descriptors
           ((w, np.array([0.5])), {}, np.zeros((0, 32), np.uint8)),              # one word, no descriptor
           ((np.zeros(0, np.uint32), np.zeros(0)), {}, np.zeros((0, 32), np.uint8)), full]
    dev, host = pair(mc, voc, kfs)
    for i, (bow, fv, desc) in enumerate(kfs):
        (ids, vals), gfv, gdesc = dev.entry(i)
        assert np.array_equal(ids, bow[0]) and vals.tobytes() == np.asarray(bow[1], np.float64).tobytes(), i
        assert sorted(gfv) == sorted(fv) and np.array_equal(gdesc, desc), i
    for q in [kf[0] for kf in kfs]:
        same(dev.query(q, -1, -1), host.query(q, -1, -1))
    for a, b in itertools.product(range(4), range(4)):
        assert dev.score(a, b) == host.score(a, b), (a, b)
    assert len(dev.query(kfs[1][0], -1, -1)[0]) == 2 and len(dev.query(kfs[0][0], -1, -1)[0]) == 0


def test_score_equals_host_only(qdbs):
    dev, host = qdbs
    n = dev.size()
    for a, b in itertools.product(range(n), range(n)):
        assert dev.score(a, b) == host.score(a, b), (a, b)
    assert dev.score(0, 3) == 0.0 and dev.score(9, 1) == 0.0


def test_feature_matches_equal_host_only(mc, voc):
    dev, host = pair(mc, voc, list(K.match_pair()) + K.ragged_pair())
    ref = kfdb_ref.RefDatabase()
    for kf in list(K.match_pair()) + K.ragged_pair():
        ref.add(*kf)
    for (a, b), ratio in itertools.product(((0, 1), (1, 0), (2, 3), (3, 2), (2, 2)), (0.85, 1.0)):
        got, want = dev.featureMatchesBow(a, b, ratio), host.featureMatchesBow(a, b, ratio)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (a, b, ratio)
        r = ref.feature_matches(a, b, ratio)
        assert np.array_equal(got[0], r[0]) and np.array_equal(got[1], r[1]), (a, b, ratio)
    assert len(dev.featureMatchesBow(0, 1)[0]) > 20 and len(dev.featureMatchesBow(2, 3)[0]) > 50


@pytest.fixture(scope="module")
def small():
    return K.small_keyframes(257)


@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 257])
def test_entry_counts_and_batched_queries(mc, voc, small, count):
    """a workgroup scores 32 entries, a wave 8 of them: counts around those; 1 and 3 queries per call equal one at a time"""
    dev, host = pair(mc, voc, small[:count], max_entries=count, max_words=64, max_feats=64)
    ents = sorted(set([0, count // 2, count - 1] + list(range(0, count, 37))))
    max_ids = [(-1, count - 1, e, e + 1)[i % 4] for i, e in enumerate(ents)]
    one = [dev.query_entries([e], [m], -1)[0] for e, m in zip(ents, max_ids)]
    for e, m, g in zip(ents, max_ids, one):
        same(g, dev.query(small[e][0], -1, m), "entry %d as a vector" % e)
        same(g, host.query(small[e][0], -1, m), "entry %d on the host" % e)
    for i in range(0, len(ents), 3):
        for g, o in zip(dev.query_entries(ents[i:i + 3], max_ids[i:i + 3], -1), one[i:i + 3]):
            same(g, o, "three per call")
    same(dev.query_entries([count - 1], [-1], 5)[0], host.query_entries([count - 1], [-1], 5)[0])


def test_add_then_query_equals_interleaved(mc, voc, small):
    """only entries below max_id count: add 8, then query each with max_id = entry - 2 == add / query interleaved.  Entry 1's
    max_id is -1, DBoW2's "no limit" (max_id == -1 || (int)e < max_id): queried after all 8 are in, it finds all that share a
    word with it, as the host-only database does -- callerDetectLoop never asks that (it queries only when entryId > dislocal,
    LoopCloser.cpp:102-109, so its maxId is >= 1)"""
    kfs = small[:8]
    first = mc.ORBDatabase(voc, device=0, max_entries=8, max_words=64, max_feats=64)
    inter = []
    for kf in kfs:
        e = first.add(*kf)
        inter.append(first.query_entries([e], [e - 2], 4)[0])
    after, host = pair(mc, voc, kfs, max_entries=8, max_words=64, max_feats=64)
    max_ids = [e - 2 for e in range(8)]
    got = after.query_entries(list(range(8)), max_ids, 4)
    for e in range(8):
        same(got[e], host.query_entries([e], [max_ids[e]], 4)[0], "entry %d on the host" % e)
        if max_ids[e] != -1:
            same(got[e], inter[e], "entry %d" % e)
    assert [len(g[0]) for g in got[:3]] == [0, 4, 0] and [len(g[0]) for g in inter[:3]] == [0, 2, 0] and len(got[7][0]) > 0


def test_add_rig_frame(mc):
    """lfBoW, lfFeatVec and the LF descriptors of a job's frames straight into the database"""
    C, W, H, F, levelsup = 4, 320, 240, 3, 2
    voc4 = mc.ORBVocabulary().create(**O.make_vocabulary(10, 4, seed=3))
    rig = mc.Rig(C, W, H, F, 1, nfeatures=300)
    rig.set_vocabulary(voc4, levelsup=levelsup)
    rig.set_lf(*calib(C, W, H))
    caps = dict(max_entries=4, max_words=2048, max_feats=2048)
    dev, host = mc.ORBDatabase(voc4, device=0, **caps), mc.ORBDatabase(voc4, device=-1, **caps)
    rig.upload(frames(mc, F, C, W, H, f0=11))
    rig.extract(2 * C)
    with pytest.raises(mc.McorbError) as ei:          # the job ran the LF stage on frames 0 and 1 only
        dev.add_rig_frame(rig, 2)
    assert ei.value.code == mc.E_STATE and dev.size() == 0
    rig.extract(F * C)
    for f in range(F):
        assert dev.add_rig_frame(rig, f) == f
        bow, fv = rig.lf_bow(f)
        desc = rig.lf_features(f)[0]["desc"]
        assert len(desc) > 0 and len(bow[0]) > 0
        assert host.add(bow, fv, desc) == f
        (ids, vals), gfv, gdesc = dev.entry(f)
        assert np.array_equal(ids, bow[0]) and vals.tobytes() == bow[1].tobytes(), f
        assert sorted(gfv) == sorted(fv) and all(np.array_equal(gfv[k], fv[k]) for k in fv), f
        assert np.array_equal(gdesc, desc), f
    hostrig = mc.ORBDatabase(voc4, device=-1, **caps)
    assert [hostrig.add_rig_frame(rig, f) for f in range(F)] == [0, 1, 2]
    for q in range(F):
        same(dev.query_entries([q], [-1], -1)[0], host.query_entries([q], [-1], -1)[0], "frame %d" % q)
        same(hostrig.query_entries([q], [-1], -1)[0], host.query_entries([q], [-1], -1)[0], "frame %d" % q)
    assert dev.score(0, 2) == host.score(0, 2)
    got, want = dev.featureMatchesBow(0, 2), host.featureMatchesBow(0, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    other = hostrig.featureMatchesBow(0, 2)
    assert np.array_equal(other[0], want[0]) and np.array_equal(other[1], want[1])
    rig.close()


def test_full_width_query(mc):
    """max_words = 4096, the LDS staging limit, with a query of 4096 words"""
    v = K.vocabulary(10, 4)
    voc4 = mc.ORBVocabulary().create(**v)
    sizes = (4096, 3000, 4095, 64)
    kfs = []
    for i, n in enumerate(sizes):
        bow, _, _ = K.keyframe(n, 40 + i, k=10, L=4, pool=60000, extra=0)
        kfs.append((bow, {}, np.zeros((0, 32), np.uint8)))
    assert len(kfs[0][0][0]) == 4096
    dev, host = pair(mc, voc4, kfs, max_words=4096, max_feats=8)
    ref = kfdb_ref.RefDatabase()
    for kf in kfs:
        ref.add(*kf)
    for e in range(len(kfs)):
        got = dev.query_entries([e], [-1], -1)[0]
        same(got, host.query_entries([e], [-1], -1)[0], "entry %d" % e)
        same_query(got, ref.query_entry_full(e), -1, "entry %d" % e)
        assert len(got[0]) == len(kfs)
    with pytest.raises(mc.McorbError) as ei:
        mc.ORBDatabase(voc4, device=0, max_entries=1, max_words=4097, max_feats=8)
    assert ei.value.code == mc.E_ARG
