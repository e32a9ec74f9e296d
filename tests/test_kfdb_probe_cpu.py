"""The keyframe database's probe slots (mcorb_kfdb_reserve_probes ... mcorb_kfdb_probe_inter_matches_bf) on the host-only database
(device -1), against the plain-Python restatement of tests/kfdb_probe_ref.py: frames that are queried, scored and matched against
entries -- FrontEnd::InterMatchingBow, Relocalization::featureMatchesBow, FrontEnd::findInterMatches -- without becoming one.
No GPU is needed."""
import numpy as np
import pytest

import kfdb_cases as K
import kfdb_probe_cases as P
import kfdb_probe_ref as R
import mcorb
from kfdb_ref import same_query


def host_voc():
    return mcorb.ORBVocabulary(device=-1).create(**K.vocabulary())


def fill(kfs, probes=(), nprobes=8, **caps):
    """a host-only database of the entries kfs with probe slots 0 .. set to `probes`, and the restatement of both"""
    caps = dict(dict(max_entries=len(kfs) + 2, max_words=P.MAX_WORDS, max_feats=P.MAX_FEATS), **caps)
    db = mcorb.ORBDatabase(host_voc(), device=-1, **caps)
    ref = R.RefDatabase()
    for i, kf in enumerate(kfs):
        assert db.add(*kf) == i == ref.add(*kf)
    rp = R.RefProbes(ref)
    if nprobes:
        db.reserve_probes(nprobes)
    for p, fr in enumerate(probes):
        db.set_probe(p, *fr)
        rp.set_probe(p, *fr)
    return db, rp


def same_frame(got, want, what=""):
    (ids, vals), gfv, gdesc = got
    bow, fv, desc = want
    assert np.array_equal(ids, bow[0]) and vals.tobytes() == np.asarray(bow[1], np.float64).tobytes(), what
    assert sorted(gfv) == sorted(fv) and all(np.array_equal(gfv[k], fv[k]) for k in fv), what
    assert np.array_equal(gdesc, desc), what


def same_matches(got, want, what=""):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


def snapshot(db, kfs):
    """everything the entry-only calls return"""
    n = db.size()
    ents = list(range(n))
    return (n, [db.entry(e) for e in ents], [db.query(kf[0], -1) for kf in kfs], [db.query(kf[0], 3, n - 1) for kf in kfs],
            db.query_entries(ents, [-1] * n, -1), db.query_entries(ents, [e for e in ents], 2),
            [db.score(a, b) for a in ents for b in ents], [db.featureMatchesBow(a, b) for a in ents[:3] for b in ents[:3]])


def same_snapshot(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        same_frame(x, (y[0], y[1], y[2]))
    for i in (2, 3, 4, 5, 7):
        assert len(a[i]) == len(b[i])
        for x, y in zip(a[i], b[i]):
            assert np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes(), i
    assert a[6] == b[6]


def test_probe_round_trip_and_overwrite():
    frames = [K.match_pair()[1], P.EMPTY, P.size_pair()[1], K.ragged_pair()[1], K.keyframe(K.MAX_WORDS, 3)]
    db, _ = fill([], frames)
    for p, fr in enumerate(frames):
        same_frame(db.get_probe(p), fr, "probe %d" % p)
    db.set_probe(2, *frames[3])                       # setting a probe overwrites it, longer or shorter
    db.set_probe(3, *P.EMPTY)
    same_frame(db.get_probe(2), frames[3])
    same_frame(db.get_probe(3), P.EMPTY)
    same_frame(db.get_probe(0), frames[0])
    assert db.size() == 0


def test_a_probe_is_not_an_entry():
    kfs = K.query_keyframes()
    db, rp = fill(kfs, max_words=K.MAX_WORDS, max_feats=K.MAX_FEATS)
    before = snapshot(db, kfs)
    probes = [kfs[4], K.keyframe(100, 99), kfs[8], P.EMPTY, K.match_pair()[1]]
    for p, fr in enumerate(probes):
        db.set_probe(p, *fr)
        rp.set_probe(p, *fr)
    n = db.size()
    for max_id, max_results in ((-1, -1), (-1, 3), (0, -1), (1, 2), (n - 1, -1), (n + 5, 4)):
        got = db.query_probes(list(range(len(probes))), [max_id] * len(probes), max_results)
        for p, fr in enumerate(probes):
            one = db.query(fr[0], max_results, max_id)          # mcorb_kfdb_query of the same host vectors
            assert np.array_equal(got[p][0], one[0]) and got[p][1].tobytes() == one[1].tobytes(), (p, max_id, max_results)
            same_query(got[p], rp.query_full(p, max_id), max_results, "probe %d max_id %d" % (p, max_id))
    assert len(db.query_probes([0], [-1], -1)[0][0]) >= 2       # the copy of entry 4 finds entries 4 and 7 at least
    assert db.query_probes([3], [-1], -1)[0][0].size == 0 and db.query_probes([], [], -1) == []
    each = db.query_probes([0, 1, 2], [-1, 3, n], 3)           # each probe with its own max_id
    for p, m in zip((0, 1, 2), (-1, 3, n)):
        one = db.query_probes([p], [m], 3)[0]
        assert np.array_equal(each[p][0], one[0]) and np.array_equal(each[p][1], one[1])
    for e in range(n):
        for p in range(len(probes)):
            assert db.score_probe(e, p) == rp.score(e, p), (e, p)
    assert db.score_probe(4, 0) == db.score(4, 4) and db.score_probe(0, 0) == 0.0 and db.score_probe(4, 3) == 0.0
    db.probe_feature_matches(0, [0, 4])
    db.set_probe(0, *probes[1])
    same_snapshot(snapshot(db, kfs), before)
    assert db.size() == len(kfs)
    assert db.add(*kfs[1]) == len(kfs)                           # the next entry id is the next one


@pytest.fixture(scope="module")
def mdb():
    """entries: match_pair's A, size_pair's A, a vocabulary frame; probes: their B frames and an empty one"""
    a1, b1 = K.match_pair()
    a2, b2 = P.size_pair()
    a3, b3 = K.ragged_pair()
    return fill([a1, a2, a3], [b1, P.EMPTY, b2, b3])


def test_probe_feature_matches_against_restatement(mdb):
    db, rp = mdb
    for ratio in (0.85, 1.0):
        for e in range(3):
            for probes in ([0], [1], [2], [3], [0, 1, 2], [2, 1, 3], [3, 3, 0]):           # np = 1 and 3, one probe empty
                got = db.probe_feature_matches(e, probes, ratio)
                assert len(got) == len(probes)
                for p, g in zip(probes, got):
                    same_matches(g, rp.feature_matches(e, p, ratio), (e, probes, p, ratio))
    assert db.probe_feature_matches(0, []) == []
    assert len(db.probe_feature_matches(0, [1])[0][0]) == 0
    assert len(db.probe_feature_matches(1, [2])[0][0]) > 100 and len(db.probe_feature_matches(2, [3])[0][0]) > 50


def test_probe_feature_matches_branch_by_branch(mdb):
    """match_pair's nodes, one branch of getMatches_distRatio each, with the probe in B's place"""
    db, _ = mdb
    fa, fb = K.match_pair()[0][1], K.match_pair()[1][1]
    m = dict(zip(*[x.tolist() for x in db.probe_feature_matches(0, [0], 0.85)[0]]))      # A feature -> B feature
    assert m[fa[3][0]] == fb[3][0]                           # a single candidate: the second best is none (1e9)
    assert m[fa[4][0]] == fb[4][0] and fa[14][0] not in m    # 17 / 20 passes, 18 / 20 does not
    assert fa[6][0] not in m                                 # a distance tie in B: 5 / 5
    assert fa[7][0] not in m and m[fa[7][1]] == fb[7][0]     # a later A displaces the holder when strictly closer
    assert m[fa[8][0]] == fb[8][0] and fa[8][1] not in m     # not when equal
    assert m[fa[9][0]] == fb[9][0] and fa[9][1] not in m     # nor when farther
    assert fa[13][0] not in m and not any(f in m for f in fa[2] + fa[11])      # 0 / 0 refused; nodes only one frame has
    m1 = dict(zip(*[x.tolist() for x in db.probe_feature_matches(0, [0], 1.0)[0]]))
    assert m1[fa[6][0]] == fb[6][0] and fa[13][0] not in m1                     # the first of the tie wins


def test_probe_equals_entry_of_the_same_frame(mdb):
    """probe_feature_matches(entry, probe of X) == feature_matches(entry, entry of X) on a scratch database where X was added"""
    db, _ = mdb
    frames = [K.match_pair()[1], P.EMPTY, P.size_pair()[1], K.ragged_pair()[1]]
    scratch, _ = fill([K.match_pair()[0], P.size_pair()[0], K.ragged_pair()[0]] + frames, nprobes=0)
    for e in range(3):
        for p in range(4):
            for ratio in (0.85, 1.0):
                same_matches(db.probe_feature_matches(e, [p], ratio)[0], scratch.featureMatchesBow(e, 3 + p, ratio), (e, p, ratio))
            assert db.score_probe(e, p) == scratch.score(e, 3 + p)


def best2_paths(db, ratio):
    """the one shared-node best / second-best search through featureMatchesBow and probe_feature_matches on P.best2_frames(),
    stored in db as entries 0 (A) and 1 .. 5 (B0 .. B4) and probes 0 .. 4 (B0 .. B4) -> the matches of A and each B"""
    _, Bs, near, _ = P.best2_frames()
    single = [db.probe_feature_matches(0, [p], ratio)[0] for p in range(len(Bs))]
    for p in range(len(Bs)):
        same_matches(db.featureMatchesBow(0, 1 + p, ratio), single[p], (p, ratio))
    for order in P.BEST2_ORDERS:
        got = db.probe_feature_matches(0, order, ratio)
        assert len(got) == len(order)
        for p, g in zip(order, got):
            same_matches(g, single[p], (order, p, ratio))
    assert len(single[4][0]) == 0                                   # no shared node: no item, no launch
    for p in range(4):
        assert 2 * len(single[p][0]) >= near[p] > 0, (p, len(single[p][0]), near[p])
    return single


def best2_edge_counts(A, B):
    """getMatches_distRatio's search over the shared nodes of two frames in plain numpy -> how many A features meet an empty B
    list, a single candidate or two equal minima, and how many B features are the best of two A features of a node at equal and
    at unequal distances"""
    bits_a, bits_b = np.unpackbits(A[2], axis=1).astype(np.int32), np.unpackbits(B[2], axis=1).astype(np.int32)
    c = dict(empty=0, single=0, tie=0, contested_equal=0, contested_unequal=0)
    for node in sorted(set(A[1]) & set(B[1])):
        best = {}
        for a in A[1][node]:
            d = [int(np.abs(bits_a[a] - bits_b[b]).sum()) for b in B[1][node]]
            c["empty"] += len(d) == 0
            c["single"] += len(d) == 1
            c["tie"] += len(d) > 1 and sorted(d)[0] == sorted(d)[1]
            if d and min(d) <= 75:
                best.setdefault(d.index(min(d)), []).append(min(d))
        for ds in best.values():
            c["contested_equal"] += len(ds) > 1 and len(set(ds)) == 1
            c["contested_unequal"] += len(set(ds)) > 1
    return c


@pytest.mark.parametrize("ratio", [0.85, 1.0])
def test_best2_search_paths_agree(ratio):
    """featureMatchesBow(A, B as an entry), probe_feature_matches(A, [B as a probe]) and a many-probe call give the same lists on
    frames whose shared nodes hold 1, 255, 256, 257 and 0 items, and the lists are the restatement's.  The constructed cases occur
    (counted over B0 .. B3 by best2_edge_counts): an empty B list, a single candidate, two equal minima, a contested B feature."""
    A, Bs, _, marks = P.best2_frames()
    db, rp = fill([A] + Bs, Bs)
    single = best2_paths(db, ratio)
    want = [rp.feature_matches(0, p, ratio) for p in range(len(Bs))]
    for p in range(len(Bs)):
        same_matches(single[p], want[p], (p, ratio))
    counts = [best2_edge_counts(A, B) for B in Bs[:4]]
    total = {k: sum(c[k] for c in counts) for k in counts[0]}
    assert all(v >= 1 for v in total.values()), total
    assert counts[0]["single"] == 1 and all(c["empty"] == 3 and c["tie"] >= 1 and c["contested_equal"] >= 1 and c["contested_unequal"] >= 1
                                            for c in counts[1:]), counts
    # ... and the restatement alone decides them as constructed
    for i, p in enumerate((1, 2, 3)):
        m = dict(zip(want[p][0].tolist(), want[p][1].tolist()))                 # A feature -> B feature
        (a130, b130), (a140, b140), (a150, b150), (a160, _) = ((marks[n][0], marks[n][1][i]) for n in (130, 140, 150, 160))
        assert a130[0] not in m and m[a130[1]] == b130[0]                       # the later, strictly closer A takes the B feature
        assert m[a140[0]] == b140[1] and a140[1] not in m                       # at equal distances the holder stays
        assert (m.get(a150[0]) == b150[1]) if ratio == 1.0 else (a150[0] not in m)     # the first of two equal minima
        assert not any(a in m for a in a160)
    m0, m3 = (dict(zip(want[p][0].tolist(), want[p][1].tolist())) for p in (0, 3))
    assert m0 == {marks[110][0][0]: Bs[0][1][110][0]} and m3[marks[120][0][0]] == marks[120][1][2][1]


def bf_db(prev, cur):
    db, _ = fill([(P.ONE_WORD, {}, prev)], [(P.ONE_WORD, {}, cur)], max_feats=64)
    return db


def same_bf(got, want, what=""):
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), (what, got, want)


def test_inter_matches_bf_gate_by_gate():
    c = P.bf_case()
    (dq, lids, m1, p1), (dt, m2, p2) = c["prev"], c["cur"]
    db = bf_db(dq, dt)
    got = db.probe_inter_matches_bf(0, 0, lids, m1, p1, m2, p2)
    same_bf(got, R.inter_matches_bf(dq, dt, lids, m1, p1, m2, p2))
    kept = dict(zip(got[0].tolist(), got[1].tolist()))
    assert kept == {q: t for q, t in c["want"].items() if t is not None}
    assert got[0].tolist() == [0, 2, 4, 6, 7, 8, 9, 13, 16]                # the replacing query 13 sits where query 12 claimed
    assert got[2][got[0].tolist().index(13)] == 10 and got[2][0] == 10 and got[1][0] == 0      # the tie: the lower train index
    # no landmark at all, every feature mono, points ignored
    z1, z2 = np.zeros_like(m1) + 1, np.zeros_like(m2) + 1
    none = np.full_like(lids, -1)
    same_bf(db.probe_inter_matches_bf(0, 0, none, z1, p1, z2, p2), R.inter_matches_bf(dq, dt, none, z1, p1, z2, p2))


def test_inter_matches_bf_on_random_sets():
    rng = np.random.default_rng(5)
    dt = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    dq = np.array([P._flip(rng, dt[int(rng.integers(0, 40))], 60) for _ in range(64)], np.uint8)
    lids = np.where(rng.random(64) < 0.3, rng.integers(0, 99, 64), -1).astype(np.int32)
    m1, m2 = (rng.random(64) < 0.3).astype(np.uint8), (rng.random(40) < 0.3).astype(np.uint8)
    p2 = rng.normal(0, 3, (40, 3))
    p1 = np.array([p2[int(rng.integers(0, 40))] + rng.normal(0, 1.1, 3) for _ in range(64)])
    got = bf_db(dq, dt).probe_inter_matches_bf(0, 0, lids, m1, p1, m2, p2)
    same_bf(got, R.inter_matches_bf(dq, dt, lids, m1, p1, m2, p2))
    assert 5 < len(got[0]) < 40 and len(set(got[1].tolist())) == len(got[1])


@pytest.mark.parametrize("nprev,ncur", [(3, 0), (3, 1), (3, 2), (0, 3), (0, 0), (1, 1)])
def test_inter_matches_bf_small_sets(nprev, ncur):
    """a probe of 0, 1 or 2 features, an entry of none: an empty side gives no match; with one train there is no second
    neighbour, and only a landmark's row survives (the reference reads m[1] out of bounds there)"""
    rng = np.random.default_rng(9)
    dt = rng.integers(0, 256, (ncur, 32), dtype=np.uint8)
    dq = np.array([P._flip(rng, dt[0], 20) if ncur else rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(nprev)], np.uint8).reshape(-1, 32)
    lids = np.array([-1, 7, -1][:nprev], np.int32)
    m1, m2, p1, p2 = np.zeros(nprev, np.uint8), np.zeros(ncur, np.uint8), np.zeros((nprev, 3)), np.zeros((ncur, 3))
    got = bf_db(dq, dt).probe_inter_matches_bf(0, 0, lids, m1, p1, m2, p2)
    same_bf(got, R.inter_matches_bf(dq, dt, lids, m1, p1, m2, p2), (nprev, ncur))
    if nprev == 0 or ncur == 0:
        assert len(got[0]) == 0
    elif ncur == 1 and nprev == 3:
        assert got[0].tolist() == [1] and got[1].tolist() == [0]
    elif ncur == 1:
        assert len(got[0]) == 0
    else:
        assert len(got[0]) == 1            # all three rows claim train 0 (the second train is random): one holder


def test_probe_errors():
    kfs = K.query_keyframes()
    db, _ = fill(kfs[:2], nprobes=0, max_words=64, max_feats=80)
    with pytest.raises(mcorb.McorbError) as ei:                  # no slots yet
        db.set_probe(0, *kfs[1])
    assert ei.value.code == mcorb.E_ARG
    for bad in (0, 129, -1):
        with pytest.raises(mcorb.McorbError) as ei:
            db.reserve_probes(bad)
        assert ei.value.code == mcorb.E_ARG
    db.reserve_probes(3)
    with pytest.raises(mcorb.McorbError) as ei:                  # once per database
        db.reserve_probes(3)
    assert ei.value.code == mcorb.E_STATE
    calls = (lambda p: db.get_probe(p), lambda p: db.query_probes([p], [-1], -1), lambda p: db.score_probe(0, p),
             lambda p: db.probe_feature_matches(0, [p]), lambda p: db.probe_inter_matches_bf(0, p, [], [], [], [], []))
    for call in calls:
        with pytest.raises(mcorb.McorbError) as ei:              # a slot that was never set
            call(1)
        assert ei.value.code == mcorb.E_STATE
        for bad in (-1, 3):
            with pytest.raises(mcorb.McorbError) as ei:          # an index out of range
                call(bad)
            assert ei.value.code == mcorb.E_ARG
    db.set_probe(1, *kfs[3])                                     # 64 words fit
    for bad in (kfs[4], kfs[5]):                                 # 65 words > max_words; more descriptors than max_feats
        with pytest.raises(mcorb.McorbError) as ei:
            db.set_probe(1, *bad)
        assert ei.value.code == mcorb.E_CAP
    with pytest.raises(mcorb.McorbError) as ei:                  # ids that do not ascend
        db.set_probe(1, (np.array([3, 2], np.uint32), np.array([0.5, 0.5])), {}, np.zeros((0, 32), np.uint8))
    assert ei.value.code == mcorb.E_ARG
    with pytest.raises(mcorb.McorbError) as ei:                  # a feature outside the descriptor set
        db.set_probe(1, (np.array([2], np.uint32), np.array([1.0])), {4: [0, 1]}, np.zeros((1, 32), np.uint8))
    assert ei.value.code == mcorb.E_ARG
    same_frame(db.get_probe(1), kfs[3])                          # the old probe is intact
    for bad in (-1, 2):
        with pytest.raises(mcorb.McorbError) as ei:
            db.score_probe(bad, 1)
        assert ei.value.code == mcorb.E_ARG
    full, _ = fill(kfs[:1], [kfs[1]], max_entries=1, max_words=64, max_feats=80)       # a full database still takes probes
    full.set_probe(1, *kfs[2])
    assert full.size() == 1
