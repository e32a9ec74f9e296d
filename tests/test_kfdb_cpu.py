"""The keyframe database (mcorb_kfdb: DBoW2's TemplatedDatabase add / query, the vocabulary's score, LoopCloser::featureMatchesBow)
in its host-only form (device -1), against the plain-Python restatement of tests/kfdb_ref.py.  No GPU is needed."""
import itertools

import numpy as np
import pytest

import kfdb_cases as K
import kfdb_ref
import mcorb
import oracle_lib as O
from kfdb_ref import same_query


def host_voc(**kw):
    return mcorb.ORBVocabulary(device=-1).create(**(O.make_vocabulary(**kw) if kw else K.vocabulary()))


def fill(kfs, device=-1, voc=None, **caps):
    caps = dict(dict(max_entries=len(kfs) + 2, max_words=K.MAX_WORDS, max_feats=K.MAX_FEATS), **caps)
    db = mcorb.ORBDatabase(voc or host_voc(), device=device, **caps)
    ref = kfdb_ref.RefDatabase()
    for i, kf in enumerate(kfs):
        assert db.add(*kf) == i == ref.add(*kf)
    return db, ref


@pytest.fixture(scope="module")
def qdb():
    return fill(K.query_keyframes())


def test_entry_ids_count_from_zero_and_entries_round_trip(qdb):
    db, _ = qdb
    kfs = K.query_keyframes()
    assert db.size() == len(kfs)
    assert [len(kf[0][0]) for kf in kfs[:7]] == list(K.WORD_COUNTS)
    for i, (bow, fv, desc) in enumerate(kfs):
        (ids, vals), gfv, gdesc = db.entry(i)
        assert np.array_equal(ids, bow[0]) and vals.tobytes() == np.asarray(bow[1], np.float64).tobytes(), i
        assert sorted(gfv) == sorted(fv) and all(np.array_equal(gfv[k], fv[k]) for k in fv), i
        assert np.array_equal(gdesc, desc), i


def test_query_against_restatement(qdb):
    """every entry and the hand vectors as queries, every max_id and max_results of the issue"""
    db, ref = qdb
    n = db.size()
    queries = [kf[0] for kf in K.query_keyframes()] + K.hand_queries()
    seen_tie = seen_zero = False
    for max_id, max_results in itertools.product((-1, 0, 1, n - 1, n, n + 5), (-1, 0, 1, 3, n + 5)):
        for qi, q in enumerate(queries):
            full = ref.query_full(q, max_id)
            got = db.query(q, max_results, max_id)
            same_query(got, full, max_results, "query %d max_id %d max_results %d" % (qi, max_id, max_results))
            assert all(max_id == -1 or e < max_id for e in got[0])
            seen_tie |= len(full) > len(set(s for _, s in full))
            seen_zero |= any(s == 0.0 for _, s in full)
    assert seen_tie and seen_zero      # the identical entries tie; the 0.0-valued word is present with score zero
    assert db.query(queries[len(K.query_keyframes())], -1)[0].size == 0     # the empty vector finds nothing
    # the entry that shares no word with anyone finds only itself
    ids, scores = db.query(K.query_keyframes()[9][0], -1)
    assert ids.tolist() == [9] and scores.tolist() == [1.0]


def test_query_entries_equals_query(qdb):
    db, ref = qdb
    n = db.size()
    ents = list(range(n))
    for max_results in (-1, 3):
        max_ids = [(-1, 0, 1, n - 1, n, n + 5)[e % 6] for e in ents]
        got = db.query_entries(ents, max_ids, max_results)
        for e, g in zip(ents, got):
            one = db.query(K.query_keyframes()[e][0], max_results, max_ids[e])
            assert np.array_equal(g[0], one[0]) and np.array_equal(g[1], one[1])
            same_query(g, ref.query_entry_full(e, max_ids[e]), max_results, "entry %d" % e)
    assert db.query_entries([], [], -1) == []


def test_score_against_restatement(qdb):
    db, ref = qdb
    n = db.size()
    for a, b in itertools.product(range(n), range(n)):
        assert db.score(a, b) == ref.score(a, b), (a, b)
    for a in range(1, 7):
        assert db.score(a, a) == ref.score(a, a) and abs(db.score(a, a) - 1.0) < 1e-12      # L1-normalised vectors
    assert db.score(0, 3) == 0.0 and db.score(9, 1) == 0.0 and db.score(1, 9) == 0.0     # empty / disjoint vectors
    assert db.score(4, 7) == db.score(4, 4)                                            # the identical entries


def test_known_answer_by_hand():
    """three entries of three words with dyadic values: per shared word |q - d| - |q| - |d|, the score is -sum / 2
    E0 vs E0: 3 words, -2v each = -2 -> 1.0;  E0 vs E1: word 1: 0.25 - 0.5 - 0.25 = -0.5, word 2: 0.25 - 0.25 - 0.5 = -0.5 -> 0.5;
    E2 shares nothing"""
    none = ({}, np.zeros((0, 32), np.uint8))
    kfs = [((np.array(w, np.uint32), np.array(v)),) + none for w, v in
           (((1, 2, 3), (0.5, 0.25, 0.25)), ((1, 2, 4), (0.25, 0.5, 0.25)), ((5, 6, 7), (0.5, 0.25, 0.25)))]
    db, _ = fill(kfs)
    ids, scores = db.query(kfs[0][0], -1)
    assert ids.tolist() == [0, 1] and scores.tolist() == [1.0, 0.5]
    ids, scores = db.query(kfs[1][0], -1)
    assert ids.tolist() == [1, 0] and scores.tolist() == [1.0, 0.5]
    ids, scores = db.query(kfs[2][0], 1)
    assert ids.tolist() == [2] and scores.tolist() == [1.0]
    assert db.query(kfs[0][0], -1, max_id=1)[0].tolist() == [0]
    assert db.query(kfs[0][0], 1)[0].tolist() == [0]
    assert (db.score(0, 1), db.score(1, 0), db.score(0, 2), db.score(2, 2)) == (0.5, 0.5, 0.0, 1.0)
    got = db.query_entries([0, 1, 2], [-1, 1, 2], -1)
    assert [g[0].tolist() for g in got] == [[0, 1], [0], []] and got[1][1].tolist() == [0.5]


def test_feature_matches_branch_by_branch():
    a, b = K.match_pair()
    db, ref = fill([a, b])
    for ratio in (0.85, 1.0):
        i1, i2 = db.featureMatchesBow(0, 1, ratio)
        r1, r2 = ref.feature_matches(0, 1, ratio)
        assert np.array_equal(i1, r1) and np.array_equal(i2, r2), ratio
    fa, fb = a[1], b[1]
    m = dict(zip(*[x.tolist() for x in db.featureMatchesBow(0, 1, 0.85)]))      # A feature -> B feature
    assert m[fa[3][0]] == fb[3][0]                      # one B: second best 1e9
    assert m[fa[4][0]] == fb[4][0]                      # 17 / 20 == 0.85 passes
    assert fa[14][0] not in m                           # 18 / 20 does not
    assert fa[6][0] not in m                            # duplicates: 5 / 5
    assert fa[7][0] not in m and m[fa[7][1]] == fb[7][0]     # strictly better: replaced
    assert m[fa[8][0]] == fb[8][0] and fa[8][1] not in m     # equal: kept
    assert m[fa[9][0]] == fb[9][0] and fa[9][1] not in m     # worse: kept
    assert m[fa[10][0]] == fb[10][0] and fa[10][1] not in m  # 75 passes, 76 does not
    assert fa[13][0] not in m and not any(f in m for f in fa[2] + fa[11])
    m1 = dict(zip(*[x.tolist() for x in db.featureMatchesBow(0, 1, 1.0)]))
    assert m1[fa[6][0]] == fb[6][0] and fa[13][0] not in m1      # the first duplicate wins; 0 / 0 is refused at any ratio
    assert len([f for f in fa[20] if f in m]) > 20               # the 65 x 65 node matches, with replacements
    # the other way round the roles swap
    i1, i2 = db.featureMatchesBow(1, 0)
    r1, r2 = ref.feature_matches(1, 0)
    assert np.array_equal(i1, r1) and np.array_equal(i2, r2)


def test_feature_matches_on_vocabulary_keyframes():
    kfs = K.ragged_pair()
    db, ref = fill(kfs)
    for a, b in ((0, 1), (1, 0), (0, 0)):
        i1, i2 = db.featureMatchesBow(a, b)
        r1, r2 = ref.feature_matches(a, b)
        assert np.array_equal(i1, r1) and np.array_equal(i2, r2)
        assert len(i1) > 50


def test_caps_and_errors():
    kfs = K.query_keyframes()
    db, _ = fill(kfs[:3], max_entries=3)
    with pytest.raises(mcorb.McorbError) as ei:
        db.add(*kfs[3])
    assert ei.value.code == mcorb.E_CAP and db.size() == 3
    db, _ = fill(kfs[:2], max_entries=4, max_words=64, max_feats=80)
    before = [db.query(kf[0], -1) for kf in kfs[:5]]
    for bad in (kfs[4], kfs[5]):                        # 65 words > max_words; more descriptors than max_feats
        with pytest.raises(mcorb.McorbError) as ei:
            db.add(*bad)
        assert ei.value.code == mcorb.E_CAP
    assert db.size() == 2
    after = [db.query(kf[0], -1) for kf in kfs[:5]]
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(before, after))
    assert db.add(*kfs[3]) == 2                         # 64 words fit
    with pytest.raises(mcorb.McorbError) as ei:         # ids that do not ascend
        db.add((np.array([3, 2], np.uint32), np.array([0.5, 0.5])), {}, np.zeros((0, 32), np.uint8))
    assert ei.value.code == mcorb.E_ARG
    with pytest.raises(mcorb.McorbError) as ei:         # a feature outside the descriptor set
        db.add((np.array([2], np.uint32), np.array([1.0])), {4: [0, 1]}, np.zeros((1, 32), np.uint8))
    assert ei.value.code == mcorb.E_ARG and db.size() == 3
    for bad in (-1, 3):
        with pytest.raises(mcorb.McorbError) as ei:
            db.score(0, bad)
        assert ei.value.code == mcorb.E_ARG


def test_only_l1_vocabularies():
    for scoring in (1, 2, 5):
        with pytest.raises(mcorb.McorbError) as ei:
            mcorb.ORBDatabase(host_voc(k=10, L=3, scoring=scoring), device=-1)
        assert ei.value.code == mcorb.E_ARG
    voc = host_voc()
    with pytest.raises(mcorb.McorbError) as ei:         # a host-only vocabulary has no device tables
        voc.transform(np.zeros((1, 32), np.uint8))
    assert ei.value.code == mcorb.E_NODEVICE
