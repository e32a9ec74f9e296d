"""Inputs shared by the keyframe database's CPU and GPU tests (test_kfdb_cpu.py, test_gpu_kfdb.py): keyframes as
(BowVector, FeatureVector, descriptors) triples, built once per process."""
import functools

import numpy as np

import oracle_lib as O

LEVELSUP = 2
MAX_WORDS, MAX_FEATS = 200, 256
WORD_COUNTS = (0, 1, 63, 64, 65, 129, MAX_WORDS)


@functools.lru_cache(maxsize=None)
def vocabulary(k=10, L=3):
    return O.make_vocabulary(k=k, L=L)     # its 5 % zero-weight words stay in


@functools.lru_cache(maxsize=None)
def _pool(k, L, n, seed):
    """n random descriptors and, per vocabulary word that any of them reaches with a weight, the descriptors that reach it;
    `stopped`: the descriptors that reach a zero-weight word"""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    _, fv = O.bow_transform(vocabulary(k, L), desc, 0)     # levelsup 0: the FeatureVector is keyed by the word's own node
    groups = [np.asarray(fv[node]) for node in sorted(fv)]
    seen = np.zeros(n, bool)
    for g in groups:
        seen[g] = True
    return desc, groups, np.flatnonzero(~seen)


def keyframe(nwords, seed, k=10, L=3, pool=4000, extra=8):
    """a descriptor set whose BowVector has exactly nwords words: one descriptor for each of nwords words, a second one for up to
    `extra` of them, and up to 4 descriptors of zero-weight words; transformed as a whole"""
    desc, groups, stopped = _pool(k, L, pool, 1)
    rng = np.random.default_rng(seed)
    assert nwords <= len(groups)
    pick = rng.permutation(len(groups))[:nwords]
    rows = [groups[g][0] for g in pick]
    rows += [groups[g][1] for g in pick[:extra] if len(groups[g]) > 1]
    if nwords:
        rows += stopped[:4].tolist()
    rows = np.array(rows, np.int64)[rng.permutation(len(rows))] if rows else np.zeros(0, np.int64)
    d = desc[rows]
    bow, fv = O.bow_transform(vocabulary(k, L), d, LEVELSUP)
    assert len(bow[0]) == nwords
    return bow, fv, d


@functools.lru_cache(maxsize=None)
def query_keyframes():
    """the entries of the query / score tests, in add order"""
    kfs = [keyframe(n, 10 + i) for i, n in enumerate(WORD_COUNTS)]
    kfs.append(kfs[4])                                                    # identical to the 65-word entry: a score tie
    w = kfs[3][0][0][0]
    kfs.append(((np.array([w], np.uint32), np.array([0.0])), {}, np.zeros((0, 32), np.uint8)))   # a 0.0 on a shared word
    kfs.append(((np.array([10 ** 6], np.uint32), np.array([1.0])), {}, np.zeros((0, 32), np.uint8)))   # shares no word
    return kfs


def hand_queries():
    """query vectors that are no entry: empty, a 0.0 value on a shared word, a fresh keyframe's"""
    kfs = query_keyframes()
    return [(np.zeros(0, np.uint32), np.zeros(0)), kfs[8][0], keyframe(100, 99)[0]]


def small_keyframes(n, seed=5):
    """n keyframes of 20 .. 40 words over a narrow range of the vocabulary, so that they share words"""
    desc, groups, _ = _pool(10, 3, 4000, 1)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        pick = rng.permutation(120)[:int(rng.integers(20, 41))]
        d = desc[[groups[g][0] for g in pick]]
        bow, fv = O.bow_transform(vocabulary(), d, LEVELSUP)
        out.append((bow, fv, d))
    return out


def _bits(k, start=0):
    """a descriptor with k bits set from bit `start` on: Hamming distance k from zero"""
    d = np.zeros(256, np.uint8)
    d[start:start + k] = 1
    return np.packbits(d)


@functools.lru_cache(maxsize=None)
def match_pair():
    """two hand-built keyframes (best = A, current = B) whose shared nodes walk getMatches_distRatio's branches, one per node"""
    rng = np.random.default_rng(3)
    A, B, fa, fb = [], [], {}, {}

    def node(nid, a_descs, b_descs):
        if a_descs is not None:
            fa[nid] = list(range(len(A), len(A) + len(a_descs)))
            A.extend(a_descs)
        if b_descs is not None:
            fb[nid] = list(range(len(B), len(B) + len(b_descs)))
            B.extend(b_descs)

    far = _bits(200, 56)
    node(1, [], [_bits(0), far])                                        # empty A list
    node(2, [_bits(3), _bits(4)], [])                                   # empty B list
    node(3, [_bits(10)], [_bits(0)])                                    # one B: the second best is 1e9
    node(4, [_bits(0)], [_bits(17), _bits(20, 128)])                    # 17 / 20 = 0.85 passes
    node(5, None, [_bits(1)])                                           # a node only B has
    node(6, [_bits(5)], [_bits(0), _bits(0), far])                      # duplicates in B: 5 / 5 fails at 0.85, passes at 1.0, first wins
    node(7, [_bits(20), _bits(10)], [_bits(0), far])                    # the later A is strictly better: replaces
    node(8, [_bits(20), _bits(20, 100)], [_bits(0), far])               # equal: the holder stays
    node(9, [_bits(20), _bits(30)], [_bits(0), far])                    # worse: the holder stays
    node(10, [_bits(75), _bits(76)], [_bits(0)])                        # TH_LOW: 75 passes, 76 does not
    node(11, [_bits(2)], None)                                          # a node only A has
    node(13, [_bits(0)], [_bits(0), _bits(0)])                          # 0 / 0: NaN, refused at any ratio
    node(14, [_bits(0)], [_bits(18), _bits(20, 128)])                   # 18 / 20 does not pass
    b65 = rng.integers(0, 256, (65, 32), dtype=np.uint8)                # 65 x 65: flipped copies, some B taken twice
    a65 = []
    for i in range(65):
        d = np.unpackbits(b65[int(rng.integers(0, 40))])
        d[rng.permutation(256)[:int(rng.integers(0, 40))]] ^= 1
        a65.append(np.packbits(d))
    node(20, a65, list(b65))
    node(21, [_bits(7), _bits(9)], [_bits(8, 3), _bits(1)])             # two of each
    node(30, None, [_bits(1)])
    bow = (np.array([1], np.uint32), np.array([1.0]))
    return (bow, fa, np.array(A, np.uint8).reshape(-1, 32)), (bow, fb, np.array(B, np.uint8).reshape(-1, 32))


def ragged_pair(seed=8):
    """two keyframes from the vocabulary whose descriptors are near copies of each other: many shared nodes of small lists"""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    bits = np.unpackbits(d1, axis=1)
    for r in bits:
        r[rng.permutation(256)[:int(rng.integers(0, 12))]] ^= 1
    d2 = np.packbits(bits, axis=1)[rng.permutation(200)]
    out = []
    for d in (d1, d2):
        bow, fv = O.bow_transform(vocabulary(), d, LEVELSUP)
        out.append((bow, fv, d))
    return out
