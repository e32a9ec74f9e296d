"""Inputs shared by the probe-slot tests of the keyframe database (test_kfdb_probe_cpu.py, test_gpu_kfdb_probe.py), next to
kfdb_cases.py: the same small synthetic vocabulary, frames as (BowVector, FeatureVector, descriptors) triples, built once."""
import functools

import numpy as np

import kfdb_cases as K
import oracle_lib as O

MAX_WORDS, MAX_FEATS = 300, 520      # (520 is no multiple of 64: the device database's descriptor stride is rounded up inside)
NODE_SIZES = ((0, 1), (1, 0), (1, 1), (2, 2), (2, 63), (63, 2), (63, 63), (64, 64), (64, 65), (65, 64), (65, 1), (1, 65), (0, 65), (65, 0))
ONE_WORD = (np.array([1], np.uint32), np.array([1.0]))
EMPTY = ((np.zeros(0, np.uint32), np.zeros(0)), {}, np.zeros((0, 32), np.uint8))


def _flip(rng, row, nmax):
    d = np.unpackbits(row)
    d[rng.permutation(256)[:int(rng.integers(0, nmax))]] ^= 1
    return np.packbits(d)


@functools.lru_cache(maxsize=None)
def size_pair():
    """an (A, B) pair of frames whose shared nodes have 0, 1, 2, 63, 64 and 65 features on either side (NODE_SIZES, node ids from
    100 on); A's descriptors are flipped copies of B's of the same node, some B taken twice"""
    rng = np.random.default_rng(11)
    A, B, fa, fb = [], [], {}, {}
    for k, (na, nb) in enumerate(NODE_SIZES):
        b = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
        a = [_flip(rng, b[int(rng.integers(0, nb))], 40) if nb else rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(na)]
        fa[100 + k] = list(range(len(A), len(A) + na))
        fb[100 + k] = list(range(len(B), len(B) + nb))
        A.extend(a)
        B.extend(list(b))
    perm_a, perm_b = rng.permutation(len(A)), rng.permutation(len(B))     # feature ids are not in node order

    def frame(rows, fv, perm):
        inv = np.argsort(perm)
        return ONE_WORD, {n: [int(inv[i]) for i in f] for n, f in fv.items()}, np.array(rows, np.uint8).reshape(-1, 32)[perm]
    return frame(A, fa, perm_a), frame(B, fb, perm_b)


BEST2_ITEMS = (1, 255, 256, 257, 0)      # A's features over the nodes it shares with B0 .. B4: a lane, the 256-lane workgroup's edge, none
BEST2_ORDERS = ([0, 1, 2, 3], [3, 4, 1, 1, 0, 2])


@functools.lru_cache(maxsize=None)
def best2_frames():
    """frame A and frames B0 .. B4 from explicit FeatureVectors (exact node sizes), for the one best / second-best search behind
    featureMatchesBow, probe_feature_matches and the local map.  A's nodes (id: features) and who shares them:
      110: 1  B0, B2, B3   one B candidate: no second neighbour
      120: 1  B3           two B candidates
      130: 2  B1 .. B3     both A features are closest to the same B feature, the later one strictly closer
      140: 2  B1 .. B3     the same at equal distances
      150: 1  B1 .. B3     two equal minima in B: 4 / 4 passes at ratio 1.0 only, the first wins
      160: 3  B1 .. B3     an empty B list
      170: 100, 180: 64, 190: 81   B1 .. B3   near copies of distinct B rows (each B its own flips and order), 15 far A rows among them
      200: 1, 210: 1  B1 .. B3     near copies, three B candidates
      220: 5  nobody
    Nodes 105, 155 and 500 are in B frames only; B4 has only those.  -> (A, [B0 .. B4], near, marks): near[p] = A's near-copy
    features with a candidate in Bp; marks: node -> (A feature ids, Bp feature ids of B1 .. B3) of the hand-built nodes"""
    rng = np.random.default_rng(31)

    def rand(n):
        return rng.integers(0, 256, (n, 32), dtype=np.uint8)

    bulk = {170: 100, 180: 64, 190: 81}
    base = {n: rand(k) for n, k in bulk.items()}
    y, z, x, s1, s2, t1, t2 = rand(7)
    far = rand(40)
    a_rows = {110: [s1 ^ _bits(5)], 120: [s2 ^ _bits(9)], 130: [y ^ _bits(20), y ^ _bits(10, 100)], 140: [z ^ _bits(20), z ^ _bits(20, 100)],
              150: [x], 160: [far[0], far[1], far[2]], 200: [t1 ^ _bits(3)], 210: [t2 ^ _bits(6, 50)], 220: list(rand(5))}
    a_near = {n: [True] * len(r) for n, r in a_rows.items()}
    for n, k in bulk.items():
        a_near[n] = [bool(i % 17 != 5) for i in range(k)]                     # 6 + 4 + 5 = 15 far rows
        a_rows[n] = [_flip(rng, base[n][i], 10) if a_near[n][i] else rand(1)[0] for i in range(k)]
    assert sum(not v for n in bulk for v in a_near[n]) == 15

    def b_rows(p):
        r = np.random.default_rng(40 + p)
        rows = {105: [far[3]], 155: [far[4], far[5]], 500: [far[6]]}
        if p in (0, 2, 3):
            rows[110] = [s1]
        if p == 3:
            rows[120] = [far[7], s2]
        if p in (1, 2, 3):
            rows.update({130: [y, far[8]], 140: [far[9], z], 150: [far[10], x ^ _bits(4), x ^ _bits(4, 100), far[11]], 160: [],
                         200: [far[12], t1, far[13]], 210: [t2, far[14], far[15]]})
            for n, k in bulk.items():
                rows[n] = [_flip(r, base[n][i], 4) for i in r.permutation(k)] + list(far[16 + p:19 + p])
        return rows

    def frame(rows, seed):
        nodes = sorted(rows)
        flat = [d for n in nodes for d in rows[n]]
        perm = np.random.default_rng(seed).permutation(len(flat))              # feature ids are not in node order
        inv, fv, at = np.argsort(perm), {}, 0
        for n in nodes:
            fv[n] = [int(inv[at + i]) for i in range(len(rows[n]))]
            at += len(rows[n])
        return (ONE_WORD, fv, np.array(flat, np.uint8).reshape(-1, 32)[perm])

    A = frame(a_rows, 50)
    Bs = [frame(b_rows(p), 60 + p) for p in range(5)]
    near = []
    for p, B in enumerate(Bs):
        shared = [n for n in sorted(a_rows) if n in B[1]]
        assert sum(len(a_rows[n]) for n in shared) == BEST2_ITEMS[p]
        near.append(sum(sum(a_near[n]) for n in shared if len(B[1][n])))
    marks = {n: (A[1][n], [Bs[p][1].get(n) for p in (1, 2, 3)]) for n in (110, 120, 130, 140, 150, 160)}
    return A, Bs, tuple(near), marks


@functools.lru_cache(maxsize=None)
def _lf_pool():
    return np.random.default_rng(7).integers(0, 256, (257, 32), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def lf_frame(n, seed):
    """a frame of n LF features from the vocabulary: near copies of the first n rows of one pool, shuffled; seed -1: the pool's
    first n rows themselves"""
    pool = _lf_pool()
    if seed < 0:
        d = pool[:n].copy()
    else:
        rng = np.random.default_rng(1000 + seed)
        d = np.array([_flip(rng, r, 12) for r in pool[:n]], np.uint8).reshape(-1, 32)[rng.permutation(n)]
    bow, fv = O.bow_transform(K.vocabulary(), d, K.LEVELSUP)
    return bow, fv, d


LF_SIZES = (1, 63, 64, 65, 257)


def _bits(k, start=0):
    d = np.zeros(256, np.uint8)
    d[start:start + k] = 1
    return np.packbits(d)


@functools.lru_cache(maxsize=None)
def bf_case():
    """findInterMatches' gates one group of features at a time.  A group has a random base descriptor (about 128 bits from every
    other group's); its queries (entry) and trains (probe) are the base with k bits flipped, so distances inside a group are chosen
    and every other train is far.  -> dict(prev=(desc, lids, mono, p3d), cur=(desc, mono, p3d), want={query: train or None})"""
    rng = np.random.default_rng(21)
    Q, T, lids, m1, p1, m2, p2, want = [], [], [], [], [], [], [], {}
    above2 = float(np.nextafter(np.float32(2.0), np.float32(3.0)))

    def group(queries, trains):
        """queries: (flip start, flip count, lid, mono, point, expected train offset in the group or None); trains: (start, count, mono, point)"""
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        t0 = len(T)
        for s, k, mono, pt in trains:
            T.append(base ^ _bits(k, s)); m2.append(mono); p2.append(pt)
        for s, k, lid, mono, pt, exp in queries:
            want[len(Q)] = None if exp is None else t0 + exp
            Q.append(base ^ _bits(k, s)); lids.append(lid); m1.append(mono); p1.append(pt)

    O3 = (0.0, 0.0, 0.0)
    far = (9.0, 9.0, 9.0)
    two = [(0, 0, 0, O3), (100, 50, 0, O3)]                                   # trains at 0 and 50 bits: the ratio test passes
    group([(0, 0, 3, 0, O3, 0)], [(0, 10, 0, O3), (10, 10, 0, O3)])           # a landmark: 10 > 0.7 * 10, kept; tie: the lower train
    group([(0, 0, -1, 0, O3, None)], [(0, 10, 0, O3), (10, 10, 0, O3)])       # the same row of no landmark: dropped
    group([(0, 0, -1, 0, O3, 0)], [(0, 7, 0, O3), (100, 10, 0, O3)])          # 7 > 0.7 * 10 is false (7.0): kept
    group([(0, 0, -1, 0, O3, None)], [(0, 8, 0, O3), (100, 10, 0, O3)])       # 8 > 7.0: dropped
    group([(0, 0, -1, 0, (2.0, 0.0, 0.0), 0)], two)                           # distance exactly 2.0: kept
    group([(0, 0, -1, 0, (above2, 0.0, 0.0), None)], two)                     # the next float above: dropped
    group([(0, 0, -1, 0, (2.00000001, 0.0, 0.0), 0)], two)                    # above 2 in fp64, 2.0f as a float: kept
    group([(0, 0, -1, 0, (1.2, 1.2, 1.0), 0)], two)                           # three components: sqrt(3.88) = 1.97: kept
    group([(0, 0, -1, 1, far, 0)], two)                                       # mono in the keyframe: no depth gate
    group([(0, 0, -1, 0, far, 0)], [(0, 0, 1, O3), (100, 50, 0, O3)])         # mono in the frame: no depth gate
    group([(0, 0, -1, 0, far, None)], two)                                    # neither: dropped
    group([(0, 0, 5, 0, far, None)], two)                                     # a landmark passes the ratio gate, not the depth gate
    # four queries claim one train: 20 first, 10 replaces it in place, an equal 10 does not, 30 does not
    group([(0, 20, -1, 0, O3, None), (20, 10, -1, 0, O3, 0), (30, 10, -1, 0, O3, None), (40, 30, -1, 0, O3, None)], [(0, 0, 0, O3)])
    group([(0, 3, -1, 0, O3, 0)], two)                                        # a later group: comes after the claimed position
    return dict(prev=(np.array(Q, np.uint8), np.array(lids, np.int32), np.array(m1, np.uint8), np.array(p1, np.float64)),
                cur=(np.array(T, np.uint8), np.array(m2, np.uint8), np.array(p2, np.float64)), want=want)
