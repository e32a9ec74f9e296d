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
