"""What the keyframe database costs (mcorb_kfdb), device against host-only, on the same machine and inputs:
  (a) query_entries with 32 queries per call over 1 000 and 10 000 entries of ~3000 words each (word ids drawn from 100 000, so
      two keyframes share ~90 words): k_kfdb_score between HIP events against its algorithmic bytes (4 B per stored word id of
      every eligible entry + 8 B per shared word), the whole call, and the host-only database's call;
  (b) featureMatchesBow between two keyframes of 3000 LF features (near copies; ~100 FeatureVector nodes): k_kfdb_best2 between
      HIP events, the whole call, and the host-only database's call.
    python scripts/kfdb_rate.py [--entries 1000 10000] [--queries 32] [--reps 5] [--out profiles/kfdb_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WORDS, WORD_SPACE, MAX_WORDS = 3000, 100_000, 3072


def tiny_vocabulary(mcorb, device):
    """the database reads the vocabulary's scoring type and device only: two words under the root"""
    return mcorb.ORBVocabulary(device=device).create(2, 1, 0, 0, [0, 0], [1, 1], np.zeros((2, 32), np.uint8), [1.0, 1.0])


def bow(rng):
    n = int(rng.integers(WORDS - 200, WORDS + 1))
    ids = np.sort(rng.choice(WORD_SPACE, n, replace=False)).astype(np.uint32)
    v = rng.random(n) + 0.05
    return ids, v / v.sum()


def median_ms(fn, reps, min_max=None):
    """the median of reps runs; min_max: a list that receives the fastest and the slowest run, as the other rate scripts print them"""
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    if min_max is not None:
        min_max[:] = [round(min(t) * 1e3, 3), round(max(t) * 1e3, 3)]
    return float(np.median(t)) * 1e3


def query_leg(mcorb, n_entries, nq, reps):
    rng = np.random.default_rng(n_entries)
    caps = dict(max_entries=n_entries, max_words=MAX_WORDS, max_feats=1)
    dev = mcorb.ORBDatabase(tiny_vocabulary(mcorb, 0), device=0, **caps)
    host = mcorb.ORBDatabase(tiny_vocabulary(mcorb, -1), device=-1, **caps)
    none = ({}, np.zeros((0, 32), np.uint8))
    stored = 0
    for _ in range(n_entries):
        b = bow(rng)
        stored += len(b[0])
        dev.add(b, *none)
        host.add(b, *none)
    ents = [int(e) for e in rng.choice(n_entries, nq, replace=False)]
    max_ids = [-1] * nq
    got = dev.query_entries(ents, max_ids, 50)                    # (also the warm-up)
    want = host.query_entries(ents, max_ids, 50)
    same = all(np.array_equal(g[0], w[0]) and g[1].tobytes() == w[1].tobytes() for g, w in zip(got, want))
    shared = sum(len(g[0]) for g in dev.query_entries(ents, max_ids, -1))     # entries sharing a word, not words: a lower bound
    kus = []
    for _ in range(reps):
        dev.query_entries(ents, max_ids, 50)
        kus.append(dev.timing()[0])
    k_us = float(np.median(kus))
    mm = []
    alg = 4.0 * stored * nq        # the ids of every eligible entry, per query (+ 8 B per shared word: ~90 x 8 B per pair, < 7 %)
    return {"entries": n_entries, "queries_per_call": nq, "stored_words": stored, "device_equals_host": bool(same),
            "entries_listed_per_query": round(shared / nq, 1), "k_kfdb_score_us": round(k_us, 1),
            "algorithmic_MB": round(alg / 1e6, 1), "k_kfdb_score_GBps": round(alg / (k_us * 1e-6) / 1e9, 1),
            "device_call_ms": round(median_ms(lambda: dev.query_entries(ents, max_ids, 50), reps, mm), 3), "device_call_ms_min_max": mm,
            "host_only_call_ms": round(median_ms(lambda: host.query_entries(ents, max_ids, 50), max(2, reps // 2)), 3)}


def match_leg(mcorb, reps, n=3000, nodes=100):
    rng = np.random.default_rng(1)
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    bits = np.unpackbits(d1, axis=1)
    for r in bits:
        r[rng.permutation(256)[:int(rng.integers(0, 30))]] ^= 1
    perm = rng.permutation(n)
    d2 = np.packbits(bits, axis=1)[perm]
    node1 = rng.integers(0, nodes, n)
    kf = []
    for d, nd in ((d1, node1), (d2, node1[perm])):
        kf.append(((np.array([1], np.uint32), np.array([1.0])), {int(k): np.flatnonzero(nd == k) for k in np.unique(nd)}, d))
    caps = dict(max_entries=2, max_words=8, max_feats=n)
    dev = mcorb.ORBDatabase(tiny_vocabulary(mcorb, 0), device=0, **caps)
    host = mcorb.ORBDatabase(tiny_vocabulary(mcorb, -1), device=-1, **caps)
    for k in kf:
        dev.add(*k)
        host.add(*k)
    got, want = dev.featureMatchesBow(0, 1), host.featureMatchesBow(0, 1)
    kus = []
    for _ in range(reps):
        dev.featureMatchesBow(0, 1)
        kus.append(dev.timing()[1])
    mm = []
    return {"features": n, "nodes": nodes, "matches": int(len(got[0])),
            "device_equals_host": bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])),
            "k_kfdb_best2_us": round(float(np.median(kus)), 1),
            "device_call_ms": round(median_ms(lambda: dev.featureMatchesBow(0, 1), reps, mm), 3), "device_call_ms_min_max": mm,
            "host_only_call_ms": round(median_ms(lambda: host.featureMatchesBow(0, 1), reps), 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mcorb
    res = {"cores": len(os.sched_getaffinity(0)), "words_per_entry": WORDS, "word_space": WORD_SPACE,
           "query": [query_leg(mcorb, n, a.queries, a.reps) for n in a.entries], "feature_matches": match_leg(mcorb, a.reps)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
