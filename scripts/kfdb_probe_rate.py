"""What matching a slot's worth of frames against one keyframe costs (mcorb_kfdb_probe_feature_matches), on the same machine and inputs:
one entry and 1, 8, 32 and 128 probes of ~3000 LF features (near copies of the entry's; ~100 FeatureVector nodes):
  device   k_kfdb_best2, many-probe launch, between HIP events against its algorithmic bytes (32 B per A descriptor of a shared node once,
           + 32 B per candidate B descriptor), and the whole probe_feature_matches call;
  (a)      the same call on the host-only database;
  (b)      the same pairs as np calls of mcorb_kfdb_feature_matches on a scratch device database where the frames were added.
The three are timed in alternating runs, `reps` each; medians are reported.
    python scripts/kfdb_probe_rate.py [--probes 1 8 32 128] [--reps 5] [--out profiles/kfdb_probe_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from kfdb_rate import tiny_vocabulary  # noqa: E402

N, NODES = 3000, 100


def frames(count):
    """the entry and `count` probes: the entry's descriptors with up to 30 bits flipped, shuffled, on the entry's nodes"""
    rng = np.random.default_rng(1)
    d1 = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    node1 = rng.integers(0, NODES, N)
    bow = (np.array([1], np.uint32), np.array([1.0]))

    def frame(d, nd):
        return bow, {int(k): np.flatnonzero(nd == k) for k in np.unique(nd)}, d
    out = [frame(d1, node1)]
    bits1 = np.unpackbits(d1, axis=1)
    for _ in range(count):
        bits = bits1.copy()
        flips = rng.integers(0, 30, N)
        for r, f in zip(bits, flips):
            r[rng.integers(0, 256, f)] ^= 1
        perm = rng.permutation(N)
        out.append(frame(np.packbits(bits, axis=1)[perm], node1[perm]))
    return out


def algorithmic_bytes(entry, probes):
    total = 0
    for p in probes:
        for node, fa in entry[1].items():
            fb = p[1].get(node)
            if fb is not None:
                total += 32 * len(fa) + 32 * len(fa) * len(fb)
    return total


def leg(mcorb, fr, np_, reps):
    caps = dict(max_words=8, max_feats=N)
    dev = mcorb.ORBDatabase(tiny_vocabulary(mcorb, 0), device=0, max_entries=1, **caps)
    host = mcorb.ORBDatabase(tiny_vocabulary(mcorb, -1), device=-1, max_entries=1, **caps)
    scratch = mcorb.ORBDatabase(tiny_vocabulary(mcorb, 0), device=0, max_entries=np_ + 1, **caps)
    sel = list(range(np_))
    for db in (dev, host):
        db.add(*fr[0])
        db.reserve_probes(np_)
        for p in sel:
            db.set_probe(p, *fr[1 + p])
    for f in fr[:np_ + 1]:
        scratch.add(*f)
    calls = {"device_call_ms": lambda: dev.probe_feature_matches(0, sel),
             "host_only_call_ms": lambda: host.probe_feature_matches(0, sel),
             "np_feature_matches_calls_ms": lambda: [scratch.featureMatchesBow(0, 1 + p) for p in sel]}
    got = {k: f() for k, f in calls.items()}                       # (also the warm-up)
    same = all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(g[0], s[0]) and np.array_equal(g[1], s[1])
               for g, w, s in zip(*got.values()))
    t = {k: [] for k in calls}
    kus = []
    for _ in range(reps):                                           # alternating
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "device_call_ms":
                kus.append(dev.probe_timing())
    alg = algorithmic_bytes(fr[0], fr[1:np_ + 1])
    k_us = float(np.median(kus))
    res = {"probes": np_, "features": N, "nodes": NODES, "matches": int(sum(len(g[0]) for g in got["device_call_ms"])),
           "device_equals_host_and_entry_calls": bool(same), "k_kfdb_best2_probes_us": round(k_us, 1),
           "algorithmic_MB": round(alg / 1e6, 2), "k_kfdb_best2_probes_GBps": round(alg / (k_us * 1e-6) / 1e9, 1)}
    for k in calls:
        res[k] = round(float(np.median(t[k])), 3)
        res[k + "_min_max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mcorb
    fr = frames(max(a.probes))
    res = {"cores": len(os.sched_getaffinity(0)), "legs": [leg(mcorb, fr, n, a.reps) for n in a.probes]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
