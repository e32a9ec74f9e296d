"""An independent restatement of the keyframe database (mcorb_kfdb) in plain Python: DBoW2's TemplatedDatabase add / queryL1 and
L1 score, and LoopCloser::featureMatchesBow (MCSlam/src/LoopCloser.cpp:195-241).  Python floats are fp64 and add sequentially,
so the sums are the reference's.  The inverted file is a dict of lists; a query adds abs(q - d) - abs(q) - abs(d) per shared
word in query-word order.  featureMatchesBow is a merge walk that calls oracle_lib.get_matches_dist_ratio per shared node (held
against the reference's own compiled getMatches_distRatio by tests/test_reference_cpu.py).

What it cannot reproduce is std::sort's order among equal scores: `same_query` compares the score sequence exactly, the id sets
within each run of equal scores, and for a run cut by max_results only that the returned ids belong to it."""
import numpy as np

import oracle_lib as O


class RefDatabase:
    def __init__(self):
        self.ifile = {}      # word id -> [(entry id, value)], entries ascending
        self.entries = []    # (ids, vals, fv as {node: feature indices}, desc)

    def add(self, bow, fv, desc):
        e = len(self.entries)
        ids, vals = [int(w) for w in bow[0]], [float(v) for v in bow[1]]
        for w, v in zip(ids, vals):
            self.ifile.setdefault(w, []).append((e, v))
        self.entries.append((ids, vals, {int(k): [int(i) for i in f] for k, f in fv.items()},
                             np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)))
        return e

    def size(self):
        return len(self.entries)

    def query_full(self, bow, max_id=-1):
        """the whole result list before the cut: [(entry id, score)] by raw value ascending (ties in ascending id)"""
        pairs = {}
        for w, q in zip(bow[0], bow[1]):
            q = float(q)
            for e, d in self.ifile.get(int(w), ()):
                if e < max_id or max_id == -1:
                    value = abs(q - d) - abs(q) - abs(d)
                    if e in pairs:
                        pairs[e] += value
                    else:
                        pairs[e] = value
        ret = sorted(sorted(pairs.items()), key=lambda p: p[1])
        return [(e, -s / 2.0) for e, s in ret]

    def query_entry_full(self, entry, max_id=-1):
        ids, vals = self.entries[entry][:2]
        return self.query_full((ids, vals), max_id)

    def score(self, a, b):
        da = dict(zip(*self.entries[a][:2]))
        s = 0.0
        for w, v in zip(*self.entries[b][:2]):     # ascending word id
            if w in da:
                s += abs(da[w] - v) - abs(da[w]) - abs(v)
        return -s / 2.0

    def feature_matches(self, best_entry, curr_entry, ratio=0.85):
        fa, A = self.entries[best_entry][2:]
        fb, B = self.entries[curr_entry][2:]
        i1, i2 = [], []
        for node in sorted(set(fa) & set(fb)):
            mA, mB, _ = O.get_matches_dist_ratio(A, fa[node], B, fb[node], ratio)
            i1 += mA.tolist()
            i2 += mB.tolist()
        return np.array(i1, np.uint32), np.array(i2, np.uint32)


def same_query(got, full, max_results, what=""):
    """got: (ids, scores) of a database under test; full: RefDatabase.query_full's uncut list"""
    ids, scores = got
    n = len(full) if max_results <= 0 else min(max_results, len(full))
    assert len(ids) == len(scores) == n, "%s: %d results, expected %d" % (what, len(ids), n)
    ref_scores = np.array([s for _, s in full], np.float64)
    assert np.array_equal(np.asarray(scores, np.float64), ref_scores[:n]), "%s: scores differ" % what
    assert len(set(int(i) for i in ids)) == n, "%s: an entry is listed twice" % what
    i = 0
    while i < n:
        j = i
        while j < len(full) and full[j][1] == full[i][1]:
            j += 1
        run = set(e for e, _ in full[i:j])
        part = set(int(e) for e in ids[i:min(j, n)])
        if j <= n:
            assert part == run, "%s: ids of the run of score %r differ" % (what, full[i][1])
        else:
            assert part <= run, "%s: ids of the cut run of score %r are not of it" % (what, full[i][1])
        i = j
