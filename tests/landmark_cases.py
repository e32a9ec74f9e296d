"""Inputs and helpers of the landmark tests (test_landmark_cpu.py, test_gpu_landmark.py): frames as the plain dicts landmark_ref.py
reads, the comparison of a store against the restatement (doubles as raw bytes, no tolerance), seeded batches of a chosen size and
the seeded life cycle: fill, triangulate (mapping_cases), record, then keyframes of observe, update_points and delete."""
import collections

import numpy as np

import landmark_ref as R
import mapping_cases as Mc


def bits(x):
    return np.asarray(x, np.float64).tobytes()


def frame(kf_id, match_index, centres):
    return dict(kf_id=int(kf_id), match_index=[[int(v) for v in row] for row in match_index],
                centres=[[float(v) for v in c] for c in centres])


def to_obs(mc, fr):
    mi = np.array(fr["match_index"], np.int32).reshape(len(fr["match_index"]), len(fr["centres"]))
    return mc.obs_frame(fr["kf_id"], mi, fr["centres"])


def expect(mc, code, fn):
    import pytest
    with pytest.raises(mc.McorbError) as ei:
        fn()
    assert ei.value.code == code, ei.value


def same_landmark(mc, lm, lid, l, what=""):
    """slot lid of the store against the restatement's landmark: point, normal, n_rays, observations"""
    p, q, _, _ = lm.get(lid)
    assert bits(p) == bits(l.pt3D), (what, lid, "pt3D", p.tolist(), l.pt3D)
    assert bits(q) == bits(l.normal), (what, lid, "normal", q.tolist(), l.normal)
    assert lm.observations(lid) == (l.n_rays, l.observations()), (what, lid, lm.observations(lid), l.n_rays, l.observations())


def same_map(mc, lm, ref, gone=(), what=""):
    for lid, l in ref.mapPoints.items():
        same_landmark(mc, lm, lid, l, what)
    for lid in gone:
        expect(mc, mc.E_STATE, lambda: lm.get(int(lid)))


def snapshot(lm, lids):
    """everything a store holds of the slots, for `nothing changed` checks"""
    out = []
    for l in lids:
        p, q, d, mono = lm.get(int(l))
        out.append((bits(p), bits(q), None if d is None else d.tobytes(), mono, lm.observations(int(l))))
    return out


def random_frame(rng, kf_id, ncams, nfeat, blind=0.1):
    """a keyframe near the origin: half of its features have one view, the others 2 .. ncams; a fraction `blind` has none"""
    mi = np.full((nfeat, ncams), -1, np.int32)
    for i in range(nfeat):
        if rng.random() < blind:
            continue
        nv = 1 if ncams == 1 or rng.random() < 0.5 else int(rng.integers(2, ncams + 1))
        mi[i, rng.choice(ncams, nv, replace=False)] = rng.integers(0, 1000, nv)
    base = rng.uniform(-1.0, 1.0, 3)
    return frame(kf_id, mi, base + rng.uniform(-0.2, 0.2, (ncams, 3)))


def seen_feats(fr):
    return np.array([i for i, row in enumerate(fr["match_index"]) if any(v != -1 for v in row)], np.int32)


def random_points(rng, n):
    return np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(3, 15, n)], axis=1)


def with_repeats(rng, lids, n):
    """lids plus n more occurrences of ids among them, a third of those a third time, shuffled"""
    twice = rng.choice(lids, n, replace=len(lids) < n) if n and len(lids) else np.zeros(0, np.int32)
    thrice = twice[:n // 3]
    return rng.permutation(np.concatenate([lids, twice, thrice]).astype(np.int32))


def batch(n, ncams, seed, lid0=0):
    """n observe items on a rig of ncams cameras: about half of the landmarks have two observations already (of keyframes 1 and 2,
    so that first and later observations mix within every wave), -> (points, frames before, frame, lids, feats)"""
    rng = np.random.default_rng(1000 * ncams + seed)
    nl = max(n, 1)
    pts = random_points(rng, nl)
    old = [random_frame(rng, 1 + k, ncams, 40, blind=0.0) for k in range(2)]
    had = rng.random(nl) < 0.5
    fr = random_frame(rng, 3, ncams, 200)
    lids = (lid0 + rng.permutation(nl)[:n]).astype(np.int32)
    feats = rng.choice(seen_feats(fr), n).astype(np.int32)
    return pts, old, had, fr, lids, feats


def run_batch(mc, stores, pts, old, had, fr, lids, feats, lid0=0):
    """the batch on every store and on the restatement; every touched slot compared afterwards -> the restatement"""
    ref = R.GlobalMap()
    all_lids = np.arange(lid0, lid0 + len(pts), dtype=np.int32)
    for l, p in zip(all_lids, pts):
        ref.insert(int(l), p)
    for lm in stores:
        lm.set(all_lids, pts, np.zeros_like(pts))
    pre = all_lids[had]
    rng = np.random.default_rng(len(pts))
    for k, f in enumerate(old):
        pf = rng.integers(0, len(f["match_index"]), len(pre)).astype(np.int32)
        ref.observe(f, pre, pf)
        for lm in stores:
            lm.observe(to_obs(mc, f), pre, pf)
    want = ref.observe(fr, lids, feats)
    for lm in stores:
        assert lm.observe(to_obs(mc, fr), lids, feats).tolist() == want
        same_map(mc, lm, ref)
    return ref


GATE_PT = (1.0, -2.0, 0.5)


def gate_items():
    """update_points at the gate, from the stored point GATE_PT: (name, pt_new, max_diff, replaced).  pt - pt_new is exact in every
    row (the offsets are small integers, or touch z = 0.5 alone, where 0.5 - (0.5 - d) == d for the d used)"""
    x, y, z = GATE_PT
    dn, up = float(np.nextafter(5.0, 0.0)), float(np.nextafter(5.0, np.inf))
    rows = [("d = (3, 4, 0): exactly 5.0", (x - 3.0, y - 4.0, z), 5.0, False),
            ("d = (0, 0, below 5)", (x, y, z - dn), 5.0, True),
            ("d = (0, 0, above 5)", (x, y, z - up), 5.0, False),
            ("nan", (x, float("nan"), z), 5.0, False),
            ("inf", (float("inf"), y, z), 5.0, False),
            ("-inf", (x, y, float("-inf")), 5.0, False),
            ("d = 0", (x, y, z), 5.0, True),
            ("max_diff 2.5: d = (1.5, 2, 0) equals it", (x - 1.5, y - 2.0, z), 2.5, False),
            ("max_diff 2.5: d = 2", (x, y - 2.0, z), 2.5, True),
            ("max_diff 0: d = 0 is not smaller", (x, y, z), 0.0, False),
            ("max_diff inf: d = 1e200 (its square overflows: inf < inf is false)", (x, y, 1e200), float("inf"), False),
            ("max_diff inf: d = 1e100", (x, y, 1e100), float("inf"), True),
            ("max_diff nan", (x, y, z), float("nan"), False)]
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded life cycle
# ---------------------------------------------------------------------------------------------------------------------------
def life_cycle(mc, stores, ncams, seed=7, keyframes=5):
    """On every store of `stores` and on the restatement, compared after each step:
    fill (the neighbours' landmarks of a mapping scene), triangulate_neighbours, the two observations of every new landmark
    recorded, then `keyframes` keyframes of: fresh landmarks set, observe (old, new and fresh landmarks, some of them two and three
    times), update_points over every landmark (some twice) and delete.  -> (restatement, statistics, the scene)"""
    rng = np.random.default_rng(seed)
    sc = Mc.scene(ncams, sizes=(80, 80), seed=seed, zero_f=None)
    S = len(sc["neigh"])
    results = []
    for lm in stores:
        Mc.fill_store(lm, sc["store"])
        results.append(Mc.run_scene(mc, lm, sc))
    got = results[0]
    for other in results[1:]:
        assert np.array_equal(got.new_lid, other.new_lid) and bits(got.pt3d) == bits(other.pt3d) and bits(got.normal) == bits(other.normal)
    ref = R.GlobalMap()
    for lid, X in sc["store"].items():
        ref.insert(lid, X, (0.0, 0.0, 1.0))
    # the new landmarks: point and normal as returned; n_rays is the number of views of the two features, counted here
    rec = [([], []) for _ in range(S + 1)]
    for s in range(S):
        for j, (q, t) in enumerate(sc["matches"][s]):
            i = int(got.offsets[s]) + j
            lid = int(got.new_lid[i])
            if lid < 0:
                continue
            views = int((sc["neigh"][s]["match_index"][q] != -1).sum() + (sc["cur"]["match_index"][t] != -1).sum())
            ref.insert(lid, got.pt3d[i], got.normal[i], views)
            rec[s][0].append(lid), rec[s][1].append(int(q))
            rec[S][0].append(lid), rec[S][1].append(int(t))
    stats = collections.Counter(triangulated=len(rec[S][0]))
    for lm in stores:
        same_map(mc, lm, ref, what="triangulated")
    frames = [frame(10 + s, f["match_index"], f["centre_w"]) for s, f in enumerate(sc["neigh"])] + [frame(20, sc["cur"]["match_index"], sc["cur"]["centre_w"])]
    for fr, (lids, feats) in zip(frames, rec):
        want = ref.observe(fr, lids, feats, record=True)
        for lm in stores:
            assert lm.observe(to_obs(mc, fr), lids, feats, mode=mc.OBS_RECORD).tolist() == want
    for lm in stores:
        same_map(mc, lm, ref, what="recorded")
    next_fresh, gone = 600, []
    for k in range(keyframes):
        what = "keyframe %d" % k
        fr = random_frame(rng, 30 + k, ncams, 120)
        alive = np.array(sorted(ref.mapPoints), np.int32)
        fresh = np.arange(next_fresh, next_fresh + 20, dtype=np.int32)
        next_fresh += 20
        fpts = random_points(rng, len(fresh))
        for l, p in zip(fresh, fpts):
            ref.insert(int(l), p)
        for lm in stores:
            lm.set(fresh, fpts, np.zeros_like(fpts))
        lids = with_repeats(rng, np.concatenate([rng.choice(alive, 60, replace=False), fresh]), 12)
        feats = rng.choice(seen_feats(fr), len(lids)).astype(np.int32)
        seen = set()
        for l in lids.tolist():
            repeated = l in seen
            first = not repeated and not ref.mapPoints[l].KFs       # the constructor's path; everything else is addLfFrame's
            stats["observe"] += 1
            stats["first"] += first
            stats["later"] += not first
            stats["repeated"] += repeated
            seen.add(l)
        want = ref.observe(fr, lids, feats)
        for lm in stores:
            assert lm.observe(to_obs(mc, fr), lids, feats).tolist() == want, what
            same_map(mc, lm, ref, gone, what + " observe")
        # the back-end's corrections: most small, some beyond the gate; a repeated id compares against its first result
        alive = np.array(sorted(ref.mapPoints), np.int32)
        ulids = with_repeats(rng, alive, 9)
        new_pts, want = np.zeros((len(ulids), 3)), []
        for i, l in enumerate(ulids.tolist()):
            d = rng.normal(size=3)
            r = rng.choice([rng.uniform(0.0, 1.0), rng.uniform(4.0, 4.99), rng.uniform(5.01, 9.0)], p=[0.6, 0.15, 0.25])
            new_pts[i] = np.array(ref.mapPoints[l].pt3D) + d / np.linalg.norm(d) * r
            want.append(ref.update_landmark(l, new_pts[i]))
            stats["update"] += 1
            stats["accepted" if want[-1][0] else "rejected"] += 1
        for lm in stores:
            upd, diff = lm.update_points(ulids, new_pts)
            assert upd.tolist() == [w[0] for w in want] and bits(diff) == bits([w[1] for w in want]), what
            same_map(mc, lm, ref, gone, what + " update")
        dl = rng.choice(alive, 8, replace=False).astype(np.int32)
        for lm in stores:
            assert lm.observers(alive[::3]).tolist() == ref.observers(alive[::3]), what
        pairs = [p for l in dl.tolist() for p in ref.delete_landmark(l)]
        gone += dl.tolist()
        stats["deleted_pairs"] += len(pairs)
        for lm in stores:
            assert lm.delete(dl) == pairs, what
            same_map(mc, lm, ref, gone, what + " delete")
    return ref, stats, sc


def life_cycle_is_rich(stats):
    """what the scene must exercise, shown on the restatement's own counts"""
    o, u = stats["observe"], stats["update"]
    assert stats["triangulated"] >= 20 and stats["deleted_pairs"] >= 20, stats
    assert stats["first"] >= 0.2 * o and stats["later"] >= 0.2 * o and stats["repeated"] >= 0.05 * o, stats
    assert stats["rejected"] >= 0.05 * u and stats["accepted"] >= 0.2 * u, stats
