"""Inputs and helpers of the fast-tracking tests (test_track_cpu.py, test_gpu_track.py): views as the plain dicts track_ref.py
reads, the comparison of a LocalMap.track result against the restatement (floats as raw bytes, no tolerance), flat scenes in
which a landmark's pixel is known by hand, and the seeded scene: a forward-looking rig, a few hundred landmarks around it,
keypoints made from a subset of the true projections plus noise and clutter, descriptors made from the landmark's with a few
bits flipped, and twin landmarks that compete for one keypoint."""
import math

import numpy as np

import track_ref as R

EYE = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def cam(R_=EYE, t=(0.0, 0.0, 0.0), fx=1.0, fy=1.0, s=0.0, u0=0.0, v0=0.0):
    return dict(R=[[float(v) for v in row] for row in R_], t=[float(v) for v in t], fx=float(fx), fy=float(fy), s=float(s),
                u0=float(u0), v0=float(v0))


def view(cams, cols, rows, R0=EYE, t0=(0.0, 0.0, 0.0)):
    return dict(R0=[[float(v) for v in row] for row in R0], t0=[float(v) for v in t0], cols=int(cols), rows=int(rows), cams=list(cams))


def to_view(mc, v):
    K = [[[c["fx"], c["s"], c["u0"]], [0.0, c["fy"], c["v0"]], [0.0, 0.0, 1.0]] for c in v["cams"]]
    return mc.track_view(v["R0"], v["t0"], [c["R"] for c in v["cams"]], [c["t"] for c in v["cams"]], K, v["cols"], v["rows"])


def flat_view(cols=1280, rows=720, ncams=1):
    """fx = fy = 1, u0 = v0 = 0, identity rotations, no translation: a landmark (X, Y, 1) projects to exactly (X, Y)"""
    return view([cam() for _ in range(ncams)], cols, rows)


def desc_at(base, nbits, rng=None):
    """base with nbits bits flipped (the first nbits, or a random choice)"""
    bits = np.unpackbits(np.asarray(base, np.uint8))
    idx = np.arange(nbits) if rng is None else rng.choice(256, nbits, replace=False)
    bits[idx] ^= 1
    return np.packbits(bits)


def fill(lm, store):
    lids = sorted(store)
    if lids:
        pts = np.array([store[l][0] for l in lids], np.float64).reshape(-1, 3)
        lm.set(lids, pts, np.zeros_like(pts), np.array([store[l][1] for l in lids], np.uint8))


def kp_arrays(kps, descs):
    return ([np.asarray(k, np.float32).reshape(-1, 2) for k in kps], [np.asarray(d, np.uint8).reshape(-1, 32) for d in descs])


def f32bits(v):
    return np.asarray(v, np.float32).tobytes()


def as_lists(res):
    """a TrackResult as comparable plain data, floats as raw bytes"""
    n = len(res.proj_lid)
    return dict(n_candidates=res.n_candidates, proj=[[(int(l), f32bits(p[0]), f32bits(p[1])) for l, p in zip(res.proj_lid[c], res.proj_xy[c])] for c in range(n)],
                best=[list(zip(res.best_kp[c].tolist(), res.best_dist[c].tolist())) for c in range(n)],
                matches=[list(zip(res.match_kp[c].tolist(), res.match_lid[c].tolist(), res.match_dist[c].tolist())) for c in range(n)],
                pts=[res.match_pt[c].tobytes() for c in range(n)])


def ref_lists(ref, store):
    return dict(proj=[[(l, f32bits(x), f32bits(y)) for l, x, y in p] for p in ref["proj"]], best=ref["best"], matches=ref["matches"],
                pts=[np.array([store[l][0] for _, l, _ in m], np.float64).reshape(-1, 3).tobytes() for m in ref["matches"]])


def same(got, want, what=""):
    for f in ("proj", "best", "matches", "pts"):
        assert len(got[f]) == len(want[f]), (what, f)
        for c, (a, b) in enumerate(zip(got[f], want[f])):
            assert a == b, (what, f, "camera %d" % c, a, b)


def run(mc, lm, v, store, kps, descs, lids, **kw):
    """LocalMap.track on a store that holds `store`, held against the restatement -> (the result as lists, the restatement)"""
    xy, ds = kp_arrays(kps, descs)
    got = as_lists(lm.track(to_view(mc, v), xy, ds, lids, **kw))
    ref = R.track(v, store, [a.tolist() for a in xy], ds, [int(l) for l in lids], **kw)
    same(got, ref_lists(ref, store), "store against the restatement")
    return got, ref


def snapshot(lm, lids):
    out = []
    for l in lids:
        p, q, d, mono = lm.get(int(l))
        out.append((p.tobytes(), q.tobytes(), None if d is None else d.tobytes(), mono, lm.observations(int(l))))
    return out


def expect(mc, code, fn):
    import pytest
    with pytest.raises(mc.McorbError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return ei.value


# ---------------------------------------------------------------------------------------------------------------------------
# boundary rows: (name, view, point, expected) -- expected is None (dropped from every camera) or per camera None / (x, y)
# ---------------------------------------------------------------------------------------------------------------------------
def up32(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def down32(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


COLS, ROWS = 640, 480
FLIP_Y = [[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]   # half a turn about y: a camera that looks the other way


def boundary_rows():
    v1 = flat_view(COLS, ROWS)
    rows = []
    for name, X, kept in (("x = 0", 0.0, True), ("x one ulp below 0", down32(0.0), False), ("x one ulp above 0", up32(0.0), True),
                          ("x = cols", float(COLS), True), ("x one ulp below cols", down32(COLS), True),
                          ("x one ulp above cols", up32(COLS), False),
                          # the comparison is made on the float: a double above cols that rounds to cols is kept
                          ("x a double above cols that rounds to it", COLS + 1e-9, True), ("x = -0.0", -0.0, True)):
        # (1.0 * X + 0.0 * Y + 0.0 * Z) + 0.0: X itself, and +0.0 for -0.0
        rows.append((name, v1, (X, 7.0, 1.0), [(np.float32(X + 0.0), np.float32(7.0))] if kept else [None]))
    for name, Y, kept in (("y = 0", 0.0, True), ("y one ulp below 0", down32(0.0), False), ("y one ulp above 0", up32(0.0), True),
                          ("y = rows", float(ROWS), True), ("y one ulp below rows", down32(ROWS), True),
                          ("y one ulp above rows", up32(ROWS), False), ("y a double above rows that rounds to it", ROWS + 1e-9, True)):
        rows.append((name, v1, (9.0, Y, 1.0), [(np.float32(9.0), np.float32(Y))] if kept else [None]))
    nan = np.float32(np.nan)
    rows += [("z = 0.0", v1, (1.0, 1.0, 0.0), None), ("z = -0.0", v1, (1.0, 1.0, -0.0), None),
             ("z = -1e-300", v1, (1.0, 1.0, -1e-300), None),
             ("z = 1e-300", v1, (3e-298, 2e-298, 1e-300), [(np.float32(3e-298 * (1.0 / 1e-300)), np.float32(2e-298 * (1.0 / 1e-300)))]),
             ("z = 1e-300 far outside", v1, (1.0, 1.0, 1e-300), [None]),       # x = 1e300 as a float: inf > cols
             ("z = NaN", v1, (1.0, 1.0, float("nan")), [(nan, nan)])]          # not dropped: NaN <= 0 is false, and so is NaN < 0
    # two cameras that face opposite ways: in front of one is behind the other, and project2 throws for the rig
    v2 = view([cam(), cam(R_=FLIP_Y)], COLS, ROWS)
    rows += [("opposite cameras, in front of camera 0", v2, (10.0, 10.0, 2.0), None),
             ("opposite cameras, in front of camera 1", v2, (10.0, 10.0, -2.0), None)]
    # camera 1 stands 5 ahead of camera 0: a point between them is in view of camera 0 and still leaves both
    v3 = view([cam(), cam(t=(0.0, 0.0, 5.0))], COLS, ROWS)
    rows += [("behind camera 1, in view of camera 0", v3, (30.0, 20.0, 3.0), None),
             ("in front of both", v3, (60.0, 40.0, 10.0), [(np.float32(60.0 * (1.0 / 10.0)), np.float32(40.0 * (1.0 / 10.0))),
                                                            (np.float32(60.0 * (1.0 / 5.0)), np.float32(40.0 * (1.0 / 5.0)))]),
             ("in view of camera 0 alone", v3, (3500.0, 40.0, 10.0), [(np.float32(3500.0 * (1.0 / 10.0)), np.float32(40.0 * (1.0 / 10.0))), None])]
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# flat scenes: one camera, landmark i at (x, y, 1) with descriptor d -- its query is exactly (x, y)
# ---------------------------------------------------------------------------------------------------------------------------
def flat_store(queries, first_lid=0):
    """queries: [(x, y, descriptor)] -> store with lids first_lid .."""
    return {first_lid + i: ((float(x), float(y), 1.0), np.asarray(d, np.uint8)) for i, (x, y, d) in enumerate(queries)}


def ring(cx, cy, n, r0=10.0, step=1.0):
    """n keypoints left of (cx, cy) at distances r0, r0 + step, .. -- exact in float, so keypoint i is the (i + 1)-th nearest"""
    return [(cx - (r0 + step * i), cy) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded scene
# ---------------------------------------------------------------------------------------------------------------------------
def rot(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    M = np.eye(3)
    M[i, i], M[i, j], M[j, i], M[j, j] = c, -s, s, c
    return M


def scene(ncams, seed=0, n_landmarks=340, n_twins=260, cols=1280, rows=720):
    """-> (view, store, kps, descs, lids).  The rig looks along +z from near the origin (a landmark behind any camera leaves all of
    them); landmarks fill a box around it, so some are behind and some beside the images; twins sit almost on their original and
    carry the same descriptor with other bits flipped, so two or three landmarks reach for one keypoint; keypoints come from 70 % of
    the projections left of 0.78 * cols (the right edge stays bare), moved by a pixel or two, plus scattered clutter and one dense
    clump; lids names every landmark, in shuffled order, with -1 and repeats mixed in"""
    rng = np.random.default_rng(1000 * ncams + seed)
    cams = []
    for c in range(ncams):
        Rc = rot(1, rng.uniform(-0.06, 0.06)) @ rot(0, rng.uniform(-0.04, 0.04)) @ rot(2, rng.uniform(-0.03, 0.03))
        t = (0.25 * (c % 4) - 0.4 + rng.uniform(-0.02, 0.02), 0.2 * (c // 4) - 0.3, rng.uniform(-0.05, 0.05))
        cams.append(cam(Rc, t, fx=700.0 + rng.uniform(-20, 20), fy=700.0 + rng.uniform(-20, 20), s=rng.uniform(-0.5, 0.5),
                        u0=cols / 2 + rng.uniform(-10, 10), v0=rows / 2 + rng.uniform(-10, 10)))
    R0 = rot(1, 0.05) @ rot(0, -0.03)
    v = view(cams, cols, rows, R0, (0.3, -0.2, 0.5))
    pts = np.stack([rng.uniform(-7, 7, n_landmarks), rng.uniform(-4, 4, n_landmarks), rng.uniform(-5, 9, n_landmarks)], axis=1)
    base = rng.integers(0, 256, (n_landmarks, 32), dtype=np.uint8)
    store = {i: (tuple(pts[i].tolist()), desc_at(base[i], int(rng.integers(0, 9)), rng)) for i in range(n_landmarks)}
    origin = {i: i for i in range(n_landmarks)}
    seen0 = [lid for lid, _, _ in R.project(v, store, range(n_landmarks))[0][0]]     # twins of what camera 0 sees
    for k in range(n_twins):
        o = int(rng.choice(seen0))
        lid = n_landmarks + k
        store[lid] = (tuple((pts[o] + rng.normal(0, 0.002, 3)).tolist()), desc_at(base[o], int(rng.integers(0, 9)), rng))
        origin[lid] = o
    lids = list(rng.permutation(len(store)))
    proj, _ = R.project(v, store, lids)
    kps, descs = [], []
    for c in range(ncams):
        xy, ds, done = [], [], set()
        for lid, x, y in proj[c]:
            o = origin[lid]
            if o in done or float(x) > 0.78 * cols or rng.random() > 0.7:
                continue
            done.add(o)
            xy.append((float(x) + rng.normal(0, 1.5), float(y) + rng.normal(0, 1.5)))
            ds.append(desc_at(base[o], int(rng.choice([2, 5, 9, 14, 18, 19, 20, 21, 26, 40])), rng))
        nclutter = max(len(xy) // 3, 8) if c % 5 != 3 else 0
        for _ in range(nclutter):
            xy.append((rng.uniform(0, 0.8 * cols), rng.uniform(0, rows)))
            ds.append(rng.integers(0, 256, 32, dtype=np.uint8))
        for _ in range(40 if c % 5 != 3 else 0):                       # the clump: more than 10 keypoints within reach
            xy.append((0.3 * cols + rng.normal(0, 50), 0.4 * rows + rng.normal(0, 50)))
            ds.append(rng.integers(0, 256, 32, dtype=np.uint8))
        if ncams > 4 and c == 3:                                          # one camera of a larger rig sees nothing
            xy, ds = [], []
        order = rng.permutation(len(xy))
        kps.append(np.array(xy, np.float32).reshape(-1, 2)[order])
        descs.append(np.array(ds, np.uint8).reshape(-1, 32)[order])
    lids = [int(l) for l in lids]
    for at in sorted(rng.integers(0, len(lids), 25).tolist(), reverse=True):
        lids.insert(at, -1 if at % 2 else lids[at // 2])
    return v, store, kps, descs, lids


def shares(stats):
    s = dict(stats)
    for k in ("z", "bounds", "projected"):
        s[k + "_share"] = stats[k] / max(stats["pairs"], 1)
    for k in ("matched", "gated", "empty", "crowded"):
        s[k + "_share"] = stats[k] / max(stats["queries"], 1)
    return s
