"""Inputs shared by the local map's CPU and GPU tests (test_lmap_cpu.py, test_gpu_lmap.py): views as plain dicts (lmap_ref.py
reads them; to_view turns one into the library's struct), hand-derived gate cases, a seeded random scene and frames whose shared
nodes have chosen sizes.  Built once per process."""
import functools
import math

import numpy as np

import kfdb_cases as K
import oracle_lib as O

W, H = 1280, 720
I3 = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
ULP = np.nextafter


def cam(R=I3, t=(0.0, 0.0, 0.0), Kmat=I3, centre=(0.0, 0.0, 0.0)):
    return dict(R=[list(map(float, r)) for r in R], t=list(map(float, t)), K=[list(map(float, r)) for r in Kmat], centre_w=list(map(float, centre)))


def view_of(cams, Rcw=I3, tcw=(0.0, 0.0, 0.0), width=W, height=H):
    return dict(Rcw=[list(map(float, r)) for r in Rcw], tcw=list(map(float, tcw)), cams=cams, width=width, height=height)


def to_view(mc, v):
    return mc.lmap_view(v["Rcw"], v["tcw"], [c["R"] for c in v["cams"]], [c["t"] for c in v["cams"]], [c["K"] for c in v["cams"]],
                        [c["centre_w"] for c in v["cams"]], v["width"], v["height"])


UP = (0.0, 0.0, 1e6)     # a normal that passes the view-angle gate for every point in front of a camera at the origin


@functools.lru_cache(maxsize=None)
def gate_cases():
    """(view, [(name, pt3D, normal, expected camera mask)]): one camera at the origin, identity rotations and K = identity, so that
    for a point (X, Y, 1) the projection is x = X, y = Y exactly (0.0 + 1 * X + 0 * Y + 0 * 1, times 1.0 / 1.0) and the bounds can
    be placed to the ulp.  With z = 0 on the optical axis tmp = (0, 0, 0), 1.0 / 0 = inf and 0 * inf = NaN: no comparison drops it.
    (z below zero with everything else passing is in normal_cases, whose K keeps the projection inside the image.)"""
    v = view_of([cam()])
    f = float
    rows = [
        # --- z == 0 (the view-angle gate reads 0 < 0.5 * 0 or 1 < 0.5: passes)
        ("z = -0.0: 0 * inf = NaN fails no comparison", (0.0, 0.0, -0.0), (0.0, 0.0, 0.0), 1),
        ("z = 0.0: the same", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1),
        ("z = 0 off the axis: x = inf", (1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0),
        ("z positive", (640.0, 360.0, 1.0), UP, 1),
        # --- bounds, (X, Y, 1)
        ("x == 30", (30.0, 360.0, 1.0), UP, 1),
        ("x one ulp below 30", (f(ULP(30.0, 0.0)), 360.0, 1.0), UP, 0),
        ("x one ulp above 30", (f(ULP(30.0, 99.0)), 360.0, 1.0), UP, 1),
        ("x == width - 30", (1250.0, 360.0, 1.0), UP, 1),
        ("x one ulp above width - 30", (f(ULP(1250.0, 9999.0)), 360.0, 1.0), UP, 0),
        ("x one ulp below width - 30", (f(ULP(1250.0, 0.0)), 360.0, 1.0), UP, 1),
        ("y == 30", (640.0, 30.0, 1.0), UP, 1),
        ("y one ulp below 30", (640.0, f(ULP(30.0, 0.0)), 1.0), UP, 0),
        ("y one ulp above 30", (640.0, f(ULP(30.0, 99.0)), 1.0), UP, 1),
        ("y == height - 30", (640.0, 690.0, 1.0), UP, 1),
        ("y one ulp above height - 30", (640.0, f(ULP(690.0, 9999.0)), 1.0), UP, 0),
        ("y one ulp below height - 30", (640.0, f(ULP(690.0, 0.0)), 1.0), UP, 1),
    ]
    return v, rows


@functools.lru_cache(maxsize=None)
def normal_cases():
    """the view-angle gate alone, to the ulp.  One camera whose projection always lands inside the image: K = [[0,0,640],[0,0,360],
    [0,0,1]] gives tmp = (640 z, 360 z, z) and (640 z) * (1 / z) within an ulp of 640.  Landmark (0, 0, 2).
    camera A: centre (0, 0, 0), curDir = (0, 0, 2), 0.5 * sqrt(4) = 1.0, normal (0, 0, n): dot = 2n, exact.
    camera B: centre (-3, -4, 2), curDir = (3, 4, 0), 0.5 * sqrt(25) = 2.5, normal (0.5, b, 0): dot = 1.5 + 4b, exact for the b used
    (4 * (0.25 -+ 2^-53) = 1 -+ 2^-51, and 2.5 -+ 2^-51 is representable: the neighbours of 2.5).
    -> [(name, view, pt, normal, expected mask)]"""
    Kc = [[0.0, 0.0, 640.0], [0.0, 0.0, 360.0], [0.0, 0.0, 1.0]]
    va, vb = view_of([cam(Kmat=Kc)]), view_of([cam(Kmat=Kc, centre=(-3.0, -4.0, 2.0))])
    pt = (0.0, 0.0, 2.0)
    return [
        ("(0,0,2): equal", va, pt, (0.0, 0.0, 0.5), 1),
        ("(0,0,2): one ulp below", va, pt, (0.0, 0.0, 0.5 - 2.0 ** -54), 0),
        ("(0,0,2): one ulp above", va, pt, (0.0, 0.0, 0.5 + 2.0 ** -53), 1),
        ("(3,4,0): equal", vb, pt, (0.5, 0.25, 0.0), 1),
        ("(3,4,0): one ulp below", vb, pt, (0.5, 0.25 - 2.0 ** -53, 0.0), 0),
        ("(3,4,0): one ulp above", vb, pt, (0.5, 0.25 + 2.0 ** -53, 0.0), 1),
        ("z negative, otherwise in bounds and well angled", va, (0.0, 0.0, -2.0), (0.0, 0.0, -1.0), 0),
        ("z slightly negative, otherwise in bounds and well angled", va, (0.0, 0.0, -1e-300), (0.0, 0.0, -1.0), 0),
        ("z slightly positive", va, (0.0, 0.0, 1e-300), (0.0, 0.0, 1.0), 1),
    ]


@functools.lru_cache(maxsize=None)
def coverage_cases():
    """four cameras that differ in t.x (0, 100, 200, 300), K = identity: the point (X, 360, 1) projects to x = X + t.x
    -> (view, [(name, pt, normal, mask)]): seen by all, by three, by one, by none"""
    v = view_of([cam(t=(100.0 * c, 0.0, 0.0)) for c in range(4)])
    return v, [("all", (640.0, 360.0, 1.0), UP, 15), ("three", (1000.0, 360.0, 1.0), UP, 7), ("one", (1240.0, 360.0, 1.0), UP, 1),
               ("none", (2000.0, 360.0, 1.0), UP, 0), ("only the last", (-265.0, 360.0, 1.0), UP, 8)]


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


@functools.lru_cache(maxsize=None)
def random_scene(ncams=4, n=2000, seed=0):
    """a rig of ncams cameras looking outwards around the y axis, posed somewhere in the world, and n landmarks around it with
    normals that mostly face away from the rig -> (view, pts, normals)"""
    rng = np.random.default_rng(100 + seed)
    Rwb = _rot(rng.normal(size=3), 0.4)                      # body in world
    twb = rng.normal(0, 2, 3)
    Rcw, tcw = Rwb.T, -Rwb.T @ twb
    cams = []
    for c in range(ncams):
        R = _rot([0, 1, 0], 2 * math.pi * c / ncams) @ _rot(rng.normal(size=3), 0.05)     # body -> camera
        t = rng.normal(0, 0.2, 3)
        f = float(rng.uniform(380, 420))
        Kc = [[f, 0.0, 640.0 + float(rng.normal(0, 5))], [0.0, f, 360.0 + float(rng.normal(0, 5))], [0.0, 0.0, 1.0]]
        centre = Rwb @ (-R.T @ t) + twb                      # translation of pose * cur_T_ref.inv()
        cams.append(cam(R, t, Kc, centre))
    body = np.stack([rng.uniform(-10, 10, n), rng.uniform(-2.5, 2.5, n), rng.uniform(-10, 10, n)], axis=1)
    pts = body @ Rwb.T + twb
    nrm = pts - twb
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm += rng.normal(0, 0.7, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return view_of(cams, Rcw, tcw), pts, nrm


@functools.lru_cache(maxsize=None)
def pool():
    """descriptors of the small vocabulary that reach a word with a weight, and their FeatureVector node at LEVELSUP"""
    desc, groups, _ = K._pool(10, 3, 4000, 1)
    rows = np.concatenate(groups)
    d = desc[np.sort(rows)]
    _, fv = O.bow_transform(K.vocabulary(), d, K.LEVELSUP)
    node = np.zeros(len(d), np.int64)
    for nid, f in fv.items():
        node[f] = nid
    return d, node


def probe_of(desc, levelsup=K.LEVELSUP):
    bow, fv = O.bow_transform(K.vocabulary(), desc, levelsup)
    return bow, fv, np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)


def flip(rng, row, nmax):
    d = np.unpackbits(row)
    d[rng.permutation(256)[:int(rng.integers(0, nmax))]] ^= 1
    return np.packbits(d)


NODE_SIZES = ((0, 1), (1, 0), (1, 1), (2, 2), (2, 63), (63, 2), (64, 64), (64, 65), (65, 64), (65, 1))


@functools.lru_cache(maxsize=None)
def sized_frames():
    """landmark descriptors (A) and a probe frame (B) whose shared FeatureVector nodes at LEVELSUP hold NODE_SIZES features, one
    pair per level-1 node of the vocabulary; half of A's rows are rows of B (some taken twice), the others are not
    -> (A descriptors, probe frame)"""
    d, node = pool()
    rng = np.random.default_rng(17)
    nodes = sorted(set(node.tolist()))
    assert len(nodes) >= len(NODE_SIZES)
    A, B = [], []
    for nid, (na, nb) in zip(nodes, NODE_SIZES):
        rows = np.flatnonzero(node == nid)
        assert len(rows) >= na + nb
        b = d[rows[:nb]]
        for i in range(na):
            A.append(b[int(rng.integers(0, nb))] if nb and i % 2 == 0 else d[rows[nb + i]])
        B.extend(list(b))
    A = np.array(A, np.uint8).reshape(-1, 32)[rng.permutation(len(A))]
    B = np.array(B, np.uint8).reshape(-1, 32)[rng.permutation(len(B))]
    return A, probe_of(B)


def _bits(k, start=0):
    d = np.zeros(256, np.uint8)
    d[start:start + k] = 1
    return np.packbits(d)


@functools.lru_cache(maxsize=None)
def branch_frames():
    """getMatches_distRatio's branches, one per FeatureVector node: K.match_pair()'s hand-built lists.  The landmarks' nodes come
    from the vocabulary, so every list is XORed with a mask (Hamming distances stay) that sends all its A rows to one node no other
    list uses -- found by trial; the probe's FeatureVector, which the caller supplies, is keyed with those nodes.
    -> (A descriptors, probe frame, levelsup, {node: name})"""
    (_, fa, Ad), (_, fb, Bd) = K.match_pair()
    levelsup = 1
    rng = np.random.default_rng(5)
    A, B, pfv, used = [], [], {}, set()
    for nid in sorted(fa):
        if nid == 20 or not fa[nid]:
            continue                                    # (65 random bases cannot share a node; sized_frames covers the sizes)
        for _ in range(400):
            mask = rng.integers(0, 256, 32, dtype=np.uint8)
            a = Ad[fa[nid]] ^ mask
            _, fv = O.bow_transform(K.vocabulary(), a, levelsup)
            if len(fv) == 1 and len(next(iter(fv.values()))) == len(a) and next(iter(fv)) not in used:
                break
        else:
            raise AssertionError("no mask found for node %d" % nid)
        vn = next(iter(fv))
        used.add(vn)
        A.extend(list(a))
        if nid in fb:
            pfv[vn] = list(range(len(B), len(B) + len(fb[nid])))
            B.extend(list(Bd[fb[nid]] ^ mask))
    pfv[10 ** 6] = [len(B)]                              # a node only the probe has
    B.append(_bits(1))
    bow = (np.array([1], np.uint32), np.array([1.0]))
    return np.array(A, np.uint8).reshape(-1, 32), (bow, pfv, np.array(B, np.uint8).reshape(-1, 32)), levelsup


def front_store(descs, mono=None, lid0=0):
    """landmarks lid0 .. that one camera at the origin sees: (lids, pts, normals, descs, mono) and the one-camera view"""
    n = len(descs)
    lids = np.arange(lid0, lid0 + n, dtype=np.int32)
    pts = np.tile(np.array([640.0, 360.0, 1.0]), (n, 1))
    nrm = np.tile(np.array(UP), (n, 1))
    mono = np.ones(n, np.uint8) if mono is None else np.asarray(mono, np.uint8)
    return view_of([cam()]), (lids, pts, nrm, np.ascontiguousarray(descs, np.uint8).reshape(-1, 32), mono)
