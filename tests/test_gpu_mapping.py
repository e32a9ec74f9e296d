"""The mapping step on the device (device >= 0: k_map_depth, k_map_triangulate, k_map_put) against the host-only store (device -1)
on the same inputs, bit for bit: every integer, and every double compared as raw bytes; on the inputs of test_mapping_cpu.py."""
import numpy as np
import pytest

import kfdb_cases as K
import lmap_cases as Lc
import mapping_cases as Mc
from test_lmap_cpu import free, make, same_result
from test_mapping_cpu import I3, bits, gate_cases, ref_gate, ref_of, same_as_ref, same_gate

pytestmark = pytest.mark.gpu

FIELDS = ("inliers", "verdict", "new_lid", "pt3d", "normal", "dist2", "cos_parallax", "neigh_skipped", "depth_vec", "lids_cur", "offsets")


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def stores(mc, vocs, sc, max_landmarks=4096):
    out = []
    for voc, dev in zip(vocs, (0, -1)):
        lm = mc.LocalMap(voc, device=dev, max_landmarks=max_landmarks, max_candidates=16)
        Mc.fill_store(lm, sc["store"])
        out.append(lm)
    return out


def same(got, want, what=""):
    for f in FIELDS:
        a, b = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, f)
    assert len(got.lids_neigh) == len(want.lids_neigh) and all(np.array_equal(a, b) for a, b in zip(got.lids_neigh, want.lids_neigh)), what
    assert (got.n_triangulated, got.next_lid) == (want.n_triangulated, want.next_lid), what


def both(mc, vocs, sc):
    lm_d, lm_h = stores(mc, vocs, sc)
    got, want = Mc.run_scene(mc, lm_d, sc), Mc.run_scene(mc, lm_h, sc)
    same(got, want)
    return lm_d, lm_h, got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_match_counts(mc, vocs, n):
    """the wave edges of k_map_triangulate (64 lanes, one neighbour per wave) in one neighbour"""
    sc = Mc.scene(4, sizes=(n,), seed=n + 1, zero_f=None)
    lm_d, _, got = both(mc, vocs, sc)
    assert len(got.verdict) == n and lm_d.last_triangulate_timing()[2] <= n
    if n >= 63:
        assert 0 < got.n_triangulated < n and len(set(got.verdict.tolist())) >= 5


@pytest.mark.parametrize("sizes", [(257,), (100, 157), (60, 0, 97, 50, 50)])
def test_segments(mc, vocs, sizes):
    """the same total over 1, 2 and 5 neighbours: the segment boundaries of the one submission, a neighbour of 0 matches between
    two others and a skipped neighbour"""
    sc = Mc.scene(4, sizes=sizes, seed=11, zero_f=None)
    if len(sizes) == 5:
        sc["neigh"][3]["twc"] = sc["cur"]["twc"].copy()      # no baseline: skipped
    _, _, got = both(mc, vocs, sc)
    assert len(got.verdict) == 257 and got.n_triangulated > 40
    if len(sizes) == 5:
        assert got.neigh_skipped.tolist() == [0, 0, 0, 1, 0] and (got.verdict[157:207] == 7).all() and (got.verdict[207:] != 7).all()


def test_view_counts_in_one_call(mc, vocs):
    """1 + 1, 2 + 1, 2 + 2, 4 + 4 and 8 + 8 views in one mixed batch: both instances of k_map_triangulate run, 8 + 8 is the most
    the general one takes"""
    rng = np.random.default_rng(4)
    Ks, rigT = Mc.make_rig(8, rng)
    cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(0.02, -0.01, 0.03), np.zeros(3)), rigT), Ks)
    nb = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(-0.03, 0.05, 0.0), np.array([1.1, 0.05, -0.1])), rigT), Ks)
    nb.add(np.array([0.0, 0.0, 5.0]), [0], rng, lid=900)
    shapes = [(1, 1), (2, 1), (2, 2), (4, 4), (8, 8)]
    ms, nvs = [], []
    for i in range(150):
        a, b = shapes[i % 5]
        X = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 15)])
        ms.append((nb.add(X, sorted(rng.choice(8, a, replace=False).tolist()), rng), cur.add(X, sorted(rng.choice(8, b, replace=False).tolist()), rng)))
        nvs.append(a + b)
    F = np.array([[Mc.fundamental(cur.g["full"][cc], nb.g["full"][cn], Ks[cc], Ks[cn]) for cn in range(8)] for cc in range(8)])
    Tcw = np.linalg.inv(cur.g["pose"])
    sc = dict(K=np.array(Ks), inv_sigma2=Mc.INV_SIGMA2, cur=cur.done(), neigh=[nb.done()], F21=[F], store={900: np.array([0.0, 0.0, 5.0])},
              matches=[np.array(ms, np.int32)], Rcw=Tcw[:3, :3], tcw=Tcw[:3, 3], next_lid=0)
    lm_d, _, got = both(mc, vocs, sc)
    assert lm_d.last_triangulate_timing()[2] == 150
    nvs = np.array(nvs)
    for nv in (2, 3, 4, 8, 16):
        assert (got.verdict[nvs == nv] == 0).sum() >= 20, nv
    same_as_ref(got, ref_of(sc), 150)


def test_boundary_cases_in_one_launch(mc):
    rows = gate_cases()
    got = Mc.run_gates(mc, [r[1] for r in rows], device=0)
    host = Mc.run_gates(mc, [r[1] for r in rows])
    for (name, c, v), g, h in zip(rows, got, host):
        assert g[0] == v, (name, g)
        same_gate(g, h, name)
        same_gate(g, ref_gate(c), name)


def test_random_scene_and_write_back(mc, vocs):
    """3 neighbours x 300 matches on a 4-camera rig; every new id reads back from HBM as returned, every other slot is unchanged,
    and a search that includes the new ids equals the host-only store's"""
    sc = Mc.scene(4, sizes=(300, 300, 300), seed=3)
    pool = Lc.pool()[0]
    probe = Lc.probe_of(pool[:257])
    (lm_d, db_d), (lm_h, db_h) = make(mc, vocs[0], 0, probe), make(mc, vocs[1], -1, probe)
    old = np.array(sorted(sc["store"]), np.int32)
    for lm in (lm_d, lm_h):
        Mc.fill_store(lm, sc["store"])
    before = [lm_d.get(int(l)) for l in old]
    got, want = Mc.run_scene(mc, lm_d, sc), Mc.run_scene(mc, lm_h, sc)
    same(got, want)
    same_as_ref(got, ref_of(sc), 900)
    us = lm_d.last_triangulate_timing()
    assert us[0] > 0 and us[1] > 0 and 0 < us[2] <= 900 and us[3] == len(old)
    new = got.new_lid[got.new_lid >= 0]
    assert len(new) == got.n_triangulated > 200 and new.tolist() == list(range(sc["next_lid"], sc["next_lid"] + len(new)))
    for i in np.nonzero(got.new_lid >= 0)[0]:
        p, q, d, _ = lm_d.get(int(got.new_lid[i]))
        assert bits(p) == bits(got.pt3d[i]) and bits(q) == bits(got.normal[i]) and d is None
    for l, b in zip(old, before):
        a = lm_d.get(int(l))
        assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1])
    with pytest.raises(mc.McorbError):
        lm_d.get(int(new[-1]) + 1)
    # the new landmarks get descriptors and are searched: a camera at the current frame's place, 640 x 480
    rng = np.random.default_rng(8)
    desc = np.array([Lc.flip(rng, pool[i % 257], 10) for i in range(len(new))], np.uint8)
    pose = np.linalg.inv(np.vstack([np.hstack([sc["Rcw"], sc["tcw"].reshape(3, 1)]), [0, 0, 0, 1]]))
    view = mc.lmap_view(sc["Rcw"], sc["tcw"], [I3], [np.zeros(3)], [sc["K"][0]], [pose[:3, 3]], 640, 480)
    res = []
    for lm, db in ((lm_d, db_d), (lm_h, db_h)):
        lm.set(new, desc=desc, mono=np.ones(len(new), np.uint8))
        res.append(lm.search(view, np.concatenate([new, old[:5]]), old[:5], db, 0, *free(257), levelsup=K.LEVELSUP))
    same_result(res[0], res[1])
    assert len(res[0].new_lids) > 20 and len(res[0].ind1) > 0


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_depths(mc, vocs, n):
    """k_map_depth against the host-only store and the written-out sum"""
    rng = np.random.default_rng(n)
    lids = rng.permutation(4096)[:n].astype(np.int32)
    pts = rng.uniform(-50, 50, (n, 3))
    R, t = Mc.rot(0.3, -0.2, 0.1), np.array([0.5, -1.0, 2.0])
    lm_d, lm_h = stores(mc, vocs, dict(store={int(l): p for l, p in zip(lids, pts)}))
    order = rng.permutation(n)
    zd, zh = lm_d.depths(R, t, lids[order]), lm_h.depths(R, t, lids[order])
    assert bits(zd) == bits(zh)
    want = []
    for i in order[:50]:
        s = 0.0
        for k in range(3):
            s += float(R[2][k]) * float(pts[i][k])
        want.append(s + float(t[2]))
    assert zh[:50].tolist() == want
