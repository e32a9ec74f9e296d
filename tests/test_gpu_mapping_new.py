"""FrontEnd::TriangulateNewLandmarks on the device (device >= 0: k_map_refine_new, k_map_put) against the host-only store (device
-1) and the restatement (mapping_new_ref.py) on the same inputs, bit for bit: every integer, and every double and float compared
as raw bytes; on the inputs of test_mapping_new_cpu.py.

On the commit before the call existed every test of this file fails: LocalMap has no triangulate_new and the package no
map_refine."""
import numpy as np
import pytest

import kfdb_cases as K
import lmap_cases as Lc
import mapping_cases as Mc
import mapping_new_cases as Nc
from test_lmap_cpu import free, make, same_result
from test_mapping_new_cpu import I3, Mini, check_refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def stores(mc, vocs, max_landmarks=4096):
    return [mc.LocalMap(voc, device=dev, max_landmarks=max_landmarks, max_candidates=16) for voc, dev in zip(vocs, (0, -1))]


def both(mc, vocs, sc):
    lm_d, lm_h = stores(mc, vocs)
    got, want = Nc.run_scene(mc, lm_d, sc), Nc.run_scene(mc, lm_h, sc)
    Nc.same(got, want)
    return lm_d, lm_h, got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_match_counts(mc, vocs, n):
    """the wave edges of k_map_refine_new (64 lanes) on a 4-camera rig"""
    sc = Nc.scene(4, n=n, seed=n + 1)
    lm_d, _, got = both(mc, vocs, sc)
    Nc.same_as_ref(got, Nc.ref_of(mc, sc))
    free_on_entry = int((sc["cur"]["lids"][sc["matches"][:, 1]] == -1).sum()) if n else 0
    if free_on_entry:
        assert lm_d.last_triangulate_new_timing()[1] == free_on_entry
    if n >= 63:
        assert 0 < got.n_triangulated < n and len(set(got.verdict.tolist())) >= 5


def test_view_counts_in_one_call(mc, vocs):
    """1 + 1, 2 + 1, 2 + 2, 4 + 4 and 8 + 8 views in one mixed batch: both instances of k_map_refine_new run, 8 + 8 is the most
    the general one takes"""
    m = Mini(ncams=8, seed=4)
    shapes = [(1, 1), (2, 1), (2, 2), (4, 4), (8, 8)]
    ms, nvs = [], []
    for i in range(150):
        a, b = shapes[i % 5]
        X = np.array([m.rng.uniform(-2, 2), m.rng.uniform(-1.5, 1.5), m.rng.uniform(3, 15)])
        q = m.prev.add(X, sorted(m.rng.choice(8, a, replace=False).tolist()), m.rng)
        t = m.cur.add(X, sorted(m.rng.choice(8, b, replace=False).tolist()), m.rng)
        Nc.jitter(m.prev, q, m.rng, 0.5), Nc.jitter(m.cur, t, m.rng, 0.5)
        ms.append((q, t))
        nvs.append(a + b)
    sc = m.scene(ms, next_lid=0)
    lm_d, _, got = both(mc, vocs, sc)
    assert lm_d.last_triangulate_new_timing()[1] == 150
    nvs = np.array(nvs)
    for nv in (2, 3, 4, 8, 16):
        assert (got.verdict[nvs == nv] == 0).sum() >= 15, nv
    Nc.same_as_ref(got, Nc.ref_of(mc, sc))


def test_every_match_assigned_on_entry_makes_no_launch(mc, vocs):
    sc = Nc.scene(4, n=65, seed=3)
    lm_d, _, first = both(mc, vocs, sc)
    before = lm_d.last_triangulate_new_timing()
    assert before[0] > 0 and before[1] > 0
    sc["cur"]["lids"][:] = 7
    got = Nc.run_scene(mc, lm_d, sc)
    assert (got.verdict == 6).all() and got.n_triangulated == 0 and got.next_lid == sc["next_lid"]
    assert lm_d.last_triangulate_new_timing() == before
    Nc.same_as_ref(got, Nc.ref_of(mc, sc))


def test_hook_cases_in_one_launch(mc):
    """every boundary case of test_mapping_new_cpu.py in one wave, whose lanes end after 0, 1, 2, 6 and 50 solves"""
    rows = Nc.hook_cases()
    got = Nc.run_cases(mc, [r[1] for r in rows], Nc.SIGMA2, device=0)
    host = Nc.run_cases(mc, [r[1] for r in rows], Nc.SIGMA2)
    assert {1, 2, 50} <= {int(g["solves"]) for g in got} and len(rows) <= 64
    for (name, c, verdict, solves), g, h in zip(rows, got, host):
        assert verdict is None or g["verdict"] == verdict, (name, g)
        assert solves is None or g["solves"] == solves, (name, g)
        Nc.same_case(g, h, name)
        Nc.same_case(g, Nc.ref_case(c, Nc.SIGMA2), name)


def test_seeded_scene_and_write_back(mc, vocs):
    """300 matches on a 4-camera rig; every new id reads back from HBM as returned, every other slot is unchanged, and a search
    that includes the new ids equals the host-only store's"""
    sc = Nc.scene(4)
    pool = Lc.pool()[0]
    probe = Lc.probe_of(pool[:257])
    (lm_d, db_d), (lm_h, db_h) = make(mc, vocs[0], 0, probe), make(mc, vocs[1], -1, probe)
    old = np.arange(3000, 3040, dtype=np.int32)
    rng = np.random.default_rng(8)
    old_pts = rng.uniform(-5, 5, (40, 3)) + [0, 0, 10]
    for lm in (lm_d, lm_h):
        lm.set(old, old_pts, np.tile([0.0, 0.0, 1.0], (40, 1)))
    before = [lm_d.get(int(l)) for l in old]
    got, want = Nc.run_scene(mc, lm_d, sc), Nc.run_scene(mc, lm_h, sc)
    Nc.same(got, want)
    Nc.same_as_ref(got, Nc.ref_of(mc, sc))
    us, launched = lm_d.last_triangulate_new_timing()
    assert us > 0 and 0 < launched <= 300
    new = got.new_lid[got.new_lid >= 0]
    assert len(new) == got.n_triangulated > 60 and new.tolist() == list(range(sc["next_lid"], sc["next_lid"] + len(new)))
    for i in np.nonzero(got.new_lid >= 0)[0]:
        p, q, d, _ = lm_d.get(int(got.new_lid[i]))
        assert Nc.dcat(p) == Nc.dcat(got.pt3d[i]) and Nc.dcat(q) == Nc.dcat(got.normal[i]) and d is None
        assert lm_d.observations(int(got.new_lid[i]))[0] == lm_h.observations(int(got.new_lid[i]))[0] > 1
    for l, b in zip(old, before):
        a = lm_d.get(int(l))
        assert Nc.dcat(a[0]) == Nc.dcat(b[0]) and Nc.dcat(a[1]) == Nc.dcat(b[1])
    with pytest.raises(mc.McorbError):
        lm_d.get(int(new[-1]) + 1)
    # the new landmarks get descriptors and are searched from the current frame's place, 640 x 480
    desc = np.array([Lc.flip(rng, pool[i % 257], 10) for i in range(len(new))], np.uint8)
    Tcw = np.vstack([sc["cur"]["proj"][0], [0, 0, 0, 1]])
    view = mc.lmap_view(Tcw[:3, :3], Tcw[:3, 3], [I3], [np.zeros(3)], [sc["K"][0]], [np.linalg.inv(Tcw)[:3, 3]], 640, 480)
    res = []
    for lm, db in ((lm_d, db_d), (lm_h, db_h)):
        lm.set(new, desc=desc, mono=np.ones(len(new), np.uint8))
        res.append(lm.search(view, np.concatenate([new, old[:5]]), old[:5], db, 0, *free(257), levelsup=K.LEVELSUP))
    same_result(res[0], res[1])
    assert len(res[0].new_lids) > 20 and len(res[0].ind1) > 0


def test_then_triangulate_neighbours(mc, vocs):
    """the whole of FrontEnd::mapping on the store: triangulate_new against the previous keyframe, then triangulate_neighbours on
    the lids_cur it returned, device store against host-only store"""
    sc = Mc.scene(4, sizes=(150, 100), seed=5, zero_f=None)
    first = dict(K=sc["K"], inv_sigma2=Nc.inv_sigma2(1.0), cur=sc["cur"], prev=sc["neigh"][0], matches=sc["matches"][0][:60], next_lid=100)
    out = []
    for lm in stores(mc, vocs):
        Mc.fill_store(lm, sc["store"])
        a = Nc.run_scene(mc, lm, first)
        sc2 = dict(sc, next_lid=a.next_lid, cur=dict(sc["cur"], lids=a.lids_cur),
                   neigh=[dict(sc["neigh"][0], lids=a.lids_prev), sc["neigh"][1]])
        out.append((a, Mc.run_scene(mc, lm, sc2)))
    (a_d, b_d), (a_h, b_h) = out
    Nc.same(a_d, a_h)
    from test_gpu_mapping import same
    same(b_d, b_h)
    assert a_d.n_triangulated > 10 and b_d.n_triangulated > 10 and (b_d.verdict == 6).sum() >= a_d.n_triangulated
    assert b_d.new_lid[b_d.new_lid >= 0].min() == a_d.next_lid


def test_refusals_on_a_device_store(mc, vocs):
    check_refusals(mc, lambda: mc.LocalMap(vocs[0], device=0, max_landmarks=4096, max_candidates=16))
