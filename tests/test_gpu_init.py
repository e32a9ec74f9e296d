"""Map initialization on the device (device >= 0: k_init_triangulate, k_init_select, k_init_put) against the host-only store
(device -1) on the same inputs, bit for bit: every integer, and every double compared as raw bytes, on every output and on the
store read back; on the inputs of test_init_cpu.py."""
import math

import numpy as np
import pytest

import init_cases as Ic
import init_ref as IR
import kfdb_cases as K
import lmap_cases as Lc
import mapping_cases as Mc
from test_init_cpu import TH, bits, boundary_cases, run_refusals, same_scene, snapshot
from test_lmap_cpu import free, make, same_result

pytestmark = pytest.mark.gpu

ARRAYS = ("inliers", "verdict", "new_lid", "pt3d", "normal", "dist2", "cos_parallax", "t_out")
SCALARS = ("status", "parallax", "median_scene_depth", "n_matches", "n_initial_inliers", "n_parallax", "n_triangulated", "scaled", "next_lid")


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture(scope="module")
def big():
    """a 4-camera scene of 1 025 matches, cut to size by the tests"""
    return Ic.scene(4, n=1025, seed=11)


def stores(mc, vocs, max_landmarks=4096):
    return [mc.LocalMap(voc, device=dev, max_landmarks=max_landmarks, max_candidates=16) for voc, dev in zip(vocs, (0, -1))]


def same(got, want, what="", lids=True):
    for f in ARRAYS + (("lids_prev", "lids_cur") if lids else ("n_rays",)):
        a, b = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, f)
    for f in SCALARS:
        a, b = getattr(got, f), getattr(want, f)
        assert (bits(a) == bits(b)) if isinstance(a, float) else a == b, (what, f, a, b)


def same_store(lm_d, lm_h, ids, what=""):
    for l in ids:
        a, b = lm_d.get(int(l)), lm_h.get(int(l))
        assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1]) and lm_d.observations(int(l))[0] == lm_h.observations(int(l))[0], (what, l)


def both(mc, vocs, sc, what=""):
    lm_d, lm_h = stores(mc, vocs)
    got, want = Ic.run_scene(mc, lm_d, sc), Ic.run_scene(mc, lm_h, sc)
    same(got, want, what)
    same_store(lm_d, lm_h, got.new_lid[got.new_lid >= 0], what)
    return lm_d, lm_h, got


@pytest.mark.parametrize("third_clear", [False, True])
@pytest.mark.parametrize("n", [0, 1, 51, 63, 64, 65, 255, 256, 257, 1025])
def test_match_counts(mc, vocs, big, n, third_clear):
    """the wave edges of k_init_triangulate, the 256 lanes of k_init_put and the 1 024 of k_init_select's walk"""
    sc = Ic.cut(big, n, third_clear)
    lm_d, _, got = both(mc, vocs, sc, (n, third_clear))
    flagged = int(sc["flags"].sum())
    assert len(got.verdict) == n and got.n_initial_inliers == flagged and lm_d.last_initialize_timing()[3] == flagged
    assert (got.verdict[~sc["flags"]] == 9).all() and (got.verdict[sc["flags"]] != 9).all()
    if n >= 255:
        assert got.status == IR.DONE and 50 < got.n_triangulated < n and len(set(got.verdict.tolist())) >= 4
    if n <= 51:
        assert got.status in (IR.FEW, IR.PARALLAX) and (got.new_lid == -1).all()


def test_view_counts_in_one_call(mc, vocs):
    """1 + 1, 2 + 1, 2 + 2, 4 + 4 and 8 + 8 views in one call: both instances of k_init_triangulate run"""
    rng = np.random.default_rng(4)
    Ks, rigT = Mc.make_rig(8, rng)
    T = Mc.T4(Mc.rot(-0.03, 0.05, 0.0), np.array([1.1, 0.05, -0.1]))
    prev, cur = Mc.FrameBuilder(Mc.frame_geometry(np.eye(4), rigT), Ks), Mc.FrameBuilder(Mc.frame_geometry(T, rigT), Ks)
    shapes = [(1, 1), (2, 1), (2, 2), (4, 4), (8, 8)]
    ms, nvs = [], []
    for i in range(150):
        a, b = shapes[i % 5]
        X = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 15)])
        ms.append((prev.add(X, sorted(rng.choice(8, a, replace=False).tolist()), rng), cur.add(X, sorted(rng.choice(8, b, replace=False).tolist()), rng)))
        nvs.append(a + b)
    sc = dict(ncams=8, K=np.array(Ks), inv_sigma2=Mc.INV_SIGMA2, prev=prev.done(), cur=cur.done(), R=T[:3, :3].copy(), t=T[:3, 3].copy(),
              body=np.array([np.linalg.inv(M)[:3, 3] for M in rigT]), matches=np.array(ms, np.int32), flags=np.ones(150, bool), next_lid=0,
              min_baseline=0.25)
    lm_d, _, got = both(mc, vocs, sc)
    assert lm_d.last_initialize_timing()[3] == 150 and got.status == IR.DONE
    nvs = np.array(nvs)
    for nv in (2, 3, 4, 8, 16):
        assert (got.verdict[nvs == nv] == 0).sum() >= 20, nv
    same_scene(got, Ic.ref_scene(sc), sc)


def hook_both(mc, cases, what="", **kw):
    got, want = Ic.run_hook(mc, cases, device=0, **kw), Ic.run_hook(mc, cases, **kw)
    same(got, want, what, lids=False)
    return got


def test_boundary_cases_in_one_launch(mc):
    rows = [r for r in boundary_cases() if r[0] != "cos NaN"]
    got = hook_both(mc, [r[1] for r in rows] + Ic.good_cases(52), "boundaries")
    assert got.status == IR.DONE
    for (name, _, v), gv in zip(rows, got.verdict):
        assert v is None or gv == v, (name, gv)
    nan = Ic.case((0.0, 0.0, 0.0), c2=(0.0, 0.0, -1.0))
    got = hook_both(mc, [nan] + Ic.good_cases(52), "cos NaN", t=np.array([0.0, 0.0, -1.0]))
    assert got.verdict[0] == 5 and math.isnan(got.cos_parallax[0])


def test_median_cases(mc):
    """each is one launch of k_init_select: member counts, ties, a NaN that sorts last, an empty depthVec, the two thresholds"""
    for n in (1, 2, 3, 64, 65):
        got = hook_both(mc, Ic.good_cases(n, seed=n), "members %d" % n)
        assert got.parallax == sorted(got.cos_parallax.tolist())[n // 2]
    g = Ic.good_cases(5, seed=9)
    hook_both(mc, [g[0], g[1], g[1], g[1], g[2], g[1]], "ties")
    nan, one, t = Ic.case((0.0, 0.0, 0.0), c2=(0.0, 0.0, -1.0)), Ic.case((0.3, 0.2, 2.0), c2=(0.0, 0.0, -1.0)), np.array([0.0, 0.0, -1.0])
    assert math.isnan(hook_both(mc, [nan, one, nan], "(x, NaN, NaN)", t=t).parallax)
    assert not math.isnan(hook_both(mc, [nan, one, one], "(x, x, NaN)", t=t).parallax)
    assert hook_both(mc, [Ic.case_cos(TH), Ic.case((1e7, 0.0, 1.0))], "depthVec empty").n_triangulated == 0
    assert hook_both(mc, Ic.good_cases(50), "50").status == IR.FEW
    assert hook_both(mc, Ic.good_cases(51), "51").status == IR.DONE
    low = Ic.good_cases(52)
    assert hook_both(mc, low + [Ic.case_cos(TH)] * 53, "median at 0.99998").status == IR.PARALLAX
    assert hook_both(mc, low + [Ic.case_cos(math.nextafter(TH, 0.0))] * 53, "one double below").status == IR.DONE
    got = hook_both(mc, Ic.good_cases(2100, seed=2), "more members than two trips of k_init_select's walk")
    assert got.n_triangulated == 2100 and got.parallax == sorted(got.cos_parallax.tolist())[1050]


def test_statuses_and_timing(mc, vocs, big):
    sc = Ic.cut(big, 300)
    lm_d, lm_h, got = both(mc, vocs, sc, "DONE")
    assert got.status == IR.DONE
    us = lm_d.last_initialize_timing()
    assert us[0] > 0 and us[1] > 0 and us[2] > 0 and us[3] == 300
    far = dict(sc, min_baseline=50.0)
    a, b = Ic.run_scene(mc, lm_d, far), Ic.run_scene(mc, lm_h, far)
    assert a.status == b.status == IR.BASELINE and a.t_out.tolist() == b.t_out.tolist() == sc["t"].tolist()
    assert lm_d.last_initialize_timing() == us, "BASELINE launches nothing and leaves the timing"
    few = Ic.cut(big, 60)
    few["flags"][40:] = False
    before = snapshot(lm_d, range(95, 440))
    assert both(mc, vocs, few, "FEW")[2].status == IR.FEW
    a = Ic.run_scene(mc, lm_d, few)
    assert a.status == IR.FEW and snapshot(lm_d, range(95, 440)) == before, "a failed verdict leaves the store unchanged"
    flat = Ic.cut(big, 120)
    flat["flags"] = far_only(big, 120)
    got = both(mc, vocs, flat, "PARALLAX")[2]
    assert got.status == IR.PARALLAX and got.n_triangulated == 3 and got.parallax >= TH and (got.new_lid == -1).all()


def far_only(big, n):
    """the matches among the first n that end at verdict 5 (points 1 500 away) and three that end at 0: depthVec is not empty
    and the median cos lies above 0.99998"""
    v = np.array(Ic.ref_scene(Ic.cut(big, n))["verdict"])
    flags = v == 5
    flags[np.nonzero(v == 0)[0][:3]] = True
    assert flags.sum() >= 9
    return flags


def test_scaled_one_camera_scene(mc, vocs):
    sc = Ic.scene(1)
    _, _, got = both(mc, vocs, sc)
    assert got.status == IR.DONE and got.scaled and got.t_out.tolist() != sc["t"].tolist()
    same_scene(got, Ic.ref_scene(sc), sc)


def test_search_over_the_new_ids(mc, vocs, big):
    """the new landmarks get descriptors and are searched: the device store's result equals the host-only store's"""
    sc = Ic.cut(big, 300)
    pool = Lc.pool()[0]
    probe = Lc.probe_of(pool[:257])
    (lm_d, db_d), (lm_h, db_h) = make(mc, vocs[0], 0, probe), make(mc, vocs[1], -1, probe)
    got, want = Ic.run_scene(mc, lm_d, sc), Ic.run_scene(mc, lm_h, sc)
    same(got, want)
    new = got.new_lid[got.new_lid >= 0]
    same_store(lm_d, lm_h, new)
    for i in np.nonzero(got.new_lid >= 0)[0]:
        p, q, d, _ = lm_d.get(int(got.new_lid[i]))
        assert bits(p) == bits(got.pt3d[i]) and bits(q) == bits(got.normal[i]) and d is None
    with pytest.raises(mc.McorbError):
        lm_d.get(int(new[-1]) + 1)
    rng = np.random.default_rng(8)
    desc = np.array([Lc.flip(rng, pool[i % 257], 10) for i in range(len(new))], np.uint8)
    view = mc.lmap_view(np.eye(3), np.zeros(3), [np.eye(3)], [np.zeros(3)], [sc["K"][0]], [np.zeros(3)], 640, 480)
    res = []
    for lm, db in ((lm_d, db_d), (lm_h, db_h)):
        lm.set(new, desc=desc, mono=np.ones(len(new), np.uint8))
        res.append(lm.search(view, new, new[:0], db, 0, *free(257), levelsup=K.LEVELSUP))
    same_result(res[0], res[1])
    assert len(res[0].new_lids) > 20 and len(res[0].ind1) > 0


def test_refusals(mc, vocs):
    run_refusals(mc, stores(mc, vocs)[0], Ic.scene(4))
