"""FrontEnd::TriangulateNewLandmarks on a host-only store (LocalMap.triangulate_new, device -1) and its hook (map_refine) against
the plain-Python restatement (mapping_new_ref.py), bit for bit: doubles and floats as raw bytes, every NaN the default one.

On the commit before the call existed every test of this file fails: LocalMap has no triangulate_new and the package no
map_refine."""
import os
import subprocess

import numpy as np
import pytest

import kfdb_cases as K
import mapping_cases as Mc
import mapping_new_cases as Nc
import mapping_new_ref as N

I3 = np.eye(3)


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def store(mc, voc, device=-1, max_landmarks=4096):
    return mc.LocalMap(voc, device=device, max_landmarks=max_landmarks, max_candidates=16)


def expect(mc, code, fn):
    with pytest.raises(mc.McorbError) as ei:
        fn()
    assert ei.value.code == code, ei.value


# ---------------------------------------------------------------------------------------------------------------------------
# the hook: gates and stopping rules on exact values
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hook_rows():
    return Nc.hook_cases()


def test_hook_cases_one_by_one(mc, hook_rows):
    assert len(hook_rows) == 20
    for name, c, verdict, solves in hook_rows:
        got = Nc.run_cases(mc, [c], Nc.SIGMA2)[0]
        want = Nc.ref_case(c, Nc.SIGMA2)
        assert verdict is None or got["verdict"] == verdict, (name, got)
        assert solves is None or got["solves"] == solves, (name, got)
        Nc.same_case(got, want, name)


def test_hook_cases_in_one_call(mc, hook_rows):
    got = Nc.run_cases(mc, [r[1] for r in hook_rows], Nc.SIGMA2)
    for (name, c, _, _), g in zip(hook_rows, got):
        Nc.same_case(g, Nc.ref_case(c, Nc.SIGMA2), name)


def test_no_trial_accepted_runs_the_gates_at_x0(mc, hook_rows):
    """g exactly zero: 6 trials (lambda 1 .. 1e5), then lambda = 1e6 > 1e5 ends the loop; X, and both costs, are X0's"""
    c = [r[1] for r in hook_rows if r[0] == "g zero"][0]
    got = Nc.run_cases(mc, [c], Nc.SIGMA2)[0]
    assert got["solves"] == 6 and got["X"].tolist() == [0.0, 0.0, 2.0] and got["cost_initial"] == got["cost_final"] == 1.0
    assert got["verdict"] == 0 and got["n_rays"] == 2 and got["dist"] == float(np.sqrt(5.0))


def test_parallax_at_the_two_floats_next_to_the_threshold(mc, hook_rows):
    lo, hi = [r[1] for r in hook_rows if r[0].startswith("cos ") and "0.99998" in r[0]]
    g_lo, g_hi = Nc.run_cases(mc, [lo, hi], Nc.SIGMA2)
    assert float(Nc.COS_LO) < 0.99998 <= float(Nc.COS_HI) and np.nextafter(Nc.COS_LO, np.float32(2)) == Nc.COS_HI
    assert g_lo["cos"] == Nc.COS_LO and g_lo["verdict"] == 0 and g_lo["n_rays"] == 2
    assert g_hi["cos"] == Nc.COS_HI and g_hi["verdict"] == 5 and g_hi["n_rays"] == 0 and not g_hi["normal"].any()
    assert g_hi["dist"] > 0                                                    # dist and cos are reported for verdict 5


def test_absolute_tolerance_either_side(mc, hook_rows):
    """a decrease of exactly 1.0 is not constructible (it is the difference of two rounded sums of the data); the rule
    `<= 1.0` is held by the nearest grid cases either side: the costs at X0 straddle 1.0 and the minimum is about 0"""
    below, above = [r[1] for r in hook_rows if r[0].startswith("decrease")]
    g_b, g_a = Nc.run_cases(mc, [below, above], Nc.SIGMA2)
    assert g_b["solves"] == 1 and g_a["solves"] == 2
    assert g_b["cost_initial"] - g_b["cost_final"] <= 1.0 < g_a["cost_initial"] and g_a["cost_final"] < 1e-6
    assert abs(g_a["cost_initial"] - g_b["cost_initial"]) < 0.01


def test_driven_behind_a_camera_ends_at_the_cull(mc, hook_rows):
    c = [r[1] for r in hook_rows if r[0] == "driven behind a camera"][0]
    got = Nc.run_cases(mc, [c], Nc.SIGMA2)[0]
    assert got["verdict"] == 4 and got["X"][2] < 0 and got["cost_final"] < got["cost_initial"]   # view A is [I | 0]: p.z = X.z
    assert 4.0 <= got["cost_final"] < 4.01                                      # 0.5 * (2 fx)^2 * 2 with fx = 1, and view B's rest


def test_hook_arguments(mc):
    c = Nc.pair(2.0)
    for nv1, nv in ((0, 2), (2, 2), (1, 17)):
        bad = dict(c, nv1=nv1, nv=nv)
        with pytest.raises((mc.McorbError, ValueError)):
            Nc.run_cases(mc, [bad], Nc.SIGMA2)
    bad = dict(c, octave=[0, 2])
    expect(mc, mc.E_ARG, lambda: Nc.run_cases(mc, [bad], Nc.SIGMA2))


# ---------------------------------------------------------------------------------------------------------------------------
# the call: the walk
# ---------------------------------------------------------------------------------------------------------------------------
class Mini:
    """a 2-camera rig, the previous keyframe one to the right of the current frame, exact keypoints"""

    def __init__(self, ncams=2, seed=5):
        self.rng = np.random.default_rng(seed)
        self.Ks, rigT = Mc.make_rig(ncams, self.rng)
        self.cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(I3, np.zeros(3)), rigT), self.Ks)
        self.prev = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(0.01, -0.02, 0.0), np.array([1.0, 0.05, 0.0])), rigT), self.Ks)

    def point(self, i):
        return np.array([0.3 * i - 0.5, 0.1 * i, 5.0 + i])

    def scene(self, ms, next_lid=10):
        return dict(K=np.array(self.Ks), inv_sigma2=Nc.inv_sigma2(1.0), cur=self.cur.done(), prev=self.prev.done(),
                    matches=np.array(ms, np.int32).reshape(-1, 2), next_lid=next_lid)


FAR = np.array([20.0, -10.0, 1500.0])


def test_walk_shared_train(mc, voc):
    """a second match to a current feature: after an accepted match it is verdict 6; after a rejected one it is computed"""
    m = Mini()
    q0, q1, t0 = m.prev.add(m.point(0), [0], m.rng), m.prev.add(m.point(0), [1], m.rng), m.cur.add(m.point(0), [0, 1], m.rng)
    f0, f1, ft = m.prev.add(FAR, [0], m.rng), m.prev.add(FAR, [1], m.rng), m.cur.add(FAR, [0], m.rng)
    sc = m.scene([(q0, t0), (q1, t0), (f0, ft), (f1, ft)])
    got = Nc.run_scene(mc, store(mc, voc), sc)
    assert got.verdict.tolist() == [0, 6, 5, 5] and got.inliers.tolist() == [True, False, False, False]
    assert got.new_lid.tolist() == [10, -1, -1, -1] and got.lids_cur.tolist() == [10, -1] and got.lids_prev.tolist() == [10, -1, -1, -1]
    assert got.n_by_verdict.tolist() == [1, 0, 0, 0, 0, 2, 1, 0, 0] and got.n_rays_hist.tolist() == [0, 1] + [0] * 14
    assert got.dist[2] > 1000 and got.dist[1] == 0 and got.iterations[1] == 0
    Nc.same_as_ref(got, Nc.ref_of(mc, sc))


def test_walk_shared_query_overwrites_lids_prev(mc, voc):
    """only the current frame's id is tested (:6486): a previous-keyframe feature is matched twice, makes two landmarks and keeps
    the later id, as in the reference; an id it had on entry is overwritten too"""
    m = Mini()
    q0 = m.prev.add(m.point(1), [0, 1], m.rng, lid=77)
    t0, t1 = m.cur.add(m.point(1), [0], m.rng), m.cur.add(m.point(1), [1], m.rng)
    sc = m.scene([(q0, t0), (q0, t1)])
    lm = store(mc, voc)
    got = Nc.run_scene(mc, lm, sc)
    assert got.verdict.tolist() == [0, 0] and got.new_lid.tolist() == [10, 11]
    assert got.lids_prev.tolist() == [11] and got.lids_cur.tolist() == [10, 11] and got.next_lid == 12
    Nc.same_as_ref(got, Nc.ref_of(mc, sc))


def test_walk_ids_set_on_entry_and_the_order_of_everything(mc, voc):
    m = Mini()
    ms = []
    for i in range(6):
        ms.append((m.prev.add(m.point(i), [i % 2], m.rng), m.cur.add(m.point(i), [0, 1] if i % 3 == 0 else [1], m.rng)))
    m.cur.lids[ms[1][1]] = 3                                                   # set on entry: verdict 6, kept
    m.prev.lids[ms[2][0]] = 4                                                  # the previous keyframe's: not tested, overwritten
    sc = m.scene(ms[::-1], next_lid=20)                                        # matches 5, 4, 3, 2, 1, 0
    lm = store(mc, voc)
    got = Nc.run_scene(mc, lm, sc)
    assert got.verdict.tolist() == [0, 0, 0, 0, 6, 0] and got.new_lid.tolist() == [20, 21, 22, 23, -1, 24]
    assert got.lids_cur[ms[1][1]] == 3 and got.lids_prev[ms[2][0]] == 23 and got.next_lid == 25 and got.n_triangulated == 5
    made = [0, 1, 2, 3, 5]
    assert got.depth_vec.tolist() == got.dist[made].tolist()
    s = 0.0
    for d in got.depth_vec.tolist():
        s += d
    assert got.avg_depth == s
    assert got.n_rays_hist.tolist() == [3, 2] + [0] * 14                        # matches 5, 4, 2 have one current view; 3 and 0 two
    for i in made:                                                              # the slots hold what was returned
        p, q, d, _ = lm.get(int(got.new_lid[i]))
        assert N.dbits(p[0]) + N.dbits(p[1]) + N.dbits(p[2]) == Nc.dcat(got.pt3d[i]) and Nc.dcat(q) == Nc.dcat(got.normal[i]) and d is None
    assert lm.observations(int(got.new_lid[0]))[0] == 2 and lm.observations(int(got.new_lid[2]))[0] == 3   # n_rays
    Nc.same_as_ref(got, Nc.ref_of(mc, sc))


def test_view_counts(mc, voc):
    """1 + 1, 2 + 1, 4 + 4 and 8 + 8 views"""
    m = Mini(ncams=8)
    ms = []
    for i, (a, b) in enumerate([(1, 1), (2, 1), (4, 4), (8, 8)]):
        X = m.point(i)
        ms.append((m.prev.add(X, sorted(m.rng.choice(8, a, replace=False).tolist()), m.rng),
                   m.cur.add(X, sorted(m.rng.choice(8, b, replace=False).tolist()), m.rng)))
    sc = m.scene(ms)
    got = Nc.run_scene(mc, store(mc, voc), sc)
    want = Nc.ref_of(mc, sc)
    assert got.verdict.tolist() == [0, 0, 0, 0] and [r["n_rays"] for r in want["records"]] == [2, 3, 8, 16]
    assert got.n_rays_hist.tolist() == [2, 0, 0, 1, 0, 0, 0, 1] + [0] * 8
    for i in range(4):
        assert np.allclose(got.pt3d[i], m.point(i), rtol=1e-4)
    Nc.same_as_ref(got, want)


def test_no_matches(mc, voc):
    m = Mini()
    m.prev.add(m.point(0), [0], m.rng), m.cur.add(m.point(0), [0], m.rng)
    got = Nc.run_scene(mc, store(mc, voc), m.scene([]))
    assert len(got.verdict) == 0 and got.n_triangulated == 0 and got.next_lid == 10 and len(got.depth_vec) == 0 and got.avg_depth == 0
    assert got.lids_cur.tolist() == [-1] and got.lids_prev.tolist() == [-1] and not got.n_by_verdict.any()


# ---------------------------------------------------------------------------------------------------------------------------
# the call: refusals
# ---------------------------------------------------------------------------------------------------------------------------
def good_mini(n=3):
    m = Mini()
    ms = [(m.prev.add(m.point(i), [0], m.rng), m.cur.add(m.point(i), [0], m.rng)) for i in range(n)]
    return m, ms


def untouched(mc, lm, sc, lid=10):
    """nothing ran: no slot was set and the call's copies of both lIds are as they came in"""
    expect(mc, mc.E_STATE, lambda: lm.get(lid))
    lc, lp = lm.map_new_lids
    assert lc.tolist() == sc["cur"]["lids"].tolist() and lp.tolist() == sc["prev"]["lids"].tolist()


def refusal_changes():
    def two_cams(sc):                                                          # a previous keyframe of another rig
        f = sc["prev"]
        f["match_index"] = np.concatenate([f["match_index"], f["match_index"]], axis=1)[:, :3]
        for k in ("kps", "centre_w", "proj"):
            f[k] = (list(f[k]) * 2)[:3]
    return [("queryIdx outside", lambda sc: sc["matches"].__setitem__((0, 0), len(sc["prev"]["lids"]))),
            ("trainIdx outside", lambda sc: sc["matches"].__setitem__((1, 1), -1)),
            ("keypoint outside a camera", lambda sc: sc["prev"]["match_index"].__setitem__((2, 0), len(sc["prev"]["kps"][0]))),
            ("match index below -1", lambda sc: sc["cur"]["match_index"].__setitem__((0, 0), -2)),
            ("a feature without a view", lambda sc: sc["cur"]["match_index"].__setitem__((1, 0), -1)),
            ("octave = nlevels", lambda sc: sc["cur"]["kps"][0]["octave"].__setitem__(0, Mc.NLEVELS)),
            ("octave -1", lambda sc: sc["prev"]["kps"][0]["octave"].__setitem__(1, -1)),
            ("current id outside the store", lambda sc: sc["cur"]["lids"].__setitem__(0, 4096)),
            ("previous id outside the store", lambda sc: sc["prev"]["lids"].__setitem__(1, -2)),
            ("next_lid < 0", lambda sc: sc.__setitem__("next_lid", -1)),
            ("camera counts differ", two_cams)]


def check_refusals(mc, make_store):
    for what, change in refusal_changes():
        m, ms = good_mini()
        sc = m.scene(ms)
        change(sc)
        lm = make_store()
        expect(mc, mc.E_ARG, lambda: Nc.run_scene(mc, lm, sc))
        untouched(mc, lm, sc)
    # 9 + 8 views: beyond the solver's design limit
    rng = np.random.default_rng(2)
    Ks, rigT = Mc.make_rig(16, rng)
    cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(I3, np.zeros(3)), rigT), Ks)
    prev = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(I3, np.array([1.0, 0, 0])), rigT), Ks)
    X = np.array([0.2, 0.1, 6.0])
    q9, q8, t8 = prev.add(X, list(range(9)), rng), prev.add(X, list(range(8)), rng), cur.add(X, list(range(8, 16)), rng)
    sc = dict(K=np.array(Ks), inv_sigma2=Nc.inv_sigma2(1.0), cur=cur.done(), prev=prev.done(), matches=np.array([(q8, t8), (q9, t8)], np.int32),
              next_lid=10)
    lm = make_store()
    expect(mc, mc.E_ARG, lambda: Nc.run_scene(mc, lm, sc))
    assert "MCORB_MAX_CAMS" in str(mc._lib.load().mcorb_last_error())
    untouched(mc, lm, sc)
    # the caps
    m, ms = good_mini()
    sc = m.scene(ms, next_lid=20)
    lm = make_store()
    expect(mc, mc.E_CAP, lambda: Nc.run_scene(mc, lm, sc, caps=(2, 3)))          # per-match outputs short
    assert lm.map_new_out.n_matches == 3
    untouched(mc, lm, sc, 20)
    expect(mc, mc.E_CAP, lambda: Nc.run_scene(mc, lm, sc, caps=(3, 2)))          # depth_vec short: counts set, nothing stored
    o = lm.map_new_out
    assert (o.n_matches, o.n_depth, o.n_triangulated, o.next_lid) == (3, 3, 3, 20)
    untouched(mc, lm, sc, 20)
    sc["next_lid"] = 4094                                                        # ids 4094, 4095, 4096: one beyond the store
    expect(mc, mc.E_CAP, lambda: Nc.run_scene(mc, lm, sc))
    untouched(mc, lm, sc, 4094)
    sc["next_lid"] = 4093
    assert Nc.run_scene(mc, lm, sc).new_lid.tolist() == [4093, 4094, 4095]


def test_refusals(mc, voc):
    check_refusals(mc, lambda: store(mc, voc))


def test_refused_while_a_tracking_call_is_pending(mc, voc):
    import track_cases as T
    v, landmarks, kps, descs, lids = T.scene(4)
    lm = mc.LocalMap(voc, device=-1, max_landmarks=4096, max_candidates=1024)
    T.fill(lm, landmarks)
    m, ms = good_mini()
    sc = m.scene(ms, next_lid=4000)
    lm.track_submit(T.to_view(mc, v), kps, descs, lids)
    expect(mc, mc.E_STATE, lambda: Nc.run_scene(mc, lm, sc))
    lm.track_wait()
    untouched(mc, lm, sc, 4000)
    assert Nc.run_scene(mc, lm, sc).n_triangulated == 3


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded scene
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncams", [1, 4, 8])
def test_seeded_scene(mc, voc, ncams):
    sc = Nc.scene(ncams)
    want = Nc.ref_of(mc, sc)
    # shown on the restatement alone: at least 5 % of the matches at each of verdicts 0, 3, 4, 5 and 6, 20 % at 0, and at least
    # 10 % of the new landmarks after two or more accepted steps
    n = len(want["verdict"])
    assert n == 300
    for v in (0, 3, 4, 5, 6):
        assert want["n_by_verdict"][v] >= 0.05 * n, (v, want["n_by_verdict"])
    assert want["n_by_verdict"][0] >= 0.2 * n
    made = [r for r in want["records"] if r["verdict"] == 0]
    assert sum(r["accepted"] >= 2 for r in made) >= 0.1 * len(made)
    got = Nc.run_scene(mc, store(mc, voc), sc)
    assert (got.verdict == 5).any() and not got.inliers[got.verdict == 5].any()      # a parallax failure is no inlier here
    Nc.same_as_ref(got, want)


def test_header_host_path_under_asan_ubsan(mc, voc, tmp_path):
    """csrc/mcorb_mapping_new.h in a stand-alone g++ program built with -fsanitize=address,undefined on the seeded 8-camera scene
    with nothing assigned on entry: no report, and every record equal to the library's, bit for bit"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, txt = str(tmp_path / "test_mapping_new_sanitize"), str(tmp_path / "scene.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "mc-slam_amd", "csrc"), "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "test_mapping_new_sanitize.cpp"), "-o", exe])
    sc = Nc.scene(8)
    sc["cur"]["lids"][:] = -1
    seen, keep = set(), []
    for q, t in sc["matches"].tolist():                                        # every current feature once: no match is skipped
        if t not in seen:
            keep.append((q, t))
            seen.add(t)
    sc["matches"] = np.array(keep, np.int32)
    num = lambda a: " ".join(repr(float(x)) for x in np.asarray(a, np.float64).reshape(-1))
    with open(txt, "w") as f:
        f.write("%d %d\n%s\n%s\n" % (sc["ncams"], Nc.NLEVELS, num(sc["K"]), num(sc["inv_sigma2"])))
        for fr in (sc["cur"], sc["prev"]):
            f.write(num(fr["twc"]) + "\n")
            for c in range(sc["ncams"]):
                f.write(num(fr["proj"][c]) + " " + num(fr["centre_w"][c]) + "\n")
            for kps in fr["kps"]:
                f.write("%d %s\n" % (len(kps), " ".join("%r %r %d" % (float(k["x"]), float(k["y"]), k["octave"]) for k in kps)))
            f.write("%d %s\n" % (len(fr["match_index"]), " ".join(str(int(v)) for v in fr["match_index"].reshape(-1))))
        f.write("%d %s\n" % (len(keep), " ".join("%d %d" % m for m in keep)))
    out = subprocess.run([exe, txt], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr
    got = Nc.run_scene(mc, store(mc, voc), sc)
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(keep) and set(got.verdict.tolist()) >= {0, 3, 4, 5}
    for i, line in enumerate(lines):
        v, n_rays, solves, X, normal, dist, ci, cf, cos = line.split()
        lm = got.verdict[i] == 0
        assert int(v) == got.verdict[i] and int(solves) == got.iterations[i], i
        assert bytes.fromhex(dist) == got.dist[i].tobytes() and bytes.fromhex(cos) == got.cos_parallax[i].tobytes(), i
        assert bytes.fromhex(ci) == got.cost_initial[i].tobytes() and bytes.fromhex(cf) == got.cost_final[i].tobytes(), i
        assert bytes.fromhex(normal) == got.normal[i].tobytes() and (not lm or bytes.fromhex(X) == got.pt3d[i].tobytes()), i
