"""Map initialization on the host-only store (device -1): mcorb_lmap_initialize and the hook mcorb_host_init_cases against the
plain-Python restatement of FrontEnd::initialization (init_ref.py, FrontEnd.cpp:2633-2839).  The hook takes the caller's X, so
its doubles are compared exactly; the whole call goes through the DLT and is held to 1e-9 (DESIGN.md section 9d's figure)."""
import copy
import math
import os
import subprocess

import numpy as np
import pytest

import init_cases as Ic
import init_ref as IR
import kfdb_cases as K
import mapping_cases as Mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = 0.99998


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def store(mc, voc, device=-1, max_landmarks=4096):
    return mc.LocalMap(voc, device=device, max_landmarks=max_landmarks, max_candidates=16)


@pytest.fixture(scope="module")
def scenes():
    """the seeded scenes and their restatement, computed once"""
    out = {}
    for C in (1, 4, 8):
        sc = Ic.scene(C)
        out[C] = (sc, Ic.ref_scene(sc))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def default_nan(x):
    """the restatement's value as a record holds it: a NaN leaves the library as the default quiet NaN, whatever sign the
    operation that made it gave it (test_mapping_cpu.default_nan)"""
    x = np.array(x, np.float64)
    x[np.isnan(x)] = np.frombuffer(np.array([0x7ff8000000000000], np.uint64).tobytes(), np.float64)[0]
    return x


def same_nan(a, b):
    """the library's double(s) a == the restatement's b on the bytes, a NaN of b's as the default quiet NaN"""
    return bits(a) == bits(default_nan(b))


def same_hook(got, ref, what="", n_rays=True):
    """every output of the hook equals the restatement's: integers, and doubles bit for bit, a NaN as the default quiet NaN that
    the records promise; n_rays: the hook's per-match count of rays, which the whole call's result does not carry"""
    assert got.status == ref["status"], (what, got.status, ref["status"])
    if ref["status"] == IR.BASELINE:
        return
    for f in ("n_initial_inliers", "n_parallax", "n_triangulated", "scaled", "next_lid"):
        assert getattr(got, f) == ref[f], (what, f, getattr(got, f), ref[f])
    assert got.verdict.tolist() == ref["verdict"] and got.inliers.tolist() == ref["inliers"], what
    assert got.new_lid.tolist() == ref["new_lid"] and (not n_rays or got.n_rays.tolist() == ref["n_rays"]), what
    assert same_nan(got.parallax, ref["parallax"]) and same_nan(got.median_scene_depth, ref["median_scene_depth"]), what
    assert bits(got.t_out) == bits(ref["t_out"]), what
    for i in range(len(ref["verdict"])):
        assert same_nan(got.dist2[i], ref["dist2"][i]) and same_nan(got.cos_parallax[i], ref["cos"][i]), (what, i)
        assert same_nan(got.pt3d[i], ref["pt3d"][i]) and same_nan(got.normal[i], ref["normal"][i]), (what, i)


def hook(mc, cases, what="", **kw):
    got, ref = Ic.run_hook(mc, cases, **kw), Ic.ref_hook(cases, **kw)
    same_hook(got, ref, what)
    return got


def close(a, b, tol=1e-9):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))


def same_scene(got, ref, sc, what=""):
    """the whole call against the restatement: integers equal, pt3d / normal / medians / t_out to 1e-9; no match is left out"""
    assert not any(ref["near"]), "the seed puts no gate quantity within 1e-6 of its threshold"
    assert got.status == ref["status"] == IR.DONE, what
    assert got.verdict.tolist() == ref["verdict"] and got.inliers.tolist() == ref["inliers"] and got.new_lid.tolist() == ref["new_lid"], what
    for f in ("n_initial_inliers", "n_parallax", "n_triangulated", "scaled", "next_lid"):
        assert getattr(got, f) == ref[f], (what, f)
    assert got.lids_prev.tolist() == ref["lids_prev"] and got.lids_cur.tolist() == ref["lids_cur"], what
    assert close(got.pt3d, ref["pt3d"]) and close(got.normal, ref["normal"]), what
    assert close(got.parallax, ref["parallax"]) and close(got.median_scene_depth, ref["median_scene_depth"]) and close(got.t_out, ref["t_out"]), what
    assert close(got.dist2, ref["dist2"]) and close(got.cos_parallax, ref["cos"]), what


# ---------------------------------------------------------------------------------------------------------------------------
# the gates, through the hook
# ---------------------------------------------------------------------------------------------------------------------------
def boundary_cases():
    """(name, case, verdict): 52 good matches are added by the callers so that the call as a whole is DONE"""
    up, down = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, -math.inf))
    z = lambda v: Ic.case((0.25, 0.1, v), kp1=(0.0, 0.0), kp2=(0.0, 0.0))
    return [("p.z -0.0", z(-0.0), None), ("p.z 0.0", z(0.0), None), ("p.z 1e-300", z(1e-300), None), ("p.z -1e-300", z(-1e-300), 3),
            ("p.z NaN", z(IR.NAN), None),
            ("err at 5.991", Ic.case_err(5.991), 0), ("err one ulp above", Ic.case_err(up(5.991)), 4),
            ("err one ulp below", Ic.case_err(down(5.991)), 0),
            ("cos at 0.99998", Ic.case_cos(TH), 5), ("cos one ulp above", Ic.case_cos(up(TH)), 5),
            ("cos one ulp below", Ic.case_cos(down(TH)), 0),
            ("cos 0.4", Ic.case((0.5, 0.0, 0.7638)), 0),
            ("cos NaN", Ic.case((0.0, 0.0, 0.0), c2=(0.0, 0.0, -1.0)), 5)]


def test_gates_on_exact_values(mc):
    rows = boundary_cases()
    # cos NaN has cur's camera elsewhere: its own call (T's translation is that camera's centre); the rest share one
    shared = [r for r in rows if r[0] != "cos NaN"]
    got = hook(mc, [r[1] for r in shared] + Ic.good_cases(52), "boundaries")
    assert got.status == IR.DONE
    for (name, _, v), gv, gi in zip(shared, got.verdict, got.inliers):
        assert v is None or gv == v, (name, gv)
        assert gv != 3 or name == "p.z -1e-300", name      # -0.0, 0.0, 1e-300 and a NaN are not behind
        assert gi == (gv == 0), name
    i = [r[0] for r in shared].index("cos 0.4")
    assert 0.39 < got.cos_parallax[i] < 0.41 and got.new_lid[i] >= 0, "a landmark here, outside section 9d's window"
    nan = [r for r in rows if r[0] == "cos NaN"][0][1]
    got = hook(mc, [nan] + Ic.good_cases(52), "cos NaN", t=np.array([0.0, 0.0, -1.0]))
    assert got.verdict[0] == 5 and not got.inliers[0] and math.isnan(got.cos_parallax[0]) and got.n_parallax == 53


def test_flag_clear_on_entry(mc):
    cases = Ic.good_cases(60)
    flags = [i % 4 != 1 for i in range(60)]
    got = hook(mc, cases, "flags", flags=flags)
    assert got.n_initial_inliers == 45 and (got.verdict[1::4] == 9).all() and not got.inliers[1::4].any()
    assert (got.pt3d[1::4] == 0).all() and (got.new_lid[1::4] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the medians and the verdict
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65])
def test_median_member_counts(mc, n):
    got = hook(mc, Ic.good_cases(n, seed=n), "members %d" % n)
    assert got.n_parallax == got.n_triangulated == n
    assert got.parallax == sorted(got.cos_parallax.tolist())[n // 2] and got.median_scene_depth == sorted(got.dist2.tolist())[n // 2]
    assert got.status == (IR.DONE if n > 50 else IR.FEW)


def test_median_ties_nan_and_empty_depth(mc):
    g = Ic.good_cases(5, seed=9)
    got = hook(mc, [g[0], g[1], g[1], g[1], g[2], g[1]], "ties")
    assert got.parallax == got.cos_parallax[1] and got.median_scene_depth == got.dist2[1]
    nan = Ic.case((0.0, 0.0, 0.0), c2=(0.0, 0.0, -1.0))
    t = np.array([0.0, 0.0, -1.0])
    one = Ic.case((0.3, 0.2, 2.0), c2=(0.0, 0.0, -1.0))
    got = hook(mc, [nan, one, nan], "a NaN sorts last: the median of (x, NaN, NaN)", t=t)
    assert math.isnan(got.parallax) and got.status == IR.PARALLAX and got.n_parallax == 3 and got.n_triangulated == 1
    got = hook(mc, [nan, one, one], "a NaN sorts last: the median of (x, x, NaN)", t=t)
    assert got.parallax == got.cos_parallax[1]
    far = [Ic.case_cos(TH), Ic.case((1e7, 0.0, 1.0)), Ic.case_cos(TH)]
    got = hook(mc, far, "depthVec empty, parllaxVec not")
    # (parallax stays 0.0, which passes :2776 as in the reference; the count then fails)
    assert (got.n_parallax, got.n_triangulated, got.parallax, got.median_scene_depth, got.status) == (3, 0, 0.0, 0.0, IR.FEW)


def test_triangulated_50_and_51(mc):
    assert hook(mc, Ic.good_cases(50), "50").status == IR.FEW
    got = hook(mc, Ic.good_cases(51), "51")
    assert got.status == IR.DONE and got.new_lid.tolist() == list(range(51)) and got.next_lid == 51
    few = hook(mc, Ic.good_cases(50) + [Ic.case_cos(TH)] * 3, "50 of 53")
    assert few.status == IR.FEW and (few.new_lid == -1).all() and (few.normal == 0).all() and few.n_parallax == 53


def test_median_cos_at_the_threshold(mc):
    below = math.nextafter(TH, 0.0)
    low = Ic.good_cases(52)
    got = hook(mc, low + [Ic.case_cos(TH)] * 53, "median at 0.99998")
    assert got.parallax == TH and got.status == IR.PARALLAX and got.n_triangulated == 52
    got = hook(mc, low + [Ic.case_cos(below)] * 53, "median one double below")
    assert got.parallax == below and got.status == IR.DONE and got.n_triangulated == 105


def test_baseline_gate(mc):
    t = np.array([3.0, 4.0, 0.0])     # the norm is 5.0 exactly
    cases = Ic.good_cases(51, c2=(3.0, 4.0, 0.0))
    got = hook(mc, cases, "equal: refused by >", t=t, min_baseline=5.0)
    assert got.status == IR.BASELINE and got.t_out.tolist() == t.tolist()
    assert hook(mc, cases, "the next double above", t=t, min_baseline=math.nextafter(5.0, 0.0)).status == IR.DONE


def test_one_camera_rig_scales(mc):
    """t_out, the points and the normals against written-out values, on a median where * (1 / m) and / m differ"""
    for t0 in (1.0, 0.3, 0.7, 1.1, 1.3, 1.7, 1.9):
        cases, t = Ic.good_cases(51, seed=21, c2=(t0, 0.0, 0.0)), np.array([t0, 0.0, 0.0])
        m = Ic.ref_hook(cases, ncams=1, t=t)["median_scene_depth"]
        if t0 * (1.0 / m) != t0 / m:
            break
    else:
        raise AssertionError("no candidate separates the two forms")
    got = hook(mc, cases, "scaled", ncams=1, t=t)
    m = got.median_scene_depth
    s = 1.0 / m
    assert got.scaled and got.status == IR.DONE and got.t_out.tolist() == [t0 * s, 0.0, 0.0] and got.t_out[0] != t0 / m
    for i, c in enumerate(cases):
        X = [v * s for v in c["X"]]
        assert got.pt3d[i].tolist() == X
        d1 = X                                          # prev's camera is at the origin
        d2 = [X[0] - t0 * s, X[1], X[2]]                # cur's at t_out: body centre 0
        i1 = 1.0 / math.sqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2])
        i2 = 1.0 / math.sqrt(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2])
        want = [(((0.0 + d1[k] * i1) * 1.0) * 1.0 + (0.0 + d2[k] * i2)) * 0.5 for k in range(3)]
        assert got.normal[i].tolist() == want and got.n_rays[i] == 2
    unscaled = hook(mc, cases, "4 cameras, n >= 50", ncams=4, t=t)
    assert not unscaled.scaled and unscaled.t_out.tolist() == t.tolist() and unscaled.pt3d[0].tolist() == cases[0]["X"]
    assert hook(mc, cases[:49], "n < 50 cannot be DONE", ncams=4, t=t).status == IR.FEW


# ---------------------------------------------------------------------------------------------------------------------------
# the whole call
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_covers_every_verdict(scenes):
    for C, (sc, ref) in scenes.items():
        assert ref["status"] == IR.DONE and not any(ref["near"]), C
        for v in (0, 3, 4, 5, 9):
            assert ref["verdict"].count(v) >= 0.05 * len(ref["verdict"]), (C, v)


@pytest.mark.parametrize("ncams", [1, 4, 8])
def test_scene_against_the_restatement(mc, voc, scenes, ncams):
    sc, ref = scenes[ncams]
    lm = store(mc, voc)
    got = Ic.run_scene(mc, lm, sc)
    same_scene(got, ref, sc, ncams)
    assert got.scaled == (ncams == 1) and got.n_initial_inliers == int(sc["flags"].sum())
    # ids in match order, the later match wins in lIds, ids from before are overwritten
    new = got.new_lid[got.new_lid >= 0]
    assert new.tolist() == list(range(sc["next_lid"], sc["next_lid"] + got.n_triangulated)) and got.next_lid == sc["next_lid"] + len(new)
    q, t = sc["matches"][:, 0], sc["matches"][:, 1]
    acc = np.nonzero(got.new_lid >= 0)[0]
    assert len(set(q[acc].tolist())) < len(acc) and len(set(t[acc].tolist())) < len(acc), "duplicate queryIdx and trainIdx among the accepted"
    for i in acc:
        later = [j for j in acc if j > i and q[j] == q[i]]
        assert got.lids_prev[q[i]] == got.new_lid[later[-1] if later else i]
        later = [j for j in acc if j > i and t[j] == t[i]]
        assert got.lids_cur[t[i]] == got.new_lid[later[-1] if later else i]
    untouched = np.setdiff1d(np.arange(len(got.lids_prev)), q[acc])
    assert (got.lids_prev[untouched] == sc["prev"]["lids"][untouched]).all()
    # the store holds what was returned, and nothing beyond
    for i in acc:
        p, nrm, d, _ = lm.get(int(got.new_lid[i]))
        assert bits(p) == bits(got.pt3d[i]) and bits(nrm) == bits(got.normal[i]) and d is None
        assert lm.observations(int(got.new_lid[i]))[0] == ref["n_rays"][i]
    with pytest.raises(mc.McorbError):
        lm.get(int(new[-1]) + 1)


def test_cur_centre_and_twc_are_not_read(mc, voc, scenes):
    sc, _ = scenes[4]
    a = Ic.run_scene(mc, store(mc, voc), sc)
    sc2 = copy.deepcopy(sc)
    sc2["cur"]["centre_w"] = [np.full(3, 1e9) for _ in range(4)]
    sc2["cur"]["twc"], sc2["prev"]["twc"] = np.full(3, -7.0), np.full(3, 1e5)
    b = Ic.run_scene(mc, store(mc, voc), sc2)
    assert bits(a.normal) == bits(b.normal) and bits(a.pt3d) == bits(b.pt3d)


def snapshot(lm, ids):
    out = []
    for l in ids:
        try:
            out.append(tuple(bits(x) for x in lm.get(l)[:2]))
        except Exception:
            out.append(None)
    return out


def test_failed_verdict_stores_nothing(mc, voc, scenes):
    sc, _ = scenes[4]
    few = Ic.cut(sc, 60)
    few["flags"][40:] = False
    lm = store(mc, voc)
    lm.set([100, 101], np.ones((2, 3)), np.ones((2, 3)))
    before = snapshot(lm, range(95, 140))
    got = Ic.run_scene(mc, lm, few)
    ref = Ic.ref_scene(few)
    assert got.status == ref["status"] == IR.FEW and got.verdict.tolist() == ref["verdict"] and got.n_triangulated == ref["n_triangulated"] > 0
    assert (got.new_lid == -1).all() and got.next_lid == sc["next_lid"] and (got.normal == 0).all() and (got.pt3d != 0).any()
    assert got.lids_prev.tolist() == sc["prev"]["lids"].tolist() and got.lids_cur.tolist() == sc["cur"]["lids"].tolist()
    assert snapshot(lm, range(95, 140)) == before
    far = copy.deepcopy(sc)
    far["min_baseline"] = 50.0
    got = Ic.run_scene(mc, lm, far)
    assert got.status == IR.BASELINE and got.t_out.tolist() == sc["t"].tolist() and snapshot(lm, range(95, 140)) == before
    assert got.lids_prev.tolist() == sc["prev"]["lids"].tolist()


REFUSALS = [
    ("queryIdx outside its frame", lambda sc: sc["matches"].__setitem__((3, 0), 10 ** 6), "ARG", "match index outside a frame"),
    ("trainIdx -1", lambda sc: sc["matches"].__setitem__((3, 1), -1), "ARG", "match index outside a frame"),
    ("keypoint index outside a camera", lambda sc: sc["cur"]["match_index"].__setitem__((0, 0), 10 ** 6), "ARG", "match index outside a frame's keypoints"),
    ("a feature without a view", lambda sc: sc["prev"]["match_index"].__setitem__((int(sc["matches"][0, 0]), slice(None)), -1), "ARG",
     "a matched feature without a view"),
    ("octave at nlevels", lambda sc: sc.__setitem__("inv_sigma2", sc["inv_sigma2"][:1]), "ARG", "octave outside nlevels"),
    ("current lid at max_landmarks", lambda sc: sc["cur"]["lids"].__setitem__(0, 4096), "ARG", "landmark id outside the store"),
    ("previous lid -2", lambda sc: sc["prev"]["lids"].__setitem__(0, -2), "ARG", "landmark id outside the store"),
    ("next_lid -1", lambda sc: sc.__setitem__("next_lid", -1), "ARG", "bad argument"),
    ("camera counts differ", lambda sc: sc.__setitem__("prev", Ic.scene(1, n=20)["prev"]), "ARG", "bad frame"),
    ("per-match outputs one short", lambda sc: sc.__setitem__("cap", len(sc["matches"]) - 1), "CAP", "output too small"),
    ("ids one beyond the store", lambda sc: sc.__setitem__("next_lid", 4096 - int(sc["flags"].sum()) + 1), "CAP", "new landmark ids beyond max_landmarks"),
    ("more than MCORB_INIT_MAX_MATCHES", lambda sc: sc.__setitem__("many", True), "ARG", "more than MCORB_INIT_MAX_MATCHES matches"),
    ("a tracking call is pending", lambda sc: sc.__setitem__("pending", True), "STATE", "a submitted tracking call has not been waited for"),
    ("more than MCORB_MAX_CAMS views", lambda sc: Ic.seventeen_views(), "ARG",
     "a match of more than MCORB_MAX_CAMS views in total (the solver's design limit)"),
    ("cap_matches -1", lambda sc: sc.__setitem__("cap", -1), "ARG", "bad argument"),
]
# the arguments of mcorb_lmap_initialize by position (the wrapper never passes a NULL): each is replaced in the C call itself
ARG_AT = dict(store=0, prev=1, lids_prev=2, cur=3, lids_cur=4, R=5, t=6, cam_centre_body=7, match_query=8, match_train=9, K=11, inv_sigma2=12,
              out=16)
REFUSALS += [(k + " NULL", (lambda at: lambda sc: sc.__setitem__("edit", lambda a: a.__setitem__(at, None)))(at), "ARG", "bad argument")
             for k, at in ARG_AT.items()]
REFUSALS += [("nlevels 0", lambda sc: sc.__setitem__("edit", lambda a: a.__setitem__(13, 0)), "ARG", "bad argument")]
REFUSALS += [("out->" + f + " NULL", (lambda f: lambda sc: sc.__setitem__("edit", lambda a: setattr(a[16]._obj, f, None)))(f), "ARG", "bad argument")
             for f in ("inliers", "verdict", "new_lid", "pt3d", "normal", "dist2", "cos_parallax")]


class EditedCall:
    """the library with the arguments of mcorb_lmap_initialize changed by `edit` just before the C call"""

    def __init__(self, L, edit):
        self.L, self.edit = L, edit

    def __getattr__(self, name):
        fn = getattr(self.L, name)
        if name != "mcorb_lmap_initialize":
            return fn

        def call(*a):
            a = list(a)
            self.edit(a)
            return fn(*a)
        return call


def run_refusals(mc, lm, sc0):
    from test_lmap_refusals_cpu import last_error, pending
    assert len({r[0] for r in REFUSALS}) == len(REFUSALS) == 36
    lm.set([100, 101], np.ones((2, 3)), np.ones((2, 3)))
    before = snapshot(lm, range(95, 140))
    L = lm.L
    for name, change, code, text in REFUSALS:
        sc = copy.deepcopy(sc0)
        sc = change(sc) or sc
        if sc.pop("many", False):
            k = mc.INIT_MAX_MATCHES + 1
            sc["matches"], sc["flags"] = np.tile(sc["matches"][:1], (k, 1)), np.ones(k, bool)
        if sc.pop("pending", False):
            pending(mc, lm)
        kw = dict(cap=sc.pop("cap")) if "cap" in sc else {}
        if "edit" in sc:
            lm.L = EditedCall(L, sc.pop("edit"))
        try:
            with pytest.raises(mc.McorbError) as ei:
                Ic.run_scene(mc, lm, sc, **kw)
        finally:
            lm.L = L
        text_got = last_error(mc)
        lm.L.mcorb_lmap_track_wait(lm.h, None)    # (ends the pending call where there is one)
        assert ei.value.code == getattr(mc, "E_" + code) and text_got == "lmap initialize: " + text, (name, text_got)
        lp, lc = lm.init_lids
        assert lp.tolist() == sc["prev"]["lids"].tolist() and lc.tolist() == sc["cur"]["lids"].tolist(), name
        assert snapshot(lm, range(95, 140)) == before, name
    assert Ic.run_scene(mc, lm, sc0).status == IR.DONE     # and the call runs after all that


def test_refusals(mc, voc, scenes):
    run_refusals(mc, store(mc, voc), scenes[4][0])


def test_sanitized_serial_run(mc, voc, scenes, tmp_path):
    """tests/cpp/test_init_sanitize.cpp: init_run_serial on the seeded scene under -fsanitize=address,undefined gives no report,
    and its records equal the library's"""
    sc, _ = scenes[4]
    exe = str(tmp_path / "init_sanitize")
    csrc = os.path.join(ROOT, "mc-slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "cpp", "test_init_sanitize.cpp"), "-o", exe])
    got = Ic.run_scene(mc, store(mc, voc), sc)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    C = sc["ncams"]
    with open(inp, "wb") as f:
        n = len(sc["matches"])
        np.array([C, n, len(sc["inv_sigma2"]), sc["next_lid"], len(sc["prev"]["match_index"]), len(sc["cur"]["match_index"])], np.int32).tofile(f)
        for a in (sc["R"], sc["t"], sc["body"], sc["K"]):
            np.ascontiguousarray(a, np.float64).tofile(f)
        np.ascontiguousarray(sc["inv_sigma2"], np.float32).tofile(f)
        sc["matches"].astype(np.int32).tofile(f)
        sc["flags"].astype(np.uint8).tofile(f)
        for fr in (sc["cur"], sc["prev"]):
            np.ascontiguousarray(fr["match_index"], np.int32).tofile(f)
            np.ascontiguousarray(fr["proj"], np.float64).tofile(f)
            np.ascontiguousarray(fr["centre_w"], np.float64).tofile(f)
            np.array([len(k) for k in fr["kps"]], np.int32).tofile(f)
            for k in fr["kps"]:
                np.stack([k["x"], k["y"]], axis=1).astype(np.float32).tofile(f)
                k["octave"].astype(np.int32).tofile(f)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = np.fromfile(outp, np.uint8)
    rec = np.dtype([("X", "<f8", 3), ("normal", "<f8", 3), ("dist2", "<f8"), ("cos", "<f8"), ("verdict", "<i4"), ("n_rays", "<i4")])
    recs = raw[:n * rec.itemsize].view(rec)
    call = raw[n * rec.itemsize:]
    assert recs["verdict"].tolist() == got.verdict.tolist()
    assert bits(recs["X"]) == bits(got.pt3d) and bits(recs["normal"]) == bits(got.normal)
    assert bits(recs["dist2"]) == bits(got.dist2) and bits(recs["cos"]) == bits(got.cos_parallax)
    assert bits(call[:40].view("<f8")) == bits([got.parallax, got.median_scene_depth] + got.t_out.tolist())
    assert call[40:64].view("<i4").tolist() == [got.status, got.n_initial_inliers, got.n_parallax, got.n_triangulated, int(got.scaled), got.next_lid]
