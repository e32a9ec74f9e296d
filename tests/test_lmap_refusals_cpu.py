"""The single-fault refusals of mcorb_lmap_refine_pose, mcorb_lmap_ransac_pose, mcorb_lmap_triangulate_neighbours and
mcorb_lmap_triangulate_new on a host-only store: every call below has exactly one thing wrong, and the return code and the text
of mcorb_last_error() are compared with literals, character for character.  The literals were written down from the library as
it was before the four entries' checks were shared, so a check that moves, merges or changes its words shows here.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import kfdb_cases as K
import mapping_cases as Mc
import mapping_new_cases as Nc
import pose_cases as PC
import sac_cases as SC
import test_mapping_cpu as TM
import test_mapping_new_cpu as TN
import track_cases as T

ARG, CAP, STATE = "E_ARG", "E_CAP", "E_STATE"
MAXL = 4096


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def store(mc, voc):
    return mc.LocalMap(voc, device=-1, max_landmarks=MAXL, max_candidates=1024)


def last_error(mc):
    return mc._lib.load().mcorb_last_error().decode()


def run_table(mc, table, call, want):
    """table: (name, change of the argument dict); call: dict -> return code; want: name -> (code name, text)"""
    assert sorted(n for n, _ in table) == sorted(want), "the table and the literals name the same faults"
    got = {}
    for name, change in table:
        got[name] = call(change)
    for name, (code, text) in got.items():
        print("%-40s %d %s" % (name, code, text))
    for name, (code, text) in got.items():
        assert (code, text) == (getattr(mc, want[name][0]), want[name][1]), name


def put(key, value):
    return lambda a: a.__setitem__(key, value)


def put_at(key, i, value):
    def change(a):
        a[key] = a[key].copy()
        a[key][i] = value
    return change


# ---------------------------------------------------------------------------------------------------------------------------
# refine_pose and ransac_pose: one observation input
# ---------------------------------------------------------------------------------------------------------------------------
def obs_args(mc, lm):
    cams, truth, obs, match, moved = SC.scene(2, nlm=12, seed=7, per_match=2)
    cam, uv, octave, pts = PC.arrays(obs)
    cc = PC.to_cams(mc, cams)
    a = dict(n=len(obs), cam=cam, uv=uv, octave=octave, match=np.asarray(match, np.int32), lids=PC.fill_points(lm, obs), pts=None, ncams=2,
             cams=C.addressof(cc.cams), R=np.eye(3).reshape(9), t=np.zeros(3), pose=mc.pose_params(PC.INV_SIGMA2), res=True,
             inlier=np.zeros(len(obs), np.uint8), keep=cc)
    return a, pts


def ptr(v):
    return None if v is None else v if isinstance(v, int) else v.ctypes.data


def obs_faults(pts, nlevels):
    """what both entries refuse"""
    return [("cam NULL", put("cam", None)), ("uv NULL", put("uv", None)), ("octave NULL", put("octave", None)),
            ("cams NULL", put("cams", None)), ("res NULL", put("res", False)), ("n negative", put("n", -1)),
            ("ncams 0", put("ncams", 0)), ("ncams MAX + 1", put("ncams", mc_max_cams() + 1)),
            ("camera at ncams", put_at("cam", 5, 2)), ("camera -1", put_at("cam", 0, -1)),
            ("octave at nlevels", put_at("octave", 3, nlevels)), ("octave -1", put_at("octave", 3, -1)),
            ("lid at max_landmarks", put_at("lids", 4, MAXL)), ("lid -1", put_at("lids", 4, -1)),
            ("both lids and pts", put("pts", pts)), ("neither lids nor pts", put("lids", None)),
            ("a landmark without a point", put_at("lids", 2, 3000))]


def mc_max_cams():
    import mcorb
    return mcorb._lib.MAX_CAMS


POSE_WANT = {
    "cam NULL": (ARG, "lmap pose: bad argument"),
    "uv NULL": (ARG, "lmap pose: bad argument"),
    "octave NULL": (ARG, "lmap pose: bad argument"),
    "cams NULL": (ARG, "lmap pose: bad argument"),
    "res NULL": (ARG, "lmap pose: bad argument"),
    "n negative": (ARG, "lmap pose: bad argument"),
    "R NULL": (ARG, "lmap pose: bad argument"),
    "t NULL": (ARG, "lmap pose: bad argument"),
    "params NULL": (ARG, "lmap pose: bad argument"),
    "ncams 0": (ARG, "lmap pose: 1 .. MCORB_MAX_CAMS cameras"),
    "ncams MAX + 1": (ARG, "lmap pose: 1 .. MCORB_MAX_CAMS cameras"),
    "camera at ncams": (ARG, "lmap pose: a camera index outside the rig"),
    "camera -1": (ARG, "lmap pose: a camera index outside the rig"),
    "octave at nlevels": (ARG, "lmap pose: an octave outside the levels"),
    "octave -1": (ARG, "lmap pose: an octave outside the levels"),
    "lid at max_landmarks": (ARG, "lmap pose: landmark id outside the store"),
    "lid -1": (ARG, "lmap pose: landmark id outside the store"),
    "both lids and pts": (ARG, "lmap pose: exactly one of lids and pts"),
    "neither lids nor pts": (ARG, "lmap pose: exactly one of lids and pts"),
    "a landmark without a point": (STATE, "lmap pose: a landmark has no point"),
    "iterations 0": (ARG, "lmap pose: 1 .. 100 iterations"),
    "iterations 101": (ARG, "lmap pose: 1 .. 100 iterations"),
    "levels 0": (ARG, "lmap pose: 1 .. MCORB_MAX_LEVELS levels"),
    "levels MAX + 1": (ARG, "lmap pose: 1 .. MCORB_MAX_LEVELS levels"),
    "store NULL": (ARG, "lmap refine_pose: bad argument"),
    "a tracking call is pending": (STATE, "lmap refine_pose: a submitted tracking call has not been waited for"),
}


def pending(mc, lm):
    lm.track_submit(T.to_view(mc, T.flat_view()), [np.zeros((0, 2), np.float32)], [np.zeros((0, 32), np.uint8)], [])


def test_refine_pose_refusals(mc, voc):
    lm = store(mc, voc)
    base, pts = obs_args(mc, lm)
    rig, _, obs, _, _ = SC.scene(2, nlm=12, seed=7, per_match=2)
    want = PC.refine(mc, lm, rig, PC.IDENT, obs)

    def call(change):
        a = dict(base)
        change(a)
        res = mc._lib.PoseResultC()
        if a.pop("pending", False):
            pending(mc, lm)
        code = lm.L.mcorb_lmap_refine_pose(lm.h if a.get("store", True) else None, a["n"], ptr(a["cam"]), ptr(a["uv"]), ptr(a["octave"]),
                                           ptr(a["lids"]), ptr(a["pts"]), a["ncams"], a["cams"], ptr(a["R"]), ptr(a["t"]),
                                           None if a["pose"] is None else C.byref(a["pose"]), C.byref(res) if a["res"] else None,
                                           ptr(a["inlier"]))
        text = last_error(mc)
        lm.L.mcorb_lmap_track_wait(lm.h, None)    # (ends the pending call where there is one)
        return code, text

    table = obs_faults(pts, len(PC.INV_SIGMA2)) + [
        ("R NULL", put("R", None)), ("t NULL", put("t", None)), ("params NULL", put("pose", None)),
        ("iterations 0", put("pose", mc.pose_params(PC.INV_SIGMA2, 0))), ("iterations 101", put("pose", mc.pose_params(PC.INV_SIGMA2, 101))),
        ("levels 0", put("pose", mc.pose_params([]))), ("levels MAX + 1", put("pose", mc.pose_params([1.0] * (mc._lib.MAX_LEVELS + 1)))),
        ("store NULL", put("store", False)), ("a tracking call is pending", put("pending", True))]
    run_table(mc, table, call, POSE_WANT)
    # and the call runs after all that, with the result it had
    again = PC.refine(mc, lm, rig, PC.IDENT, obs)
    PC.same(PC.as_ref(again), PC.as_ref(want), "after the refusals")


SAC_WANT = {
    "cam NULL": (ARG, "lmap ransac_pose: bad argument"),
    "uv NULL": (ARG, "lmap ransac_pose: bad argument"),
    "octave NULL": (ARG, "lmap ransac_pose: bad argument"),
    "cams NULL": (ARG, "lmap ransac_pose: bad argument"),
    "res NULL": (ARG, "lmap ransac_pose: bad argument"),
    "n negative": (ARG, "lmap ransac_pose: bad argument"),
    "params NULL": (ARG, "lmap ransac_pose: bad argument"),
    "ncams 0": (ARG, "lmap ransac_pose: 1 .. MCORB_MAX_CAMS cameras"),
    "ncams MAX + 1": (ARG, "lmap ransac_pose: 1 .. MCORB_MAX_CAMS cameras"),
    "camera at ncams": (ARG, "lmap ransac_pose: a camera index outside the rig"),
    "camera -1": (ARG, "lmap ransac_pose: a camera index outside the rig"),
    "octave at nlevels": (ARG, "lmap ransac_pose: an octave outside the levels"),
    "octave -1": (ARG, "lmap ransac_pose: an octave outside the levels"),
    "octave at MAX_LEVELS, no refinement": (ARG, "lmap ransac_pose: an octave outside the levels"),
    "lid at max_landmarks": (ARG, "lmap ransac_pose: landmark id outside the store"),
    "lid -1": (ARG, "lmap ransac_pose: landmark id outside the store"),
    "both lids and pts": (ARG, "lmap ransac_pose: exactly one of lids and pts"),
    "neither lids nor pts": (ARG, "lmap ransac_pose: exactly one of lids and pts"),
    "a landmark without a point": (STATE, "lmap ransac_pose: a landmark has no point"),
    "a decreasing match index": (ARG, "lmap ransac_pose: a match index that is negative or decreases"),
    "a negative match index": (ARG, "lmap ransac_pose: a match index that is negative or decreases"),
    "iterations 0": (ARG, "lmap ransac_pose: 1 .. MCORB_SAC_MAX_ITERATIONS iterations"),
    "iterations MAX + 1": (ARG, "lmap ransac_pose: 1 .. MCORB_SAC_MAX_ITERATIONS iterations"),
    "threshold 0": (ARG, "lmap ransac_pose: a threshold that is not finite and positive"),
    "threshold NaN": (ARG, "lmap ransac_pose: a threshold that is not finite and positive"),
    "threshold inf": (ARG, "lmap ransac_pose: a threshold that is not finite and positive"),
    "an unknown solver": (ARG, "lmap ransac_pose: a solver that is not one of MCORB_SAC_SOLVER_*"),
    "refinement: iterations 0": (ARG, "lmap pose: 1 .. 100 iterations"),
    "refinement: iterations 101": (ARG, "lmap pose: 1 .. 100 iterations"),
    "refinement: levels MAX + 1": (ARG, "lmap pose: 1 .. MCORB_MAX_LEVELS levels"),
    "store NULL": (ARG, "lmap ransac_pose: bad argument"),
    "a tracking call is pending": (STATE, "lmap ransac_pose: a submitted tracking call has not been waited for"),
}


def test_ransac_pose_refusals(mc, voc):
    lm = store(mc, voc)
    base, pts = obs_args(mc, lm)
    base.update(threshold=SC.THRESHOLD, max_iterations=32, solver=0, par=True)

    def call(change):
        a = dict(base)
        change(a)
        par, res = mc._lib.SacParams(), mc._lib.SacResultC()
        par.threshold, par.seed, par.max_iterations, par.solver = a["threshold"], 0, a["max_iterations"], a["solver"]
        if a.pop("pending", False):
            pending(mc, lm)
        code = lm.L.mcorb_lmap_ransac_pose(lm.h if a.get("store", True) else None, a["n"], ptr(a["cam"]), ptr(a["uv"]), ptr(a["octave"]),
                                           ptr(a["match"]), ptr(a["lids"]), ptr(a["pts"]), a["ncams"], a["cams"],
                                           C.byref(par) if a["par"] else None, None if a["pose"] is None else C.byref(a["pose"]),
                                           C.byref(res) if a["res"] else None, ptr(a["inlier"]))
        text = last_error(mc)
        lm.L.mcorb_lmap_track_wait(lm.h, None)
        return code, text

    def no_refine(change):
        def both(a):
            a["pose"] = None
            change(a)
        return both

    dec = base["match"].copy()
    dec[6], dec[7] = dec[7] + 1, dec[6]
    assert dec[7] < dec[6]
    table = obs_faults(pts, len(PC.INV_SIGMA2)) + [
        ("octave at MAX_LEVELS, no refinement", no_refine(put_at("octave", 3, mc._lib.MAX_LEVELS))),
        ("params NULL", put("par", False)), ("a decreasing match index", put("match", dec)),
        ("a negative match index", put("match", base["match"] - 1)),
        ("iterations 0", put("max_iterations", 0)), ("iterations MAX + 1", put("max_iterations", 1025)),
        ("threshold 0", put("threshold", 0.0)), ("threshold NaN", put("threshold", float("nan"))),
        ("threshold inf", put("threshold", float("inf"))), ("an unknown solver", put("solver", 2)),
        ("refinement: iterations 0", put("pose", mc.pose_params(PC.INV_SIGMA2, 0))),
        ("refinement: iterations 101", put("pose", mc.pose_params(PC.INV_SIGMA2, 101))),
        ("refinement: levels MAX + 1", put("pose", mc.pose_params([1.0] * (mc._lib.MAX_LEVELS + 1)))),
        ("store NULL", put("store", False)), ("a tracking call is pending", put("pending", True))]
    run_table(mc, table, call, SAC_WANT)
    assert call(lambda a: None)[0] == mc.OK


# ---------------------------------------------------------------------------------------------------------------------------
# triangulate_neighbours and triangulate_new: one skeleton
# ---------------------------------------------------------------------------------------------------------------------------
def frame_faults(other):
    """what both entries refuse; other: the scene's key of the second frame (a neighbour, the previous keyframe)"""
    f2 = (lambda sc: sc[other][0]) if other == "neigh" else (lambda sc: sc[other])
    ms = (lambda sc: sc["matches"][0]) if other == "neigh" else (lambda sc: sc["matches"])

    def two_cams(sc):
        f = f2(sc)
        f["match_index"] = np.concatenate([f["match_index"], f["match_index"]], axis=1)
        for k in ("kps", "centre_w", "proj"):
            f[k] = list(f[k]) * 2

    return [("queryIdx outside its frame", lambda sc: ms(sc).__setitem__((0, 0), len(f2(sc)["lids"]))),
            ("trainIdx -1", lambda sc: ms(sc).__setitem__((1, 1), -1)),
            ("keypoint index outside a camera", lambda sc: f2(sc)["match_index"].__setitem__((2, 0), len(f2(sc)["kps"][0]))),
            ("keypoint index -2", lambda sc: sc["cur"]["match_index"].__setitem__((0, 0), -2)),
            ("a feature without a view", lambda sc: sc["cur"]["match_index"].__setitem__((1, 0), -1)),
            ("octave at nlevels", lambda sc: sc["cur"]["kps"][0]["octave"].__setitem__(0, Mc.NLEVELS)),
            ("octave -1", lambda sc: f2(sc)["kps"][0]["octave"].__setitem__(1, -1)),
            ("current lid at max_landmarks", lambda sc: sc["cur"]["lids"].__setitem__(0, MAXL)),
            ("other lid -2", lambda sc: f2(sc)["lids"].__setitem__(1, -2)),
            ("next_lid -1", lambda sc: sc.__setitem__("next_lid", -1)),
            ("camera counts differ", two_cams),
            ("per-match outputs one short", lambda sc: sc.__setitem__("caps", (2, 3))),
            ("depth_vec one short", lambda sc: sc.__setitem__("caps", (3, 2))),
            ("ids one beyond the store", lambda sc: sc.__setitem__("next_lid", MAXL - 2))]


def seventeen_views(other):
    """9 + 8 views of one match: beyond MCORB_MAX_CAMS"""
    rng = np.random.default_rng(2)
    Ks, rigT = Mc.make_rig(16, rng)
    cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(TM.I3, np.zeros(3)), rigT), Ks)
    nb = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(TM.I3, np.array([1.0, 0, 0])), rigT), Ks)
    X = np.array([0.2, 0.1, 6.0])
    nb.add(X, [0], rng, lid=900)
    q9, t8 = nb.add(X, list(range(9)), rng), cur.add(X, list(range(8, 16)), rng)
    m = np.array([(q9, t8)], np.int32)
    if other == "prev":
        return dict(K=np.array(Ks), inv_sigma2=Nc.inv_sigma2(1.0), cur=cur.done(), prev=nb.done(), matches=m, next_lid=10)
    F = np.zeros((16, 16, 3, 3))
    return dict(K=np.array(Ks), inv_sigma2=Mc.INV_SIGMA2, cur=cur.done(), neigh=[nb.done()], F21=[F], store={900: X}, matches=[m], Rcw=TM.I3,
                tcw=np.zeros(3), next_lid=10)


NEIGH_WANT = {
    "queryIdx outside its frame": (ARG, "lmap triangulate_neighbours: match index outside a frame"),
    "trainIdx -1": (ARG, "lmap triangulate_neighbours: match index outside a frame"),
    "keypoint index outside a camera": (ARG, "lmap triangulate_neighbours: match index outside a frame's keypoints"),
    "keypoint index -2": (ARG, "lmap triangulate_neighbours: match index outside a frame's keypoints"),
    "a feature without a view": (ARG, "lmap triangulate_neighbours: a matched feature without a view"),
    "octave at nlevels": (ARG, "lmap triangulate_neighbours: octave outside nlevels"),
    "octave -1": (ARG, "lmap triangulate_neighbours: octave outside nlevels"),
    "current lid at max_landmarks": (ARG, "lmap triangulate_neighbours: landmark id outside the store"),
    "other lid -2": (ARG, "lmap triangulate_neighbours: landmark id outside the store"),
    "next_lid -1": (ARG, "lmap triangulate_neighbours: bad argument"),
    "lids_cur NULL": (ARG, "lmap triangulate_neighbours: bad argument"),
    "match_query NULL": (ARG, "lmap triangulate_neighbours: bad argument"),
    "K NULL": (ARG, "lmap triangulate_neighbours: bad argument"),
    "out NULL": (ARG, "lmap triangulate_neighbours: bad argument"),
    "camera counts differ": (ARG, "lmap triangulate_neighbours: bad frame"),
    "per-match outputs one short": (CAP, "lmap triangulate_neighbours: output too small"),
    "depth_vec one short": (CAP, "lmap triangulate_neighbours: output too small"),
    "ids one beyond the store": (CAP, "lmap triangulate_neighbours: new landmark ids beyond max_landmarks"),
    "a neighbour's landmark never set": (STATE, "lmap triangulate_neighbours: a neighbour's landmark was never set"),
    "more than MCORB_MAX_CAMS views": (ARG, "lmap triangulate_neighbours: a match of more than MCORB_MAX_CAMS views in total (the solver's design limit)"),
    "a tracking call is pending": (STATE, "lmap triangulate_neighbours: a submitted tracking call has not been waited for"),
}


class NullArg:
    """the library with one pointer argument of the mapping entries replaced by NULL (the wrappers never pass one)"""

    def __init__(self, L, at):
        self.L, self.at = L, at

    def __getattr__(self, name):
        fn = getattr(self.L, name)
        if not name.startswith("mcorb_lmap_triangulate_ne"):
            return fn
        return lambda *a: fn(*[None if i == self.at else v for i, v in enumerate(a)])


def run_mapping(mc, voc, run, make, table, want):
    def call(change):
        sc = make() if not isinstance(change, dict) else change
        if not isinstance(change, dict):
            change(sc)
        lm = store(mc, voc)
        Mc.fill_store(lm, sc.get("store", {}))
        if sc.pop("pending", False):
            pending(mc, lm)
        kw = dict(caps=sc.pop("caps")) if "caps" in sc else {}
        if "null" in sc:
            lm.L = NullArg(lm.L, sc.pop("null"))
        try:
            run(mc, lm, sc, **kw)
        except mc.McorbError as e:
            return e.code, last_error(mc)
        return mc.OK, ""
    run_table(mc, table, call, want)
    assert call(lambda sc: None)[0] == mc.OK


def test_triangulate_neighbours_refusals(mc, voc):
    def make():
        m, ms = TM.good_mini()
        return m.scene([ms])
    table = frame_faults("neigh") + [("lids_cur NULL", lambda sc: sc.__setitem__("null", 2)), ("match_query NULL", lambda sc: sc.__setitem__("null", 7)),
                                     ("K NULL", lambda sc: sc.__setitem__("null", 10)), ("out NULL", lambda sc: sc.__setitem__("null", 16)),
                                     ("a neighbour's landmark never set", lambda sc: sc["store"].pop(900)),
                                     ("more than MCORB_MAX_CAMS views", seventeen_views("neigh")),
                                     ("a tracking call is pending", lambda sc: sc.__setitem__("pending", True))]
    run_mapping(mc, voc, Mc.run_scene, make, table, NEIGH_WANT)


NEW_WANT = {
    "queryIdx outside its frame": (ARG, "lmap triangulate_new: match index outside a frame"),
    "trainIdx -1": (ARG, "lmap triangulate_new: match index outside a frame"),
    "keypoint index outside a camera": (ARG, "lmap triangulate_new: match index outside a frame's keypoints"),
    "keypoint index -2": (ARG, "lmap triangulate_new: match index outside a frame's keypoints"),
    "a feature without a view": (ARG, "lmap triangulate_new: a matched feature without a view"),
    "octave at nlevels": (ARG, "lmap triangulate_new: octave outside nlevels"),
    "octave -1": (ARG, "lmap triangulate_new: octave outside nlevels"),
    "current lid at max_landmarks": (ARG, "lmap triangulate_new: landmark id outside the store"),
    "other lid -2": (ARG, "lmap triangulate_new: landmark id outside the store"),
    "next_lid -1": (ARG, "lmap triangulate_new: bad argument"),
    "lids_cur NULL": (ARG, "lmap triangulate_new: bad argument"),
    "match_query NULL": (ARG, "lmap triangulate_new: bad argument"),
    "K NULL": (ARG, "lmap triangulate_new: bad argument"),
    "out NULL": (ARG, "lmap triangulate_new: bad argument"),
    "camera counts differ": (ARG, "lmap triangulate_new: bad frame"),
    "per-match outputs one short": (CAP, "lmap triangulate_new: output too small"),
    "depth_vec one short": (CAP, "lmap triangulate_new: output too small"),
    "ids one beyond the store": (CAP, "lmap triangulate_new: new landmark ids beyond max_landmarks"),
    "more than MCORB_MAX_CAMS views": (ARG, "lmap triangulate_new: a match of more than MCORB_MAX_CAMS views in total (the solver's design limit)"),
    "a tracking call is pending": (STATE, "lmap triangulate_new: a submitted tracking call has not been waited for"),
}


def test_triangulate_new_refusals(mc, voc):
    def make():
        m, ms = TN.good_mini()
        return m.scene(ms)
    table = frame_faults("prev") + [("lids_cur NULL", lambda sc: sc.__setitem__("null", 2)), ("match_query NULL", lambda sc: sc.__setitem__("null", 5)),
                                    ("K NULL", lambda sc: sc.__setitem__("null", 8)), ("out NULL", lambda sc: sc.__setitem__("null", 12)),
                                    ("more than MCORB_MAX_CAMS views", seventeen_views("prev")),
                                    ("a tracking call is pending", lambda sc: sc.__setitem__("pending", True))]
    run_mapping(mc, voc, Nc.run_scene, make, table, NEW_WANT)
