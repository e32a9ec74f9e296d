"""The back end's and mapping's calls on degenerate and hostile inputs, without a GPU: on every row of the tables of
hostile_backend_cases.py the host-only store == the restatement (ba_ref.py, retri_ref.py, pose_ref.py, mapping_new_ref.py,
mapping_ref.py, init_ref.py) -- doubles as raw bytes, every NaN the default quiet NaN, no tolerance, no excluded row.
triangulate_neighbours' and initialize's restatements take the point of a match from the library's DLT hook here, as
mapping_new_ref.py always does (their own SVD agrees with it to 1e-9 on well-posed matches only), so that everything behind the
point compares on the bytes.  The tables themselves are held to what they are for, on the restatement alone: the well-posed
row ends in the good status, every status or verdict a call can return after a launch ends some row, rows with non-finite input
leave what the bad value does not touch as the well-posed row has it, and the scaled rows lie either side of the scale at which
the restatement's answer changes.  And the branch outcomes of the seven shared headers that docs/design/09q_hostile_backend.md
lists as reached by the tables are taken by them (scripts/header_coverage.py).

test_gpu_hostile_backend.py runs the same rows on a device store."""
import os

import numpy as np
import pytest

import ba_cases as BC
import ba_ref as B
import hostile_backend_cases as HB
import init_cases as Ic
import init_ref as IR
import kfdb_cases as K
import landmark_cases as Lc
import mapping_cases as Mc
import mapping_new_cases as Nc
import mapping_new_ref as N
import mapping_ref as MR
import pose_cases as PC
import pose_ref as P
import retri_cases as RC
import retri_ref as R
from hostile_backend_cases import names
from test_hostile_cpu import ROOT, doc_lists, header_coverage, hold_the_lists
from test_init_cpu import same_hook

MAXL = 65536
# where each call's rows keep what they write: retriangulate's apply rows, and the new landmarks of the front end's three calls
# (the neighbours' old landmarks are the scenes' own 3000 .., the frames' preset ids 3900 ..)
AT = dict(apply=(40000, 70), new=(8000, 100), neigh=(14000, 150), init=(24000, 100))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lm(mc):
    return mc.LocalMap(mc.ORBVocabulary(device=-1).create(**K.vocabulary()), device=-1, max_landmarks=MAXL, max_candidates=1024)


def at(call, rows, row):
    first, step = AT[call]
    return first + step * names(rows).index(row[0])


# ---------------------------------------------------------------------------------------------------------------------------
# one launch of a row on a store against the restatement -> (result, restatement); test_gpu_hostile_backend.py uses these on
# both stores.  A row's restatement is computed once
# ---------------------------------------------------------------------------------------------------------------------------
_REF = {}


def cached(key, fn):
    if key not in _REF:
        with np.errstate(all="ignore"):
            _REF[key] = fn()
    return _REF[key]


def ba_ref(row):
    name, sc, kw = row
    return cached(("ba", name), lambda: BC.ref(sc, kw.get("max_iterations", HB.BA_ITERATIONS)))


def ba_check(mc, lm, row, who, forms=("pts", "lids")):
    name, sc, kw = row
    ref, got = ba_ref(row), []
    for form in forms:
        got.append(BC.run(mc, lm, sc, kw.get("max_iterations", HB.BA_ITERATIONS), form))
        BC.same(BC.as_ref(got[-1]), ref, "%s: %s, %s" % (name, who, form))
        assert got[-1].n_obs == len(sc["obs"])
    return got, ref


def retri_ref(row):
    name, sc, kw = row
    return cached(("retri", name), lambda: RC.ref(sc, **kw))


def retri_check(mc, lm, row, who):
    """report mode: the store is not written"""
    name, sc, kw = row
    ref = retri_ref(row)
    before = Lc.snapshot(lm, RC.fill(lm, sc))
    got = RC.run(mc, lm, sc, **kw)
    RC.same(got, ref, "%s: %s" % (name, who))
    assert Lc.snapshot(lm, range(len(sc["pts"]))) == before, (name, who, "report mode wrote the store")
    return got, ref


def retri_apply(mc, lm, row, who):
    """apply mode on ids of the row's own, with a cap that holds every pair: the slots afterwards are what the restatement says
    -- the new point where the verdict is VALID_UPDATED, no landmark where it is a failed one, the old point elsewhere
    -> (result, the slots of the landmarks that are left)"""
    name, sc, kw = row
    ref = retri_ref(row)
    what = "%s, apply: %s" % (name, who)
    lids = RC.fill(lm, sc, first_lid=at("apply", HB.retri_rows(), row))
    got = RC.run(mc, lm, sc, lids=lids, apply=True, cap=len(sc["obs"]), **kw)
    RC.same(got, ref, what)
    alive = [j for j, v in enumerate(ref["verdict"]) if v not in R.FAILED]
    for j, v in enumerate(ref["verdict"]):
        if v in R.FAILED:
            Lc.expect(mc, mc.E_STATE, lambda: lm.get(int(lids[j])))
        else:
            want = ref["pts"][j] if v == R.VALID_UPDATED else sc["pts"][j]
            assert Nc.dcat(lm.get(int(lids[j]))[0]) == Nc.dcat(want), (what, "the store's point", j)
    return got, Lc.snapshot(lm, lids[alive])


def pose_ref(row):
    name, cams, init, obs, kw = row
    return cached(("pose", name), lambda: P.refine(cams, init, obs, kw.get("inv_sigma2", PC.INV_SIGMA2), kw.get("max_iterations", 25)))


def pose_check(mc, lm, row, who, forms=("pts", "lids")):
    name, cams, init, obs, kw = row
    ref, got = pose_ref(row), []
    for form in forms:
        got.append(PC.refine(mc, lm, cams, init, obs, kw.get("inv_sigma2", PC.INV_SIGMA2), kw.get("max_iterations", 25), form))
        PC.same(PC.as_ref(got[-1]), ref, "%s: %s, %s" % (name, who, form))
        assert got[-1].n_obs == len(obs)
    return got, ref


def lib_dlt(mc):
    return lambda views: N.initial_point(mc, views)


def new_scene(row):
    return dict(row[1], next_lid=at("new", HB.new_rows(), row))


def new_ref(mc, row):
    return cached(("new", row[0]), lambda: Nc.ref_of(mc, new_scene(row)))


def new_check(mc, lm, row, who):
    ref = new_ref(mc, row)
    got = Nc.run_scene(mc, lm, new_scene(row))
    try:
        Nc.same_as_ref(got, ref)
    except AssertionError as e:
        raise AssertionError((row[0], who) + e.args)
    return got, ref


def neigh_scene(row):
    return dict(row[1], next_lid=at("neigh", HB.neigh_rows(), row))


def neigh_ref(mc, row):
    sc = neigh_scene(row)
    return cached(("neigh", row[0]), lambda: MR.triangulate_neighbours(
        sc["store"], sc["cur"], sc["cur"]["lids"], sc["neigh"], [f["lids"] for f in sc["neigh"]], sc["F21"], sc["matches"], sc["K"],
        sc["inv_sigma2"], sc["Rcw"], sc["tcw"], sc["next_lid"], triangulate=lib_dlt(mc)))


def neigh_same(got, want, what):
    """a NeighboursResult against the restatement's walk: every integer, and every double as raw bytes"""
    assert got.verdict.tolist() == want["verdict"], (what, "verdict", np.bincount(got.verdict, minlength=8), np.bincount(want["verdict"], minlength=8))
    assert got.neigh_skipped.tolist() == want["skipped"], (what, "skipped")
    assert got.inliers.tolist() == want["inliers"] and got.new_lid.tolist() == want["new_lid"], (what, "inliers, new_lid")
    assert got.lids_cur.tolist() == want["lids_cur"] and [l.tolist() for l in got.lids_neigh] == want["lids_neigh"], (what, "lids")
    assert (got.next_lid, got.n_triangulated) == (want["next_lid"], len(want["depth_vec"])), (what, "next_lid")
    for f, key in (("pt3d", "pt3d"), ("normal", "normal"), ("depth_vec", "depth_vec")):
        a, b = np.asarray(getattr(got, f), np.float64).reshape(-1), np.asarray(want[key], np.float64).reshape(-1)
        assert len(a) == len(b) and Nc.dcat(a) == Nc.dcat(b), (what, f)
    sel = np.array(want["verdict"]) == 0
    assert Nc.dcat(got.dist2[sel]) == Nc.dcat(want["depth_vec"]), (what, "dist2 of the landmarks")
    # (every match: the distance and the cosine of a match that the parallax window refuses are returned too)
    assert Nc.dcat(got.dist2) == Nc.dcat(want["dist2"]) and Nc.dcat(got.cos_parallax) == Nc.dcat(want["cos"]), (what, "dist2, cos")
    raw = np.concatenate([np.ravel(getattr(got, f)) for f in ("dist2", "cos_parallax", "pt3d", "normal", "depth_vec")])
    assert raw.tobytes() == b"".join(N.dbits(v) for v in raw), (what, "a NaN that is not the default quiet NaN")


def neigh_check(mc, lm, row, who):
    ref = neigh_ref(mc, row)
    sc = neigh_scene(row)
    Mc.fill_store(lm, sc["store"])
    got = Mc.run_scene(mc, lm, sc)
    neigh_same(got, ref, "%s: %s" % (row[0], who))
    return got, ref


def init_scene(row):
    return dict(row[1], next_lid=at("init", HB.init_rows(), row))


def init_ref(mc, row):
    sc = init_scene(row)
    return cached(("init", row[0]), lambda: IR.initialize(
        sc["prev"], sc["prev"]["lids"], sc["cur"], sc["cur"]["lids"], sc["R"], sc["t"], sc["body"], sc["matches"], sc["flags"], sc["K"],
        sc["inv_sigma2"], sc["next_lid"], sc["min_baseline"], triangulate=lib_dlt(mc)))


def init_check(mc, lm, row, who):
    ref = init_ref(mc, row)
    got = Ic.run_scene(mc, lm, init_scene(row))
    what = "%s: %s" % (row[0], who)
    same_hook(got, ref, what, n_rays=False)
    assert got.lids_prev.tolist() == ref["lids_prev"] and got.lids_cur.tolist() == ref["lids_cur"], (what, "lids")
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------------
# the host-only store == the restatement on every row
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", HB.ba_rows(), ids=names(HB.ba_rows()))
def test_bundle_adjust(mc, lm, row):
    ba_check(mc, lm, row, "host-only store")


@pytest.mark.parametrize("row", HB.retri_rows(), ids=names(HB.retri_rows()))
def test_retriangulate(mc, lm, row):
    got, ref = retri_check(mc, lm, row, "host-only store")
    if HB.failed(ref):
        retri_apply(mc, lm, row, "host-only store")


@pytest.mark.parametrize("row", HB.pose_rows(), ids=names(HB.pose_rows()))
def test_refine_pose(mc, lm, row):
    pose_check(mc, lm, row, "host-only store")


@pytest.mark.parametrize("row", HB.new_rows(), ids=names(HB.new_rows()))
def test_triangulate_new(mc, lm, row):
    new_check(mc, lm, row, "host-only store")


@pytest.mark.parametrize("row", HB.neigh_rows(), ids=names(HB.neigh_rows()))
def test_triangulate_neighbours(mc, lm, row):
    neigh_check(mc, lm, row, "host-only store")


@pytest.mark.parametrize("row", HB.init_rows(), ids=names(HB.init_rows()))
def test_initialize(mc, lm, row):
    init_check(mc, lm, row, "host-only store")


# ---------------------------------------------------------------------------------------------------------------------------
# what the tables are for, on the restatement alone
# ---------------------------------------------------------------------------------------------------------------------------
def flat_bytes(x):
    return np.array(BC.flat([x])).tobytes()


def has_nan(*values):
    return any(np.isnan(np.asarray(BC.flat([v]), np.float64)).any() for v in values)


def test_the_shapes():
    """the launch shapes the tables are cut to"""
    for name, sc, kw in HB.ba_rows():
        assert len(sc["pts"]) == HB.NLM and len(sc["poses"]) == 4 and sum(sc["fixed"]) in (0, 2), name
        per = np.bincount([o[2] for o in sc["obs"]], minlength=HB.NLM)
        assert per.max() <= (64 if "64" in name else 3 if "twice" not in name else 6), name
    for name, sc, kw in HB.retri_rows():
        assert len(sc["pts"]) == HB.NLM and len(sc["poses"]) == 4 and len(sc["cams"]) == 4, name
    base = HB.retri_rows()[0][1]
    per = np.bincount([o[2] for o in base["obs"]], minlength=HB.NLM)
    assert per.tolist() == HB.RETRI_VIEWS and set(per[:64].tolist()) == {2, 3, 15, 16, 17}        # mixed within the first wave
    assert all(len(r[3]) in (HB.NOBS, HB.NOBS + 14) and len(r[1]) == 4 for r in HB.pose_rows())
    assert all(64 <= len(r[1]["matches"]) <= 70 + 14 and r[1]["K"].shape[0] == HB.NCAMS for r in HB.new_rows())
    assert all(64 <= len(m) <= 70 + 14 for r in HB.neigh_rows() for m in r[1]["matches"])


def test_bundle_adjust_table():
    rows = HB.ba_rows()
    refs = {r[0]: ba_ref(r) for r in rows}
    assert refs["well posed"]["status"] == B.CONVERGED and refs["well posed, 100 iterations"]["status"] == B.CONVERGED
    assert set(r["status"] for r in refs.values()) == {B.NO_STEP, B.MAX_ITER, B.CONVERGED}
    # a NaN anywhere is a NaN cost: nothing is accepted and the state comes back as it went in; keypoints that are all inf are not
    # NaN residuals under Huber, the loop runs on them to the last iteration
    for name, sc, kw in rows:
        if has_nan(sc["poses"], sc["pts"], [o[3:5] for o in sc["obs"]]):
            ref = refs[name]
            assert ref["status"] == B.NO_STEP and ref["iterations"] == HB.BA_ITERATIONS and ref["cost_initial"] != ref["cost_initial"], name
            assert flat_bytes(ref["R"]) == flat_bytes([p[0] for p in sc["poses"]]) and flat_bytes(ref["pts"]) == flat_bytes(sc["pts"]), name
    assert refs["keypoints times 1e36, all inf"]["status"] == B.MAX_ITER
    # what the rows built for one outcome are about
    assert refs["no fixed keyframe"]["status"] == B.CONVERGED
    behind = refs["every landmark behind every camera"]
    assert behind["status"] == B.NO_STEP and behind["n_inliers"] == 0
    sc = HB.row_of(rows, "inactive landmarks between active ones")[1]
    mixed = refs["inactive landmarks between active ones"]
    assert mixed["status"] == B.CONVERGED
    moved = [flat_bytes(a) != flat_bytes(b) for a, b in zip(mixed["pts"], sc["pts"])]
    seen = set(o[2] for o in sc["obs"])
    assert not any(moved[j] for j in range(1, HB.NLM, 2) if j in seen) and sum(moved[0::2]) > 20      # the inactive ones stay, lane by lane
    sc = HB.row_of(rows, "one landmark in all 64 cameras")[1]
    assert sum(o[2] == 0 for o in sc["obs"]) == 64 and refs["one landmark in all 64 cameras"]["status"] == B.CONVERGED
    assert refs["well posed, 1 iteration"]["status"] == B.MAX_ITER


def test_retriangulate_table():
    rows = HB.retri_rows()
    refs = {r[0]: retri_ref(r) for r in rows}
    assert refs["well posed"]["counts"][R.VALID_UPDATED] == HB.NLM
    seen = set(v for r in refs.values() for v in r["verdict"])
    assert seen == set(range(8)), "a verdict that ends no landmark of the table"
    well = refs["well posed"]
    # a landmark none of whose observations has a NaN keypoint ends as in the well-posed row, on the bytes
    for name in ("NaN in keypoint column 0", "NaN in keypoint column 1", "landmarks whose errors are all NaN"):
        sc, ref = HB.row_of(rows, name)[1], refs[name]
        bad = set(o[2] for o in sc["obs"] if o[3] != o[3] or o[4] != o[4])
        clean = [j for j in range(HB.NLM) if j not in bad]
        assert clean and bad, name
        assert all(ref["verdict"][j] == R.VALID_UPDATED and flat_bytes(ref["pts"][j]) == flat_bytes(well["pts"][j]) for j in clean), name
        assert all(ref["verdict"][j] == R.DEGENERATE for j in bad), name
    ref = refs["the first failing observation in lane 15 and in observation 16"]
    sc = HB.row_of(rows, "the first failing observation in lane 15 and in observation 16")[1]
    for j, nv in ((0, 16), (1, 17)):
        order = [i for i in R.sort_obs(sc["obs"]) if sc["obs"][i][2] == j]
        assert len(order) == nv and sc["obs"][order[-1]][:2] == (3, 3) and all(sc["obs"][i][1] != 3 for i in order[:-1])
        assert ref["verdict"][j] == R.BEHIND
    # the rows that run in apply mode too
    assert sum(HB.failed(r) for r in refs.values()) > 20


def test_refine_pose_table():
    rows = HB.pose_rows()
    refs = {r[0]: pose_ref(r) for r in rows}
    assert refs["well posed"]["status"] == P.CONVERGED
    assert set(r["status"] for r in refs.values()) == {P.NO_STEP, P.MAX_ITER, P.CONVERGED}
    for name, cams, init, obs, kw in rows:
        if has_nan(init, [o[1:3] for o in obs], [o[4] for o in obs]):
            assert refs[name]["status"] == P.NO_STEP and flat_bytes(refs[name]["R"]) == flat_bytes(init[0]), name


def test_front_end_tables(mc):
    rows = HB.new_rows()
    refs = {r[0]: new_ref(mc, r) for r in rows}
    assert refs["well posed"]["n_by_verdict"][0] >= 20
    assert set(v for r in refs.values() for v in r["verdict"]) == {0, 3, 4, 5, 6, 8}
    for name in ("NaN in keypoint column 0", "NaN in R of the current frame", "a third of the keypoints inf"):
        assert refs[name]["n_by_verdict"][0] > 0 and refs[name]["n_by_verdict"][8] > 0, name
    rows = HB.neigh_rows()
    refs = {r[0]: neigh_ref(mc, r) for r in rows}
    assert refs["well posed"]["verdict"].count(0) >= 40 and refs["well posed"]["skipped"] == [0, 0]
    assert set(v for r in refs.values() for v in r["verdict"]) == set(range(8))
    assert refs["the second frame did not move"]["skipped"] == [1, 1] and refs["pure rotation"]["skipped"] == [1, 0]
    assert refs["every match behind"]["verdict"].count(3) == len(refs["every match behind"]["verdict"])
    for name in ("NaN in keypoint column 0", "NaN in R of the current frame", "a third of the keypoints inf"):
        assert refs[name]["verdict"].count(0) > 0, name
    # depths that are all NaN: the median is NaN, and the baseline gate does not skip on a NaN
    assert refs["a neighbour whose depths are all NaN"]["skipped"] == [0, 0]
    # a depth list of one value, which is the median: the gate's decision is that depth's
    one = HB.row_of(rows, "a neighbour with one depth")[1]
    assert int((one["neigh"][0]["lids"] != -1).sum()) == 1
    assert refs["a neighbour with one depth"]["skipped"] == [0, 0] and refs["a neighbour with one depth"]["verdict"].count(0) > 20
    assert refs["a neighbour with one depth, far"]["skipped"] == [1, 0]
    assert refs["a neighbour whose depths are one value and a NaN"]["skipped"] == [0, 0]
    rows = HB.init_rows()
    refs = {r[0]: init_ref(mc, r) for r in rows}
    assert refs["well posed"]["status"] == IR.DONE
    assert set(r["status"] for r in refs.values()) == {IR.DONE, IR.BASELINE, IR.PARALLAX, IR.FEW}
    # the smallest count at which the scene ends DONE
    sc = dict(Ic.cut(Ic.scene(HB.NCAMS, n=300, seed=3), HB.NINIT - 1))
    with np.errstate(all="ignore"):
        fewer = IR.initialize(sc["prev"], sc["prev"]["lids"], sc["cur"], sc["cur"]["lids"], sc["R"], sc["t"], sc["body"], sc["matches"], sc["flags"],
                              sc["K"], sc["inv_sigma2"], sc["next_lid"], sc["min_baseline"], triangulate=lib_dlt(mc))
    assert fewer["status"] == IR.FEW and fewer["n_triangulated"] == 50 and refs["well posed"]["n_triangulated"] == 51
    # the median over parallaxes that are NaN: a NaN, which is not below the limit
    for name in ("NaN in keypoint column 0", "NaN in R of the previous frame"):
        assert refs[name]["parallax"] != refs[name]["parallax"] and refs[name]["status"] == IR.PARALLAX and refs[name]["n_triangulated"] > 0, name
    assert refs["NaN in body of the call"]["status"] == IR.DONE and refs["inf in t of the call"]["status"] == IR.DONE


def test_the_dlt_against_the_svd_where_both_are_well_posed(mc):
    """triangulate_neighbours' and initialize's restatements take their point from the library's DLT on these tables, so on the
    CPU the DLT is compared with itself.  Where the design is well conditioned -- the well-posed rows and the rows that place
    points on one point and on one plane -- the restatement's own route, numpy's SVD, gives the same verdicts and, for the
    landmarks, the same point to 1e-9 of its largest coordinate (the bound of test_mapping_cpu.py and test_init_cpu.py).  On the
    hostile designs null_vector has no independent check: it is held device against host alone"""
    for name in ("well posed", "every match the same point", "points on one plane"):
        row = HB.row_of(HB.neigh_rows(), name)
        sc = neigh_scene(row)
        with np.errstate(all="ignore"):
            svd = MR.triangulate_neighbours(sc["store"], sc["cur"], sc["cur"]["lids"], sc["neigh"], [f["lids"] for f in sc["neigh"]], sc["F21"],
                                            sc["matches"], sc["K"], sc["inv_sigma2"], sc["Rcw"], sc["tcw"], sc["next_lid"])
        dlt = neigh_ref(mc, row)
        near = np.array(svd["near"])
        assert near.sum() <= len(near) // 50 and (np.array(svd["verdict"])[~near] == np.array(dlt["verdict"])[~near]).all(), name
        both = [i for i, (a, b) in enumerate(zip(svd["verdict"], dlt["verdict"])) if a == b == 0]
        assert len(both) > 20, name
        for i in both:
            a, b = np.array(svd["pt3d"][i]), np.array(dlt["pt3d"][i])
            assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max(), (name, i)
        row = HB.row_of(HB.init_rows(), name)
        sc = init_scene(row)
        with np.errstate(all="ignore"):
            svd = Ic.ref_scene(sc)
        dlt = init_ref(mc, row)
        assert not any(svd["near"]) and svd["status"] == dlt["status"] == IR.DONE and svd["verdict"] == dlt["verdict"], name
        a, b = np.array(svd["pt3d"]), np.array(dlt["pt3d"])
        assert (np.abs(a - b).max(axis=1) <= 1e-9 * np.maximum(1.0, np.abs(a).max(axis=1))).all(), name


def test_the_scale_rows_are_at_the_edge(mc):
    """where a call's answer changes with the scale of points and translations, on the restatement: the rows lie either side"""
    ba = {r[0]: ba_ref(r)["status"] for r in HB.ba_rows()}
    pose = {r[0]: pose_ref(r)["status"] for r in HB.pose_rows()}
    for refs, good in ((ba, B.CONVERGED), (pose, P.CONVERGED)):
        assert refs["points and translations times 1e-155"] == B.NO_STEP and refs["points and translations times 1e-150"] == good
        assert refs["points and translations times 1e+155"] == good
    assert ba["points and translations times 1e+160"] == B.NO_STEP
    # (refine_pose has no point's square in its sums: at 1e160 it still converges, there is no upper edge below the largest double's root)
    assert pose["points and translations times 1e+160"] == P.CONVERGED
    p = HB.row_of(HB.ba_rows(), "points and translations times 1e-155")[1]["pts"][0]
    assert 0.0 < p[0] * p[0] < 2.3e-308
    p = HB.row_of(HB.ba_rows(), "points and translations times 1e+160")[1]["pts"][0]
    assert p[0] * p[0] == float("inf")
    retri = {r[0]: retri_ref(r)["counts"] for r in HB.retri_rows()}
    got = [retri["points and translations times %g" % k] for k in HB.SCALES]
    assert got[0][R.VALID_UPDATED] == 0 and 0 < got[1][R.VALID_UPDATED] < got[2][R.VALID_UPDATED]      # 1e-160, 1e-155, 1e-150
    assert got[3][R.DEGENERATE] == 0 and got[4][R.DEGENERATE] == HB.NLM                                 # 1e150, 1e155
    new = {r[0]: new_ref(mc, r)["n_by_verdict"] for r in HB.new_rows()}
    neigh = {r[0]: np.bincount(neigh_ref(mc, r)["verdict"], minlength=8).tolist() for r in HB.neigh_rows()}
    init = {r[0]: (lambda ref: (ref["status"], ref.get("verdict")))(init_ref(mc, r)) for r in HB.init_rows()}
    for lo, hi in HB.EDGES:
        assert new["translations times %g" % lo] != new["translations times %g" % hi], (lo, hi)
        assert neigh["points and translations times %g" % lo] != neigh["points and translations times %g" % hi], (lo, hi)
        assert init["translations times %g, min_baseline too" % lo] != init["translations times %g, min_baseline too" % hi], (lo, hi)
    assert new["translations times 1e-27"][0] >= 20 and new["translations times 1e+08"][0] >= 20 and new["translations times 1e+09"][0] == 0
    assert init["translations times 1e-27, min_baseline too"][0] == IR.DONE and init["translations times 1e-28, min_baseline too"][0] == IR.FEW


# ---------------------------------------------------------------------------------------------------------------------------
# the branch outcomes of the seven shared headers
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_headers_branch_outcomes():
    """docs/design/09q_hostile_backend.md's lists against scripts/header_coverage.py's reading of the back end's serial programs;
    needs g++ and gcov, as the sanitizer tests of the calls need g++: fails without them"""
    H = header_coverage()
    lists = doc_lists(os.path.join(ROOT, "docs", "design", "09q_hostile_backend.md"))
    hold_the_lists(H, lists, H.BACKEND_HEADERS, H.coverage("hostile", "backend"), H.coverage("existing", "backend"))
    committed = open(os.path.join(ROOT, "profiles", "header_coverage.txt")).read()
    assert all(h + ": taken by neither" in committed for h in H.BACKEND_HEADERS)
