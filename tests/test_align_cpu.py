"""The rig pose between two frames from 3D-3D pairs on the host-only store (device -1): mcorb_lmap_align_pose against the numpy
restatement (align_ref.py) and against answers written out by hand.  Bit for bit, floats as raw bytes, but for the comparisons of
the solver, which state their tolerances.  No GPU.

On the commit before this call existed every test of this file fails (`python -m pytest tests/test_align_cpu.py`): LocalMap has
no align_pose."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
import kfdb_cases as K
import pose_ref as P
import track_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb.LocalMap, "align_pose")
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture()
def lm(mc, voc):
    return mc.LocalMap(voc, device=-1, max_landmarks=4096, max_candidates=1024)


SEED = 0     # what AC.first_seed finds, recorded
MODES = [dict(mode=AR.SAC, refit=True), dict(mode=AR.SAC, refit=False), dict(mode=AR.ALL)]


@pytest.fixture(scope="module")
def seeded(mc):
    """the seeded scene and its three restatements (refit, no refit, mode 0) at the reference's values, computed once"""
    truth, p1, p2, moved = AC.scene(seed=SEED)
    return truth, p1, p2, moved, [AC.ref(mc, p1, p2, **kw) for kw in MODES]


def check(mc, lm, p1, p2, what, **kw):
    want = AC.ref(mc, p1, p2, **kw)
    AC.same(AC.run(mc, lm, p1, p2, **kw), want, what)
    if kw.get("mode", AR.SAC) == AR.SAC and want["status"] != AR.NO_OBS:
        AC.same_counts(lm, want, what)
    return want


# ---------------------------------------------------------------------------------------------------------------------------
# the solver (the comparisons of this file with a tolerance)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts,count", [(3, 4000), (4, 400), (64, 400), (1000, 400)])
def test_solver_recovers_the_generating_pose(mc, npts, count):
    """seeded noise-free fits: points with x in +-4, y in +-3, depth 2 - 10, rotation Cayley of N(0, 0.05) per axis, translation
    N(0, 0.3 m).  A case is included iff the second singular value of the cross-covariance is at least 1e-3 of the first; at most
    2 % may be left out.  On every included case numpy's Kabsch recovers the pose to 1e-10 and mcorb_align_solve to 1e-9 (max
    |dR_ij|, |dt| / max(1, |t|)).  Measured with six Jacobi sweeps: left out 12 of 4 000 triangles and none of the larger fits;
    worst error of mcorb_align_solve 1.7e-13 (3 points), 4.8e-14 (4), 3.1e-15 (64), 3.1e-15 (1 000); Kabsch 2.4e-13, 7.0e-14,
    4.2e-14, 4.1e-14; the smallest eigenvalue gap (l1 - l2) / (l1 - l4) of an included triangle 1.08e-3"""
    cases = AC.solver_cases(npts, count, 100 + npts)
    assert len(cases) == count
    left, worst, worst_np, gap_min = 0, 0.0, 0.0, 1.0
    for truth, p1, p2 in cases:
        if not AR.well_shaped(p1, p2):
            left += 1
            continue
        alone = AR.pose_distance(AR.kabsch(p1, p2), truth)
        got, gap = mc.align_solve(p1, p2, with_gap=True)
        assert got is not None, (p1, p2)
        d = AR.pose_distance(got, truth)
        worst, worst_np, gap_min = max(worst, d), max(worst_np, alone), min(gap_min, gap)
        assert alone <= 1e-10 and d <= 1e-9, (alone, d, p1, p2)
    print("%d points: left out %d of %d, worst error %.3g (Kabsch %.3g), smallest gap %.3g" % (npts, left, count, worst, worst_np, gap_min))
    assert left <= 0.02 * count


@pytest.mark.parametrize("npts", [3, 4, 64, 1000])
def test_solver_agrees_with_kabsch_on_noisy_fits(mc, npts):
    """400 seeded fits with N(0, 0.02 m) per axis on frame 1: the closed form and the SVD solve the same least-squares problem and
    agree to 1e-12 on every included case.  Measured: 5.5e-14, 8.1e-14, 2.7e-14, 3.8e-14"""
    worst = 0.0
    for truth, p1, p2 in AC.solver_cases(npts, 400, 200 + npts, noise=0.02):
        if not AR.well_shaped(p1, p2):
            continue
        got = mc.align_solve(p1, p2)
        assert got is not None
        worst = max(worst, AR.pose_distance(got, AR.kabsch(p1, p2)))
    print("%d points with noise: the library against Kabsch %.3g" % (npts, worst))
    assert worst <= 1e-12


def test_member_set(mc):
    """mcorb_align_solve over a member set of 600 pairs does not read the other pairs -- NaNs there change no byte -- and agrees
    with the fit over the members gathered, whose pairs fall into other lanes of the sum (the lane of pair i is i mod 256), to
    1e-13"""
    truth, p1, p2 = AC.solver_cases(600, 1, 7, noise=0.02)[0]
    member = (np.arange(600) % 3 != 1)
    a = mc.align_solve(p1, p2, member)
    junk1 = p1.copy()
    junk1[~member] = np.nan
    b = mc.align_solve(junk1, p2, member)
    assert a is not None and b is not None and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    gathered = mc.align_solve(p1[member], p2[member])
    assert AR.pose_distance(a, gathered) <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------------
# degenerate and edge cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", MODES, ids=["refit", "winner", "all"])
def test_degenerate_sets_have_no_model(mc, lm, kw):
    """a collinear triple in exact doubles and rounded to float, three coincident points, n = 1 and n = 2: NO_MODEL, the identity,
    every flag 0; n = 0: NO_OBS.  The eigenvalue gap (l1 - l2) / (l1 - l4) of the collinear triple is 0 in doubles and 1.7e-16
    rounded to float, against the limit of 1e-12 and the 1.08e-3 of the narrowest included triangle"""
    for name, (p1, p2) in (("collinear", AC.collinear()), ("collinear as float", AC.collinear(True)), ("coincident", AC.coincident())):
        pose, gap = mc.align_solve(p1, p2, with_gap=True)
        print("%s: gap %.3g" % (name, gap))
        assert pose is None and not gap > 1e-12
        want = check(mc, lm, p1, p2, name, max_iterations=20, **kw)
        assert want["status"] == AR.NO_MODEL and want["n_models"] == 0
        got = AC.run(mc, lm, p1, p2, max_iterations=20, **kw)
        assert P.same_bits(got.R.tolist(), AR.IDENT[0]) and got.t.tolist() == [0.0] * 3 and not got.inliers.any() and got.mean_error == 0.0
    truth, p1, p2, moved = AC.scene(seed=SEED)
    for n in (1, 2):
        want = check(mc, lm, p1[:n], p2[:n], "n = %d" % n, max_iterations=5, **kw)
        assert want["status"] == AR.NO_MODEL and len(want["inliers"]) == n
        assert kw["mode"] == AR.ALL or want["samples"][2] == [-1] * 3
    want = check(mc, lm, p1[:0], p2[:0], "n = 0", **kw)
    assert want["status"] == AR.NO_OBS
    got = AC.run(mc, lm, p1[:0], p2[:0], **kw)
    assert got.status == AR.NO_OBS and got.n_matches == 0 and len(got.inliers) == 0 and P.same_bits(got.R.tolist(), AR.IDENT[0])


def test_half_turn(mc, lm):
    """a rotation by 180 degrees, where the quaternion's scalar part is 0: recovered to 1e-12 by the fit and by a sample"""
    truth, p1, p2 = AC.half_turn()
    want = check(mc, lm, p1, p2, "half turn, all", mode=AR.ALL)
    assert want["status"] == AR.OK and AR.pose_distance((want["R"], want["t"]), truth) <= 1e-12 and want["n_inliers"] == 40
    want = check(mc, lm, p1, p2, "half turn, sac", max_iterations=10, refit=False)
    assert want["status"] == AR.OK and AR.pose_distance((want["R"], want["t"]), truth) <= 1e-11 and want["sac_n_inliers"] == 40


def test_three_pairs_tie(mc, lm):
    """n = 3 in mode 1: every hypothesis draws the same set in its own order, all counts tie at 3, hypothesis 0 wins"""
    truth, p1, p2, moved = AC.scene(n=3, moved=0, noise=0.0)
    want = check(mc, lm, p1, p2, "n = 3", max_iterations=40)
    assert all(sorted(s) == [0, 1, 2] for s in want["samples"]) and len(set(tuple(s) for s in want["samples"])) > 1
    assert want["n_models"] == 40 and all(c == 3 for c in want["counts"]) and want["best"] == 0 and want["status"] == AR.OK
    assert want["used"] == AR.USED_FIT and AC.pose_error((want["R"], want["t"]), truth)[0] < 1e-12


def threshold_rows(mc):
    """-> (p1, p2, k, d): 40 noisy pairs and one hypothesis; k is the first pair outside its sample, d its distance at the model"""
    truth, p1, p2, moved = AC.scene(n=40, seed=11, moved=0)
    want = AC.ref(mc, p1, p2, max_iterations=1, refit=False)
    assert want["status"] == AR.OK
    k = next(i for i in range(40) if i not in want["sample"])
    d = AR.dist((want["R"], want["t"]), p1[k].tolist(), p2[k].tolist())
    assert 1e-6 < d < 1.0
    return p1, p2, k, d, (want["R"], want["t"])


def nan_rows():
    """the rows of threshold_rows with pair 7's frame-1 point a NaN"""
    truth, p1, p2, moved = AC.scene(n=40, seed=11, moved=0)
    p1[7, 0] = float("nan")
    return p1, p2


def test_thresholds_are_strict_and_nan_is_no_inlier(mc, lm):
    """a limit equal to a pair's distance leaves the pair out, the next double above takes it in: for `threshold`, seen in the
    winner's count, and for `inlier_dist`, seen in the flag.  The scalar and the vector form of the restatement and the
    mcorb_align_eval hook agree on the bits.  A NaN point is no inlier at any limit, a hypothesis that draws it has no model, and
    a mode-0 fit that contains it gives NO_MODEL"""
    p1, p2, k, d, model = threshold_rows(mc)
    many, hook = AR.dist_many(model, p1, p2), mc.align_eval(model[0], model[1], p1, p2)
    for i in range(40):
        assert AR.bits(float(many[i])) == AR.bits(AR.dist(model, p1[i].tolist(), p2[i].tolist())) == AR.bits(float(hook[i])), i
    at = check(mc, lm, p1, p2, "threshold = the distance", threshold=d, inlier_dist=10.0, max_iterations=1, refit=False)
    above = check(mc, lm, p1, p2, "threshold = the next double", threshold=AR.next_up(d), inlier_dist=10.0, max_iterations=1, refit=False)
    assert above["sac_n_inliers"] == at["sac_n_inliers"] + 1 and above["counts"][0] == at["counts"][0] + 1
    at = check(mc, lm, p1, p2, "inlier_dist = the distance", threshold=10.0, inlier_dist=d, max_iterations=1, refit=False)
    above = check(mc, lm, p1, p2, "inlier_dist = the next double", threshold=10.0, inlier_dist=AR.next_up(d), max_iterations=1, refit=False)
    assert not at["inliers"][k] and above["inliers"][k] and above["n_inliers"] == at["n_inliers"] + 1
    # the refit reads its members at `threshold`: with pair k out and in the two fits differ
    fit_at = check(mc, lm, p1, p2, "refit, threshold = the distance", threshold=d, max_iterations=1)
    fit_above = check(mc, lm, p1, p2, "refit, the next double", threshold=AR.next_up(d), max_iterations=1)
    assert fit_at["used"] == fit_above["used"] == AR.USED_FIT and not P.same_bits(fit_at["R"], fit_above["R"])
    p1, p2 = nan_rows()
    for refit in (False, True):
        wide = check(mc, lm, p1, p2, "a NaN row", threshold=1e9, inlier_dist=1e9, max_iterations=60, refit=refit)
        assert wide["status"] == AR.OK and not wide["inliers"][7] and wide["n_inliers"] == 39 and wide["sac_n_inliers"] == 39
        assert wide["mean_error"] != wide["mean_error"]
        drew = [h for h, s in enumerate(wide["samples"]) if 7 in s]
        assert len(drew) >= 3 and all(wide["models"][h] is None for h in drew) and wide["n_models"] == 60 - len(drew)
    assert check(mc, lm, p1, p2, "a NaN row, all", mode=AR.ALL)["status"] == AR.NO_MODEL


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded scene
# ---------------------------------------------------------------------------------------------------------------------------
# the pose errors of the restatement against the truth (max |dR_ij|, |dt| in m), read from the restatement alone: with the refit,
# the winner alone, the all-correspondence fit.  The library's pass mark with the refit is ten times the reading
READ = {"refit": (5.61e-4, 5.85e-3), "winner": (1.80e-2, 1.78e-1), "all": (1.00e-2, 6.52e-2)}


def test_first_seed_is_recorded():
    assert AC.first_seed() == SEED


def test_seeded_scene(mc, lm, seeded):
    """200 pairs, 20 of them moved by 1 m, N(0, 0.02 m) per axis on the other 180; 100 hypotheses, thresholds 0.2 and 0.1 (the
    reference's values).  On the restatement alone, with the refit: the inliers are exactly the 180 unmoved pairs, and the pose
    error is READ["refit"].  Without it the answer is the winner bit for bit, and its error READ["winner"] -- thirty times the
    refit's: a three-point model carries its sample's noise -- is what the refit buys.  Mode 0 is pulled by the 20 moved pairs to
    READ["all"], which is why the SAC switch exists.  The library equals the restatement on the bits every time"""
    truth, p1, p2, moved, wants = seeded
    assert len(moved) == 200 and sum(moved) == 20
    d = AR.dist_many(truth, p1, p2)
    assert not any(d[i] < AC.THRESHOLD for i, v in enumerate(moved) if v)
    for kw, want, name in zip(MODES, wants, ("refit", "winner", "all")):
        assert want["status"] == AR.OK
        err = AC.pose_error((want["R"], want["t"]), truth)
        print("restatement, %s: %.3g in R, %.3g m, %d inliers, mean distance %.3g" % (name, err[0], err[1], want["n_inliers"], want["mean_error"]))
        assert err[0] <= READ[name][0] and err[1] <= READ[name][1]
        got = AC.run(mc, lm, p1, p2, **kw)
        AC.same(got, want, name)
        if kw["mode"] == AR.SAC:
            AC.same_counts(lm, want, name)
    refit, winner, fit_all = wants
    assert refit["inliers"] == [not v for v in moved] and refit["n_inliers"] == 180 and refit["used"] == AR.USED_FIT
    assert refit["sac_n_inliers"] == 180 and P.same_bits(refit["sac_R"], winner["R"]) and P.same_bits(refit["sac_t"], winner["t"])
    assert winner["used"] == AR.USED_SAC and P.same_bits(winner["R"], winner["sac_R"]) and P.same_bits(winner["t"], winner["sac_t"])
    assert winner["best"] == refit["best"] and winner["models"][winner["best"]] == (winner["R"], winner["t"])
    assert fit_all["used"] == AR.USED_FIT and fit_all["best"] == -1 and fit_all["counts"] == []
    got = AC.run(mc, lm, p1, p2, **MODES[0])
    err = AC.pose_error((got.R.tolist(), got.t.tolist()), truth)
    assert err[0] <= 10 * READ["refit"][0] and err[1] <= 10 * READ["refit"][1]


def test_landmarks_from_the_store(mc, lm, seeded):
    """lids1 naming slots that hold frame 1's points gives the bytes of the pts1 call, in every mode, and writes nothing"""
    truth, p1, p2, moved, wants = seeded
    lids = np.arange(300, 700, 2, dtype=np.int32)
    lm.set(lids, p1, np.zeros_like(p1))
    before = read_back(lm, lids)
    for kw, want in zip(MODES, wants):
        by_lid = AC.run(mc, lm, None, p2, lids1=lids, **kw)
        AC.same(by_lid, want, "lids1")
        AC.same_results(by_lid, AC.run(mc, lm, p1, p2, **kw), "lids1 against pts1")
    assert read_back(lm, lids) == before


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def read_back(lm, lids):
    return [(p.tobytes(), q.tobytes()) for p, q, _, _ in (lm.get(int(l)) for l in lids)]


def check_refusals(mc, lm):
    truth, p1, p2, moved = AC.scene(n=30, seed=2, moved=3)
    lids = np.arange(10, 40, dtype=np.int32)
    lm.set(lids, p1, np.zeros_like(p1))
    before = read_back(lm, lids)
    want = AC.ref(mc, p1, p2)

    def refused(code, pending=False, **kw):
        a = dict(pts2=p2, pts1=p1, mode="sac", threshold=AC.THRESHOLD, inlier_dist=AC.INLIER_DIST, max_iterations=100)
        a.update(kw)
        with pytest.raises(mc.McorbError) as e:
            lm.align_pose(**a)
        assert e.value.code == code, (kw.keys(), e.value)
        assert pending or read_back(lm, lids) == before

    refused(mc.E_ARG, lids1=lids)                    # both
    refused(mc.E_ARG, pts1=None)                     # neither
    for bad in (40, -1, 4096):                       # an unset slot, a negative id, one past the store
        named = lids.copy()
        named[7] = bad
        refused(mc.E_ARG, pts1=None, lids1=named)
    for v in (0.0, -1e-7, float("nan"), float("inf")):
        refused(mc.E_ARG, threshold=v)
        refused(mc.E_ARG, inlier_dist=v)
        refused(mc.E_ARG, mode="all", inlier_dist=v)
    refused(mc.E_ARG, max_iterations=0)
    refused(mc.E_ARG, max_iterations=mc.ALIGN_MAX_ITERATIONS + 1)
    refused(mc.E_ARG, mode=2)
    refused(mc.E_ARG, mode=-1)
    assert lm.align_pose(p2, pts1=p1, mode="all", max_iterations=0).status == AR.OK     # (mode 0 does not read max_iterations)
    # NULLs and bad counts, through the C entry
    res, par = mc._lib.AlignResultC(), mc._lib.AlignParams()
    par.threshold, par.inlier_dist, par.max_iterations, par.mode, par.refit = AC.THRESHOLD, AC.INLIER_DIST, 100, 1, 1
    good = [lm.h, 30, None, p1.ctypes.data, p2.ctypes.data, C.byref(par), C.byref(res), None]
    for at, v in ((0, None), (3, None), (4, None), (5, None), (6, None), (1, -1)):
        args = list(good)
        args[at] = v
        assert lm.L.mcorb_lmap_align_pose(*args) == mc.E_ARG, at
    assert lm.L.mcorb_lmap_align_pose(*good) == mc.OK     # (inlier may be NULL)
    assert read_back(lm, lids) == before
    # while a tracking call is pending
    v = T.to_view(mc, T.flat_view())
    lm.track_submit(v, [np.zeros((0, 2), np.float32)], [np.zeros((0, 32), np.uint8)], [])
    refused(mc.E_STATE, pending=True)
    lm.track_wait()
    assert read_back(lm, lids) == before
    # and it runs after all that
    AC.same(AC.run(mc, lm, p1, p2), want, "after the refusals")
    AC.same(AC.run(mc, lm, None, p2, lids1=lids), want, "after the refusals, lids1")
    assert read_back(lm, lids) == before


def test_refusals(mc, lm):
    check_refusals(mc, lm)


# ---------------------------------------------------------------------------------------------------------------------------
# the header's host path as a stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_under_asan_ubsan(mc, lm, seeded, tmp_path):
    """tests/cpp/test_align_sanitize.cpp (its own main, -fsanitize=address,undefined) runs align_run_serial on the seeded scene in
    both modes: no report, and every record -- the result, the flags, and the model, sample and count of each hypothesis --
    equals the library's result and the restatement"""
    truth, p1, p2, moved, wants = seeded
    exe = str(tmp_path / "test_align_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_align_sanitize.cpp"),
                           "-o", exe])
    n = len(p1)
    for kw, want in zip(MODES, wants):
        sac = kw["mode"] == AR.SAC
        H = 100 if sac else 0
        blob = struct.pack("<4i2dQ", n, H, kw["mode"], int(kw.get("refit", False)), AC.THRESHOLD, AC.INLIER_DIST, 0)
        (tmp_path / "in.bin").write_bytes(blob + p1.tobytes() + p2.tobytes())
        out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "bad=0" in out.stdout and not out.stderr, out.stdout + out.stderr
        raw = (tmp_path / "out.bin").read_bytes()
        assert len(raw) == 240 + n + 4 * H + 128 * H
        got = AC.run(mc, lm, p1, p2, **kw)
        assert struct.pack("<9d", *got.R.reshape(9)) == raw[:72] and struct.pack("<3d", *got.t) == raw[72:96]
        assert struct.pack("<9d", *got.sac_R.reshape(9)) == raw[96:168] and struct.pack("<3d", *got.sac_t) == raw[168:192]
        assert struct.pack("<d", got.mean_error) == raw[192:200] == struct.pack("<d", want["mean_error"])
        status, used, n_in, sac_in, best, n_models, *sample = struct.unpack("<9i", raw[200:236])
        assert (status, used, n_in, sac_in, best, n_models, tuple(sample)) == (got.status, got.used, got.n_inliers, got.sac_n_inliers,
                                                                              got.best_hypothesis, got.n_models, got.sample)
        assert [bool(v) for v in raw[240:240 + n]] == got.inliers.tolist() == want["inliers"]
        if not sac:
            continue
        counts = struct.unpack("<%di" % H, raw[240 + n:240 + n + 4 * H])
        lib_count, lib_valid = lm.last_align_counts()
        for h in range(H):
            rec = raw[240 + n + 4 * H + 128 * h:240 + n + 4 * H + 128 * (h + 1)]
            valid, *smp = struct.unpack("<4i", rec[96:112])
            assert smp == want["samples"][h] and bool(valid) == (want["models"][h] is not None) == bool(lib_valid[h]), h
            assert counts[h] == lib_count[h] == (want["counts"][h] or 0), h
            if valid:
                m = struct.unpack("<12d", rec[:96])
                assert P.same_bits([list(m[0:3]), list(m[3:6]), list(m[6:9])], want["models"][h][0]) and P.same_bits(list(m[9:12]), want["models"][h][1]), h
