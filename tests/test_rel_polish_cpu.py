"""The polish of the relative pose's RANSAC winner on the host-only store (device -1): mcorb_lmap_relative_pose_polished and the
mcorb_rel_polish_run hook against the plain-Python restatement (rel_polish_ref.py), bit for bit, floats as raw bytes; the
acceptance rule on a problem built for it; the conditions on the eight seeded scenes; the refusals.  No GPU.

On the commit before the polish existed every test of this file fails: LocalMap has no relative_pose_polished."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import kfdb_cases as K
import pose_cases as PC
import pose_ref as P
import rel_cases as RC
import rel_polish_cases as RPC
import rel_polish_ref as RP
import rel_ref as RR
import track_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(8)


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert hasattr(mcorb.LocalMap, "relative_pose_polished") and hasattr(mcorb, "rel_polish")
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture()
def lm(mc, voc):
    return mc.LocalMap(voc, device=-1, max_landmarks=4096, max_candidates=1024)


@pytest.fixture(scope="module")
def scenes(mc):
    """RC.scene(8, 200, seed, noise 0.1 px) for seeds 0 .. 7 and their restatements at 100 hypotheses, two rounds, computed once"""
    out = {}
    for seed in SEEDS:
        cams, truth, matches, moved = RC.scene(8, 200, seed, 0.1, 0.1)
        out[seed] = (cams, truth, matches) + RPC.reference(mc, cams, matches)
    return out


def test_the_round_is_pose_refs(mc):
    """rel_polish_ref.lm_round, given pose_ref's sums, is pose_ref.lm_round: pose, iterations, status and both costs"""
    cams, _, init, obs, _ = PC.scene(2, 40)
    alive = [True] * len(obs)
    want = P.lm_round(cams, init, obs, alive, 25)[:5]
    got = RP.lm_round(lambda p: P.sums(cams, p, obs, alive), init, 25)
    assert got[1:3] == want[1:3] and want[2] != P.NO_STEP
    assert P.same_bits(got[0][0], want[0][0]) and P.same_bits(got[0][1], want[0][1]) and P.same_bits(list(got[3:]), list(want[3:]))


def test_the_residuals_length_is_the_score(mc):
    """|r|^2 = 2 score / threshold (to rounding), so a member that is an inlier adds less than 2 to the cost"""
    cams, _, matches, _ = RC.scene(8, 50, 1, 0.1, 0.1)
    scale = RP.scale_of(RC.THRESHOLD)
    for m in matches:
        rays = RR.rays_of(cams, m)
        r = RP.residual(RPC.NEAR, rays, scale)
        want = 2.0 * RR.score_rays(RPC.NEAR, rays) / RC.THRESHOLD
        assert abs(sum(v * v for v in r) - want) <= 1e-9 * max(1.0, want)


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded scenes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_scene_bits(mc, lm, scenes, seed):
    cams, truth, matches, ref, rp = scenes[seed]
    got, pol = RPC.run(mc, lm, cams, matches)
    RPC.same(got, pol, ref, rp, "seed %d" % seed)
    RC.same_counts(lm, ref, "seed %d" % seed)


@pytest.mark.parametrize("rounds, its", [(1, 1), (1, 10), (2, 1), (1, 100), (2, 100)])
def test_rounds_and_iterations_bits(mc, lm, scenes, rounds, its):
    cams, truth, matches, _, _ = scenes[2]
    ref, rp = RPC.reference(mc, cams, matches, rounds=rounds, polish_iterations=its)
    got, pol = RPC.run(mc, lm, cams, matches, rounds=rounds, polish_iterations=its)
    RPC.same(got, pol, ref, rp, "rounds %d, %d solves" % (rounds, its))
    assert pol.rounds_run == rounds and all(q["iterations"] <= its for q in pol.rounds)


def test_conditions_on_the_seeded_scenes(mc, lm, scenes):
    """0.1 px, 100 hypotheses, two rounds: each round's final cost is at most its initial cost, the returned count is at least
    the winner's, and the distance to the true pose (rel_ref.pose_distance) is strictly smaller than the unpolished call's on
    every seed.  Measured on the host-only store, seeds 0 .. 7: the distance falls by factors 44, 16, 26, 5.7, 112, 14, 20 and
    10 (9.5e-3 -> 2.2e-4, 9.0e-3 -> 5.5e-4, 1.0e-2 -> 3.9e-4, 5.3e-3 -> 9.2e-4, 2.8e-2 -> 2.5e-4, 8.1e-3 -> 5.7e-4, 5.5e-3 ->
    2.7e-4, 5.9e-3 -> 5.6e-4); the count rises on seeds 2 (177 -> 178) and 5 (183 -> 185) and stays elsewhere"""
    for seed in SEEDS:
        cams, truth, matches, ref, rp = scenes[seed]
        plain = RC.run(mc, lm, cams, matches)
        got, pol = RPC.run(mc, lm, cams, matches)
        assert pol.rounds_run == 2
        for q in pol.rounds:
            assert q["cost_final"] <= q["cost_initial"], (seed, q)
        assert got.n_inliers >= plain.n_inliers == pol.n_inliers, seed
        assert np.array_equal(pol.R, plain.R) and np.array_equal(pol.t, plain.t), seed
        assert got.best_hypothesis == plain.best_hypothesis and got.sample == plain.sample and got.n_models == plain.n_models
        d0 = RR.pose_distance((plain.R.tolist(), plain.t.tolist()), truth)
        d1 = RR.pose_distance((got.R.tolist(), got.t.tolist()), truth)
        print("seed %d: %.3g -> %.3g (factor %.1f), count %d -> %d" % (seed, d0, d1, d0 / d1, plain.n_inliers, got.n_inliers))
        assert d1 < d0, (seed, d0, d1)


def test_relative_pose_is_what_it_was(mc, lm, scenes):
    """relative_pose before, between and after polished calls on one store: the same result, the restatement's"""
    cams, truth, matches, ref, rp = scenes[0]
    RC.same(RC.run(mc, lm, cams, matches), ref, "before")
    RPC.same(*RPC.run(mc, lm, cams, matches), ref, rp, "polished")
    RC.same(RC.run(mc, lm, cams, matches), ref, "after")
    RC.same_counts(lm, ref, "after")


# ---------------------------------------------------------------------------------------------------------------------------
# pass-through
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 16])
def test_without_a_winner_nothing_is_polished(mc, lm, n):
    cams, _, matches, _ = RC.scene(8, 40, 1, 0.1, 0.1)
    ref, rp = RPC.reference(mc, cams, matches[:n])
    assert ref["status"] == (RR.NO_OBS if n == 0 else RR.NO_MODEL) and not rp["rounds"]
    got, pol = RPC.run(mc, lm, cams, matches[:n])
    RPC.same(got, pol, ref, rp, "n = %d" % n)
    assert pol.rounds_run == 0 and not got.inliers.any() and np.array_equal(got.R, np.eye(3))


# ---------------------------------------------------------------------------------------------------------------------------
# the hook: noise-free problems, rows written out by hand, the acceptance rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_noise_free_scene(mc, seed):
    """60 noise-free matches (frame 2's keypoints in double) from the generating pose: the polish takes no step or leaves the
    pose within the 1e-6 the 17-point solver is held to on such input, and keeps every match"""
    cams, matches = RPC.exact_scene(8, 60, seed)
    R, t, inl, pol, rp = RPC.hook(mc, cams, matches, RPC.TRUTH, [True] * 60, what="noise-free %d" % seed)
    assert inl.all() and pol.n_inliers == 60
    for q in pol.rounds:
        assert q["status"] == P.NO_STEP or RR.pose_distance((R.tolist(), t.tolist()), RPC.TRUTH) <= 1e-6, q
        assert q["cost_initial"] < 1e-6 and q["accepted"]


def test_noise_free_scene_from_nearby(mc):
    """the same matches from a pose 2e-3 rad and 5 mm away: the polish returns to the generating pose within 1e-6"""
    cams, matches = RPC.exact_scene(8, 60, 0)
    R, t, inl, pol, rp = RPC.hook(mc, cams, matches, RPC.NEAR, [True] * 60, what="from nearby")
    assert RR.pose_distance(RPC.NEAR, RPC.TRUTH) > 1e-3
    assert RR.pose_distance((R.tolist(), t.tolist()), RPC.TRUTH) <= 1e-6 and inl.all()


HOSTILE = RPC.hostile_rows()


@pytest.mark.parametrize("row", range(len(HOSTILE)), ids=[h[0] for h in HOSTILE])
def test_rows_written_by_hand(mc, row):
    name, cams, matches, pose, member = HOSTILE[row]
    for rounds, its in ((2, 10), (1, 100)):
        R, t, inl, pol, rp = RPC.hook(mc, cams, matches, pose, member, rounds=rounds, polish_iterations=its, what=name)
        for q in pol.rounds:
            assert 1 <= q["iterations"] <= its
            if q["status"] == P.NO_STEP and q["accepted"]:
                assert q["n_inliers"] == pol.n_inliers
        if all(q["status"] == P.NO_STEP for q in pol.rounds):
            assert P.same_bits(R.tolist(), pose[0]) and P.same_bits(t.tolist(), pose[1]), name
    if name in ("0 members", "parallel rays") or name.endswith("among the members"):
        assert all(q["status"] == P.NO_STEP for q in pol.rounds), (name, pol.rounds)
    if name == "parallel rays" or name.endswith("among the members"):
        assert all(q["cost_initial"] != q["cost_initial"] for q in pol.rounds), (name, pol.rounds)


def test_a_round_that_loses_inliers_is_refused(mc):
    """the acceptance rule by construction (RPC.acceptance_problem): the round steps, its result has fewer inliers than the pose
    it began from, so it is reported as not accepted, the pose handed in comes back bit for bit with its own flags, and no
    second round runs"""
    cams, matches, start, member = RPC.acceptance_problem()
    R, t, inl, pol, rp = RPC.hook(mc, cams, matches, start, member, what="acceptance")
    assert pol.n_inliers == 150 and pol.rounds_run == 1
    q = pol.rounds[0]
    assert q["n_members"] == 12 and q["status"] != P.NO_STEP and q["cost_final"] < q["cost_initial"]
    assert q["n_inliers"] < 150 and not q["accepted"]
    assert P.same_bits(R.tolist(), start[0]) and P.same_bits(t.tolist(), start[1])
    assert inl.tolist() == [True] * 150 + [False] * 12


def test_hostile_keypoints_through_the_call(mc, lm):
    cams, rows = RPC.hostile_matches()
    ref, rp = RPC.reference(mc, cams, rows)
    RPC.same(*RPC.run(mc, lm, cams, rows), ref, rp, "hostile keypoints")
    cams, _, matches, _ = RC.scene(8, 60, 5, 0.1, 0.1)
    RPC.same(*RPC.run(mc, lm, cams, matches), *RPC.reference(mc, cams, matches), "the next call")


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def read_back(lm, lids):
    return [(p.tobytes(), q.tobytes()) for p, q, _, _ in (lm.get(int(l)) for l in lids)]


def check_refusals(mc, lm):
    cams, truth, matches, moved = RC.scene(4, 30, 2)
    lids = np.arange(10, 40, dtype=np.int32)
    pts = np.random.default_rng(1).normal(size=(30, 3))
    lm.set(lids, pts, np.zeros_like(pts))
    before = read_back(lm, lids)
    cam1, uv1, cam2, uv2 = RC.arrays(matches)
    cc = PC.to_cams(mc, cams)
    ref, rp = RPC.reference(mc, cams, matches)

    def refused(code, pending=False, **kw):
        a = dict(cams=cc, cam1=cam1, uv1=uv1, cam2=cam2, uv2=uv2, threshold=RC.THRESHOLD, max_iterations=100)
        a.update(kw)
        with pytest.raises(mc.McorbError) as e:
            lm.relative_pose_polished(**a)
        assert e.value.code == code, (kw.keys(), e.value)
        assert pending or read_back(lm, lids) == before

    for name, arr in (("cam1", cam1), ("cam2", cam2)):
        for v in (4, -1):
            bad = arr.copy()
            bad[7] = v
            refused(mc.E_ARG, **{name: bad})
    for thr in (0.0, -1e-7, float("nan"), float("inf")):
        refused(mc.E_ARG, threshold=thr)
    refused(mc.E_ARG, max_iterations=0)
    refused(mc.E_ARG, max_iterations=mc.REL_MAX_ITERATIONS + 1)
    for rounds in (0, -1, mc.REL_POLISH_ROUNDS + 1):
        refused(mc.E_ARG, rounds=rounds)
    for its in (0, -1, mc.REL_POLISH_MAX_ITERATIONS + 1):
        refused(mc.E_ARG, polish_iterations=its)
    # NULLs and bad counts, through the C entry
    res, par, pp, rec = mc._lib.RelResultC(), mc._lib.RelParams(), mc._lib.RelPolishParams(2, 10), mc._lib.RelPolishC()
    par.threshold, par.max_iterations = RC.THRESHOLD, 100
    good = [lm.h, 30, cam1.ctypes.data, uv1.ctypes.data, cam2.ctypes.data, uv2.ctypes.data, 4, C.addressof(cc.cams), C.byref(par), C.byref(pp),
            C.byref(res), None, C.byref(rec)]
    for at, v in ((0, None), (2, None), (3, None), (4, None), (5, None), (7, None), (8, None), (9, None), (10, None), (12, None), (1, -1),
                  (6, 0), (6, 17)):
        args = list(good)
        args[at] = v
        assert lm.L.mcorb_lmap_relative_pose_polished(*args) == mc.E_ARG, at
    assert lm.L.mcorb_lmap_relative_pose_polished(*good) == mc.OK     # (inlier may be NULL)
    assert read_back(lm, lids) == before
    # the hook's
    for kw in (dict(rounds=0), dict(rounds=3), dict(polish_iterations=0), dict(polish_iterations=101), dict(threshold=0.0),
               dict(threshold=float("nan"))):
        a = dict(threshold=RC.THRESHOLD)
        a.update(kw)
        with pytest.raises(mc.McorbError) as e:
            mc.rel_polish(cc, RPC.NEAR[0], RPC.NEAR[1], cam1, uv1, cam2, uv2, np.ones(30, np.uint8), **a)
        assert e.value.code == mc.E_ARG, kw
    # while a tracking call is pending
    v = T.to_view(mc, T.flat_view())
    lm.track_submit(v, [np.zeros((0, 2), np.float32)], [np.zeros((0, 32), np.uint8)], [])
    refused(mc.E_STATE, pending=True)
    lm.track_wait()
    assert read_back(lm, lids) == before
    # and it runs after all that
    RPC.same(*lm.relative_pose_polished(cc, cam1, uv1, cam2, uv2, RC.THRESHOLD, max_iterations=100), ref, rp, "after the refusals")
    assert read_back(lm, lids) == before


def test_refusals(mc, lm):
    check_refusals(mc, lm)


# ---------------------------------------------------------------------------------------------------------------------------
# the header's host path as a stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------
def blob_of(cams, matches, H, rounds, its):
    blob = struct.pack("<4idQ2i", len(cams), len(matches), H, rounds, RC.THRESHOLD, 0, its, 0)
    for c in cams:
        blob += struct.pack("<17d", *[v for row in c["R"] for v in row], *c["t"], c["fx"], c["fy"], c["s"], c["u0"], c["v0"])
    return blob + b"".join(struct.pack("<4f2i", m[1], m[2], m[4], m[5], m[0], m[3]) for m in matches)


def test_header_under_asan_ubsan(mc, lm, scenes, tmp_path):
    """tests/cpp/test_rel_polish_sanitize.cpp (its own main, -fsanitize=address,undefined) runs rel_run_serial and
    rel_polish_serial on the noisy scene and on the hostile keypoints: no report, and the accepted record, the polish record and
    the flags equal the library's on the bytes"""
    exe = str(tmp_path / "test_rel_polish_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_rel_polish_sanitize.cpp"), "-o", exe])
    hostile = RPC.hostile_matches()
    for name, cams, matches, rounds, its in (("noisy", scenes[2][0], scenes[2][2], 2, 10), ("hostile", hostile[0], hostile[1], 2, 100)):
        n, H = len(matches), 100
        (tmp_path / "in.bin").write_bytes(blob_of(cams, matches, H, rounds, its))
        out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "bad=0" in out.stdout and not out.stderr, out.stdout + out.stderr
        raw = (tmp_path / "out.bin").read_bytes()
        size = C.sizeof(mc._lib.RelPolishC)
        assert len(raw) == 192 + size + n
        got, pol = RPC.run(mc, lm, cams, matches, max_iterations=H, rounds=rounds, polish_iterations=its)
        assert struct.pack("<9d", *got.R.reshape(9)) == raw[:72] and struct.pack("<3d", *got.t) == raw[72:96], name
        status, n_in, best, n_models, *sample = struct.unpack("<21i", raw[96:180])
        assert (status, n_in, best, n_models, tuple(sample)) == (got.status, got.n_inliers, got.best_hypothesis, got.n_models, got.sample)
        rec = mc._lib.RelPolishC.from_buffer_copy(raw[192:192 + size])
        want = mc.RelPolish(rec)
        assert want.rounds_run == pol.rounds_run == rounds and want.n_inliers == pol.n_inliers, name
        assert want.R.tobytes() == pol.R.tobytes() and want.t.tobytes() == pol.t.tobytes(), name
        for q, r in zip(want.rounds, pol.rounds):
            assert struct.pack("<2d", q.pop("cost_initial"), q.pop("cost_final")) == struct.pack("<2d", r.pop("cost_initial"), r.pop("cost_final"))
            assert q == r, name
        assert [bool(v) for v in raw[192 + size:]] == got.inliers.tolist(), name
