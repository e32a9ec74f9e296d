"""Inputs and helpers of the polished relative pose tests (test_rel_polish_cpu.py, test_gpu_rel_polish.py): the comparison of a
LocalMap.relative_pose_polished result and of the mcorb_rel_polish_run hook against the restatement (rel_polish_ref.py), floats
as raw bytes with no tolerance, the rows written out by hand, and the problem that shows the acceptance rule.

A match is (cam1, u1, v1, cam2, u2, v2); a pose is (R rows, t) = b1_T_b2."""
import math

import numpy as np

import pose_cases as PC
import pose_ref as P
import rel_cases as RC
import rel_polish_ref as RP
import rel_ref as RR

INF, NAN = math.inf, math.nan


def run(mc, lm, cams, matches, threshold=RC.THRESHOLD, max_iterations=100, seed=0, rounds=2, polish_iterations=10):
    return lm.relative_pose_polished(PC.to_cams(mc, cams), *RC.arrays(matches), threshold, max_iterations=max_iterations, seed=seed,
                                     rounds=rounds, polish_iterations=polish_iterations)


def reference(mc, cams, matches, threshold=RC.THRESHOLD, max_iterations=100, seed=0, rounds=2, polish_iterations=10):
    return RP.polished(cams, matches, threshold, RC.solver_of(mc, cams), max_iterations, seed, rounds, polish_iterations)


def same_record(pol, rp, what=""):
    """a RelPolish against rel_polish_ref.polish's dict"""
    assert P.same_bits(pol.R.tolist(), rp["win_R"]) and P.same_bits(pol.t.tolist(), rp["win_t"]), (what, "the pose it began from")
    assert pol.n_inliers == rp["win_count"], (what, "the count it began from", pol.n_inliers, rp["win_count"])
    assert pol.rounds_run == len(rp["rounds"]) == len(pol.rounds), (what, "rounds run", pol.rounds_run, len(rp["rounds"]))
    for k, (q, r) in enumerate(zip(pol.rounds, rp["rounds"])):
        for key in ("n_members", "iterations", "status", "n_inliers", "accepted"):
            assert q[key] == r[key], (what, "round", k, key, q[key], r[key])
        for key in ("cost_initial", "cost_final"):
            assert P.same_bits(q[key], r[key]), (what, "round", k, key, q[key], r[key])


def same(got, pol, ref, rp, what=""):
    """(RelResult, RelPolish) of a polished call against rel_polish_ref.polished's two dicts"""
    accepted = dict(ref, R=rp["R"], t=rp["t"], n_inliers=rp["n_inliers"], inliers=rp["inliers"])
    RC.same(got, accepted, what)
    same_record(pol, rp, what)


def same_polish(a, b, what=""):
    """two RelPolish records of the library, doubles as raw bytes"""
    for k in ("R", "t"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)
    assert (a.n_inliers, a.rounds_run) == (b.n_inliers, b.rounds_run), what
    for q, r in zip(a.rounds, b.rounds):
        assert {k: (RR.bits(v) if isinstance(v, float) else v) for k, v in q.items()} == \
               {k: (RR.bits(v) if isinstance(v, float) else v) for k, v in r.items()}, what


def hook(mc, cams, matches, pose, member, threshold=RC.THRESHOLD, rounds=2, polish_iterations=10, what=""):
    """mcorb_rel_polish_run against the restatement on the bits -> (R, t, inliers, RelPolish, the restatement's dict)"""
    rays = [RR.rays_of(cams, m) for m in matches]
    flags = RP.flags_at(pose, rays, threshold)
    rp = RP.polish(rays, threshold, pose, sum(flags), flags, member, rounds, polish_iterations)
    R, t, inl, pol = mc.rel_polish(PC.to_cams(mc, cams), pose[0], pose[1], *RC.arrays64(matches), member, threshold, rounds=rounds,
                                   polish_iterations=polish_iterations)
    assert P.same_bits(R.tolist(), rp["R"]) and P.same_bits(t.tolist(), rp["t"]), (what, "pose", R, rp["R"])
    assert inl.tolist() == rp["inliers"], (what, "inliers")
    same_record(pol, rp, what)
    return R, t, inl, pol, rp


def exact_scene(ncams=8, n=60, seed=0, pose=RC.TRUTH):
    """n noise-free matches at `pose` (frame 1's keypoint a float, frame 2's a double: RC.exact_match)"""
    rng = np.random.default_rng(2000 + seed)
    cams = RC.outward_rig(ncams)
    rig = RC.rig_arrays(cams)
    return cams, [RC.exact_match(rng, cams, rig, pose[0], pose[1]) for _ in range(n)]


TRUTH = (PC.rows_of(RC.TRUTH[0]), [float(v) for v in RC.TRUTH[1]])
NEAR = (PC.rows_of(RC.TRUTH[0] @ PC.rot([1.0, 2.0, -1.0], 0.002)), [float(v) + d for v, d in zip(RC.TRUTH[1], (0.004, -0.003, 0.002))])
IDENT_SHIFT = (RR.IDENT[0], [0.1, 0.0, 0.0])


def hostile_rows():
    """-> [(name, cams, matches, pose handed in, member)]: what the residual, the differences and the solve must hold on.  The
    scene is the seeded one with N(0, 0.1 px); `bad` rows replace its first matches and are members"""
    cams, _, matches, _ = RC.scene(8, 40, 3, 0.1, 0.1)
    rays = [RR.rays_of(cams, m) for m in matches]
    inl = RP.flags_at(NEAR, rays, RC.THRESHOLD)
    good = [i for i, v in enumerate(inl) if v]
    out = []
    for k in (0, 1, 5, 6, 7):
        member = [i in good[:k] for i in range(len(matches))]
        out.append(("%d members" % k, cams, matches, NEAR, member))
    # a member whose rays are parallel at the pose handed in: the same keypoint of the same camera under R = I -> det = 0
    par = [(2, 600.0, 300.0, 2, 600.0, 300.0)] + matches[1:]
    out.append(("parallel rays", cams, par, IDENT_SHIFT, [True] * 12 + [False] * 28))
    for name, bad in (("+inf", (0, INF, 100.0, 1, 200.0, 100.0)), ("-inf", (0, 300.0, 100.0, 1, 200.0, -INF)),
                      ("NaN", (3, NAN, 100.0, 3, 200.0, NAN))):
        rows = [bad] + matches[1:]
        out.append((name + " among the members", cams, rows, NEAR, [True] + inl[1:]))
        out.append((name + " outside the members", cams, rows, NEAR, [False] + inl[1:]))
    stretched = ([[2.0 * v for v in row] for row in NEAR[0]], NEAR[1])
    sheared = ([[1.0, 0.3, 0.0], [0.0, 1.0, -0.2], [0.1, 0.0, 1.0]], [0.2, -0.1, 0.3])
    singular = ([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [0.0, 0.0, 0.0])
    for name, pose in (("twice a rotation", stretched), ("a sheared matrix", sheared), ("a singular matrix", singular)):
        out.append(("a pose that is not a rotation: " + name, cams, matches, pose, inl))
    return out


def hostile_matches():
    """the hostile keypoints as float matches, for a whole polished call: every kind among 120 matches of the seeded scene"""
    cams, _, matches, _ = RC.scene(8, 120, 4, 0.1, 0.1)
    rows = list(matches)
    big = float(np.finfo(np.float32).max)
    rows[5] = (0, INF, 100.0, 1, 200.0, 100.0)
    rows[17] = (0, 300.0, 100.0, 1, 200.0, -INF)
    rows[31] = (3, NAN, 100.0, 3, 200.0, NAN)
    rows[64] = (2, big, -big, 2, big, big)
    rows[90] = (2, 600.0, 300.0, 2, 600.0, 300.0)
    return cams, rows


def acceptance_problem():
    """-> (cams, matches, start, member): 150 noise-free matches at TRUTH and 12 at another pose, 0.05 rad and 0.2 m away, which
    are the members.  From TRUTH the round moves towards the members' pose and loses the 150"""
    other = (RC.TRUTH[0] @ PC.rot([0.0, 1.0, 0.5], 0.05), RC.TRUTH[1] + np.array([0.1, 0.15, -0.08]))
    cams, a = exact_scene(8, 150, 1, RC.TRUTH)
    _, b = exact_scene(8, 12, 2, other)
    return cams, a + b, TRUTH, [False] * 150 + [True] * 12
