"""Inputs and helpers of the polished essential pose tests (test_ess_polish_cpu.py, test_gpu_ess_polish.py): the comparison of a
LocalMap.essential_pose_polished result and of the mcorb_ess_polish_run hook against the restatement (ess_polish_ref.py), floats
as raw bytes with no tolerance, the rows written out by hand, and the problems that show the acceptance rule and the depth test.

A match is (u1, v1, u2, v2); a pose is (R as 9 floats row-major, t as 3 floats) = c1_T_c2 with |t| = 1."""
import math

import numpy as np

import ess_cases as EC
import ess_polish_ref as EP
import ess_ref as ER
import pose_ref as P

INF, NAN = math.inf, math.nan
CAM = EC.CAM
EPIPOLE = (CAM["u0"], CAM["v0"], CAM["u0"], CAM["v0"])   # both keypoints on the optical axis: x1 = x2 = (0, 0, 1) exactly


def run(mc, lm, matches, threshold_px=1.0, distance=50.0, max_iterations=100, seed=0, rounds=2, polish_iterations=10):
    uv1, uv2 = EC.arrays(matches)
    return lm.essential_pose_polished(EC.to_cam(mc), uv1, uv2, threshold_px, distance, max_iterations, seed, rounds, polish_iterations)


def reference(mc, matches, threshold_px=1.0, distance=50.0, max_iterations=100, seed=0, rounds=2, polish_iterations=10):
    return EP.polished(CAM, matches, EC.solver_of(mc), threshold_px, distance, max_iterations, seed, rounds, polish_iterations)


def same_record(pol, rp, what=""):
    """an EssentialPolish against ess_polish_ref.polish's dict"""
    assert P.same_bits(pol.R.reshape(9).tolist(), rp["win_R"]) and P.same_bits(pol.t.tolist(), rp["win_t"]), (what, "the pose it began from")
    assert P.same_bits(pol.E.reshape(9).tolist(), rp["win_E"]), (what, "the E it began from")
    assert (pol.n_ransac_inliers, pol.n_inliers) == (rp["win_ransac"], rp["win_count"]), (what, "the counts it began from")
    assert pol.rounds_run == len(rp["rounds"]) == len(pol.rounds), (what, "rounds run", pol.rounds_run, len(rp["rounds"]))
    for k, (q, r) in enumerate(zip(pol.rounds, rp["rounds"])):
        for key in ("n_members", "iterations", "status", "n_ransac_inliers", "n_inliers", "accepted"):
            assert q[key] == r[key], (what, "round", k, key, q[key], r[key])
        for key in ("cost_initial", "cost_final"):
            assert P.same_bits(q[key], r[key]), (what, "round", k, key, q[key], r[key])


def same(got, pol, ref, rp, what=""):
    """(EssentialResult, EssentialPolish) of a polished call against ess_polish_ref.polished's two dicts"""
    accepted = dict(ref, R=rp["R"], t=rp["t"], E=rp["E"], n_ransac_inliers=rp["n_ransac_inliers"], n_inliers=rp["n_inliers"],
                    inliers=rp["inliers"])
    EC.same(got, accepted, what)
    same_record(pol, rp, what)


def same_polish(a, b, what=""):
    """two EssentialPolish records of the library, doubles as raw bytes"""
    for k in ("R", "t", "E"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)
    assert (a.n_ransac_inliers, a.n_inliers, a.rounds_run) == (b.n_ransac_inliers, b.n_inliers, b.rounds_run), what
    for q, r in zip(a.rounds, b.rounds):
        assert {k: (ER.bits(v) if isinstance(v, float) else v) for k, v in q.items()} == \
               {k: (ER.bits(v) if isinstance(v, float) else v) for k, v in r.items()}, what


def hook(mc, matches, pose, member, threshold_px=1.0, distance=50.0, rounds=2, polish_iterations=10, what=""):
    """mcorb_ess_polish_run against the restatement on the bits -> (R 9, t, inliers, EssentialPolish, the restatement's dict)"""
    pts, E, n_ransac, count, flags = EP.pose_own(CAM, matches, pose, threshold_px, distance)
    rp = EP.polish(pts, ER.threshold2(CAM, threshold_px), distance, EP.inv_thr_of(CAM, threshold_px), pose, E, n_ransac, count, flags, member,
                   rounds, polish_iterations)
    a = np.array(matches, np.float64).reshape(-1, 4)
    R, t, Eo, inl, pol = mc.ess_polish_run(EC.to_cam(mc), pose[0], pose[1], a[:, 0:2], a[:, 2:4], member, threshold_px, distance, rounds=rounds,
                                           polish_iterations=polish_iterations)
    assert P.same_bits(R.reshape(9).tolist(), rp["R"]) and P.same_bits(t.tolist(), rp["t"]), (what, "pose", R, rp["R"])
    assert P.same_bits(Eo.reshape(9).tolist(), rp["E"]), (what, "E")
    assert inl.tolist() == rp["inliers"], (what, "inliers")
    same_record(pol, rp, what)
    return R.reshape(9).tolist(), t.tolist(), inl, pol, rp


def pose_of(R, t):
    """a numpy pose -> (R as 9, t / |t|)"""
    t = np.asarray(t, float)
    return [float(v) for v in np.asarray(R, float).reshape(9)], [float(v) for v in t / np.linalg.norm(t)]


def nearby(truth, angle=2e-3, shift=1e-2):
    """the pose `angle` rad and `shift` in the direction of t away from truth"""
    R, t = np.asarray(truth[0], float), np.asarray(truth[1], float)
    th = t / np.linalg.norm(t)
    side = np.cross(th, [0.3, -0.5, 0.8])
    side /= np.linalg.norm(side)
    return pose_of(R @ EC.rodrigues(angle * np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0)), th + shift * side)


def exact_scene(kind, n=80, seed=0):
    """-> (the true pose, n noise-free matches: frame 1's keypoints floats, frame 2's the projections in double)"""
    rng = np.random.default_rng(3000 + 10 * EC.KINDS.index(kind) + seed)
    R, t = EC.random_pose(rng, forward=kind == "forward", min_baseline=0.3)
    return (R, t), EC.exact_matches(rng, kind, n, R, t, off_plane=10)


def noisy(kind="general", n=40, seed=3):
    """-> (truth, matches, the pose nearby, its own flags): a seeded scene with N(0, 0.1 px) and a start about 2e-3 / 1e-2 away"""
    truth, matches, _ = EC.scene(kind, n=n, seed=seed, noise=0.1)
    start = nearby(truth)
    return truth, matches, start, EP.pose_own(CAM, matches, start)[4]


def hostile_rows():
    """-> [(name, matches, pose handed in, member)]: what the residual, the differences and the solve must hold on.  `bad` rows
    replace the scene's first match"""
    truth, matches, start, inl = noisy()
    good = [i for i, v in enumerate(inl) if v]
    out = []
    for k in (0, 1, 4, 5, 6):
        out.append(("%d members" % k, matches, start, [i in good[:k] for i in range(len(matches))]))
    for name, bad in (("+inf", (INF, 100.0, 200.0, 100.0)), ("-inf", (300.0, 100.0, 200.0, -INF)), ("NaN", (NAN, 100.0, 200.0, NAN))):
        rows = [bad] + matches[1:]
        out.append((name + " among the members", rows, start, [True] + inl[1:]))
        out.append((name + " outside the members", rows, start, [False] + inl[1:]))
    out.append(("t = 0", matches, (start[0], [0.0, 0.0, 0.0]), inl))
    out.append(("t NaN", matches, (start[0], [NAN, start[1][1], start[1][2]]), inl))
    stretched = ([2.0 * v for v in start[0]], start[1])
    sheared = ([1.0, 0.3, 0.0, 0.0, 1.0, -0.2, 0.1, 0.0, 1.0], start[1])
    singular = ([1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], start[1])
    for name, pose in (("twice a rotation", stretched), ("a sheared matrix", sheared), ("a singular matrix", singular)):
        out.append(("a pose that is not a rotation: " + name, matches, pose, inl))
    # both keypoints at the epipole of (I, e_z): a = E x2 and b = E^T x1 vanish, the residual is 0 / 0
    axis = ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0])
    out.append(("a0 = a1 = b0 = b1 = 0", [EPIPOLE] + matches[1:], axis, [True] * 12 + [False] * (len(matches) - 12)))
    return out


def hostile_matches():
    """the hostile keypoints as float matches, for a whole polished call: every kind among 120 matches of the seeded scene"""
    _, matches, _ = EC.scene("general", n=120, seed=4, noise=0.1)
    rows = list(matches)
    big = float(np.finfo(np.float32).max)
    rows[5] = (INF, 100.0, 200.0, 100.0)
    rows[17] = (300.0, 100.0, 200.0, -INF)
    rows[31] = (NAN, 100.0, 200.0, NAN)
    rows[64] = (big, -big, big, big)
    rows[90] = EPIPOLE
    return rows


def acceptance_problem():
    """-> (matches, start, member): 150 noise-free matches at a true pose and 12 at another pose 0.05 rad away, which are the
    members.  From the true pose the round moves towards the members' pose and loses the 150"""
    rng = np.random.default_rng(77)
    R, t = EC.random_pose(rng, min_baseline=0.3)
    a = EC.exact_matches(rng, "general", 150, R, t)
    R2 = R @ EC.rodrigues(0.05 * np.array([0.0, 1.0, 0.5]) / math.sqrt(1.25))
    b = EC.exact_matches(rng, "general", 12, R2, t)
    return a + b, pose_of(R, t), [False] * 150 + [True] * 12


def depth_problem():
    """-> (matches, start, member, distance, k): a noisy scene from a start nearby, members the start's own flags at distance 50.
    Match k is a member that is within the threshold at the start and at round 1's result, and `distance` lies strictly between
    its larger depth at the start and that at the result: found on the restatement, with one round"""
    truth, matches, start, member = noisy("general", 120, 5)
    pts = [ER.point(CAM, m) for m in matches]
    thr2 = ER.threshold2(CAM, 1.0)
    cand = EP.lm_round(lambda p: EP.sums(p, pts, member, EP.inv_thr_of(CAM, 1.0)), start, 10, sum(member))[0]
    E0, E1 = EP.E_of(start), EP.E_of(cand)
    best = None
    for k, p in enumerate(pts):
        if not (member[k] and ER.sampson(E0, p) < thr2 and ER.sampson(E1, p) < thr2):
            continue
        z0, z1 = max(ER.depths(start[0], start[1], p)), max(ER.depths(cand[0], cand[1], p))
        if z1 > z0 and (best is None or z1 - z0 > best[0]):
            best = (z1 - z0, k, 0.5 * (z0 + z1))
    assert best is not None
    return matches, start, member, best[2], best[1]
