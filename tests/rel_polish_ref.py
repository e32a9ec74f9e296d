"""The polish of the relative pose's RANSAC winner restated in plain Python, independently of csrc/mcorb_rel.h: Python floats
(IEEE doubles, one operation per operator, math.sqrt correctly rounded), lists, no numpy.

Restated here: the residual of a match at a pose, the six perturbed poses and the forward differences, the 28 sums and their
fold over 256 lanes, the Levenberg-Marquardt round around them, and the rounds with their acceptance rule.  Reused: pose_ref.py's
restated solve and retract (the 6 x 6 LDL^T and the Cayley retraction) and rel_ref.py's rays and score.  pose_ref.lm_round is tied
to the reprojection cost's sums, so its loop -- lambda 1e-4, halved / doubled inside [1e-16, 1e32], the stop at 1e-6 -- is written
out once more here around a `sums` callable; test_rel_polish_cpu.py holds the two loops to each other.

A pose is (R rows, t) = b1_T_b2; the rays of a match are rel_ref.rays_of's (a, c1, d2, c2)."""
import math

import pose_ref as P
import rel_ref as RR

H, INV_H = 2.0 ** -20, 2.0 ** 20
LANES, BLOCK = P.LANES, P.BLOCK
NO_OBS, NO_STEP, CONVERGED, MAX_ITER = P.NO_OBS, P.NO_STEP, P.CONVERGED, P.MAX_ITER


def scale_of(threshold):
    return 1.0 / math.sqrt(threshold)


def fit_poses(pose):
    """the pose and its six perturbations retract(pose, h e_k)"""
    return [pose] + [P.retract(pose, [H if j == k else 0.0 for j in range(6)]) for k in range(6)]


def residual(pose, rays, scale):
    """(a - P1 / |P1|, b / |b| - P2 / |P2|) * scale with the score's a, b, w, P1, P2"""
    a, c1, d2, c2 = rays
    R, t = pose
    dot, div, sqrt = RR.dot, RR.div, RR.sqrt
    b = RR.rot(R, d2)
    Rc = RR.rot(R, c2)
    w = [(Rc[i] + t[i]) - c1[i] for i in range(3)]
    aa, ab, bb, aw, bw = dot(a, a), dot(a, b), dot(b, b), dot(a, w), dot(b, w)
    det = ab * ab - aa * bb
    lam = div(ab * bw - bb * aw, det)
    mu = div(aa * bw - ab * aw, det)
    P1 = [0.5 * ((lam * a[i]) + (w[i] + mu * b[i])) for i in range(3)]
    P2 = [P1[i] - w[i] for i in range(3)]
    n1, n2, nb = sqrt(dot(P1, P1)), sqrt(dot(P2, P2)), sqrt(bb)
    return [(a[i] - div(P1[i], n1)) * scale for i in range(3)] + [(div(b[i], nb) - div(P2[i], n2)) * scale for i in range(3)]


def add(poses, rays, scale, s):
    """one member into a lane's 28 sums"""
    r0 = residual(poses[0], rays, scale)
    J = []          # J[k]: column k
    for k in range(6):
        rk = residual(poses[1 + k], rays, scale)
        J.append([(rk[c] - r0[c]) * INV_H for c in range(6)])
    at = 0
    for i in range(6):
        for j in range(i, 6):
            acc = J[i][0] * J[j][0]
            for c in range(1, 6):
                acc = acc + J[i][c] * J[j][c]
            s[at] = s[at] + acc
            at += 1
    for i in range(6):
        acc = J[i][0] * r0[0]
        for c in range(1, 6):
            acc = acc + J[i][c] * r0[c]
        s[21 + i] = s[21 + i] + acc
    e2 = r0[0] * r0[0]
    for c in range(1, 6):
        e2 = e2 + r0[c] * r0[c]
    s[27] = s[27] + e2


def fold(lanes):
    for b in range(LANES // BLOCK):
        stride = BLOCK // 2
        while stride >= 1:
            for l in range(stride):
                lo, hi = lanes[b * BLOCK + l], lanes[b * BLOCK + l + stride]
                for k in range(28):
                    lo[k] = lo[k] + hi[k]
            stride //= 2
    return [(lanes[0][k] + lanes[BLOCK][k]) + (lanes[2 * BLOCK][k] + lanes[3 * BLOCK][k]) for k in range(28)]


def sums(pose, rays, member, scale):
    """the 28 sums of a pass: match i goes to lane i mod 256 in ascending i"""
    poses = fit_poses(pose)
    lanes = []
    for l in range(LANES):
        s = [0.0] * 28
        for i in range(l, len(rays), LANES):
            if member[i]:
                add(poses, rays[i], scale, s)
        lanes.append(s)
    return fold(lanes)


def lm_round(sums_at, init, max_iterations):
    """pose_ref.lm_round's loop around sums_at(pose) -> (pose, iterations, status, cost at init, final cost)"""
    cur = init
    S = sums_at(cur)
    cost = cost0 = S[27]
    lam = 1e-4
    accepted = converged = False
    iterations = 0
    for it in range(max_iterations):
        iterations = it + 1
        delta = P.solve(S, lam)
        accept = False
        if delta is not None:
            trial = P.retract(cur, delta)
            T = sums_at(trial)
            accept = T[27] < cost
        if accept:
            dec = cost - T[27]
            stop = dec < 1e-6 or dec < 1e-6 * cost
            cur, S, cost, accepted = trial, T, T[27], True
            lam = lam * 0.5
            if stop:
                converged = True
                break
            if lam < 1e-16:
                break
        else:
            lam = lam * 2.0
            if lam > 1e32:
                break
    status = NO_STEP if not accepted else CONVERGED if converged else MAX_ITER
    return (cur if accepted else init), iterations, status, cost0, cost


def flags_at(pose, rays, threshold):
    return [RR.score_rays(pose, r) < threshold for r in rays]


def polish(rays, threshold, pose, count, flags, member, rounds=2, max_iterations=10):
    """the rounds from the current (pose, count, flags) with round 1's members -> dict(R, t, n_inliers, inliers: the accepted
    ones; win_R, win_t, win_count: what it began from; rounds: per round that ran dict(n_members, iterations, status,
    cost_initial, cost_final, n_inliers, accepted))"""
    out = dict(win_R=pose[0], win_t=pose[1], win_count=count, rounds=[])
    scale = scale_of(threshold)
    flags, member = list(flags), list(member)
    for _ in range(rounds):
        cand, its, status, c0, c1 = lm_round(lambda p: sums(p, rays, member, scale), pose, max_iterations)
        new = flags_at(cand, rays, threshold)
        n = sum(new)
        rec = dict(n_members=sum(1 for v in member if v), iterations=its, status=status, cost_initial=P.default_nan(c0),
                   cost_final=P.default_nan(c1), n_inliers=n, accepted=n >= count)
        out["rounds"].append(rec)
        if not rec["accepted"]:
            break
        pose, count, flags, member = cand, n, new, list(new)
    out.update(R=pose[0], t=pose[1], n_inliers=count, inliers=[bool(v) for v in flags])
    return out


def polished(cams, matches, threshold, solve, max_iterations=100, seed=0, rounds=2, polish_iterations=10):
    """rel_ref.ransac and the polish of its winner -> (ransac's dict, polish's dict); without a winner no round runs"""
    ref = RR.ransac(cams, matches, threshold, solve, max_iterations, seed)
    pose = (ref["R"], ref["t"])
    if ref["status"] != RR.OK:
        return ref, dict(win_R=pose[0], win_t=pose[1], win_count=0, rounds=[], R=pose[0], t=pose[1], n_inliers=0,
                         inliers=list(ref["inliers"]))
    rays = [RR.rays_of(cams, m) for m in matches]
    return ref, polish(rays, threshold, pose, ref["n_inliers"], ref["inliers"], ref["inliers"], rounds, polish_iterations)
