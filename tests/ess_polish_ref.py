"""The polish of the essential pose's RANSAC winner restated in plain Python, independently of csrc/mcorb_ess_polish.h: Python
floats (IEEE doubles, one operation per operator, math.sqrt correctly rounded), lists, no numpy.

Restated here: the basis of t's tangent plane, the retraction of (R, t) by five numbers, E = [t]x R, the residual of a match, the
six matrices of a pass and the forward differences, the 21 sums and their fold over 256 lanes, the five-unknown LDL^T solve, the
Levenberg-Marquardt round around them and the rounds with their acceptance rule.  Reused: ess_ref.py's point, sampson, depths,
in_front and threshold2, and pose_ref.py's Cayley retraction for R' = R C(delta[0 .. 2]) (its translation is not used).

A pose is (R as 9 floats row-major, t as 3 floats) = c1_T_c2, |t| = 1; a point is ess_ref.point's (x1, y1, x2, y2)."""
import ess_ref as ER
import pose_ref as P

H, INV_H = 2.0 ** -20, 2.0 ** 20
LANES, BLOCK = P.LANES, P.BLOCK
NO_OBS, NO_STEP, CONVERGED, MAX_ITER = P.NO_OBS, P.NO_STEP, P.CONVERGED, P.MAX_ITER
UNKNOWNS, SUMS, G, COST = 5, 21, 15, 20
div, sqrt, dot, cross = ER.div, ER.sqrt, ER.dot, ER.cross


def inv_thr_of(cam, threshold_px):
    return 1.0 / (threshold_px / ((cam["fx"] + cam["fy"]) / 2.0))


def basis(t):
    """b1 = (t x e_k) / |t x e_k| for the smallest |t_k| (the first of equals), b2 = t x b1"""
    k, least = 0, abs(t[0])
    if abs(t[1]) < least:
        k, least = 1, abs(t[1])
    if abs(t[2]) < least:
        k = 2
    e = [1.0 if j == k else 0.0 for j in range(3)]
    c = cross(t, e)
    n = sqrt(dot(c, c))
    b1 = [div(v, n) for v in c]
    return b1, cross(t, b1)


def retract(pose, delta):
    """R' = R C(delta[0 .. 2]) (pose_ref.retract's), t' = u / |u|, u = (t + delta[3] b1) + delta[4] b2"""
    R, t = pose
    Rn, _ = P.retract((ER.rows(R), t), [delta[0], delta[1], delta[2], 0.0, 0.0, 0.0])
    b1, b2 = basis(t)
    u = [(t[i] + delta[3] * b1[i]) + delta[4] * b2[i] for i in range(3)]
    n = sqrt(dot(u, u))
    return [v for row in Rn for v in row], [div(v, n) for v in u]


def E_of(pose):
    """[t]x R"""
    R, t = pose
    E = [0.0] * 9
    for j in range(3):
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j]
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j]
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j]
    return E


def fit_Es(pose):
    """E of the pose and of its five perturbations retract(pose, h e_k)"""
    return [E_of(pose)] + [E_of(retract(pose, [H if j == k else 0.0 for j in range(UNKNOWNS)])) for k in range(UNKNOWNS)]


def residual(E, p, inv_thr):
    x1, y1, x2, y2 = p
    a0, a1, a2 = (E[0] * x2 + E[1] * y2) + E[2], (E[3] * x2 + E[4] * y2) + E[5], (E[6] * x2 + E[7] * y2) + E[8]
    b0, b1 = (E[0] * x1 + E[3] * y1) + E[6], (E[1] * x1 + E[4] * y1) + E[7]
    r = (x1 * a0 + y1 * a1) + a2
    return div(r, sqrt(((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1)) * inv_thr


def add(Es, p, inv_thr, s):
    """one member into a lane's 21 sums"""
    r0 = residual(Es[0], p, inv_thr)
    J = [(residual(Es[1 + k], p, inv_thr) - r0) * INV_H for k in range(UNKNOWNS)]
    at = 0
    for i in range(UNKNOWNS):
        for j in range(i, UNKNOWNS):
            s[at] = s[at] + J[i] * J[j]
            at += 1
    for i in range(UNKNOWNS):
        s[G + i] = s[G + i] + J[i] * r0
    s[COST] = s[COST] + r0 * r0


def fold(lanes):
    for b in range(LANES // BLOCK):
        stride = BLOCK // 2
        while stride >= 1:
            for l in range(stride):
                lo, hi = lanes[b * BLOCK + l], lanes[b * BLOCK + l + stride]
                for k in range(SUMS):
                    lo[k] = lo[k] + hi[k]
            stride //= 2
    return [(lanes[0][k] + lanes[BLOCK][k]) + (lanes[2 * BLOCK][k] + lanes[3 * BLOCK][k]) for k in range(SUMS)]


def sums(pose, pts, member, inv_thr):
    """the 21 sums of a pass: match i goes to lane i mod 256 in ascending i"""
    Es = fit_Es(pose)
    lanes = []
    for l in range(LANES):
        s = [0.0] * SUMS
        for i in range(l, len(pts), LANES):
            if member[i]:
                add(Es, pts[i], inv_thr, s)
        lanes.append(s)
    return fold(lanes)


def solve(S, lam, members):
    """(H + lambda diag(H)) delta = -g by LDL^T on five unknowns; None when a pivot is not > 0, and for fewer than five members"""
    N = UNKNOWNS
    if members < N:
        return None
    A = [[0.0] * N for _ in range(N)]
    at = 0
    for i in range(N):
        for j in range(i, N):
            A[i][j] = S[at]
            at += 1
    for i in range(N):
        A[i][i] = A[i][i] + lam * A[i][i]
    L = [[0.0] * N for _ in range(N)]
    D = [0.0] * N
    ok = True
    for j in range(N):
        dj = A[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * D[k]
        if not dj > 0:
            ok = False
        D[j] = dj
        for i in range(j + 1, N):
            v = A[j][i]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = div(v, dj)
    if not ok:
        return None
    y = [0.0] * N
    for i in range(N):
        v = -S[G + i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    delta = [0.0] * N
    for i in range(N - 1, -1, -1):
        v = div(y[i], D[i])
        for k in range(i + 1, N):
            v = v - L[k][i] * delta[k]
        delta[i] = v
    return delta


def lm_round(sums_at, init, max_iterations, members):
    """pose_ref.lm_round's loop around sums_at(pose), the sums of `members` members -> (pose, iterations, status, cost at init, final
    cost)"""
    cur = init
    S = sums_at(cur)
    cost = cost0 = S[COST]
    lam = 1e-4
    accepted = converged = False
    iterations = 0
    for it in range(max_iterations):
        iterations = it + 1
        delta = solve(S, lam, members)
        accept = False
        if delta is not None:
            trial = retract(cur, delta)
            T = sums_at(trial)
            accept = T[COST] < cost
        if accept:
            dec = cost - T[COST]
            stop = dec < 1e-6 or dec < 1e-6 * cost
            cur, S, cost, accepted = trial, T, T[COST], True
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


def tested_at(pose, E, pts, thr2, distance):
    """-> (within the threshold, flagged: that and the depth test) per match"""
    within = [ER.sampson(E, p) < thr2 for p in pts]
    flags = [w and ER.in_front(ER.depths(pose[0], pose[1], p), distance) for w, p in zip(within, pts)]
    return within, flags


def polish(pts, thr2, distance, inv_thr, pose, E, n_ransac, count, flags, member, rounds=2, max_iterations=10):
    """the rounds from the current (pose, E, counts, flags) with round 1's members -> dict(R, t, E, n_ransac_inliers, n_inliers,
    inliers: the accepted ones; win_R, win_t, win_E, win_ransac, win_count: what it began from; rounds: per round that ran
    dict(n_members, iterations, status, cost_initial, cost_final, n_ransac_inliers, n_inliers, accepted))"""
    out = dict(win_R=list(pose[0]), win_t=list(pose[1]), win_E=list(E), win_ransac=n_ransac, win_count=count, rounds=[])
    flags, member = list(flags), list(member)
    for _ in range(rounds):
        cand, its, status, c0, c1 = lm_round(lambda p: sums(p, pts, member, inv_thr), pose, max_iterations, sum(1 for v in member if v))
        Ec = E_of(cand)
        within, new = tested_at(cand, Ec, pts, thr2, distance)
        nr, n = sum(within), sum(new)
        rec = dict(n_members=sum(1 for v in member if v), iterations=its, status=status, cost_initial=P.default_nan(c0),
                   cost_final=P.default_nan(c1), n_ransac_inliers=nr, n_inliers=n, accepted=n >= count)
        out["rounds"].append(rec)
        if not rec["accepted"]:
            break
        pose, E, n_ransac, count, flags, member = cand, Ec, nr, n, new, list(new)
    out.update(R=list(pose[0]), t=list(pose[1]), E=list(E), n_ransac_inliers=n_ransac, n_inliers=count, inliers=[bool(v) for v in flags])
    return out


def polished(cam, matches, solve5, threshold_px=1.0, distance=50.0, max_iterations=100, seed=0, rounds=2, polish_iterations=10):
    """ess_ref.ransac and the polish of its winner -> (ransac's dict, polish's dict); without a winner no round runs"""
    ref = ER.ransac(cam, matches, solve5, threshold_px, distance, max_iterations, seed)
    pose = (list(ref["R"]), list(ref["t"]))
    if ref["status"] != ER.OK:
        return ref, dict(win_R=pose[0], win_t=pose[1], win_E=list(ref["E"]), win_ransac=0, win_count=0, rounds=[], R=pose[0], t=pose[1],
                         E=list(ref["E"]), n_ransac_inliers=0, n_inliers=0, inliers=list(ref["inliers"]))
    pts = [ER.point(cam, m) for m in matches]
    return ref, polish(pts, ER.threshold2(cam, threshold_px), distance, inv_thr_of(cam, threshold_px), pose, ref["E"], ref["n_ransac_inliers"],
                       ref["n_inliers"], ref["inliers"], ref["inliers"], rounds, polish_iterations)


def pose_own(cam, matches, pose, threshold_px=1.0, distance=50.0):
    """what the hook takes as the current state of a pose handed in: (pts, E, n_ransac, count, flags) of the pose itself"""
    pts = [ER.point(cam, m) for m in matches]
    E = E_of(pose)
    within, flags = tested_at(pose, E, pts, ER.threshold2(cam, threshold_px), distance)
    return pts, E, sum(within), sum(flags), flags
