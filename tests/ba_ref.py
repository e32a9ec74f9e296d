"""The local bundle adjustment restated in plain Python, independently of csrc/mcorb_ba.h: Python floats (IEEE doubles, one
operation per operator, math.sqrt correctly rounded), lists, no numpy in the arithmetic.  DESIGN.md section 9o.

From the reference (MCSlam/src/Backend.cpp:1380-1393, 1426-1440): GenericProjectionFactor<Pose3, Point3, Cal3_S2> on the body pose
with body_P_sensor, Huber at sqrt(5.991) over Isotropic::Sigma(2, sigma[octave]); a point behind the camera gives (2 fx, 2 fx)
with zero Jacobians (GtsamFactorHelpers.h:75-100), whitened like any residual.  Stated: pose_ref.py's Levenberg-Marquardt on the
whole state, the gauge held by fixed keyframes, the landmarks eliminated by the Schur complement, every sum in a stated order.

A rig and a pose are pose_ref.py's; an observation is (kf, cam, lm, kx, ky, octave) with kx, ky the floats of a KeyPoint::pt."""
import pose_ref as P

LANES, BLOCK = P.LANES, P.BLOCK
NO_OBS, NO_STEP, CONVERGED, MAX_ITER = 0, 1, 2, 3
CHI2 = 5.991
MAX_KF = 16


def observation(cam, pose, X, kx, ky, inv_s, want_j=True):
    """-> (r, J, JX, w, rho), whitened; J is 2 x 6 by the pose's right perturbation, JX 2 x 3 by the point"""
    r, J = P.residual(cam, pose, X, kx, ky, want_j)
    r = [r[0] * inv_s, r[1] * inv_s]
    w, rho = P.huber(r)
    if not want_j:
        return r, None, None, w, rho
    R, t = pose
    pb = P.transform_to(R, t, X)
    q = P.transform_to(cam["R"], cam["t"], pb)
    if q[2] <= 0:
        JX = [[0.0 * inv_s] * 3, [0.0 * inv_s] * 3]
    else:
        d = 1.0 / q[2]
        u, v = q[0] * d, q[1] * d
        D00, D01, D02 = cam["fx"] * d, cam["s"] * d, -((cam["fx"] * u + cam["s"] * v) * d)
        D11, D12 = cam["fy"] * d, -((cam["fy"] * v) * d)
        Rc = cam["R"]
        JX = [[0.0] * 3, [0.0] * 3]
        for c in range(3):      # column c of M = Rc^T R^T
            M0 = (Rc[0][0] * R[c][0] + Rc[1][0] * R[c][1]) + Rc[2][0] * R[c][2]
            M1 = (Rc[0][1] * R[c][0] + Rc[1][1] * R[c][1]) + Rc[2][1] * R[c][2]
            M2 = (Rc[0][2] * R[c][0] + Rc[1][2] * R[c][1]) + Rc[2][2] * R[c][2]
            JX[0][c] = ((D00 * M0 + D01 * M1) + D02 * M2) * inv_s
            JX[1][c] = (D11 * M1 + D12 * M2) * inv_s
    J = [[J[0][c] * inv_s for c in range(6)], [J[1][c] * inv_s for c in range(6)]]
    return r, J, JX, w, rho


def plan(nkf, nlm, fixed, obs):
    """the stable sort by (lm, kf) and the system -> (order, per landmark its sorted observation indices, sys_of_kf, kf_of_sys)"""
    seen = [False] * nkf
    for o in obs:
        seen[o[0]] = True
    sys_of_kf, kf_of_sys = [-1] * nkf, []
    for k in range(nkf):
        if not fixed[k] and seen[k]:
            sys_of_kf[k] = len(kf_of_sys)
            kf_of_sys.append(k)
    order = sorted(range(len(obs)), key=lambda i: (obs[i][2], obs[i][0]))      # (sorted is stable)
    per_lm = [[] for _ in range(nlm)]
    for i in order:
        per_lm[obs[i][2]].append(i)
    return order, per_lm, sys_of_kf, kf_of_sys


def linearize_lm(cams, poses, X, obs, idx, inv_s, sys_of_kf):
    """a landmark's observations in order -> (V[6], gp[3], cost, views: list of (a, U[21], g[6], W[6][3]) ascending a)"""
    V, gp, cost, views = [0.0] * 6, [0.0] * 3, 0.0, []
    cur_kf = -1
    for i in idx:
        kf, cam, _, kx, ky, octave = obs[i]
        r, J, JX, w, rho = observation(cams[cam], poses[kf], X, kx, ky, inv_s[octave])
        at = 0
        for a in range(3):
            for b in range(a, 3):
                V[at] = V[at] + w * (JX[0][a] * JX[0][b] + JX[1][a] * JX[1][b])
                at += 1
        for a in range(3):
            gp[a] = gp[a] + w * (JX[0][a] * r[0] + JX[1][a] * r[1])
        cost = cost + rho
        if sys_of_kf[kf] < 0:
            continue
        if kf != cur_kf:
            views.append((sys_of_kf[kf], [0.0] * 21, [0.0] * 6, [[0.0] * 3 for _ in range(6)]))
            cur_kf = kf
        _, U, g, W = views[-1]
        at = 0
        for a in range(6):
            for b in range(a, 6):
                U[at] = U[at] + w * (J[0][a] * J[0][b] + J[1][a] * J[1][b])
                at += 1
        for a in range(6):
            g[a] = g[a] + w * (J[0][a] * r[0] + J[1][a] * r[1])
        for a in range(6):
            for c in range(3):
                W[a][c] = W[a][c] + w * (J[0][a] * JX[0][c] + J[1][a] * JX[1][c])
    return V, gp, cost, views


def cost_lm(cams, poses, X, obs, idx, inv_s):
    cost = 0.0
    for i in idx:
        kf, cam, _, kx, ky, octave = obs[i]
        cost = cost + observation(cams[cam], poses[kf], X, kx, ky, inv_s[octave], want_j=False)[4]
    return cost


def ldl3(V, lam):
    """V with d + lambda d on the diagonal as an LDL^T written out -> (l10, l20, l21, d0, d1, d2), or None when a pivot is not > 0"""
    a00, a01, a02, a11, a12, a22 = V[0] + lam * V[0], V[1], V[2], V[3] + lam * V[3], V[4], V[5] + lam * V[5]
    d0 = a00
    if not d0 > 0:
        return None
    l10, l20 = a01 / d0, a02 / d0
    d1 = a11 - (l10 * l10) * d0
    if not d1 > 0:
        return None
    l21 = (a12 - (l20 * l10) * d0) / d1
    d2 = (a22 - (l20 * l20) * d0) - (l21 * l21) * d1
    if not d2 > 0:
        return None
    return l10, l20, l21, d0, d1, d2


def solve3(L, b):
    l10, l20, l21, d0, d1, d2 = L
    y0 = b[0]
    y1 = b[1] - l10 * y0
    y2 = (b[2] - l20 * y0) - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = (y0 / d0 - l10 * x1) - l20 * x2
    return [x0, x1, x2]


def fold(nlm, K, term):
    """fold_j: lane l of 256 adds the terms of landmarks l, l + 256, .. into +0.0 (term(j) -> K floats, or None when landmark j
    does not qualify); each block of 64 lanes folds with strides 32 .. 1; the four blocks combine as (b0 + b1) + (b2 + b3)"""
    lanes = []
    for l in range(LANES):
        s = [0.0] * K
        for j in range(l, nlm, LANES):
            t = term(j)
            if t is None:
                continue
            for k in range(K):
                s[k] = s[k] + t[k]
        lanes.append(s)
    for b in range(LANES // BLOCK):
        stride = BLOCK // 2
        while stride >= 1:
            for l in range(stride):
                lo, hi = lanes[b * BLOCK + l], lanes[b * BLOCK + l + stride]
                for k in range(K):
                    lo[k] = lo[k] + hi[k]
            stride //= 2
    return [(lanes[0][k] + lanes[BLOCK][k]) + (lanes[2 * BLOCK][k] + lanes[3 * BLOCK][k]) for k in range(K)]


def solve_dense(S, rhs):
    """S delta = -rhs by pose_ref.solve's LDL^T on n unknowns (S: n x n, its upper triangle read); None when a pivot is not > 0"""
    n = len(rhs)
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    ok = True
    for j in range(n):
        dj = S[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * D[k]
        if not dj > 0:
            ok = False
        D[j] = dj
        for i in range(j + 1, n):
            v = S[j][i]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = v / dj if dj != 0 else float("nan")
    if not ok:
        return None
    y = [0.0] * n
    for i in range(n):
        v = -rhs[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        v = y[i] / D[i]
        for k in range(i + 1, n):
            v = v - L[k][i] * x[k]
        x[i] = v
    return x


def step(lin, nsys, lam):
    """one solve on a linearization (a list of linearize_lm results) -> (delta: 6 nsys floats, or None; L: per landmark its LDL^T
    or None; S, rhs: the reduced system)"""
    nlm = len(lin)
    L = [ldl3(lin[j][0], lam) for j in range(nlm)]
    slot = [{v[0]: v for v in lin[j][3]} for j in range(nlm)]
    n = 6 * nsys
    S = [[0.0] * n for _ in range(n)]
    rhs = [0.0] * n
    for a in range(nsys):
        def diag_term(j):
            if L[j] is None or a not in slot[j]:
                return None
            _, U, g, W = slot[j][a]
            z = solve3(L[j], lin[j][1])
            return U + [g[i] - ((W[i][0] * z[0] + W[i][1] * z[1]) + W[i][2] * z[2]) for i in range(6)]
        Ua = fold(nlm, 27, diag_term)
        for b in range(a, nsys):
            def pair_term(j):
                if L[j] is None or a not in slot[j] or b not in slot[j]:
                    return None
                Wa, Wb = slot[j][a][3], slot[j][b][3]
                E = [0.0] * 36
                for c in range(6):
                    y = solve3(L[j], Wb[c])
                    for i in range(6):
                        E[6 * i + c] = (Wa[i][0] * y[0] + Wa[i][1] * y[1]) + Wa[i][2] * y[2]
                return E
            E = fold(nlm, 36, pair_term)
            for i in range(6):
                for k in range(i if a == b else 0, 6):
                    if a != b:
                        S[6 * a + i][6 * b + k] = -E[6 * i + k]
                    else:
                        u = Ua[i * 6 - i * (i - 1) // 2 + (k - i)]
                        S[6 * a + i][6 * b + k] = ((u + lam * u) if i == k else u) - E[6 * i + k]
        for i in range(6):
            rhs[6 * a + i] = Ua[21 + i]
    return solve_dense(S, rhs), L, S, rhs


def backsub_lm(lin_j, L_j, nsys, delta, X):
    """an active landmark's new point"""
    V, gp, _, views = lin_j
    tt = gp[:]
    for a, _, _, W in views:        # ascending a
        d = delta[6 * a:6 * a + 6]
        for c in range(3):
            tt[c] = tt[c] + (((((W[0][c] * d[0] + W[1][c] * d[1]) + W[2][c] * d[2]) + W[3][c] * d[3]) + W[4][c] * d[4]) + W[5][c] * d[5])
    dX = solve3(L_j, [-tt[0], -tt[1], -tt[2]])
    return [X[c] + dX[c] for c in range(3)]


def adjust(cams, poses, fixed, pts, obs, sigma, max_iterations=25):
    """-> dict(R, t: per keyframe; pts; status, iterations, cost_initial, cost_final, inliers, n_inliers)"""
    nkf, nlm = len(poses), len(pts)
    out = dict(R=[p[0] for p in poses], t=[p[1] for p in poses], pts=[list(x) for x in pts], status=NO_OBS, iterations=0,
               cost_initial=0.0, cost_final=0.0, inliers=[], n_inliers=0)
    if not obs:
        return out
    inv_s = [1.0 / s for s in sigma]
    _, per_lm, sys_of_kf, kf_of_sys = plan(nkf, nlm, fixed, obs)
    nsys = len(kf_of_sys)
    cur_P, cur_X = list(poses), [list(x) for x in pts]

    def linearize(Ps, Xs):
        return [linearize_lm(cams, Ps, Xs[j], obs, per_lm[j], inv_s, sys_of_kf) for j in range(nlm)]

    lin = linearize(cur_P, cur_X)
    cost = cost0 = fold(nlm, 1, lambda j: [lin[j][2]])[0]
    lam = 1e-4
    accepted = converged = False
    solves = 0
    for it in range(max_iterations):
        solves = it + 1
        delta, L, _, _ = step(lin, nsys, lam)
        accept = False
        if delta is not None:
            trial_P = [P.retract(cur_P[k], delta[6 * sys_of_kf[k]:6 * sys_of_kf[k] + 6]) if sys_of_kf[k] >= 0 else cur_P[k]
                       for k in range(nkf)]
            trial_X = [backsub_lm(lin[j], L[j], nsys, delta, cur_X[j]) if L[j] is not None else cur_X[j] for j in range(nlm)]
            costs = [cost_lm(cams, trial_P, trial_X[j], obs, per_lm[j], inv_s) for j in range(nlm)]
            T = fold(nlm, 1, lambda j: [costs[j]])[0]
            accept = T < cost
        if accept:
            dec = cost - T
            stop = dec < 1e-6 or dec < 1e-6 * cost
            cur_P, cur_X, cost, accepted = trial_P, trial_X, T, True
            lam = lam * 0.5
            if stop:
                converged = True
                break
            if lam < 1e-16:
                break
            if it + 1 < max_iterations:
                lin = linearize(cur_P, cur_X)
        else:
            lam = lam * 2.0
            if lam > 1e32:
                break
    inliers = []
    for kf, cam, lm, kx, ky, octave in obs:
        r = observation(cams[cam], cur_P[kf], cur_X[lm], kx, ky, inv_s[octave], want_j=False)[0]
        inliers.append(not (r[0] * r[0] + r[1] * r[1]) > CHI2)
    out.update(R=[p[0] for p in cur_P], t=[p[1] for p in cur_P], pts=cur_X,
               status=NO_STEP if not accepted else CONVERGED if converged else MAX_ITER, iterations=solves,
               cost_initial=P.default_nan(cost0), cost_final=P.default_nan(cost), inliers=inliers, n_inliers=sum(inliers))
    return out
