"""The rig pose refinement restated in plain Python, independently of csrc/mcorb_pose.h: Python floats (IEEE doubles, one
operation per operator, math.sqrt correctly rounded), lists, no numpy in the arithmetic.

From the reference: the cost -- RigResectioningFactor::evaluateError (MCSlam/include/MCSlam/GtsamFactorHelpers.h:75-100: the
reprojection error through pose.compose(body_P_sensor), and (2 fx, 2 fx) with a zero Jacobian for a CheiralityException), the
Huber model at sqrt(5.991) on a one-pixel sigma (MCSlam/src/FrontEnd.cpp:4276-4279) -- and the rounds (:4354-4400): two, each
from the initial estimate, each followed by the cull dot(err, err * inv_sigma2[octave]) > 5.991.  The optimizer is the one
DESIGN.md section 9g states (gtsam's is not in the tree): diagonal damping, an LDL^T, the Cayley retraction, lambda 1e-4 halved
/ doubled inside [1e-16, 1e32], and sums added in the tree of 256 lanes.

A rig is a list of dict(R=3 x 3 rows, t, fx, fy, s, u0, v0) (body_P_sensor and Cal3_S2); a pose is (R as 3 x 3 rows, t) = w_T_b;
an observation is (cam, kx, ky, octave, X) with kx, ky the floats of a KeyPoint::pt (as Python floats) and X the point."""
import math
import struct

LANES, BLOCK = 256, 64
NO_OBS, NO_STEP, CONVERGED, MAX_ITER = 0, 1, 2, 3
HUBER_K = math.sqrt(5.991)
CHI2 = 5.991


def default_nan(x):
    """a NaN cost is returned as the default quiet NaN (host and device differ in an invalid operation's sign)"""
    return struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000000))[0] if x != x else x


def pose_of_view(R0, t0):
    """a tracking view read as a rig whose body is camera 0's frame: w_T_b = (R0^T, -(R0^T t0))"""
    R = [[R0[c][r] for c in range(3)] for r in range(3)]
    t = [-((R0[0][r] * t0[0] + R0[1][r] * t0[1]) + R0[2][r] * t0[2]) for r in range(3)]
    return R, t


def transform_to(R, t, p):
    """Pose3::transformTo: R^T * (p - t)"""
    d = [p[0] - t[0], p[1] - t[1], p[2] - t[2]]
    return [R[0][r] * d[0] + R[1][r] * d[1] + R[2][r] * d[2] for r in range(3)]


def residual(cam, pose, X, kx, ky, want_j=True):
    """evaluateError -> (r, J): J is 2 x 6 w.r.t. the right perturbation (omega, upsilon) of w_T_b"""
    R, t = pose
    pb = transform_to(R, t, X)
    q = transform_to(cam["R"], cam["t"], pb)
    if q[2] <= 0:       # the CheiralityException (a NaN does not take it)
        return [2.0 * cam["fx"], 2.0 * cam["fx"]], [[0.0] * 6, [0.0] * 6]
    d = 1.0 / q[2]
    u, v = q[0] * d, q[1] * d
    r = [((cam["fx"] * u + cam["s"] * v) + cam["u0"]) - kx, (cam["fy"] * v + cam["v0"]) - ky]
    if not want_j:
        return r, None
    D00, D01, D02 = cam["fx"] * d, cam["s"] * d, -((cam["fx"] * u + cam["s"] * v) * d)
    D11, D12 = cam["fy"] * d, -((cam["fy"] * v) * d)
    B = []
    for k in range(3):      # row k of Rc^T * [ [p_b]x | -I ]
        M0, M1, M2 = cam["R"][0][k], cam["R"][1][k], cam["R"][2][k]
        B.append([M1 * pb[2] - M2 * pb[1], M2 * pb[0] - M0 * pb[2], M0 * pb[1] - M1 * pb[0], -M0, -M1, -M2])
    J = [[(D00 * B[0][c] + D01 * B[1][c]) + D02 * B[2][c] for c in range(6)],
         [D11 * B[1][c] + D12 * B[2][c] for c in range(6)]]
    return r, J


def huber(r, k=HUBER_K):
    """-> (weight, loss)"""
    e2 = r[0] * r[0] + r[1] * r[1]
    e = math.sqrt(e2) if e2 == e2 and e2 >= 0 else float("nan")
    if e <= k:
        return 1.0, 0.5 * e2
    return k / e, k * (e - 0.5 * k)


def sums(rig, pose, obs, alive):
    """the 28 sums of a pass: lane l adds observations l, l + 256, .. into +0.0; each block of 64 lanes folds with strides
    32 .. 1; the four blocks combine as (b0 + b1) + (b2 + b3)"""
    lanes = []
    for l in range(LANES):
        s = [0.0] * 28
        for i in range(l, len(obs), LANES):
            if not alive[i]:
                continue
            cam, kx, ky, _, X = obs[i]
            r, J = residual(rig[cam], pose, X, kx, ky)
            w, rho = huber(r)
            at = 0
            for a in range(6):
                for b in range(a, 6):
                    s[at] = s[at] + w * (J[0][a] * J[0][b] + J[1][a] * J[1][b])
                    at += 1
            for a in range(6):
                s[21 + a] = s[21 + a] + w * (J[0][a] * r[0] + J[1][a] * r[1])
            s[27] = s[27] + rho
        lanes.append(s)
    for b in range(LANES // BLOCK):
        stride = BLOCK // 2
        while stride >= 1:
            for l in range(stride):
                lo, hi = lanes[b * BLOCK + l], lanes[b * BLOCK + l + stride]
                for k in range(28):
                    lo[k] = lo[k] + hi[k]
            stride //= 2
    return [(lanes[0][k] + lanes[BLOCK][k]) + (lanes[2 * BLOCK][k] + lanes[3 * BLOCK][k]) for k in range(28)]


def solve(S, lam):
    """(H + lambda diag(H)) delta = -g by LDL^T; None when a pivot is not > 0"""
    A = [[0.0] * 6 for _ in range(6)]
    at = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = S[at]
            at += 1
    for i in range(6):
        A[i][i] = A[i][i] + lam * A[i][i]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        dj = A[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * D[k]
        if not dj > 0:
            return None
        D[j] = dj
        for i in range(j + 1, 6):
            v = A[j][i]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = v / dj
    y = [0.0] * 6
    for i in range(6):
        v = -S[21 + i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i] / D[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v
    return x


def retract(pose, delta):
    """R' = R * C(omega / 2) (Cayley), t' = t + R * upsilon"""
    R, t = pose
    a0, a1, a2 = delta[0] * 0.5, delta[1] * 0.5, delta[2] * 0.5
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    den, one = 1.0 + aa, 1.0 - aa
    a01, a02, a12 = 2.0 * (a0 * a1), 2.0 * (a0 * a2), 2.0 * (a1 * a2)
    Cm = [[(one + 2.0 * (a0 * a0)) / den, (a01 - 2.0 * a2) / den, (a02 + 2.0 * a1) / den],
          [(a01 + 2.0 * a2) / den, (one + 2.0 * (a1 * a1)) / den, (a12 - 2.0 * a0) / den],
          [(a02 - 2.0 * a1) / den, (a12 + 2.0 * a0) / den, (one + 2.0 * (a2 * a2)) / den]]
    Rn = [[(R[i][0] * Cm[0][j] + R[i][1] * Cm[1][j]) + R[i][2] * Cm[2][j] for j in range(3)] for i in range(3)]
    tn = [t[i] + ((R[i][0] * delta[3] + R[i][1] * delta[4]) + R[i][2] * delta[5]) for i in range(3)]
    return Rn, tn


def lm_round(rig, init, obs, alive, max_iterations):
    """one round from init -> (pose, iterations, status, cost at init, final cost, passes)"""
    cur = init
    S = sums(rig, cur, obs, alive)
    cost = cost0 = S[27]
    lam = 1e-4
    accepted = converged = False
    iterations, passes = 0, 1
    for it in range(max_iterations):
        iterations = it + 1
        delta = solve(S, lam)
        accept = False
        if delta is not None:
            trial = retract(cur, delta)
            T = sums(rig, trial, obs, alive)
            passes += 1
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
    return (cur if accepted else init), iterations, status, cost0, cost, passes


def refine(rig, init, obs, inv_sigma2, max_iterations=25):
    """OptimizePose's two rounds -> dict(R, t, status, iterations, cost_initial, cost_final, inliers, n_inliers, culled: per
    round the observations its cull took, passes: per round)"""
    n = len(obs)
    out = dict(R=init[0], t=init[1], status=NO_OBS, iterations=(0, 0), cost_initial=0.0, cost_final=0.0, inliers=[], n_inliers=0,
               culled=[[], []], passes=[0, 0])
    if n == 0:
        return out
    alive = [True] * n
    its, culled, passes = [], [], []
    pose = init
    for rnd in range(2):
        pose, it, status, c0, c1, np_ = lm_round(rig, init, obs, alive, max_iterations)
        its.append(it)
        passes.append(np_ + 1)
        if rnd == 0:
            out["cost_initial"] = default_nan(c0)
        out["cost_final"] = default_nan(c1)
        gone = []
        for i, (cam, kx, ky, octave, X) in enumerate(obs):
            if not alive[i]:
                continue
            r, _ = residual(rig[cam], pose, X, kx, ky, want_j=False)
            if (r[0] * r[0] + r[1] * r[1]) * inv_sigma2[octave] > CHI2:
                alive[i] = False
                gone.append(i)
        culled.append(gone)
    out.update(R=pose[0], t=pose[1], status=status, iterations=tuple(its), inliers=alive, n_inliers=sum(alive), culled=culled,
               passes=passes)
    return out


def same_bits(a, b):
    """two floats (or nested lists of floats) as raw bytes"""
    fa = [a] if isinstance(a, float) else [float(v) for row in a for v in (row if isinstance(row, (list, tuple)) else [row])]
    fb = [b] if isinstance(b, float) else [float(v) for row in b for v in (row if isinstance(row, (list, tuple)) else [row])]
    return struct.pack("<%dd" % len(fa), *fa) == struct.pack("<%dd" % len(fb), *fb)
