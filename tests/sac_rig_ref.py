"""The RANSAC with the rig solver (solver="rig", MCORB_SAC_SOLVER_RIG) restated in plain Python on top of sac_ref.py.

Restated here: the sample walk -- all 16 draws mod S pick from the consensus list in input order, whatever their cameras, a
draw equal to an earlier member being dropped, four members or no model -- and the pick by the fourth point, scored in its own
camera.  Everything else is sac_ref's, reused and not copied: the draws, the bearing, the score, the counting over the consensus
set, the pick of the winner, the fold of observations to matches and the rule of FrontEnd.cpp:4786.  `ransac` and `ransac_refine`
below are sac_ref's own functions, the same code objects, run with this module's `sample` and `model` in place of sac_ref's.

NOT restated: the solver.  A hypothesis's candidate poses come from the library's mcorb_sac_solve_rig hook through the `solve`
argument, as sac_ref takes them from mcorb_sac_solve, so everything behind the solver compares on the bits.

Also here, and used only to judge mcorb_sac_solve_rig: an independent solver -- Grunert's quartic on the rays' directions through
numpy.polynomial.polyroots, 20 Newton steps on the three distance equations through numpy.linalg.solve, Kabsch through
numpy.linalg.svd."""
import math
import types

import numpy as np

import sac_ref as S

OK, NO_OBS, NO_MODEL = S.OK, S.NO_OBS, S.NO_MODEL
NEWTON = 20


def sample(seed, h, obs, cons):
    """-> ([s0, s1, s2, s3] with -1 for members not drawn, complete?)"""
    s, have = [-1, -1, -1, -1], 0
    for j in range(S.DRAWS):
        i = cons[S.draw(seed, h, j) % len(cons)]
        if i in s[:have]:
            continue
        s[have] = i
        have += 1
        if have == 4:
            return s, True
    return s, False


def candidates(cams, obs, s, solve):
    """the solver's poses on s[0 .. 2] and their scores at s[3] in its own camera, in root order"""
    return [(pose, S.obs_score(cams, pose, obs[s[3]])) for pose in solve([obs[i] for i in s[:3]])]


def model(cams, obs, s, solve):
    """of the solver's poses the one with the smallest score at s[3]; a tie goes to the lowest index, a NaN never wins -> pose or
    None"""
    best, best_score = None, None
    for pose, sc in candidates(cams, obs, s, solve):
        if sc != sc:
            continue
        if best is None or sc < best_score:
            best, best_score = pose, sc
    return best


def _rebound():
    g = dict(vars(S), sample=sample, model=model)
    g["ransac"] = types.FunctionType(S.ransac.__code__, g, "ransac", S.ransac.__defaults__)
    g["ransac_refine"] = types.FunctionType(S.ransac_refine.__code__, g, "ransac_refine", S.ransac_refine.__defaults__)
    return g["ransac"], g["ransac_refine"]


# sac_ref.ransac(cams, obs, threshold, solve, match=None, max_iterations=100, seed=0) and sac_ref.ransac_refine(cams, obs, threshold,
# solve, inv_sigma2, match=None, max_iterations=100, seed=0, refine_iterations=25) with the sample and the model above; solve(three
# observations) -> poses
ransac, ransac_refine = _rebound()


# ---------------------------------------------------------------------------------------------------------------------------
# the independent solver: judges mcorb_sac_solve_rig, is never compared on the bits
# ---------------------------------------------------------------------------------------------------------------------------
def numpy_rig(c, d, X):
    """the rig poses w_T_b (R 3 x 3, t) of three rays c_i + l d_i of the body's frame (c, d: 3 x 3, rows) on the world points X
    (3 x 3): the depths of the central P3P on (d, X) as a start, Newton on |B_i - B_j|^2 = |X_i - X_j|^2, Kabsch"""
    c, d, X = np.asarray(c, np.float64), np.asarray(d, np.float64), np.asarray(X, np.float64)
    a2, b2, c2 = np.sum((X[1] - X[2]) ** 2), np.sum((X[0] - X[2]) ** 2), np.sum((X[0] - X[1]) ** 2)
    ca, cb, cg = d[1] @ d[2], d[0] @ d[2], d[0] @ d[1]
    K, Cq = (a2 - c2) / b2, c2 / b2
    N = np.array([1 + K, -2 * K * cb, K - 1])
    D = np.array([2 * cg, -2 * ca])
    Q = np.array([1.0, -2 * cb, 1.0])
    npp = np.polynomial.polynomial
    D2 = npp.polymul(D, D)
    E = npp.polyadd(npp.polyadd(D2, npp.polymul(N, N)), -npp.polyadd(2 * cg * npp.polymul(N, D), Cq * npp.polymul(Q, D2)))
    poses = []
    for v in npp.polyroots(E):
        if abs(v.imag) > 1e-7 * max(1.0, abs(v)) or v.real <= 0:
            continue
        v = v.real
        u = npp.polyval(v, N) / npp.polyval(v, D)
        if not u > 0:
            continue
        s1 = math.sqrt(b2 / npp.polyval(v, Q))
        lam = np.array([s1, u * s1, v * s1])
        try:
            for _ in range(NEWTON):
                B = c + lam[:, None] * d
                D12, D13, D23 = B[0] - B[1], B[0] - B[2], B[1] - B[2]
                F = np.array([D12 @ D12 - c2, D13 @ D13 - b2, D23 @ D23 - a2])
                J = 2 * np.array([[D12 @ d[0], -(D12 @ d[1]), 0.0], [D13 @ d[0], 0.0, -(D13 @ d[2])], [0.0, D23 @ d[1], -(D23 @ d[2])]])
                lam = lam - np.linalg.solve(J, F)
        except np.linalg.LinAlgError:
            continue
        if not (np.isfinite(lam).all() and (lam > 0).all()):
            continue
        B = c + lam[:, None] * d
        mb, mx = B.mean(axis=0), X.mean(axis=0)
        U, _, Vt = np.linalg.svd((X - mx).T @ (B - mb))
        R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
        poses.append((R, mx - R @ mb))
    return poses
