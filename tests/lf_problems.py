"""Triangulation problems for the shared solver (mc-slam_amd/csrc/mcorb_triangulate.h), host and device tests alike: each is
(nv, x: 2 * nv normalised coordinates, P: nv row-major 3x4 matrices).  Kinds: exact correspondences, pixel noise, one gross
wrong correspondence, near-zero baselines, points near infinity, all-zero designs (zero trace), and two constructed designs that
steer the solver's iteration: one whose start vector is the null vector (settles in the unshifted steps), one whose smallest
eigenvector is orthogonal to the start vector to 1e-8 (the Rayleigh steps polish the second one, the Sylvester check re-runs)."""
import numpy as np

KINDS = ("exact", "noise", "gross", "baseline", "infinity", "zero", "start", "sylvester")


def _rot(rng, s):
    w = rng.normal(0, s, 3)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _rig(rng, nv, baseline):
    Ps = []
    for i in range(nv):
        R = _rot(rng, 0.05)
        t = np.array([-baseline * i, rng.normal(0, baseline * 0.1), rng.normal(0, baseline * 0.1)])
        Ps.append(np.hstack([R, t[:, None]]))
    return Ps


def _project(Ps, X):
    out = []
    for P in Ps:
        p = P @ np.append(X, 1.0)
        out += [p[0] / p[2], p[1] / p[2]]
    return np.array(out)


def _designed(nv_unused, eig, u1):
    """a 2-view problem whose 4x4 DLT design D has D^T D = U diag(eig) U^T, U's first column u1: x = 0 and D = -[P0 rows 0, 1;
    P1 rows 0, 1] (x * P[8 + i] - P[i] with x = 0)"""
    Q, _ = np.linalg.qr(np.column_stack([u1, np.eye(4)[:, :3]]))
    Q[:, 0] = u1 / np.linalg.norm(u1)
    D = np.diag(np.sqrt(eig)) @ Q.T
    P0, P1 = np.zeros((3, 4)), np.zeros((3, 4))
    P0[0], P0[1], P1[0], P1[1] = -D[0], -D[1], -D[2], -D[3]
    P0[2] = P1[2] = [0.3, -0.2, 1.0, 0.5]
    return 2, np.zeros(4), np.concatenate([P0.ravel(), P1.ravel()])


def problem(rng, kind, nv):
    v0 = np.array([1.0 + 0.01 * i for i in range(4)]) / 2.0
    if kind == "start":
        return _designed(nv, [1e-30, 1.0, 3.0, 7.0], v0)
    if kind == "sylvester":
        a = rng.normal(size=4)
        a -= a @ v0 / (v0 @ v0) * v0            # orthogonal to the start vector ...
        a += 1e-8 * v0                           # ... but not exactly
        return _designed(nv, [0.9, 1.0, 5.0, 10.0], a)
    if kind == "zero":
        return nv, np.zeros(2 * nv), np.zeros(12 * nv)
    baseline = 1e-9 if kind == "baseline" else rng.uniform(0.05, 0.3)
    Ps = _rig(rng, nv, baseline)
    X = np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(1, 30)])
    if kind == "infinity":
        X = X * 1e9
    x = _project(Ps, X)
    if kind == "noise":
        x = x + rng.normal(0, 1e-3, x.shape)     # about a pixel at f = 1000
    if kind == "gross":
        i = rng.integers(nv)
        x[2 * i:2 * i + 2] = rng.uniform(-0.5, 0.5, 2)
    return nv, x, np.concatenate([P.ravel() for P in Ps])


def problems(n, max_views, seed):
    """n problems cycling through KINDS, 2 .. max_views views -> (nv int32 [n], x float64 [sum 2 nv], P float64 [sum 12 nv], kinds)"""
    rng = np.random.default_rng(seed)
    nvs, xs, Ps, kinds = [], [], [], []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        nv, x, P = problem(rng, kind, int(rng.integers(2, max_views + 1)))
        nvs.append(nv); xs.append(x); Ps.append(P); kinds.append(kind)
    return np.array(nvs, np.int32), np.concatenate(xs), np.concatenate(Ps), kinds
