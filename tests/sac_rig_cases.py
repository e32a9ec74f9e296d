"""Inputs and helpers of the rig-solver RANSAC tests (test_sac_rig_cpu.py, test_gpu_sac_rig.py): the solver's seeded cases over
rigs, the thin scenes -- a few observations per camera, no landmark seen twice -- and LocalMap.ransac_pose with a solver."""
import math

import numpy as np

import pose_cases as PC
import sac_cases as SC
import sac_ref as S


def solver_of(mc, cams):
    """the `solve` argument of sac_rig_ref: mcorb_sac_solve_rig on three observations of any cameras"""
    cc = PC.to_cams(mc, cams)

    def solve(three):
        return [SC.lists(p) for p in mc.sac_solve_rig(cc, [o[0] for o in three], [[o[1], o[2]] for o in three], [o[4] for o in three])]
    return solve


def solver_cases(ncams, n=4000, seed=11):
    """-> (cams, [(truth (R, t as numpy), cam: 3 camera indices, uv: 3 x (u, v) floats, X: 3 x 3)]): SC.solver_cases over the
    outward-facing rig of ncams cameras at 0.2 m offsets -- rotations up to 3.1 rad about a random axis, translation N(0, 1) per
    axis, each of the three observations in a camera drawn for it (repeats allowed), its point at depth 2 - 10 within +-0.5 x
    +-0.4 normalised.  The keypoints are rounded to float first and the points placed on their rays: no noise"""
    rng = np.random.default_rng(seed + ncams)
    cams = SC.outward_rig(ncams)
    out = []
    for _ in range(n):
        Rwb, twb = PC.rot(rng.normal(size=3), rng.uniform(0, 3.1)), rng.normal(size=3)
        ci, uv, X = [int(c) for c in rng.integers(ncams, size=3)], [], []
        for c in ci:
            cam = cams[c]
            x, y, z = rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), rng.uniform(2, 10)
            u, v = PC.f32(cam["fx"] * x + cam["s"] * y + cam["u0"]), PC.f32(cam["fy"] * y + cam["v0"])
            f = np.asarray(S.bearing(cam, u, v))
            pb = np.asarray(cam["R"]) @ (f / f[2] * z) + np.asarray(cam["t"])
            X.append(Rwb @ pb + twb)
            uv.append((u, v))
        out.append(((Rwb, twb), ci, uv, np.array(X)))
    return cams, out


def rays(cams, ci, uv):
    """-> (c, d): the body-frame rays of three observations, 3 x 3 each (numpy)"""
    c = np.array([cams[k]["t"] for k in ci], np.float64)
    d = np.array([np.asarray(cams[k]["R"]) @ np.asarray(S.bearing(cams[k], u, v)) for k, (u, v) in zip(ci, uv)])
    return c, d


def thin_scene(ncams, per_cam=3, seed=3, moved=0.4, noise=0.1):
    """-> (cams, truth, obs, match, is_moved): per_cam landmarks in the view of each camera of SC.scene's rig at SC.scene's pose,
    each observed by that camera alone, so no camera has four observations; the projections are rounded to float after N(0,
    noise px) is added, and round(moved * n) of the n observations, chosen by a seeded permutation, are moved by 50 px in a
    random direction.  Every observation is its own match"""
    rng = np.random.default_rng(seed)
    cams = SC.outward_rig(ncams)
    Rt = PC.rot([0.3, -0.2, 1.0], 0.7)
    tt = np.array([1.5, -0.7, 0.3])
    truth = (PC.rows_of(Rt), [float(v) for v in tt])
    n = ncams * per_cam
    is_moved = [False] * n
    for i in rng.permutation(n)[:int(round(moved * n))]:
        is_moved[int(i)] = True
    obs = []
    for c in range(ncams):
        for _ in range(per_cam):
            z = rng.uniform(2, 10)
            q = np.array([rng.uniform(-1.0, 1.0) * z, rng.uniform(-0.55, 0.55) * z, z])
            X = [float(v) for v in Rt @ (np.asarray(cams[c]["R"]) @ q + np.asarray(cams[c]["t"])) + tt]
            px, py = PC.project(cams, truth, c, X)
            px, py = px + rng.normal(scale=noise), py + rng.normal(scale=noise)
            if is_moved[len(obs)]:
                a = rng.uniform(0, 2 * math.pi)
                px, py = px + 50 * math.cos(a), py + 50 * math.sin(a)
            obs.append((c, PC.f32(px), PC.f32(py), int(rng.integers(4)), X))
    return cams, truth, obs, list(range(n)), is_moved


def run(mc, lm, cams, obs, solver="rig", threshold=SC.THRESHOLD, match=None, max_iterations=100, seed=0, refine=None, form="pts", first_lid=0):
    """SC.run with a solver"""
    cam, uv, octave, pts = PC.arrays(obs)
    kw = dict(pts=pts) if form == "pts" else dict(lids=PC.fill_points(lm, obs, first_lid))
    return lm.ransac_pose(PC.to_cams(mc, cams), cam, uv, octave, threshold, match=match, max_iterations=max_iterations, seed=seed,
                          refine=None if refine is None else mc.pose_params(*refine), solver=solver, **kw)
