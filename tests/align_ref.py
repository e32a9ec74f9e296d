"""The rig pose between two frames from 3D-3D pairs restated in numpy, independently of csrc/mcorb_align.h: Python integers for the
draws (rel_ref.py's finaliser and walk, on three draws), float64 columns for the distances -- every operator one numpy elementwise
operation, nothing fused, so one IEEE operation per element in the order written --, and the fold-ordered sum of the distances.

Restated: the draws and the walk, the distance |p1 - (R p2 + t)|, the strict threshold, the counting over all pairs, the pick
(largest count, lowest hypothesis), the refit's member set, the verdict at inlier_dist and the mean distance with its fold.  NOT
restated: the solver -- a hypothesis's pose, the refit's and mode 0's come from the library's mcorb_align_solve hook through the
`solve` argument (as rel_ref.py takes its poses from mcorb_rel_solve), so everything around the solver compares on the bits.

Also here, and used only to judge mcorb_align_solve: Kabsch's solution of the same least-squares problem by numpy.linalg.svd with
the determinant fix.

A pose is (R rows, t) = b1_T_b2: X_1 = R X_2 + t.  p1, p2: (n, 3) float64 arrays."""
import math

import numpy as np

import rel_ref as RR

OK, NO_OBS, NO_MODEL = 0, 1, 2
ALL, SAC = 0, 1
USED_SAC, USED_FIT = 0, 1
SAMPLE = 3
LANES, BLOCK = 256, 64
IDENT = RR.IDENT


def sample(seed, h, n):
    """-> (the 3 members in draw order, or 3 x -1; complete?): draw j of hypothesis h is number 1 + 32 h + j"""
    if n < SAMPLE:
        return [-1] * SAMPLE, False
    return RR.walk([RR.draw(seed, h, j) % (n - j) for j in range(SAMPLE)]), True


def dist(pose, a, b):
    """|a - (R b + t)| of one pair, Python floats"""
    R, t = pose
    q = [(R[i][0] * b[0] + R[i][1] * b[1]) + R[i][2] * b[2] for i in range(3)]
    d = [a[i] - (q[i] + t[i]) for i in range(3)]
    return RR.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def dist_many(pose, p1, p2):
    """dist for all pairs at once: the same operators in the same order on float64 columns"""
    R, t = pose
    x, y, z = p2[:, 0], p2[:, 1], p2[:, 2]
    with np.errstate(all="ignore"):
        q = [(R[i][0] * x + R[i][1] * y) + R[i][2] * z for i in range(3)]
        d = [p1[:, i] - (q[i] + t[i]) for i in range(3)]
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def fold_sum(values):
    """the sum in the order that is part of the definition: value i into lane i mod 256, a lane from 0.0 in ascending i; each
    block of 64 lanes folded with strides 32 .. 1, s[l] = s[l] + s[l + stride]; the four blocks as (b0 + b1) + (b2 + b3)"""
    lanes = np.zeros(LANES)
    with np.errstate(all="ignore"):
        for k in range(0, len(values), LANES):
            chunk = np.asarray(values[k:k + LANES], np.float64)
            lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
        b = []
        for k in range(0, LANES, BLOCK):
            s = lanes[k:k + BLOCK].copy()
            stride = BLOCK // 2
            while stride >= 1:
                s[:stride] = s[:stride] + s[stride:2 * stride]
                stride //= 2
            b.append(float(s[0]))
        return (b[0] + b[1]) + (b[2] + b[3])


def run(p1, p2, solve, mode=SAC, threshold=0.2, inlier_dist=0.1, max_iterations=100, seed=0, refit=True):
    """-> dict(status, used, R, t, sac_R, sac_t, mean_error, n_inliers, inliers, sac_n_inliers, best, sample, n_models, counts
    (None without a model), models, samples).  solve(p1, p2, member or None) -> (R rows, t) or None"""
    p1 = np.asarray(p1, np.float64).reshape(-1, 3)
    p2 = np.asarray(p2, np.float64).reshape(-1, 3)
    n = len(p1)
    out = dict(status=NO_OBS, used=USED_SAC, R=IDENT[0], t=IDENT[1], sac_R=IDENT[0], sac_t=IDENT[1], mean_error=0.0, n_inliers=0,
               inliers=[False] * n, sac_n_inliers=0, best=-1, sample=[-1] * SAMPLE, n_models=0, counts=[], models=[], samples=[])
    if not n:
        return out
    answer = None
    if mode == ALL:
        answer = solve(p1, p2, None)
        if answer is not None:
            out.update(used=USED_FIT)
    else:
        best, best_count = -1, -1
        for h in range(max_iterations):
            s, complete = sample(seed, h, n)
            pose = solve(p1[s], p2[s], None) if complete else None
            count = None
            if pose is not None:
                count = int(np.count_nonzero(dist_many(pose, p1, p2) < threshold))
                if count > best_count:
                    best, best_count = h, count
            out["counts"].append(count)
            out["models"].append(pose)
            out["samples"].append(s)
        out["n_models"] = sum(1 for m in out["models"] if m is not None)
        if best >= 0:
            answer = out["models"][best]
            out.update(sac_R=answer[0], sac_t=answer[1], sac_n_inliers=best_count, best=best, sample=out["samples"][best])
            if refit:
                fit = solve(p1, p2, dist_many(answer, p1, p2) < threshold)
                if fit is not None:
                    answer = fit
                    out.update(used=USED_FIT)
    out["status"] = NO_MODEL
    if answer is not None:
        d = dist_many(answer, p1, p2)
        flags = d < inlier_dist
        mean = fold_sum(d) / float(n)
        out.update(status=OK, R=answer[0], t=answer[1], inliers=[bool(v) for v in flags], n_inliers=int(np.count_nonzero(flags)),
                   mean_error=mean)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the independent solver: judges mcorb_align_solve, is never compared on the bits
# ---------------------------------------------------------------------------------------------------------------------------
def cross_covariance(p1, p2):
    a, b = p2 - p2.mean(axis=0), p1 - p1.mean(axis=0)
    return a.T @ b


def kabsch(p1, p2):
    """-> (R, t) minimising sum |p1 - (R p2 + t)|^2: the SVD of the cross-covariance with the determinant fix"""
    c1, c2 = p1.mean(axis=0), p2.mean(axis=0)
    U, _, Vt = np.linalg.svd(cross_covariance(p1, p2))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, c1 - R @ c2


def well_shaped(p1, p2, ratio=1e-3):
    """the second singular value of the cross-covariance is at least `ratio` of the first"""
    s = np.linalg.svd(cross_covariance(p1, p2), compute_uv=False)
    return bool(s[1] >= ratio * s[0])


def pose_distance(pose, truth):
    """max |dR_ij| and |dt| / max(1, |t|)"""
    return RR.pose_distance(pose, truth)


def same_bits(a, b):
    return RR.same_bits(a, b)


def bits(x):
    return RR.bits(x)


def next_up(x):
    return math.nextafter(x, math.inf)
