"""Inputs and helpers of the bundle adjustment tests (test_ba_cpu.py, test_gpu_ba.py, scripts/ba_rate.py): seeded windows with
known true poses and points, rows written out by hand, and the comparison of a LocalMap.bundle_adjust result against the
restatement (ba_ref.py), floats as raw bytes with no tolerance.

A scene is a dict: cams (pose_ref.py's rig), truth_poses / poses (lists of (R rows, t)), fixed, truth_pts / pts (lists of
[x, y, z]), obs (list of (kf, cam, lm, kx, ky, octave)), moved (per observation), sigma (per level)."""
import math

import numpy as np

import ba_ref as B
import pose_cases as PC
import pose_ref as P
import track_cases as T

NAMES = {B.NO_OBS: "NO_OBS", B.NO_STEP: "NO_STEP", B.CONVERGED: "CONVERGED", B.MAX_ITER: "MAX_ITER"}
# what the reference hands Isotropic::Sigma: GetInverseScaleSigmaSquares() at scaleFactor 1.2
SIGMA = [1.0 / (1.2 ** (2 * l)) for l in range(4)]
IDENT = PC.IDENT


def ring_rig(ncams, arm=0.1, fx=160.0, cols=320, rows=240, skew=0.0):
    """camera c looks outwards along the body's x-z plane at 360 / ncams degrees from the next, on a lever arm of `arm` m"""
    cams = []
    for c in range(ncams):
        ang = 2 * math.pi * c / ncams
        R_ = PC.rot([0.0, 1.0, 0.0], ang)
        t = R_ @ np.array([0.0, 0.0, arm])
        cams.append(T.cam(PC.rows_of(R_), t, fx=fx, fy=fx, s=skew * (c + 1), u0=cols / 2.0 + 0.25 * c, v0=rows / 2.0 - 0.5 * c))
    return cams


def scene(nkf=4, ncams=4, nlm=200, nfixed=2, seed=11, noise=0.3, moved=0.0, moved_px=30.0, off=(0.02, 0.1), pt_off=0.1, spacing=0.3,
          fx=160.0, cols=320, rows=240, skew=0.0, noct=4, max_views=None):
    """nkf keyframes `spacing` m apart along x with small turns, the first nfixed fixed; nlm landmarks in a ring around them,
    every one observed by every camera of every keyframe that has it in front and inside the image (at most max_views
    observations per landmark), the projections with `noise` px of Gaussian noise rounded to float, a fraction `moved` of them
    moved by moved_px; the free poses are off by off[0] rad and off[1] m, the points by pt_off m"""
    rng = np.random.default_rng(seed)
    cams = ring_rig(ncams, fx=fx, cols=cols, rows=rows, skew=skew)
    truth_poses = []
    for k in range(nkf):
        Rk = PC.rot([0.1, 1.0, 0.05], 0.05 * k) @ PC.rot([1.0, 0.0, 0.0], 0.02 * (k % 3))
        tk = np.array([spacing * k, 0.02 * (k % 2), 0.05 * k])
        truth_poses.append((PC.rows_of(Rk), [float(v) for v in tk]))
    fixed = [k < nfixed for k in range(nkf)]
    poses = []
    for k, (Rk, tk) in enumerate(truth_poses):
        if fixed[k]:
            poses.append((Rk, tk))
            continue
        d = rng.normal(size=3)
        poses.append((PC.rows_of(np.asarray(Rk) @ PC.rot(rng.normal(size=3), off[0])),
                      [float(v) for v in np.asarray(tk) + off[1] * d / np.linalg.norm(d)]))
    centre = np.array([spacing * (nkf - 1) / 2.0, 0.0, 0.0])
    truth_pts, pts, obs, is_moved = [], [], [], []
    while len(truth_pts) < nlm:
        ang, rad = rng.uniform(0, 2 * math.pi), rng.uniform(2.0, 6.0)
        X = centre + np.array([rad * math.cos(ang), rng.uniform(-1.0, 1.0), rad * math.sin(ang)])
        X = [float(v) for v in X]
        mine = []
        for k in range(nkf):
            for c in range(ncams):
                pb = P.transform_to(truth_poses[k][0], truth_poses[k][1], X)
                q = P.transform_to(cams[c]["R"], cams[c]["t"], pb)
                if q[2] < 0.5:
                    continue
                px, py = PC.project(cams, truth_poses[k], c, X)
                if not (0 <= px <= cols and 0 <= py <= rows):
                    continue
                mine.append((k, c, px, py))
        if max_views is not None:
            mine = mine[:max_views]
        if not mine:
            continue
        j = len(truth_pts)
        truth_pts.append(X)
        d = rng.normal(size=3)
        pts.append([float(v) for v in np.asarray(X) + pt_off * d / np.linalg.norm(d)])
        for k, c, px, py in mine:
            px, py = px + noise * rng.normal(), py + noise * rng.normal()
            mv = bool(rng.random() < moved)
            if mv:
                a = rng.uniform(0, 2 * math.pi)
                px, py = px + moved_px * math.cos(a), py + moved_px * math.sin(a)
            obs.append((k, c, j, PC.f32(px), PC.f32(py), int(rng.integers(noct))))
            is_moved.append(mv)
    # the caller's order is not the sorted one
    perm = rng.permutation(len(obs))
    obs = [obs[i] for i in perm]
    is_moved = [is_moved[i] for i in perm]
    return dict(cams=cams, truth_poses=truth_poses, poses=poses, fixed=fixed, truth_pts=truth_pts, pts=pts, obs=obs, moved=is_moved,
                sigma=SIGMA[:noct])


def without(sc, drop):
    """the scene without the observations flagged in `drop` and without the landmarks left with fewer than two observations;
    the landmarks are renumbered -> (scene, kept landmark indices)"""
    obs = [o for o, d in zip(sc["obs"], drop) if not d]
    count = {}
    for o in obs:
        count[o[2]] = count.get(o[2], 0) + 1
    keep = [j for j in range(len(sc["pts"])) if count.get(j, 0) >= 2]
    new = {j: i for i, j in enumerate(keep)}
    out = dict(sc)
    out.update(obs=[(o[0], o[1], new[o[2]], o[3], o[4], o[5]) for o in obs if o[2] in new], pts=[sc["pts"][j] for j in keep],
               truth_pts=[sc["truth_pts"][j] for j in keep])
    out.pop("moved", None)
    return out, keep


def errors(sc, poses):
    """(worst rotation error in rad, worst translation error in m) of the free keyframes against the truth"""
    worst = [0.0, 0.0]
    for k, p in enumerate(poses):
        if sc["fixed"][k]:
            continue
        a, d = PC.pose_error(p, sc["truth_poses"][k])
        worst = [max(worst[0], a), max(worst[1], d)]
    return worst


def arrays(obs):
    kf = np.array([o[0] for o in obs], np.int32)
    cam = np.array([o[1] for o in obs], np.int32)
    lm = np.array([o[2] for o in obs], np.int32)
    uv = np.array([[o[3], o[4]] for o in obs], np.float32).reshape(-1, 2)
    octave = np.array([o[5] for o in obs], np.int32)
    return kf, cam, lm, uv, octave


def fill_points(store, pts, first_lid=0):
    lids = np.arange(first_lid, first_lid + len(pts), dtype=np.int32)
    if len(pts):
        p = np.array(pts, np.float64).reshape(-1, 3)
        store.set(lids, p, np.zeros_like(p))
    return lids


def run(mc, store, sc, max_iterations=25, form="pts", first_lid=0, **kw):
    """LocalMap.bundle_adjust on a scene, the points given (form "pts") or read from the store (form "lids")"""
    kf, cam, lm, uv, octave = arrays(sc["obs"])
    pk = dict(pts=np.array(sc["pts"], np.float64).reshape(-1, 3)) if form == "pts" else dict(lids=fill_points(store, sc["pts"], first_lid))
    a = dict(cams=PC.to_cams(mc, sc["cams"]), kf_R=[p[0] for p in sc["poses"]], kf_t=[p[1] for p in sc["poses"]], fixed=sc["fixed"],
             obs_kf=kf, obs_cam=cam, obs_lm=lm, uv=uv, octave=octave, sigma=sc["sigma"], max_iterations=max_iterations)
    a.update(pk)
    a.update(kw)
    return store.bundle_adjust(**a)


def ref(sc, max_iterations=25):
    return B.adjust(sc["cams"], sc["poses"], sc["fixed"], sc["pts"], sc["obs"], sc["sigma"], max_iterations)


def as_ref(res):
    """a BAResult as the restatement's dict, for same()"""
    return dict(R=res.R.tolist(), t=res.t.tolist(), pts=res.pts.tolist(), status=res.status, iterations=res.iterations,
                cost_initial=res.cost_initial, cost_final=res.cost_final, inliers=res.inliers.tolist(), n_inliers=res.n_inliers)


def flat(x):
    out = []
    for v in x:
        out.extend(flat(v) if isinstance(v, (list, tuple)) else [float(v)])
    return out


def same(got, want, what=""):
    """got, want: dicts as ba_ref.adjust returns them; floats as raw bytes"""
    assert got["status"] == want["status"], (what, "status", NAMES[got["status"]], NAMES[want["status"]])
    assert got["iterations"] == want["iterations"], (what, "iterations", got["iterations"], want["iterations"])
    for f in ("cost_initial", "cost_final", "R", "t", "pts"):
        a, b = flat([got[f]]), flat([want[f]])
        assert len(a) == len(b) and np.array(a).tobytes() == np.array(b).tobytes(), (what, f, got[f], want[f])
    assert [bool(v) for v in got["inliers"]] == [bool(v) for v in want["inliers"]], (what, "inliers")
    assert got["n_inliers"] == want["n_inliers"], (what, "n_inliers")


# ---------------------------------------------------------------------------------------------------------------------------
# rows written out by hand: the flat rig, one keyframe at the identity, q = X
# ---------------------------------------------------------------------------------------------------------------------------
def hand_scene(rows, sigma=(1.0,), fixed=True, extra_kf=()):
    """one landmark per row (cam, kx, ky, octave, X) of pose_cases.py, each seen once from keyframe 0 at the identity (fixed by
    default: with one observation a landmark's V is rank 2, damped) and, with extra_kf, once more from those keyframes"""
    poses = [IDENT] + [(T.EYE, [0.1 * (k + 1), 0.0, 0.0]) for k in range(len(extra_kf))]
    obs = []
    for j, (c, kx, ky, octave, X) in enumerate(rows):
        obs.append((0, c, j, kx, ky, octave))
        for k in extra_kf:
            obs.append((k, c, j, kx, ky, octave))
    return dict(cams=PC.flat_rig(), poses=poses, fixed=[fixed] + [False] * len(extra_kf), pts=[list(r[4]) for r in rows], obs=obs,
                sigma=list(sigma))


def huber_rows(sigma):
    """whitened e exactly k and one ulp either side under a sigma that is a power of two (the whitening is then exact): the point
    (x, 0, 1) against a keypoint at the origin has r = (x, 0), whitened x / sigma"""
    k = P.HUBER_K
    return [(0, 0.0, 0.0, 0, [x * sigma, 0.0, 1.0]) for x in (math.nextafter(k, 0.0), k, math.nextafter(k, 10.0))]


def _rr(target):
    """doubles (a, b) with a * a + b * b == target in floating point, found among the neighbours of sqrt(target - a * a)"""
    for a in (1.5, 1.25, 1.75, 1.0, 2.0, 0.75, 0.5, 2.25):
        b = math.sqrt(target - a * a)
        for _ in range(32):
            b = math.nextafter(b, 0.0)
        for _ in range(64):
            if a * a + b * b == target:
                return a, b
            b = math.nextafter(b, 10.0)
    raise AssertionError("no pair of doubles squares to %r" % target)


def chi2_rows():
    """-> (rows, sigma per level, expected flags).  The point (a s, b s, 1) against a keypoint at the origin under sigma s, a power
    of two, has the whitened r = (a, b) exactly.  With a a + b b exactly 5.991 the observation stays in, with the next double
    above it goes; both under s = 1 (level 0) and s = 4 (level 1).  The last row's point is NaN: every cost is NaN, nothing is
    accepted and the flags are taken at the initial state (a NaN is not greater: in)"""
    rows, flags = [], []
    for octave, s in enumerate((1.0, 4.0)):
        for target, keep in ((5.991, True), (math.nextafter(5.991, 10.0), False)):
            a, b = _rr(target)
            rows.append((0, 0.0, 0.0, octave, [a * s, b * s, 1.0]))
            flags.append(keep)
    rows.append((0, 1.0, 2.0, 0, [1.0, 2.0, float("nan")]))
    flags.append(True)
    return rows, [1.0, 4.0], flags


# ---------------------------------------------------------------------------------------------------------------------------
# degenerate shapes, small: -> (name, scene, what the restatement must say)
# ---------------------------------------------------------------------------------------------------------------------------
def degenerate():
    """a list of (name, scene, check(scene, ref)) -- check asserts what the shape is about, on the restatement's result"""
    out = []
    base = scene(nlm=30, seed=21)

    def untouched(key, idx):
        def check(sc, ref):
            for i in idx:
                assert flat([ref[key][i]]) == flat([sc["poses"][i][0] if key == "R" else sc["poses"][i][1] if key == "t" else sc["pts"][i]])
        return check

    def moved_pts(sc, ref, idx):
        for j in idx:
            assert flat([ref["pts"][j]]) != flat([sc["pts"][j]]), j

    sc = dict(base, fixed=[True] * 4, poses=list(base["truth_poses"]))
    def all_fixed(sc, ref):
        assert ref["status"] == B.CONVERGED and ref["cost_final"] < ref["cost_initial"]
        untouched("R", range(4))(sc, ref)
        untouched("t", range(4))(sc, ref)
        moved_pts(sc, ref, range(len(sc["pts"])))
    out.append(("all keyframes fixed", sc, all_fixed))

    sc = dict(base, obs=[o for o in base["obs"] if o[0] != 3])
    def unobserved_kf(sc, ref):
        assert ref["status"] in (B.CONVERGED, B.MAX_ITER)
        untouched("R", [0, 1, 3])(sc, ref)
        untouched("t", [0, 1, 3])(sc, ref)
        assert flat([ref["t"][2]]) != flat([sc["poses"][2][1]])
    out.append(("a free keyframe nobody observes", sc, unobserved_kf))

    sc = dict(base, pts=base["pts"] + [[1.0, 2.0, 3.0]])
    def unobserved_lm(sc, ref):
        assert ref["status"] in (B.CONVERGED, B.MAX_ITER)
        untouched("pts", [len(sc["pts"]) - 1])(sc, ref)
    out.append(("a landmark nobody observes", sc, unobserved_lm))

    sc = dict(base, obs=[o for o in base["obs"] if not (o[2] == 0 and o[0] >= 2)])
    def fixed_only_lm(sc, ref):
        assert any(o[2] == 0 for o in sc["obs"]) and ref["status"] in (B.CONVERGED, B.MAX_ITER)
        moved_pts(sc, ref, [0])
    out.append(("a landmark seen only from fixed keyframes", sc, fixed_only_lm))

    first = next(i for i, o in enumerate(base["obs"]) if o[2] == 1 and o[0] >= 2)
    sc = dict(base, obs=[o for i, o in enumerate(base["obs"]) if o[2] != 1 or i == first])
    def one_obs_lm(sc, ref):
        assert sum(o[2] == 1 for o in sc["obs"]) == 1 and ref["status"] in (B.CONVERGED, B.MAX_ITER)
        moved_pts(sc, ref, [1])
    out.append(("a landmark with one observation", sc, one_obs_lm))

    rows = [(c, kx, ky, o, [-v for v in X]) for c, kx, ky, o, X in PC.z_rows(False)[:6]]
    sc = hand_scene(rows, fixed=False, extra_kf=(1,))
    def behind(sc, ref):
        assert ref["status"] == B.NO_STEP and ref["n_inliers"] == 0      # (the whitened (2 fx, 2 fx) has r.r = 8)
        untouched("R", range(2))(sc, ref)
        untouched("t", range(2))(sc, ref)
        untouched("pts", range(len(sc["pts"])))(sc, ref)
    out.append(("everything behind the rig", sc, behind))

    bad = ([row[:] for row in base["poses"][2][0]], base["poses"][2][1][:])
    bad[0][1][2] = float("nan")
    sc = dict(base, poses=base["poses"][:2] + [bad] + base["poses"][3:])
    def nan_pose(sc, ref):
        assert ref["status"] == B.NO_STEP and ref["cost_initial"] != ref["cost_initial"]
        assert np.array(flat([ref["R"]])).tobytes() == np.array(flat([[p[0] for p in sc["poses"]]])).tobytes()
        assert np.array(flat([ref["pts"]])).tobytes() == np.array(flat([sc["pts"]])).tobytes()
    out.append(("a NaN initial pose", sc, nan_pose))
    return out
