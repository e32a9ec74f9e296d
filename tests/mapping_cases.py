"""Inputs of the mapping tests (test_mapping_cpu.py, test_gpu_mapping.py): a seeded random scene of a current frame and its
neighbouring keyframes whose matches end at every verdict of triangulateMatches, hand-built one-match gate cases, and the helpers
that turn them into the library's arguments.  Everything the reference leaves to the caller -- cur_T_ref * pose.inv(), W_T_cur's
translation, F21 -- is computed here with numpy."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
NLEVELS = 8
# A 2-view match that passes the epipolar gate lies within 2 px of its epipolar line, and the DLT splits that distance between
# the two views: with inv_sigma2 <= 1 its chi-square term stays below 5.991 and the gate could not be reached on a 1-camera rig.
# The scene's table therefore stands for features located to 0.2 px at level 0.
INV_SIGMA2 = (25.0 * 1.2 ** (-2.0 * np.arange(NLEVELS))).astype(np.float32)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def T4(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def make_rig(ncams, rng):
    """camconfig_: K_mats_ and cur_T_ref = [R_mats_ | t_mats_] per camera (camera 0 is the reference)"""
    Ks, Ts = [], []
    for c in range(ncams):
        f = 480.0 + 10.0 * c
        Ks.append(np.array([[f, 0, 320.0 + c], [0, f + 1.5, 240.0 - c], [0, 0, 1.0]]))
        if c == 0:
            Ts.append(np.eye(4))
        else:
            Ts.append(T4(rot(*rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.15, 0.15, 3)))
    return Ks, Ts


def frame_geometry(pose, rig_T):
    """proj (rows 0..2 of cur_T_ref * pose.inv()), centre_w (translation of pose * cur_T_ref.inv()) per camera, twc, and the 4x4s"""
    inv = np.linalg.inv(pose)
    full = [T @ inv for T in rig_T]
    return dict(proj=[M[:3].copy() for M in full], centre_w=[(pose @ np.linalg.inv(T))[:3, 3].copy() for T in rig_T],
                twc=pose[:3, 3].copy(), full=full, pose=pose)


def fundamental(full_cur, full_neigh, K_cur, K_neigh):
    """F21 of :5841-5845 for one camera pair, from the true relative pose of the two cameras"""
    Tji = full_cur @ np.linalg.inv(full_neigh)
    t = Tji[:3, 3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return np.linalg.inv(K_cur.T) @ tx @ Tji[:3, :3] @ np.linalg.inv(K_neigh)


def project(K, P, X):
    p = P[:, :3] @ X + P[:, 3]
    q = K @ p
    return np.array([q[0] / q[2], q[1] / q[2]])


class FrameBuilder:
    """collects the features of one keyframe: match_index rows and the keypoints of every camera"""

    def __init__(self, geom, Ks):
        self.g, self.Ks, self.C = geom, Ks, len(Ks)
        self.rows, self.kps, self.lids = [], [[] for _ in Ks], []

    def add(self, X, cams, rng, octave=None, lid=-1):
        """a feature that sees X in cameras `cams` (exact projections rounded to float); -> its index"""
        row = [-1] * self.C
        for c in cams:
            uv = project(self.Ks[c], self.g["proj"][c], X)
            o = int(rng.integers(0, NLEVELS)) if octave is None else octave
            row[c] = len(self.kps[c])
            self.kps[c].append((uv[0], uv[1], o))
        self.rows.append(row)
        self.lids.append(lid)
        return len(self.rows) - 1

    def move(self, feat, cam, duv):
        k = self.rows[feat][cam]
        x, y, o = self.kps[cam][k]
        self.kps[cam][k] = (x + duv[0], y + duv[1], o)

    def first_cam(self, feat):
        return next(c for c in range(self.C) if self.rows[feat][c] != -1)

    def done(self):
        kps = []
        for lst in self.kps:
            a = np.zeros(len(lst), KP_DTYPE)
            for i, (x, y, o) in enumerate(lst):
                a[i]["x"], a[i]["y"], a[i]["octave"] = np.float32(x), np.float32(y), o
            a["size"], a["response"] = 31.0, 1.0
            kps.append(a)
        return dict(match_index=np.array(self.rows, np.int32).reshape(-1, self.C), kps=kps, centre_w=self.g["centre_w"],
                    proj=self.g["proj"], twc=self.g["twc"], lids=np.array(self.lids, np.int32))


def pick_cams(C, rng, two_view):
    if C == 1 or two_view:
        return [int(rng.integers(0, C))]
    n = int(rng.choice([1, 2, 3, min(C, 4), C], p=[0.3, 0.3, 0.2, 0.1, 0.1]))
    return sorted(rng.choice(C, size=min(n, C), replace=False).tolist())


def scene(ncams, sizes=(300, 300, 50), seed=1, zero_f=2, n_old=40):
    """A current frame and len(sizes) neighbours.  Neighbour s has sizes[s] matches of these kinds, in shuffled order:
    good (a point 3 .. 15 in front of baselines of about 1: verdict 0), an offset of 3 .. 30 px off the epipolar line (2), a point
    behind the cameras (3), an offset of 1.2 .. 1.8 px off the line at level 0 (4), points 1500 away or between the two camera
    centres (5), a feature that has a landmark on entry (6), and a second match to the current feature of an earlier good match
    (6 through the walk, lids_cur carried across neighbours).  Neighbour `zero_f` has an all-zero F table (1).  Every neighbour
    also has n_old features with landmarks of the store at depth 3 .. 8 (the baseline gate's median)."""
    rng = np.random.default_rng(seed)
    Ks, rig_T = make_rig(ncams, rng)
    cur_g = frame_geometry(T4(rot(*rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.05, 0.05, 3)), rig_T)
    cur = FrameBuilder(cur_g, Ks)
    kinds = ["good"] * 40 + ["epi"] * 10 + ["behind"] * 10 + ["chi2"] * 10 + ["far"] * 8 + ["near"] * 4 + ["preset"] * 8 + ["shared"] * 10
    neigh, matches, F21, store = [], [], [], {}
    good_trains = []
    next_old = 0
    for s, n in enumerate(sizes):
        sign = 1.0 if s % 2 == 0 else -1.0
        g = frame_geometry(T4(rot(*rng.uniform(-0.08, 0.08, 3)), np.array([sign * (1.0 + 0.3 * s), 0.0, 0.0]) + rng.uniform(-0.1, 0.1, 3)), rig_T)
        fb = FrameBuilder(g, Ks)
        F = np.zeros((ncams, ncams, 3, 3))
        if s != zero_f:
            for cc in range(ncams):
                for cn in range(ncams):
                    F[cc, cn] = fundamental(cur_g["full"][cc], g["full"][cn], Ks[cc], Ks[cn])
        mid = 0.5 * (g["twc"] + cur_g["twc"])
        ms = []
        for kind in rng.permutation([kinds[(37 * i) % len(kinds)] for i in range(n)]):   # (any n gets a mix)
            if kind == "shared" and not good_trains:
                kind = "good"
            two_view = kind in ("chi2", "epi") and rng.random() < 0.5
            X = mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 15)])
            if kind == "behind":
                X = mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), -rng.uniform(3, 15)])
            elif kind == "far":
                X = mid + np.array([rng.uniform(-200, 200), rng.uniform(-150, 150), 1500.0])
            elif kind == "near":
                X = mid + np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(0.25, 0.35)])
            octave = 0 if kind == "chi2" else None
            if kind == "shared":
                t = good_trains[int(rng.integers(0, len(good_trains)))]
                X = t[1]
                q = fb.add(X, pick_cams(ncams, rng, False), rng)
                ms.append((q, t[0]))
                continue
            q = fb.add(X, pick_cams(ncams, rng, two_view), rng, octave, lid=-1)
            t = cur.add(X, pick_cams(ncams, rng, two_view), rng, octave)
            if kind == "preset":
                if rng.random() < 0.5:
                    fb.lids[q] = 3000 + next_old
                    store[3000 + next_old] = X
                    next_old += 1
                else:
                    cur.lids[t] = 3900 + len(ms) % 90
            if kind in ("epi", "chi2") and s != zero_f:
                cn, cc = fb.first_cam(q), cur.first_cam(t)
                kq = fb.kps[cn][fb.rows[q][cn]]
                line = F[cc, cn] @ np.array([np.float32(kq[0]), np.float32(kq[1]), 1.0])
                nrm = line[:2] / np.hypot(line[0], line[1])
                d = rng.uniform(3, 30) if kind == "epi" else rng.uniform(1.2, 1.8)
                cur.move(t, cc, nrm * d * (1 if rng.random() < 0.5 else -1))
            if kind == "good":
                good_trains.append((t, X))
            ms.append((q, t))
        for _ in range(n_old):
            X = g["twc"] + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 8)])
            fb.add(X, pick_cams(ncams, rng, False), rng, lid=3000 + next_old)
            store[3000 + next_old] = X
            next_old += 1
        neigh.append(fb.done())
        matches.append(np.array(ms, np.int32).reshape(-1, 2))
        F21.append(F)
    cur_d = cur.done()
    Tcw = np.linalg.inv(cur_g["pose"])
    return dict(ncams=ncams, K=np.array(Ks), inv_sigma2=INV_SIGMA2, cur=cur_d, neigh=neigh, matches=matches, F21=F21, store=store,
                Rcw=Tcw[:3, :3].copy(), tcw=Tcw[:3, 3].copy(), next_lid=100)


def to_frame(mc, d):
    return mc.map_frame(d["match_index"], d["kps"], d["centre_w"], d["proj"], d["twc"])


def fill_store(lm, store):
    """the landmarks the neighbours already have: points of `store`, any unit normal"""
    if store:
        lids = np.array(sorted(store), np.int32)
        lm.set(lids, np.array([store[int(l)] for l in lids]), np.tile([0.0, 0.0, 1.0], (len(lids), 1)))


def run_scene(mc, lm, sc, **kw):
    return lm.triangulate_neighbours(to_frame(mc, sc["cur"]), sc["cur"]["lids"], [to_frame(mc, f) for f in sc["neigh"]],
                                     [f["lids"] for f in sc["neigh"]], sc["F21"], sc["matches"], sc["K"], sc["inv_sigma2"], sc["Rcw"],
                                     sc["tcw"], sc["next_lid"], **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# hand-built gate cases for mcorb_host_map_gates / mcorb_dev_map_gates_selftest: one match per case
# ---------------------------------------------------------------------------------------------------------------------------
I3 = np.eye(3)
P_ID = np.hstack([I3, np.zeros((3, 1))])            # [I | 0]: camera centre at the origin
F_PASS = np.array([[0.0, 0, 0], [0, 0, 1], [0, 0, 0]])   # a = 0, b = 1, c = 0: num = y2, den = 1


def P_at(centre):
    """[I | -centre]: a camera at `centre` looking along +z"""
    return np.hstack([I3, -np.asarray(centre, float).reshape(3, 1)])


def gate_case(X, views, nv1, F=F_PASS, inv_sigma2=(1.0,)):
    """views: (P, K, centre, (kx, ky), octave) per view"""
    return dict(X=np.asarray(X, float), nv1=nv1, nv=len(views), P=[np.asarray(v[0], float) for v in views],
                K=[np.asarray(v[1], float) for v in views], centre=[np.asarray(v[2], float) for v in views],
                kps=[v[3] for v in views], octave=[v[4] for v in views], F=np.asarray(F, float), inv_sigma2=inv_sigma2)


def run_gates(mc, cases, device=None):
    """all cases in one call (they must share inv_sigma2) -> list of (verdict, n_rays, dist2, cos, normal)"""
    sig = cases[0]["inv_sigma2"]
    assert all(tuple(c["inv_sigma2"]) == tuple(sig) for c in cases)
    cat = lambda key: np.concatenate([np.asarray(c[key], np.float64).reshape(c["nv"], -1) for c in cases])
    v, r, d2, cs, nr = mc.map_gates([c["X"] for c in cases], [c["nv1"] for c in cases], [c["nv"] for c in cases], cat("P"), cat("K"),
                                    cat("centre"), np.concatenate([np.asarray(c["kps"], np.float32).reshape(-1, 2) for c in cases]),
                                    np.concatenate([c["octave"] for c in cases]), [c["F"] for c in cases], sig, device=device)
    return [(int(v[i]), int(r[i]), float(d2[i]), float(cs[i]), nr[i]) for i in range(len(cases))]
