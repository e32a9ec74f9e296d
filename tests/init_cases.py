"""Inputs of the map-initialization tests (test_init_cpu.py, test_gpu_init.py): a seeded two-frame scene whose matches end at
every verdict of FrontEnd::initialization's loop, hand-built cases for the hook (caller-given X, so that a gate or a median can be
put on an exact value), and the helpers that turn both into the library's and the restatement's arguments.  Everything the
reference leaves to the caller -- the projection matrices, prev's centres, cur_T_ref.inv()'s translation -- is computed here."""
import math

import numpy as np

import init_ref as IR
import mapping_cases as Mc

NLEVELS, INV_SIGMA2 = Mc.NLEVELS, Mc.INV_SIGMA2
KINDS = ["good"] * 11 + ["behind"] * 2 + ["chi2"] * 2 + ["far"] * 2 + ["off"] * 3   # of 20: at least 10 % each


def scene(ncams, n=300, seed=3):
    """lf_prev at the identity, the current frame at T (a baseline of about 1 along x), n matches of these kinds in shuffled
    order: good (a point 3 .. 15 in front: verdict 0), behind both frames (3), a keypoint moved 3 .. 8 px across the epipolar
    line at level 0 (4), a point 1500 away (5), and good matches whose flag is clear on entry (9).  Some good matches repeat an
    earlier accepted match's queryIdx or trainIdx with a second feature of the same point (the later id wins)"""
    rng = np.random.default_rng(seed)
    Ks, rig_T = Mc.make_rig(ncams, rng)
    T = Mc.T4(Mc.rot(*rng.uniform(-0.05, 0.05, 3)), np.array([1.0, 0.0, 0.0]) + rng.uniform(-0.1, 0.1, 3))
    gp, gc = Mc.frame_geometry(np.eye(4), rig_T), Mc.frame_geometry(T, rig_T)
    prev, cur = Mc.FrameBuilder(gp, Ks), Mc.FrameBuilder(gc, Ks)
    mid = 0.5 * T[:3, 3]
    ms, flags, goods = [], [], []
    for kind in rng.permutation([KINDS[(7 * i) % len(KINDS)] for i in range(n)]):
        X = mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 15)])
        if kind == "behind":
            X = mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), -rng.uniform(3, 15)])
        elif kind == "far":
            X = mid + np.array([rng.uniform(-200, 200), rng.uniform(-150, 150), 1500.0])
        two_view = kind == "chi2"
        octave = 0 if kind == "chi2" else None
        dup = len(goods) % 15 if kind == "good" and len(goods) > 4 else -1
        if dup == 0:      # a second current feature of an earlier accepted match's point, matched to its queryIdx
            q, _, X = goods[len(goods) // 2]
            t = cur.add(X, Mc.pick_cams(ncams, rng, False), rng)
        elif dup == 7:    # .. and a second previous feature matched to its trainIdx
            _, t, X = goods[len(goods) // 2]
            q = prev.add(X, Mc.pick_cams(ncams, rng, False), rng)
        else:
            q = prev.add(X, Mc.pick_cams(ncams, rng, two_view), rng, octave)
            t = cur.add(X, Mc.pick_cams(ncams, rng, two_view), rng, octave)
        if kind == "chi2":
            cur.move(t, cur.first_cam(t), (0.0, rng.uniform(3, 8) * (1 if rng.random() < 0.5 else -1)))
        if kind == "good":
            goods.append((q, t, X))
        ms.append((q, t))
        flags.append(kind != "off")
    pd, cd = prev.done(), cur.done()
    pd["lids"][::7] = 7          # (ids from before are overwritten without a test)
    return dict(ncams=ncams, K=np.array(Ks), inv_sigma2=INV_SIGMA2, prev=pd, cur=cd, R=T[:3, :3].copy(), t=T[:3, 3].copy(),
                body=np.array([np.linalg.inv(M)[:3, 3] for M in rig_T]), matches=np.array(ms, np.int32).reshape(-1, 2),
                flags=np.array(flags, bool), next_lid=100, min_baseline=0.25)


def seventeen_views():
    """one match of 9 + 8 views on a rig of 16 cameras: beyond MCORB_MAX_CAMS, the solver's design limit"""
    rng = np.random.default_rng(2)
    Ks, rig_T = Mc.make_rig(16, rng)
    T = Mc.T4(np.eye(3), np.array([1.0, 0.0, 0.0]))
    prev, cur = Mc.FrameBuilder(Mc.frame_geometry(np.eye(4), rig_T), Ks), Mc.FrameBuilder(Mc.frame_geometry(T, rig_T), Ks)
    X = np.array([0.2, 0.1, 6.0])
    m = [(prev.add(X, list(range(9)), rng), cur.add(X, list(range(8, 16)), rng))]
    return dict(ncams=16, K=np.array(Ks), inv_sigma2=INV_SIGMA2, prev=prev.done(), cur=cur.done(), R=T[:3, :3].copy(), t=T[:3, 3].copy(),
                body=np.array([np.linalg.inv(M)[:3, 3] for M in rig_T]), matches=np.array(m, np.int32), flags=np.ones(1, bool), next_lid=100,
                min_baseline=0.25)


def cut(sc, n, every_third_clear=False):
    """the scene's first n matches, all flags set (or every third clear)"""
    flags = np.ones(n, bool)
    if every_third_clear:
        flags[2::3] = False
    return dict(sc, matches=sc["matches"][:n].copy(), flags=flags)


def run_scene(mc, lm, sc, **kw):
    return lm.initialize(Mc.to_frame(mc, sc["prev"]), sc["prev"]["lids"], Mc.to_frame(mc, sc["cur"]), sc["cur"]["lids"], sc["R"], sc["t"],
                         sc["body"], sc["matches"], sc["flags"], sc["K"], sc["inv_sigma2"], sc["next_lid"], sc["min_baseline"], **kw)


def ref_scene(sc):
    return IR.initialize(sc["prev"], sc["prev"]["lids"], sc["cur"], sc["cur"]["lids"], sc["R"], sc["t"], sc["body"], sc["matches"],
                         sc["flags"], sc["K"], sc["inv_sigma2"], sc["next_lid"], sc["min_baseline"])


# ---------------------------------------------------------------------------------------------------------------------------
# hand-built cases for mcorb_host_init_cases / mcorb_dev_init_cases_selftest: one match per case, K = I, prev's camera [I | 0]
# ---------------------------------------------------------------------------------------------------------------------------
I3 = np.eye(3)
C2 = (1.0, 0.0, 0.0)        # the current frame's camera centre in most cases
R_ID, T_X = np.eye(3), np.array([1.0, 0.0, 0.0])   # T of the hook calls: cur's body centre 0 then gives the world centre C2


def view(P, kp, centre, octave=0):
    P = np.asarray(P, float).reshape(3, 4)
    return dict(P=[[float(v) for v in row] for row in P], K=[[float(v) for v in row] for row in I3], centre=[float(v) for v in centre],
                kx=np.float32(kp[0]), ky=np.float32(kp[1]), octave=octave)


def exact_kp(P, X):
    p = np.asarray(P)[:, :3] @ np.asarray(X, float) + np.asarray(P)[:, 3]
    with np.errstate(all="ignore"):
        return (p[0] / p[2], p[1] / p[2])


def case(X, c2=C2, kp1=None, kp2=None, inv_sigma2=(1.0,)):
    """a two-view match: prev's camera at the origin, cur's at c2 (body centre 0 with T = [I | c2]); the keypoints are the
    projections rounded to float unless given"""
    P1, P2 = Mc.P_ID, Mc.P_at(c2)
    k1 = exact_kp(P1, X) if kp1 is None else kp1
    k2 = exact_kp(P2, X) if kp2 is None else kp2
    return dict(X=[float(v) for v in X], nv1=1, views=[view(P1, k1, (0, 0, 0)), view(P2, k2, (0, 0, 0))], inv_sigma2=inv_sigma2)


def solve(f, lo, hi, target):
    """x in [lo, hi] with f(x) == target exactly, f increasing up to rounding: bisection, then the neighbouring doubles"""
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(mid) < target:
            lo = mid
        else:
            hi = mid
    x = hi
    for _ in range(100):
        x = math.nextafter(x, -math.inf)
    for _ in range(4000):
        if f(x) == target:
            return x
        x = math.nextafter(x, math.inf)
    raise AssertionError("no double reaches the target")


def cos_of(x):
    return IR.gates(case((x, 0.0, 1.0))["views"], 1, (x, 0.0, 1.0), (1.0,))["cos"]


def case_cos(target):
    """a match whose cos is exactly `target`: X = (x, 0, 1) between x = 0.5 (cos 0.6) and far out along x (cos -> 1)"""
    x = solve(cos_of, 0.5, 1e6, target)
    return case((x, 0.0, 1.0))


def case_err(target):
    """a match whose first view has err * inv_sigma2 exactly `target`: keypoint (0, 0), X = (d, e, 1), err = d * d + e * e"""
    d = 2.447
    e = solve(lambda v: d * d + v * v, 0.0, 1.0, target)
    return case((d, e, 1.0), kp1=(0.0, 0.0))


def good_cases(n, seed=5, c2=C2):
    """n matches with cos in about 0.6 .. 0.99 and distinct depths"""
    rng = np.random.default_rng(seed)
    return [case((rng.uniform(-1, 2), rng.uniform(-1, 1), rng.uniform(1.0, 6.0)), c2=c2) for _ in range(n)]


def run_hook(mc, cases, flags=None, R=R_ID, t=T_X, ncams=4, min_baseline=0.25, device=None):
    sig = cases[0]["inv_sigma2"]
    assert all(tuple(c["inv_sigma2"]) == tuple(sig) for c in cases)
    flags = [True] * len(cases) if flags is None else flags
    vs = [v for c in cases for v in c["views"]]
    return mc.init_cases([c["X"] for c in cases], [c["nv1"] for c in cases], [len(c["views"]) for c in cases], [v["P"] for v in vs],
                         [v["K"] for v in vs], [v["centre"] for v in vs], [(v["kx"], v["ky"]) for v in vs], [v["octave"] for v in vs],
                         sig, ncams, R, t, min_baseline, flags, device=device)


def ref_hook(cases, flags=None, R=R_ID, t=T_X, ncams=4, min_baseline=0.25):
    flags = [True] * len(cases) if flags is None else flags
    return IR.run_cases(cases, flags, R, t, ncams, min_baseline)
