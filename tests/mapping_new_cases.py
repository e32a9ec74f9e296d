"""Inputs of the TriangulateNewLandmarks tests (test_mapping_new_cpu.py, test_gpu_mapping_new.py): a seeded scene of a current frame
and its previous keyframe whose matches end at every verdict, hand-built cases for the hooks (mcorb_host_map_refine /
mcorb_dev_map_refine_selftest), and the helpers that compare a result with the restatement (mapping_new_ref.py) bit for bit."""
import numpy as np

import mapping_cases as Mc
import mapping_new_ref as N

NLEVELS = Mc.NLEVELS
# ORB's table, 1 / 1.2^(2 level), for features located to SCALE px at level 0: the scene's keypoint noise grows with the level as
# the table assumes, so that coarse features carry residuals of many pixels, the DLT's point is more than 1.0 of cost away from the
# minimum for a share of the matches (the loop's absolute tolerance) and the refined point still passes the cull
SCALE = 16.0


def inv_sigma2(scale=SCALE):
    return (1.2 ** (-2.0 * np.arange(NLEVELS)) / scale ** 2).astype(np.float32)
KINDS = ["good"] * 40 + ["behind"] * 8 + ["chi2"] * 14 + ["far"] * 10 + ["preset"] * 8 + ["shared"] * 8


def jitter(fb, feat, rng, sigma, gross=None):
    """noise of sigma * 1.2^level on every view of a feature; gross: one view moves by that many sigmas instead"""
    cams = [c for c in range(fb.C) if fb.rows[feat][c] != -1]
    bad = cams[int(rng.integers(0, len(cams)))] if gross else None
    for c in cams:
        s = sigma * 1.2 ** fb.kps[c][fb.rows[feat][c]][2]
        if c == bad:
            a = rng.uniform(0, 2 * np.pi)
            fb.move(feat, c, gross * s * np.array([np.cos(a), np.sin(a)]))
        else:
            fb.move(feat, c, rng.normal(0.0, s, 2))


def scene(ncams, n=300, seed=1, scale=SCALE, baseline=1.0, depth=(3.0, 15.0)):
    """A current frame, its previous keyframe and n matches of these kinds in shuffled order: good (verdict 0), a point behind
    the cameras (3), one view moved by 8 .. 20 sigmas (4), a point 1500 away (5), a current feature with a landmark on entry (6)
    and a second match to the current feature of an earlier good match (6 through the walk)."""
    rng = np.random.default_rng(seed)
    sigma = 0.9 * scale
    Ks, rig_T = Mc.make_rig(ncams, rng)
    cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(*rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.05, 0.05, 3)), rig_T), Ks)
    prev = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(*rng.uniform(-0.08, 0.08, 3)),
                                                   np.array([baseline, 0.0, 0.0]) + rng.uniform(-0.05, 0.05, 3)), rig_T), Ks)
    mid = 0.5 * (prev.g["twc"] + cur.g["twc"])
    ms, good_trains = [], []
    for kind in rng.permutation([KINDS[(37 * i) % len(KINDS)] for i in range(n)]):
        if kind == "shared" and not good_trains:
            kind = "good"
        X = mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(*depth)])
        if kind == "behind":
            X = mid + np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), -rng.uniform(3, 15)])
        elif kind == "far":
            X = mid + np.array([rng.uniform(-200, 200), rng.uniform(-150, 150), 1500.0])
        if kind == "shared":
            t, X = good_trains[int(rng.integers(0, len(good_trains)))]
            q = prev.add(X, Mc.pick_cams(ncams, rng, False), rng)
            jitter(prev, q, rng, sigma)
            ms.append((q, t))
            continue
        q = prev.add(X, Mc.pick_cams(ncams, rng, False), rng)
        t = cur.add(X, Mc.pick_cams(ncams, rng, False), rng)
        jitter(prev, q, rng, 0.05 if kind in ("far", "behind") else sigma)
        jitter(cur, t, rng, 0.05 if kind in ("far", "behind") else sigma, gross=rng.uniform(8, 20) if kind == "chi2" else None)
        if kind == "preset":
            cur.lids[t] = 3900 + len(ms) % 90
        if kind == "good":
            good_trains.append((t, X))
        ms.append((q, t))
    return dict(ncams=ncams, K=np.array(Ks), inv_sigma2=inv_sigma2(scale), cur=cur.done(), prev=prev.done(),
                matches=np.array(ms, np.int32).reshape(-1, 2), next_lid=100)


def run_scene(mc, lm, sc, **kw):
    return lm.triangulate_new(Mc.to_frame(mc, sc["cur"]), sc["cur"]["lids"], Mc.to_frame(mc, sc["prev"]), sc["prev"]["lids"],
                              sc["matches"], sc["K"], sc["inv_sigma2"], sc["next_lid"], **kw)


def ref_of(mc, sc):
    return N.triangulate_new(mc, sc["cur"], sc["cur"]["lids"], sc["prev"], sc["prev"]["lids"], sc["matches"], sc["K"], sc["inv_sigma2"],
                             sc["next_lid"])


def dcat(values):
    return b"".join(N.dbits(v) for v in values)


def same_as_ref(got, want):
    """a NewLandmarksResult against the restatement's walk: every integer, and every double and float as raw bytes"""
    n = len(want["verdict"])
    recs = want["records"]
    assert got.verdict.tolist() == want["verdict"] and got.inliers.tolist() == want["inliers"] and got.new_lid.tolist() == want["new_lid"]
    assert got.lids_cur.tolist() == want["lids_cur"] and got.lids_prev.tolist() == want["lids_prev"]
    assert (got.next_lid, got.n_triangulated) == (want["next_lid"], len(want["depth_vec"]))
    assert got.n_by_verdict.tolist() == want["n_by_verdict"] and got.n_rays_hist.tolist() == want["n_rays_hist"]
    assert dcat(got.depth_vec) == dcat(want["depth_vec"]) and N.dbits(got.avg_depth) == N.dbits(want["avg_depth"])
    lm = [r["verdict"] == 0 for r in recs]
    ran = [r["verdict"] in (0, 4, 5) for r in recs]
    for i in range(n):
        r = recs[i]
        assert dcat(got.pt3d[i]) == dcat(r["X"] if lm[i] else [0.0] * 3), i
        assert dcat(got.normal[i]) == dcat(r["normal"]), i
        assert N.dbits(got.dist[i]) == N.dbits(r["dist"]) and N.fbits(got.cos_parallax[i]) == N.fbits(r["cos"]), i
        assert got.iterations[i] == (r["solves"] if ran[i] else 0), i
        assert N.dbits(got.cost_initial[i]) == N.dbits(r["cost_initial"]) and N.dbits(got.cost_final[i]) == N.dbits(r["cost_final"]), i


FIELDS = ("inliers", "verdict", "new_lid", "pt3d", "normal", "dist", "cos_parallax", "iterations", "cost_initial", "cost_final",
          "depth_vec", "n_rays_hist", "n_by_verdict", "lids_cur", "lids_prev")


def same(got, want, what=""):
    """two NewLandmarksResults (device store, host-only store) bit for bit"""
    for f in FIELDS:
        a, b = np.asarray(getattr(got, f)), np.asarray(getattr(want, f))
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, f)
    assert (got.n_triangulated, got.next_lid) == (want.n_triangulated, want.next_lid), what
    assert N.dbits(got.avg_depth) == N.dbits(want.avg_depth), what


# ---------------------------------------------------------------------------------------------------------------------------
# hand-built cases for the hooks: one match per case
# ---------------------------------------------------------------------------------------------------------------------------
I3 = np.eye(3)


def view(P, kp, K=I3, centre=(0.0, 0.0, 0.0), octave=0):
    return (np.asarray(P, float), np.asarray(K, float), np.asarray(centre, float), kp, octave)


def case(X0, views, nv1=1, twc_cur=(1.0, 0.0, 0.0), twc_prev=(0.0, 0.0, 0.0)):
    """views: view(...) per view; the first nv1 are the previous keyframe's"""
    return dict(X0=np.asarray(X0, float), nv1=nv1, nv=len(views), _views=views, P=[v[0] for v in views], K=[v[1] for v in views],
                centre=[v[2] for v in views], kps=[v[3] for v in views], octave=[v[4] for v in views],
                twc_cur=np.asarray(twc_cur, float), twc_prev=np.asarray(twc_prev, float))


def run_cases(mc, cases, inv_sigma2, device=None):
    """all cases in one call -> list of dict(verdict, n_rays, solves, cos, X, normal, dist, cost_initial, cost_final)"""
    cat = lambda key: np.concatenate([np.asarray(c[key], np.float64).reshape(c["nv"], -1) for c in cases])
    out = mc.map_refine([c["X0"] for c in cases], [c["nv1"] for c in cases], [c["nv"] for c in cases], cat("P"), cat("K"), cat("centre"),
                        np.concatenate([np.asarray(c["kps"], np.float32).reshape(-1, 2) for c in cases]),
                        np.concatenate([c["octave"] for c in cases]), [c["twc_cur"] for c in cases], [c["twc_prev"] for c in cases],
                        inv_sigma2, device=device)
    keys = ("verdict", "n_rays", "solves", "cos", "X", "normal", "dist", "cost_initial", "cost_final")
    return [dict(zip(keys, [o[i] for o in out])) for i in range(len(cases))]


def ref_case(c, inv_sigma2):
    views = [dict(kx=np.float32(c["kps"][i][0]), ky=np.float32(c["kps"][i][1]), octave=c["octave"][i], P=c["P"][i].reshape(3, 4).tolist(),
                  K=c["K"][i].reshape(3, 3).tolist(), centre=c["centre"][i].tolist()) for i in range(c["nv"])]
    return N.refine(views, c["nv1"], c["X0"], c["twc_cur"], c["twc_prev"], inv_sigma2)


def same_case(got, want, name=""):
    """a hook's result against the restatement's (or another hook's), bit for bit"""
    assert int(got["verdict"]) == int(want["verdict"]) and int(got["n_rays"]) == int(want["n_rays"]), (name, got, want)
    assert int(got["solves"]) == int(want["solves"]), (name, got, want)
    assert N.fbits(got["cos"]) == N.fbits(want["cos"]), (name, got, want)
    for k in ("X", "normal"):
        assert dcat(got[k]) == dcat(want[k]), (name, k, got, want)
    for k in ("dist", "cost_initial", "cost_final"):
        assert N.dbits(got[k]) == N.dbits(want[k]), (name, k, got, want)


P_ID = Mc.P_ID
SIGMA2 = (1.0, 0.5)          # the hooks' table: level 1 halves the error
INF, NAN = float("inf"), float("nan")
ULP_UP = lambda x: float(np.nextafter(x, np.inf))
ULP_DN = lambda x: float(np.nextafter(x, -np.inf))


def pair(z, **kw):
    """The same view entered twice with keypoints one pixel either side of the projection of X0 = (0, 0, z) (K = identity, the
    camera [I | 0]): opposite residuals and equal Jacobians, so g is exactly zero, every trial leaves X where it is, no trial
    is accepted, lambda passes 1e5 after 6 solves and the gates run at X0 itself"""
    return case((0.0, 0.0, z), [view(P_ID, (1.0, 0.0)), view(P_ID, (-1.0, 0.0))], **kw)


def stall(a, b):
    """a view whose p at X0 = (a, b, 1) is (0, 0, 1e-300): residual zero, a Jacobian that overflows, so every pivot test sees a
    NaN, every trial is rejected and the gates run at X0 itself.  (Not a rotation: the hook takes any 3 x 4 matrix.)"""
    return view([[1.0, 0, 0, -a], [0, 1.0, 0, -b], [0, 0, 1e-300, 0]], (0.0, 0.0))


def err_case(a, b, octave=0):
    """the first view's error at X0 = (a, b, 1) is a * a + b * b exactly (K = identity, [I | 0], keypoint (0, 0))"""
    return case((a, b, 1.0), [view(P_ID, (0.0, 0.0), octave=octave), stall(a, b)], twc_cur=(1.0, 0.0, 0.0))


def sum_of_squares(target):
    """a, b with fl(fl(a * a) + fl(b * b)) == target"""
    for i in range(1, 4000):
        a = 0.25 + i * 2.0 ** -12
        b0 = float(np.sqrt(target - a * a))
        for b in (b0, ULP_UP(b0), ULP_DN(b0)):
            if a * a + b * b == target:
                return a, b
    raise AssertionError("no pair found")


COS_HI = np.float32(0.99998)
if float(COS_HI) < 0.99998:
    COS_HI = np.nextafter(COS_HI, np.float32(2))
COS_LO = np.nextafter(COS_HI, np.float32(0))     # the two floats either side of the double 0.99998


def cos_case(u, z1=3.0):
    """X0 = (0, 0, z1) with prev->twc at the origin and X0 - cur->twc = (u, 0, 1): cos = z1 / (z1 * sqrt(u * u + 1))"""
    return pair(z1, twc_cur=(-u, 0.0, z1 - 1.0), twc_prev=(0.0, 0.0, 0.0))


def cos_search():
    """cases whose float cos is exactly COS_LO and COS_HI (found with the restatement's arithmetic)"""
    want = {COS_LO.tobytes(): None, COS_HI.tobytes(): None}
    u0 = float(np.sqrt(1.0 / (0.99998 * 0.99998) - 1.0))
    for i in range(-400, 401):
        c = cos_case(u0 * (1.0 + i * 2.5e-5))
        k = np.float32(ref_case(c, SIGMA2)["cos"]).tobytes()
        if k in want and want[k] is None:
            want[k] = c
    assert all(v is not None for v in want.values())
    return want[COS_LO.tobytes()], want[COS_HI.tobytes()]


def step_case(e, f=100.0):
    """two cameras one apart see (0, 0, 5) exactly; X0 is e off along x, so the first step's decrease is about cost_initial"""
    K = np.diag([f, f, 1.0])
    return case((e, 0.0, 5.0), [view(P_ID, (0.0, 0.0), K), view(Mc.P_at((1.0, 0, 0)), (np.float32(-f / 5.0), 0.0), K, (1.0, 0, 0))])


def decrease_search():
    """X0 offsets either side of the absolute tolerance: the largest e of a grid whose loop ends after its first solve (decrease
    <= 1.0) and the next one, whose loop goes on (decrease > 1.0)"""
    es = [0.04 + i * 2.0 ** -14 for i in range(400)]
    solves = [ref_case(step_case(e), SIGMA2)["solves"] for e in es]
    i = max(k for k in range(len(es) - 1) if solves[k] == 1 and solves[k + 1] > 1)
    return step_case(es[i]), step_case(es[i + 1])


# found by a seeded search with the restatement: 24 accepted steps down a long, curved valley, then rejected trials until the
# 50th solve
def fifty_case():
    K = np.diag([1000.0, 1000.0, 1.0])
    cs = [(-0.2842936555649995, 0.2598803104334012, -0.0458615127588039), (-0.08315162622211769, 0.2249217658153477, -0.0015579809230244707),
          (-0.4162888419290571, 0.283805332206701, 0.08068032437749875), (0.2713613442956185, 0.34169394945486947, 0.01452720431964318)]
    kp = [(876.0824584960938, -356.4366760253906), (734.0675659179688, -339.6713562011719), (1105.016357421875, -421.5101013183594),
          (429.97235107421875, -448.1341857910156)]
    X0 = [float.fromhex(h) for h in ("0x1.83048ba6e729fp-1", "-0x1.4e956f6c5b784p-3", "0x1.09c5fbb8430f6p+12")]
    return case(X0, [view(Mc.P_at(c), k, K, c) for c, k in zip(cs, kp)])


def driven_behind_case():
    """view A ([I | 0]) sees X0 = (0.05, 0, 0.01) at u = 5 and has its keypoint at 1000: the first step lands behind A, where A's
    residual is (2 fx, 2 fx) and its Jacobian zero; the step is accepted (the cost falls from about 5e5 to about 4), view B, ten
    behind A, keeps the point on its ray, and the cull ends the match at A with err = 8"""
    cB = (0.0, 0.0, -10.0)
    return case((0.05, 0.0, 0.01), [view(P_ID, (1000.0, 0.0)), view(Mc.P_at(cB), (np.float32(0.05 / 10.01), 0.0), I3, cB)])


def hook_cases():
    """(name, case, verdict by hand, solves by hand or None)"""
    rows = [("z 0.0", pair(0.0), 3, 0), ("z -0.0", pair(-0.0), 3, 0), ("z -1e-300", pair(-1e-300), 3, 0),
            # p.z = 1e-300 is in front: the Jacobian overflows, every trial is rejected; prev->twc is at the origin, so dist1 is 0.0f
            # and cos is 0 / 0: a NaN makes a landmark
            ("z 1e-300", pair(1e-300), 0, 6),
            # p.z = inf * 0 + 2: a NaN is not behind; every cost is NaN, nothing is accepted, a NaN error passes the cull
            ("z nan", case((0.0, 0.0, 2.0), [view([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [INF, 0, 1.0, 0]], (1.0, 0.0)), view(P_ID, (-1.0, 0.0))]), 0, 6),
            ("X0 inf", case((0.0, INF, 2.0), pair(2.0)["_views"]), 8, 0), ("X0 nan", case((NAN, 0.0, 2.0), pair(2.0)["_views"]), 8, 0),
            ("g zero", pair(2.0), 0, 6)]
    for name, t, v in (("err 5.991", 5.991, 0), ("err below", ULP_DN(5.991), 0), ("err above", ULP_UP(5.991), 4)):
        rows.append((name, err_case(*sum_of_squares(t)), v, 6))
    rows.append(("err 5.991 at 0.5", err_case(*sum_of_squares(2 * 5.991), octave=1), 0, 6))
    rows.append(("err above at 0.5", err_case(*sum_of_squares(2 * ULP_UP(5.991)), octave=1), 4, 6))
    lo, hi = cos_search()
    rows += [("cos below 0.99998", lo, 0, 6), ("cos at or above 0.99998", hi, 5, 6)]
    rows.append(("cos nan", pair(2.0, twc_cur=(0.0, 0.0, 2.0), twc_prev=(0.0, 0.0, -1.0)), 0, 6))
    below, above = decrease_search()
    rows += [("decrease <= 1.0", below, 0, 1), ("decrease > 1.0", above, 0, None)]
    rows.append(("50 solves", fifty_case(), 4, 50))
    rows.append(("driven behind a camera", driven_behind_case(), 4, None))
    return rows
