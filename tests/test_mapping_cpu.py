"""The mapping step on the host-only store (device -1): mcorb_lmap_triangulate_neighbours and the gates hook mcorb_host_map_gates
against the plain-Python restatement (mapping_ref.py) and hand-derived values.  No GPU."""
import math

import importlib.util
import os
import subprocess

import numpy as np
import pytest

import kfdb_cases as K
import mapping_cases as Mc
import mapping_ref as R

I3 = np.eye(3)
ULP_UP = lambda x: float(np.nextafter(x, np.inf))
ULP_DN = lambda x: float(np.nextafter(x, -np.inf))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


def store(mc, voc, device=-1, max_landmarks=4096):
    return mc.LocalMap(voc, device=device, max_landmarks=max_landmarks, max_candidates=16)


# ---------------------------------------------------------------------------------------------------------------------------
# the gates at exact boundaries, one match per case
# ---------------------------------------------------------------------------------------------------------------------------
GATE_SIGMA2 = (1.0, 0.5)


def two_views(X, kp1, kp2, c2=(1.0, 0.0, 0.0), F=Mc.F_PASS, octave=0):
    """K = identity, the neighbour's camera [I | 0] at the origin (its keypoint at level `octave` of GATE_SIGMA2), the current
    frame's at c2 looking along +z"""
    return Mc.gate_case(X, [(Mc.P_ID, I3, (0, 0, 0), kp1, octave), (Mc.P_at(c2), I3, c2, kp2, 0)], 1, F, GATE_SIGMA2)


def ref_gate(c):
    """the restatement on a gate case -> (verdict, n_rays, dist2, cos, normal)"""
    views = [dict(cam=0, kx=np.float32(c["kps"][i][0]), ky=np.float32(c["kps"][i][1]), octave=c["octave"][i], P=c["P"][i].tolist(),
                  K=c["K"][i].tolist(), centre=c["centre"][i].tolist()) for i in range(c["nv"])]
    v, _ = R.epipolar(views[0], views[c["nv1"]], c["F"])
    if v:
        return v, 0, 0.0, 0.0, [0.0] * 3
    r = R.after(views, c["nv1"], [float(x) for x in c["X"]], c["inv_sigma2"])
    return r["verdict"], r["n_rays"], r["dist2"], r["cos"], r["normal"]


def bits(x):
    return np.asarray(x, np.float64).tobytes()


def default_nan(x):
    """the restatement's value as the record holds it: a NaN leaves the library as the default quiet NaN, whatever sign the
    operation that made it gave it (the host and the device give different ones)"""
    x = np.array(x, np.float64)
    x[np.isnan(x)] = np.frombuffer(np.array([0x7ff8000000000000], np.uint64).tobytes(), np.float64)[0]
    return x


def same_gate(got, want, name=""):
    assert got[0] == want[0] and got[1] == want[1], (name, got, want)
    assert bits(got[2]) == bits(default_nan(want[2])) and bits(got[3]) == bits(default_nan(want[3])) and \
        bits(got[4]) == bits(default_nan(want[4])), (name, got, want)


def sum_of_squares(target):
    """a, b with fl(fl(a * a) + fl(b * b)) == target"""
    for i in range(1, 4000):
        a = 0.25 + i * 2.0 ** -12
        b0 = math.sqrt(target - a * a)
        for b in (b0, ULP_UP(b0), ULP_DN(b0)):
            if a * a + b * b == target:
                return a, b
    raise AssertionError("no pair found")


def cos_case(u, z1=3.0):
    """X = (0, 0, z1) seen from the origin and from a camera with X - o2 = (u, 0, 1): cos = z1 / (z1 * sqrt(u * u + 1))"""
    c2 = (-u, 0.0, z1 - 1.0)
    return two_views((0.0, 0.0, z1), (0.0, 0.0), (np.float32(u), 0.0), c2)


def cos_search(target):
    """cases whose cos is exactly target - 1 ulp, target, target + 1 ulp (found with the restatement's arithmetic)"""
    want = {ULP_DN(target): None, target: None, ULP_UP(target): None}
    for z1 in (3.0, 5.0, 7.0, 1.75, 2.5, 11.0):
        u = math.sqrt(1.0 / (target * target) - 1.0)
        du = max((ULP_UP(target) - target) / (8 * u / (1 + u * u) ** 1.5), ULP_UP(u) - u)   # an eighth of an ulp of cos per step
        for i in range(-60, 61):
            c = cos_case(u + i * du, z1)
            cs = ref_gate(c)[3]
            if cs in want and want[cs] is None:
                want[cs] = c
        if all(v is not None for v in want.values()):
            return [want[k] for k in sorted(want)]
    raise AssertionError("no boundary case found for %r" % target)


def gate_cases():
    """(name, case, verdict by hand)"""
    rows = []
    two = np.float32(2.0)
    X2 = (0.5, 4.0, 2.0)    # both views see it at y = 2 exactly
    rows.append(("epi y2 = 2.0f", two_views(X2, (0.25, 2.0), (-0.25, two)), 2))
    rows.append(("epi y2 below 2", two_views(X2, (0.25, 2.0), (-0.25, np.nextafter(two, np.float32(0)))), 0))
    rows.append(("epi F = 0", two_views(X2, (0.25, 2.0), (-0.25, 2.0), F=np.zeros((3, 3))), 1))
    # p.z: the first view's p is X itself.  z = +-0.0 is not behind (a sum from 0.0 is never -0.0): ex = 0 / 0 is NaN and passes,
    # the second view's p = (-1, 0, 0) gives ex = -inf but ey = 0 / 0, err = inf + NaN passes too, and X = o1 makes cos NaN: an
    # inlier without a landmark; -1e-300 is behind; 1e-300: the second view's ex = -1e300, ey = 0, err = inf; NaN: every err is
    # NaN and passes, cos is NaN
    for name, z, v in (("z -0.0", -0.0, 5), ("z 0.0", 0.0, 5), ("z -1e-300", -1e-300, 3), ("z 1e-300", 1e-300, 4), ("z nan", float("nan"), 5)):
        rows.append((name, two_views((0.0, 0.0, z), (0.0, 0.0), (0.0, 0.0)), v))
    # err * invSigma2 on the first view: K = identity, P = [I | 0], Z = 1, kp = (0, 0): err = a * a + b * b (the epipolar line
    # is y = y2 here, so that gate passes)
    line = lambda b: [[0, 0, 0], [0, 0, 1], [0, 0, -float(np.float32(b))]]
    for name, t, v in (("err 5.991", 5.991, 0), ("err below", ULP_DN(5.991), 0), ("err above", ULP_UP(5.991), 4)):
        a, b = sum_of_squares(t)
        rows.append((name, two_views((a, b, 1.0), (0.0, 0.0), (np.float32(a - 1.0), np.float32(b)), F=line(b)), v))
    # with invSigma2 = 0.5 (a float promoted): twice the threshold is the boundary
    a, b = sum_of_squares(2 * 5.991)
    rows.append(("err 5.991 at 0.5", two_views((a, b, 1.0), (0.0, 0.0), (np.float32(a - 1.0), np.float32(b)), F=line(b), octave=1), 0))
    a, b = sum_of_squares(2 * ULP_UP(5.991))
    rows.append(("err above at 0.5", two_views((a, b, 1.0), (0.0, 0.0), (np.float32(a - 1.0), np.float32(b)), F=line(b), octave=1), 4))
    for t, vs in ((0.5, (5, 5, 0)), (0.99998, (0, 5, 5))):
        for c, v, nm in zip(cos_search(t), vs, ("below", "equal", "above")):
            rows.append(("cos %r %s" % (t, nm), c, v))
    # X coincides with o1; the second camera sits behind it on the axis: every reject gate passes (the first view's err is NaN),
    # cos = 0 / 0: an inlier that makes no landmark
    rows.append(("cos nan", two_views((0.0, 0.0, 0.0), (0.0, 0.0), (0.0, 0.0), c2=(0.0, 0.0, -1.0)), 5))
    # every reject gate passes, the point is 1e6 away: outside the window
    rows.append(("far point", two_views((0.0, 0.0, 1e6), (0.0, 0.0), (np.float32(-1e-6), 0.0)), 5))
    return rows


def test_gates_at_their_boundaries(mc):
    rows = gate_cases()
    assert len(rows) == 21
    got = Mc.run_gates(mc, [r[1] for r in rows])
    for (name, c, v), g in zip(rows, got):
        assert g[0] == v, (name, g)
        same_gate(g, ref_gate(c), name)
    by = {r[0]: Mc.run_gates(mc, [r[1]])[0] for r in rows if r[0].startswith("cos") or r[0] == "far point"}
    assert by["cos 0.5 equal"][3] == 0.5 and by["cos 0.5 above"][3] == ULP_UP(0.5) and by["cos 0.5 below"][3] == ULP_DN(0.5)
    assert by["cos 0.99998 equal"][3] == 0.99998 and by["cos 0.99998 below"][3] == ULP_DN(0.99998)
    assert math.isnan(by["cos nan"][3]) and by["far point"][3] > 0.99998


def test_gate_hook_arguments(mc):
    c = two_views((0.5, 0.0, 2.0), (0.25, 0.0), (-0.25, 0.0))
    for bad in (dict(nv1=0), dict(nv1=2), dict(octave=[0, 2]), dict(octave=[-1, 0])):
        with pytest.raises(mc.McorbError) as ei:
            Mc.run_gates(mc, [dict(c, **bad)])
        assert ei.value.code == mc.E_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# the normal of the new landmark
# ---------------------------------------------------------------------------------------------------------------------------
def normal_case(centres1, centres2):
    """X = (0, 0, 2); every neighbour view is the camera at the origin, every current view the camera at (1, 0, 0) (so that all
    gates pass), with the camera centres of updateNormal given separately"""
    v1 = [(Mc.P_ID, I3, c, (0.0, 0.0), 0) for c in centres1]
    v2 = [(Mc.P_at((1, 0, 0)), I3, c, (-0.5, 0.0), 0) for c in centres2]
    return Mc.gate_case((0.0, 0.0, 2.0), v1 + v2, len(v1), inv_sigma2=GATE_SIGMA2)


def ray(c):
    """(X - c) * (1 / |X - c|) for X = (0, 0, 2)"""
    d = [0.0 - c[0], 0.0 - c[1], 2.0 - c[2]]
    inv = 1.0 / math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return [d[0] * inv, d[1] * inv, d[2] * inv]


def test_normal_of_a_new_landmark(mc):
    # 1 + 1: X - c1 = (0, 0, 3), X - c2 = (-3, 0, 4) of length 5.  -3 * (1 / 5) is -0.6000000000000001 where -3 / 5 is -0.6
    got = Mc.run_gates(mc, [normal_case([(0, 0, -1)], [(3, 0, -2)])])[0]
    assert got[0] == 0 and got[1] == 2
    assert 3 * (1.0 / 5) != 3 / 5
    first = [0.0, 0.0, (0.0 + 3 * (1.0 / 3)) * (1.0 / 1)]
    want = [(first[0] * 1.0 + (0.0 + -3 * (1.0 / 5))) * (1.0 / 2), 0.0, (first[2] * 1.0 + (0.0 + 4 * (1.0 / 5))) * (1.0 / 2)]
    assert want[0] == -0.30000000000000004 and want[0] != -0.3 and want[2] == 0.9
    assert got[4].tolist() == want
    # 2 + 1 and 4 + 4: rays summed in view order, / n_rays as a multiplication by the reciprocal, then (normal * n_rays + rays') and
    # the reciprocal of the new count
    for c1, c2 in (([(0, 0, -1), (3, 0, -2)], [(0, 4, -1)]),
                   ([(0, 0, -1), (3, 0, -2), (0, 4, -1), (1, 2, 0)], [(-3, 0, -2), (0, -4, -1), (2, 1, 0), (6, 0, -6)])):
        got = Mc.run_gates(mc, [normal_case(c1, c2)])[0]
        acc = [0.0] * 3
        for c in c1:
            acc = [acc[k] + ray(c)[k] for k in range(3)]
        n = len(c1)
        normal = [a * (1.0 / n) for a in acc]
        acc = [0.0] * 3
        for c in c2:
            acc = [acc[k] + ray(c)[k] for k in range(3)]
        normal = [normal[k] * float(n) + acc[k] for k in range(3)]
        n += len(c2)
        normal = [v * (1.0 / n) for v in normal]
        assert got[0] == 0 and got[1] == n and got[4].tolist() == normal
    with_division = [(0.0 + (-3 / 5)) / 2, 0.0, (1.0 + 4 / 5) / 2]
    assert with_division != want


# ---------------------------------------------------------------------------------------------------------------------------
# the walk and the neighbour gate on small hand-built scenes
# ---------------------------------------------------------------------------------------------------------------------------
class Mini:
    """a 1-camera rig: the current frame at the origin, neighbours at x = +-1, points a few units in front; every neighbour has
    one landmark of the store (lid 900 + s) at depth 5"""

    def __init__(self, n_neigh=1, old=True):
        self.rng = np.random.default_rng(5)
        self.Ks, self.rigT = Mc.make_rig(1, self.rng)
        self.cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(I3, np.zeros(3)), self.rigT), self.Ks)
        self.neigh = [Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(0.01, 0.02 * (s + 1), 0), np.array([(-1.0) ** s * (1 + s), 0.1, 0])), self.rigT),
                                      self.Ks) for s in range(n_neigh)]
        self.store = {}
        if old:
            for s, fb in enumerate(self.neigh):
                fb.add(np.array([0.0, 0.0, 5.0]), [0], self.rng, lid=900 + s)
                self.store[900 + s] = np.array([0.0, 0.0, 5.0])

    def point(self, i):
        return np.array([0.3 * i - 0.5, 0.2 * i, 4.0 + i])

    def scene(self, matches, next_lid=10):
        cur = self.cur.done()
        neigh = [fb.done() for fb in self.neigh]
        F = [np.array([[Mc.fundamental(self.cur.g["full"][0], fb.g["full"][0], self.Ks[0], self.Ks[0])]]) for fb in self.neigh]
        return dict(ncams=1, K=np.array(self.Ks), inv_sigma2=Mc.INV_SIGMA2, cur=cur, neigh=neigh, F21=F, store=self.store,
                    matches=[np.array(m, np.int32).reshape(-1, 2) for m in matches], Rcw=I3, tcw=np.zeros(3), next_lid=next_lid)


def run(mc, voc, sc, **kw):
    lm = store(mc, voc, max_landmarks=kw.pop("max_landmarks", 4096))
    Mc.fill_store(lm, sc["store"])
    return lm, Mc.run_scene(mc, lm, sc, **kw)


def ref_of(sc):
    return R.triangulate_neighbours(sc["store"], sc["cur"], sc["cur"]["lids"], sc["neigh"], [f["lids"] for f in sc["neigh"]], sc["F21"],
                                    sc["matches"], sc["K"], sc["inv_sigma2"], sc["Rcw"], sc["tcw"], sc["next_lid"])


def test_walk_shared_train_and_query(mc, voc):
    m = Mini()
    n, c = m.neigh[0], m.cur
    q0, q1 = n.add(m.point(0), [0], m.rng), n.add(m.point(0), [0], m.rng)        # two neighbour features of one point
    t0, t1 = c.add(m.point(0), [0], m.rng), c.add(m.point(0), [0], m.rng)
    qbad = n.add(m.point(3), [0], m.rng)                                          # another point: fails the epipolar gate against t0
    _, got = run(mc, voc, m.scene([[(q0, t0), (q1, t0)]]))
    assert got.verdict.tolist() == [0, 6] and got.inliers.tolist() == [True, False] and got.new_lid.tolist() == [10, -1]
    assert got.lids_cur[t0] == 10 and got.lids_neigh[0][q0] == 10 and got.lids_neigh[0][q1] == -1
    _, got = run(mc, voc, m.scene([[(qbad, t0), (q1, t0)]]))                      # a rejected match blocks nothing
    assert got.verdict.tolist() == [2, 0] and got.new_lid.tolist() == [-1, 10]
    _, got = run(mc, voc, m.scene([[(q0, t0), (q0, t1)]]))                        # a shared queryIdx
    assert got.verdict.tolist() == [0, 6] and got.lids_cur[t1] == -1 and got.n_triangulated == 1 and got.next_lid == 11


def test_walk_across_neighbours_ids_and_depth_order(mc, voc):
    m = Mini(n_neigh=2)
    qs = [[fb.add(m.point(i), [0], m.rng) for i in range(4)] for fb in m.neigh]
    ts = [m.cur.add(m.point(i), [0], m.rng) for i in range(4)]
    m.neigh[1].lids[qs[1][3]] = 901                                               # an id set on entry (the neighbour's own landmark)
    m.cur.lids[ts[2]] = 77                                                        # and one in the current frame
    sc = m.scene([[(qs[0][1], ts[1]), (qs[0][2], ts[2]), (qs[0][0], ts[0])], [(qs[1][0], ts[0]), (qs[1][3], ts[3]), (qs[1][3], ts[3])]], next_lid=40)
    lm, got = run(mc, voc, sc)
    #                                 accepted  cur preset  accepted | lids_cur carried over  neighbour preset (twice)
    assert got.verdict.tolist() == [0, 6, 0, 6, 6, 6]
    assert got.new_lid.tolist() == [40, -1, 41, -1, -1, -1] and got.next_lid == 42 and got.n_triangulated == 2
    assert got.lids_cur[ts[1]] == 40 and got.lids_cur[ts[0]] == 41 and got.lids_cur[ts[2]] == 77 and got.lids_cur[ts[3]] == -1
    assert got.depth_vec.tolist() == [got.dist2[0], got.dist2[2]] and got.dist2[0] != got.dist2[2]
    want = ref_of(sc)
    assert want["verdict"] == got.verdict.tolist() and want["new_lid"] == got.new_lid.tolist()
    for lid in (40, 41):                                                          # stored as returned
        p, q, d, _ = lm.get(lid)
        i = got.new_lid.tolist().index(lid)
        assert bits(p) == bits(got.pt3d[i]) and bits(q) == bits(got.normal[i]) and d is None
    with pytest.raises(mc.McorbError):
        lm.get(42)


def test_parallax_failure_is_an_inlier_without_a_landmark(mc, voc):
    m = Mini()
    far = np.array([10.0, -5.0, 2000.0])
    q, t = m.neigh[0].add(far, [0], m.rng), m.cur.add(far, [0], m.rng)
    lm, got = run(mc, voc, m.scene([[(q, t)]]))
    assert got.verdict.tolist() == [5] and got.inliers.tolist() == [True] and got.new_lid.tolist() == [-1] and got.n_triangulated == 0
    assert got.cos_parallax[0] > 0.99998 and got.lids_cur[t] == -1 and len(got.depth_vec) == 0 and not got.pt3d.any()


def gate_scene(zs, baseline=1.0):
    m = Mini(old=False)
    m.neigh[0].g["twc"] = np.array([baseline, 0.0, 0.0])      # the gate reads twc alone
    m.cur.g["twc"] = np.zeros(3)
    for i, z in enumerate(zs):
        m.neigh[0].add(np.array([0.0, 0.0, 5.0]), [0], m.rng, lid=900 + i)
        m.store[900 + i] = np.array([0.1 * i, -0.2, z])
    q, t = m.neigh[0].add(m.point(1), [0], m.rng), m.cur.add(m.point(1), [0], m.rng)
    return m.scene([[(q, t)]])


def test_neighbour_baseline_gate(mc, voc):
    up, dn = ULP_UP(100.0), ULP_DN(100.0)
    assert not 1.0 / 100.0 < 0.01 and 1.0 / up < 0.01 and not 1.0 / dn < 0.01
    #                   ratio == 0.01   below    above    even count: element (4 - 1) / 2 = 1             odd count
    for zs, skip in (([100.0], 0), ([up], 1), ([dn], 0), ([400.0, 90.0, 50.0, 110.0], 0), ([50.0, 400.0, 110.0, 120.0], 1),
                     ([110.0, 50.0, 90.0], 0), ([400.0, 90.0, 110.0], 1), ([], 2)):
        sc = gate_scene(zs)
        _, got = run(mc, voc, sc)
        assert got.neigh_skipped.tolist() == [skip] == ref_of(sc)["skipped"], zs
        assert got.verdict.tolist() == ([7] if skip else [0]) and got.inliers.tolist() == [not skip], zs


# ---------------------------------------------------------------------------------------------------------------------------
# errors and empty calls
# ---------------------------------------------------------------------------------------------------------------------------
def expect(mc, code, fn):
    with pytest.raises(mc.McorbError) as ei:
        fn()
    assert ei.value.code == code, ei.value


def good_mini(n=3):
    m = Mini()
    ms = [(m.neigh[0].add(m.point(i), [0], m.rng), m.cur.add(m.point(i), [0], m.rng)) for i in range(n)]
    return m, ms


def test_caps(mc, voc):
    m, ms = good_mini()
    sc = m.scene([ms], next_lid=20)
    lm = store(mc, voc, max_landmarks=1024)
    Mc.fill_store(lm, sc["store"])
    expect(mc, mc.E_CAP, lambda: Mc.run_scene(mc, lm, sc, caps=(2, 3)))           # per-match outputs short
    assert lm.map_out.n_matches == 3
    expect(mc, mc.E_CAP, lambda: Mc.run_scene(mc, lm, sc, caps=(3, 2)))           # depth_vec short: counts set, nothing stored
    assert (lm.map_out.n_matches, lm.map_out.n_depth, lm.map_out.n_triangulated, lm.map_out.next_lid) == (3, 3, 3, 20)
    expect(mc, mc.E_STATE, lambda: lm.get(20))
    sc["next_lid"] = 1022                                                          # ids 1022, 1023, 1024: one beyond the store
    expect(mc, mc.E_CAP, lambda: Mc.run_scene(mc, lm, sc))
    expect(mc, mc.E_STATE, lambda: lm.get(1022))
    sc["next_lid"] = 1021
    assert Mc.run_scene(mc, lm, sc).new_lid.tolist() == [1021, 1022, 1023]
    assert lm.get(1023)[2] is None


def test_bad_arguments(mc, voc):
    def attempt(change, code=None):
        m, ms = good_mini()
        sc = m.scene([ms])
        change(sc)
        lm = store(mc, voc)
        Mc.fill_store(lm, sc["store"])
        expect(mc, code or mc.E_ARG, lambda: Mc.run_scene(mc, lm, sc))
        expect(mc, mc.E_STATE, lambda: lm.get(10))                                 # nothing ran

    attempt(lambda sc: sc["matches"][0].__setitem__((0, 0), len(sc["neigh"][0]["lids"])))     # queryIdx outside the neighbour
    attempt(lambda sc: sc["matches"][0].__setitem__((1, 1), -1))                               # trainIdx outside the frame
    attempt(lambda sc: sc["neigh"][0]["match_index"].__setitem__((2, 0), len(sc["neigh"][0]["kps"][0])))   # keypoint outside a camera
    attempt(lambda sc: sc["cur"]["match_index"].__setitem__((0, 0), -2))
    attempt(lambda sc: sc["cur"]["match_index"].__setitem__((1, 0), -1))                       # a matched feature without a view
    attempt(lambda sc: sc["cur"]["kps"][0]["octave"].__setitem__(0, Mc.NLEVELS))               # octave outside nlevels
    attempt(lambda sc: sc["neigh"][0]["kps"][0]["octave"].__setitem__(1, -1))
    attempt(lambda sc: sc["cur"]["lids"].__setitem__(0, 4096))                                 # ids outside the store
    attempt(lambda sc: sc["neigh"][0]["lids"].__setitem__(1, -2))
    attempt(lambda sc: sc["store"].pop(900), mc.E_STATE)                                       # a neighbour's landmark never set
    attempt(lambda sc: sc.__setitem__("next_lid", -1))

    def two_cams(sc):                                                                          # a neighbour of another rig
        f = sc["neigh"][0]
        f["match_index"] = np.concatenate([f["match_index"], f["match_index"]], axis=1)
        for k in ("kps", "centre_w", "proj"):
            f[k] = list(f[k]) * 2
    m, ms = good_mini()
    sc = m.scene([ms])
    two_cams(sc)
    lm = store(mc, voc)
    Mc.fill_store(lm, sc["store"])
    expect(mc, mc.E_ARG, lambda: Mc.run_scene(mc, lm, sc))


def test_more_than_max_cams_views(mc, voc):
    """9 + 8 views: beyond the solver's design limit; 8 + 8 is the most a match may have"""
    rng = np.random.default_rng(2)
    Ks, rigT = Mc.make_rig(16, rng)
    cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(I3, np.zeros(3)), rigT), Ks)
    nb = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(I3, np.array([1.0, 0, 0])), rigT), Ks)
    X = np.array([0.2, 0.1, 6.0])
    nb.add(X, [0], rng, lid=900)
    q9, q8, t8 = nb.add(X, list(range(9)), rng), nb.add(X, list(range(8)), rng), cur.add(X, list(range(8, 16)), rng)
    F = np.array([[Mc.fundamental(cur.g["full"][cc], nb.g["full"][cn], Ks[cc], Ks[cn]) for cn in range(16)] for cc in range(16)])
    sc = dict(K=np.array(Ks), inv_sigma2=Mc.INV_SIGMA2, cur=cur.done(), neigh=[nb.done()], F21=[F], store={900: X},
              matches=[np.array([(q8, t8), (q9, t8)], np.int32)], Rcw=I3, tcw=np.zeros(3), next_lid=0)
    lm = store(mc, voc)
    Mc.fill_store(lm, sc["store"])
    expect(mc, mc.E_ARG, lambda: Mc.run_scene(mc, lm, sc))
    assert "MCORB_MAX_CAMS" in str(mc._lib.load().mcorb_last_error())
    sc["matches"] = [np.array([(q8, t8)], np.int32)]
    got = Mc.run_scene(mc, lm, sc)
    want = ref_of(sc)
    assert got.verdict.tolist() == [0] == want["verdict"]
    assert np.allclose(got.pt3d[0], X, rtol=1e-6) and np.abs(got.pt3d[0] - want["pt3d"][0]).max() <= 1e-9 * np.abs(X).max()


def test_no_neighbours_and_no_matches(mc, voc):
    m, ms = good_mini()
    sc = m.scene([ms])
    lm = store(mc, voc)
    Mc.fill_store(lm, sc["store"])
    got = lm.triangulate_neighbours(Mc.to_frame(mc, sc["cur"]), sc["cur"]["lids"], [], [], [], [], sc["K"], sc["inv_sigma2"], I3, np.zeros(3), 5)
    assert len(got.verdict) == 0 and got.n_triangulated == 0 and got.next_lid == 5 and len(got.depth_vec) == 0
    sc["matches"] = [np.zeros((0, 2), np.int32)]
    got = Mc.run_scene(mc, lm, sc)
    assert len(got.verdict) == 0 and got.neigh_skipped.tolist() == [0] and got.next_lid == sc["next_lid"]


# ---------------------------------------------------------------------------------------------------------------------------
# the seeded random scene against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def same_as_ref(got, want, n):
    """verdicts, inliers, ids and orders equal; pt3d, normal and depth_vec to 1e-9 relative (the triangulation's contract against
    an SVD).  Only a match with a gate quantity within 1e-6 relative of its threshold may differ in its verdict: at most 1 %"""
    near = np.array(want["near"])
    assert near.sum() <= n // 100, near.sum()
    wv = np.array(want["verdict"])
    assert np.array_equal(got.verdict[~near], wv[~near])
    if not np.array_equal(got.verdict, wv):      # a borderline match went the other way: the walk behind it differs by design
        return near.sum()
    assert got.inliers.tolist() == want["inliers"] and got.new_lid.tolist() == want["new_lid"]
    assert got.lids_cur.tolist() == want["lids_cur"] and [l.tolist() for l in got.lids_neigh] == want["lids_neigh"]
    assert got.neigh_skipped.tolist() == want["skipped"] and got.next_lid == want["next_lid"] and got.n_triangulated == len(want["depth_vec"])
    p, q, d = np.array(want["pt3d"]), np.array(want["normal"]), np.array(want["depth_vec"])
    sel = wv == 0
    assert not got.pt3d[~sel].any() and not got.normal[~sel].any()
    assert (np.abs(got.pt3d[sel] - p[sel]).max(axis=1) <= 1e-9 * np.abs(p[sel]).max(axis=1)).all()
    assert np.abs(got.normal[sel] - q[sel]).max() <= 1e-9          # unit-length scale
    assert (np.abs(got.depth_vec - d) <= 1e-9 * d).all() and np.array_equal(got.depth_vec, got.dist2[sel])
    return near.sum()


@pytest.mark.parametrize("ncams", [1, 4, 8])
def test_random_scene(mc, voc, ncams):
    sc = Mc.scene(ncams)
    assert len(sc["neigh"]) == 3
    want = ref_of(sc)
    wv = np.array(want["verdict"])
    n = len(wv)
    frac = [(wv == k).mean() for k in range(7)]
    assert min(frac) >= 0.05 and frac[0] >= 0.20, frac               # the restatement alone: every verdict is well represented
    lm, got = run(mc, voc, sc)
    same_as_ref(got, want, n)
    assert got.inliers[wv == 5].all() and (got.new_lid[wv == 5] == -1).all()
    for lid, (X, nrm) in list(want["new"].items())[::23]:
        p, q, _, _ = lm.get(lid)
        i = got.new_lid.tolist().index(lid)
        assert bits(p) == bits(got.pt3d[i]) and bits(q) == bits(got.normal[i])
    if ncams > 1:                                                     # views of 2 .. 16 in total were triangulated
        nv = [(sc["neigh"][s]["match_index"][q] != -1).sum() + (sc["cur"]["match_index"][t] != -1).sum()
              for s in range(3) for q, t in sc["matches"][s]]
        assert len(set(np.array(nv)[wv == 0].tolist())) >= 4


# ---------------------------------------------------------------------------------------------------------------------------
# the header under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_under_asan_ubsan(mc, voc, tmp_path):
    """tests/cpp/test_mapping_sanitize.cpp (its own main, -fsanitize=address,undefined) runs map_depth, the baseline gate and the
    walk through map_item on the seeded 4-camera scene, on the same scene with one neighbour at the current frame's centre
    (skipped) and on the 8-camera one (more than 4 views): no report, and its records -- verdicts, ids, dist2, cos, points,
    normals, skip flags -- equal the library's on the bytes"""
    spec = importlib.util.spec_from_file_location("header_coverage", os.path.join(ROOT, "scripts", "header_coverage.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    exe = str(tmp_path / "test_mapping_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_mapping_sanitize.cpp"),
                           "-o", exe])
    still = Mc.scene(4, sizes=(60, 0, 97, 50, 50), seed=11, zero_f=None)
    still["neigh"][3]["twc"] = still["cur"]["twc"].copy()
    for what, sc in (("4 cameras", Mc.scene(4)), ("a skipped neighbour", still), ("8 cameras", Mc.scene(8))):
        (tmp_path / "in.bin").write_bytes(H.blob_neigh(sc))
        out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "bad=0" in out.stdout and not out.stderr, (what, out.stdout + out.stderr)
        lm, got = run(mc, voc, sc)
        want = got.verdict.astype(np.int32).tobytes() + got.new_lid.astype(np.int32).tobytes() + bits(got.dist2) + bits(got.cos_parallax) + \
            bits(got.pt3d) + bits(got.normal) + got.neigh_skipped.astype(np.uint8).tobytes()
        assert (tmp_path / "out.bin").read_bytes() == want, what
        assert (got.verdict == 0).sum() > 20, what
