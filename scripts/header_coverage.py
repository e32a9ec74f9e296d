#!/usr/bin/env python3
"""Which branch outcomes of the shared pose headers (csrc/mcorb_sac.h, mcorb_rel.h, mcorb_align.h, mcorb_ess.h) a set of inputs
takes, CPU only.  The five stand-alone serial programs of tests/cpp (test_sac_sanitize.cpp, test_sac_rig_sanitize.cpp,
test_rel_sanitize.cpp, test_align_sanitize.cpp, test_ess_sanitize.cpp) are built with

    g++ -O0 --coverage -std=c++17 -ffp-contract=off -I mc-slam_amd/csrc

-- no sanitizer, nothing loaded into python, nothing preloaded -- into a temporary directory, fed input files in the format each
program's header comment documents, and read with `gcov -b -c`.  An outcome is named by the text of its source line, the
occurrence of that text in the header (0 unless two lines read the same) and gcov's index of the outcome on the line: a line
number would move with every edit above it.  The counts are this compiler's: another g++ splits a condition into a few more or
fewer outcomes; the named lines stay.

    python scripts/header_coverage.py --inputs existing     the inputs of the family's tests/test_gpu_*.py, rebuilt from the same
                                                            *_cases.py calls (rows that need the library: a host-only store)
    python scripts/header_coverage.py --inputs hostile      the tables of tests/hostile_cases.py
    python scripts/header_coverage.py --inputs hooks        the rows of tests/solver_hook_cases.py that no scene holds
    python scripts/header_coverage.py                       all three, what the tables reach that the existing inputs do not, and
                                                            what the hooks' rows reach that neither does

writes profiles/header_coverage.txt (-o: elsewhere).  tests/test_hostile_cpu.py uses coverage() and the lists of docs/design/09n.

The same for the back end's and mapping's headers (BACKEND_HEADERS: mcorb_ba.h, mcorb_retri.h, mcorb_pose.h, mcorb_mapping.h,
mcorb_mapping_new.h, mcorb_init.h, mcorb_triangulate.h) with the serial programs test_ba_sanitize.cpp, test_retri_sanitize.cpp,
test_pose_sanitize.cpp, test_init_sanitize.cpp, test_mapping_new_sanitize.cpp and test_mapping_sanitize.cpp: `existing` is what
tests/test_gpu_{ba,retri,pose,init,mapping_new,mapping}.py hand
their calls, `hostile` the tables of tests/hostile_backend_cases.py; these programs take whole scenes, so the rows that only a
hook can state (a caller-given point) are in neither.  tests/test_hostile_backend_cpu.py uses coverage(which, "backend") and the
lists of docs/design/09q."""
import argparse
import math
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

HEADERS = ("mcorb_sac.h", "mcorb_rel.h", "mcorb_align.h", "mcorb_ess.h")
PROGRAMS = dict(sac="test_sac_sanitize.cpp", sac_rig="test_sac_rig_sanitize.cpp", rel="test_rel_sanitize.cpp", align="test_align_sanitize.cpp",
                ess="test_ess_sanitize.cpp")
FLAGS = ["-O0", "--coverage", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc")]
BACKEND_HEADERS = ("mcorb_ba.h", "mcorb_retri.h", "mcorb_pose.h", "mcorb_mapping.h", "mcorb_mapping_new.h", "mcorb_init.h", "mcorb_triangulate.h")
BACKEND_PROGRAMS = dict(ba="test_ba_sanitize.cpp", retri="test_retri_sanitize.cpp", pose="test_pose_sanitize.cpp", init="test_init_sanitize.cpp",
                        new="test_mapping_new_sanitize.cpp", neigh="test_mapping_sanitize.cpp")
# how a program is called and what says that it ran: (arguments after the problem file, text its output must hold)
CALLS = dict(init=(["out.bin"], None), new=([], None))


# ---------------------------------------------------------------------------------------------------------------------------
# the programs' input files
# ---------------------------------------------------------------------------------------------------------------------------
def _cams(cams):
    return b"".join(struct.pack("<17d", *[v for row in c["R"] for v in row], *c["t"], c["fx"], c["fy"], c["s"], c["u0"], c["v0"]) for c in cams)


def _f(values):
    return np.asarray(values, np.float64).astype(np.float32).tobytes()


def blob_sac(cams, obs, match=None, threshold=None, H=100, seed=0, rig=False):
    """test_sac_sanitize.cpp's problem (rig: test_sac_rig_sanitize.cpp's), or None without an observation"""
    import sac_cases as SC
    import sac_ref as S
    cons = S.consensus(obs, match)[0]
    if not cons:
        return None
    n, ncams = len(obs), len(cams)
    blob = struct.pack("<4idQ", ncams, n, len(cons), H, SC.THRESHOLD if threshold is None else threshold, seed) + _cams(cams)
    with np.errstate(all="ignore"):
        blob += b"".join(_f([o[1], o[2]]) + struct.pack("<2i", o[0], o[3]) for o in obs)
    blob += b"".join(struct.pack("<3d", *o[4]) for o in obs) + struct.pack("<%di" % len(cons), *cons)
    if not rig:
        by_cam = [[i for i in cons if obs[i][0] == c] for c in range(ncams)]
        first = [0]
        for own in by_cam:
            first.append(first[-1] + len(own))
        blob += struct.pack("<%di" % (ncams + 1), *first) + struct.pack("<%di" % len(cons), *[i for own in by_cam for i in own])
    return blob


def blob_rel(cams, matches, threshold=None, H=100, seed=0):
    import rel_cases as RC
    if not matches:
        return None
    blob = struct.pack("<4idQ", len(cams), len(matches), H, 0, RC.THRESHOLD if threshold is None else threshold, seed) + _cams(cams)
    with np.errstate(all="ignore"):
        return blob + b"".join(_f([m[1], m[2], m[4], m[5]]) + struct.pack("<2i", m[0], m[3]) for m in matches)


def blob_align(p1, p2, mode=1, refit=True, threshold=0.2, inlier_dist=0.1, max_iterations=100, seed=0):
    p1, p2 = np.ascontiguousarray(p1, np.float64).reshape(-1, 3), np.ascontiguousarray(p2, np.float64).reshape(-1, 3)
    if not len(p1):
        return None
    return struct.pack("<4i2dQ", len(p1), max_iterations if mode == 1 else 0, mode, int(refit), threshold, inlier_dist, seed) + p1.tobytes() + p2.tobytes()


def blob_ess(matches, threshold_px=1.0, distance=50.0, max_iterations=100, seed=0):
    import ess_cases as EC
    if not matches:
        return None
    c = EC.CAM
    blob = struct.pack("<2i7dQ", len(matches), max_iterations, c["fx"], c["fy"], c["s"], c["u0"], c["v0"], threshold_px, distance, seed)
    with np.errstate(all="ignore"):
        return blob + _f(matches)


def inputs_hostile():
    """-> {program: [(name, problem)]}: every row of tests/hostile_cases.py, align_pose in both modes, ransac_pose with both solvers"""
    import hostile_cases as HC
    out = {k: [] for k in PROGRAMS}
    for name, matches, kw in HC.ess_rows():
        out["ess"].append((name, blob_ess(matches, max_iterations=HC.H, **kw)))
    for name, cams, matches, kw in HC.rel_rows():
        out["rel"].append((name, blob_rel(cams, matches, H=HC.H, **kw)))
    for name, p1, p2, kw in HC.align_rows():
        for mode in (1, 0):
            out["align"].append(("%s, mode %d" % (name, mode), blob_align(p1, p2, mode=mode, max_iterations=HC.H, **kw)))
    for name, cams, obs, match, kw in HC.sac_rows():
        out["sac"].append((name, blob_sac(cams, obs, match, H=HC.H, **kw)))
        out["sac_rig"].append((name, blob_sac(cams, obs, match, H=HC.H, rig=True, **kw)))
    return out


def inputs_hooks():
    """-> {program: [(name, problem)]}: the rows of tests/solver_hook_cases.py that no scene holds -- the hostile rows that are not
    a sample cut out of a table of hostile_cases.py, which inputs_hostile() runs whole -- each as a scene of its sample's size and
    a few hypotheses, whose samples are then permutations of the problem (the keypoints as floats, as the programs read them; the
    central solver's fourth observation is its first again).  align: the fit over the members, mode 0, and the hypotheses"""
    import solver_hook_cases as H
    out = {k: [] for k in PROGRAMS}

    def new(rows):
        return [r for r in rows if r[1] and ", h " not in r[0] and not r[0].endswith(", all pairs")]
    for name, _, five in new(H.ess_table()):
        out["ess"].append((name, blob_ess(five, max_iterations=4)))
    for name, _, cams, seventeen in new(H.rel_table()):
        out["rel"].append((name, blob_rel(cams, seventeen, H=2)))
    for name, _, p1, p2, member in new(H.align_table()):
        keep = slice(None) if member is None else np.asarray(member, bool)
        for mode in (0, 1):
            blob = blob_align(np.asarray(p1)[keep], np.asarray(p2)[keep], mode=mode, max_iterations=4)
            if blob is not None:
                out["align"].append(("%s, mode %d" % (name, mode), blob))
    for name, _, cams, c, uv, X in new(H.sac_table()):
        obs = [(c, p[0], p[1], 0, x) for p, x in zip(uv, X)]
        out["sac"].append((name, blob_sac(cams, obs + obs[:1], H=4)))
    for name, _, cams, ci, uv, X in new(H.rig_table()):
        out["sac_rig"].append((name, blob_sac(cams, [(c, p[0], p[1], 0, x) for c, p, x in zip(ci, uv, X)], H=4, rig=True)))
    return out


def inputs_existing():
    """-> {program: [(name, problem)]}: what tests/test_gpu_{sac,sac_rig,rel,align,ess}.py hand their calls (a launch of no
    observation runs nothing of the headers and has no problem file; a refinement is another header's)"""
    import mcorb as mc
    import align_cases as AC
    import ess_cases as EC
    import kfdb_cases as K
    import pose_cases as PC
    import rel_cases as RC
    import rel_ref as RR
    import sac_cases as SC
    import sac_ref as S
    import sac_rig_cases as SR
    import test_align_cpu
    import test_ess_cpu
    import test_rel_cpu
    import test_sac_cpu
    lm = mc.LocalMap(mc.ORBVocabulary(device=-1).create(**K.vocabulary()), device=-1, max_landmarks=4096, max_candidates=1024)
    out = {k: [] for k in PROGRAMS}

    def prefix(obs, match, n_matches):
        n = next((i for i, k in enumerate(match) if k >= n_matches), len(obs))
        return obs[:n], match[:n]

    # ---- test_gpu_ess.py
    add = lambda name, *a, **kw: out["ess"].append((name, blob_ess(*a, **kw)))
    truth, big, moved = EC.scene("general", n=1025, seed=21, noise=0.1)
    for size in (4, 5, 6, 63, 64, 65, 255, 256, 257, 1025):
        add("%d matches" % size, big[:size])
    for its in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1025, mc.ESS_MAX_ITERATIONS):
        add("%d hypotheses" % its, big[:64], max_iterations=its)
    for kind in EC.KINDS:
        add(kind, EC.scene(kind, seed=0, noise=0.1)[1], max_iterations=200)
    matches, E, k, s, px = test_ess_cpu.gate_rows(mc)
    add("threshold = the value", matches, threshold_px=px, max_iterations=1)
    add("the next double", matches, threshold_px=math.nextafter(px, math.inf), max_iterations=1)
    matches = list(matches)
    matches[7] = (matches[7][0], float("nan"), matches[7][2], matches[7][3])
    add("a NaN row", matches, threshold_px=1e4, max_iterations=60)
    truth, matches, moved = EC.scene("general", seed=1, noise=0.1)
    add("the scene", matches, max_iterations=200)
    got = EC.run(mc, lm, matches, max_iterations=200)
    w = max(range(4), key=lambda c: (got.cheirality[c], -c))
    z = mc.ess_decompose(got.E, EC.to_cam(mc), [m[0:2] for m in matches], [m[2:4] for m in matches])[1][:, w, :]
    for cam in (0, 1):
        k = max((i for i in range(len(matches)) if got.inliers[i] and z[i][cam] > z[i][1 - cam]), key=lambda i: z[i][cam])
        add("distance = the depth", matches, distance=float(z[k][cam]), max_iterations=200)
        add("the next double", matches, distance=math.nextafter(float(z[k][cam]), math.inf), max_iterations=200)
    add("four zero votes", matches, distance=1e-3, max_iterations=200)
    add("S = 5", EC.scene("general", n=5, seed=3, moved=0.0)[1], max_iterations=40)
    add("S = 4", big[:4], max_iterations=5)
    add("300 matches", big[:300])

    # ---- test_gpu_rel.py
    add = lambda name, *a, **kw: out["rel"].append((name, blob_rel(*a, **kw)))
    cams, truth, big, moved = RC.scene(8, 1025, 21, moved=0.1)
    for size in (16, 17, 18, 63, 64, 65, 255, 256, 257, 1025):
        add("%d matches" % size, cams, big[:size])
    for its in (1, 63, 64, 65, 100, 1025):
        add("%d hypotheses" % its, cams, big[:130], H=its)
    add("16 384 hypotheses", cams, big[:64], H=mc.REL_MAX_ITERATIONS)
    add("300 matches", cams, big[:300])
    add("S = 16", cams, big[:16], H=5)
    for ncams in (1, 4, 16):
        c, truth, matches, moved = RC.scene(ncams, 200, 30 + ncams, moved=0.1)
        add("%d cameras" % ncams, c, matches)
    c, matches, k, sc, model = test_rel_cpu.threshold_rows(mc)
    add("threshold = the score", c, matches, threshold=sc, H=1)
    add("the next double", c, matches, threshold=RR.next_up(sc), H=1)
    c, matches = test_rel_cpu.nan_rows()
    add("a NaN row", c, matches, threshold=1.5, H=60)
    c, truth, matches, moved = RC.scene(8, 17, 3, moved=0.0, noise=0.0)
    add("S = 17", c, matches, threshold=1e-9, H=40)

    # ---- test_gpu_align.py
    add = lambda name, *a, **kw: out["align"].append((name, blob_align(*a, **kw)))
    truth, p1, p2, moved = AC.scene(n=1025, seed=21, moved=100)
    for mode in (0, 1):
        for size in (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1025):
            add("%d pairs, mode %d" % (size, mode), p1[:size], p2[:size], mode=mode)
    for refit in (False, True):
        for its in (1, 63, 64, 65, 100, 1025):
            add("%d hypotheses" % its, p1[:64], p2[:64], max_iterations=its, refit=refit)
    add("16 384 hypotheses", p1[:64], p2[:64], max_iterations=mc.ALIGN_MAX_ITERATIONS)
    for kw in test_align_cpu.MODES:
        add("300 pairs", p1[:300], p2[:300], **kw)
    add("n = 2", p1[:2], p2[:2], max_iterations=5)
    for name, (a, b) in (("collinear", AC.collinear()), ("collinear as float", AC.collinear(True)), ("coincident", AC.coincident())):
        for mode in (0, 1):
            add(name, a, b, mode=mode, max_iterations=20)
    truth, a, b = AC.half_turn()
    add("half turn, all", a, b, mode=0)
    add("half turn", a, b, max_iterations=10)
    truth, a, b, moved = AC.scene(n=3, moved=0, noise=0.0)
    add("n = 3", a, b, max_iterations=40)
    a, b, k, d, model = test_align_cpu.threshold_rows(mc)
    for thr, inl in ((d, 10.0), (AC.AR.next_up(d), 10.0), (10.0, d), (10.0, AC.AR.next_up(d))):
        add("a limit on a distance", a, b, threshold=thr, inlier_dist=inl, max_iterations=1, refit=False)
    a, b = test_align_cpu.nan_rows()
    add("a NaN row", a, b, threshold=1e9, inlier_dist=1e9, max_iterations=60)
    add("a NaN row, all", a, b, mode=0)

    # ---- test_gpu_sac.py and test_gpu_sac_rig.py
    def both(name, *a, **kw):
        out["sac"].append((name, blob_sac(*a, **kw)))
        out["sac_rig"].append((name, blob_sac(*a, rig=True, **kw)))
    cams, truth, obs, match, moved = SC.scene(4, nlm=1040, seed=13)
    for size in (3, 4, 63, 64, 65, 255, 256, 257, 1025):
        out["sac"].append(("%d matches" % size, blob_sac(cams, *prefix(obs, match, size))))
    for its in (1, 63, 64, 65, 100, 1024):
        out["sac"].append(("%d hypotheses" % its, blob_sac(cams, *prefix(obs, match, 130), H=its)))
    out["sac"].append(("300 matches", blob_sac(cams, *prefix(obs, match, 300))))
    cams, truth, obs, match, moved = SC.scene(4, nlm=280, seed=13)
    for size in (3, 4, 5, 63, 64, 65, 257):
        out["sac_rig"].append(("%d matches" % size, blob_sac(cams, *prefix(obs, match, size), rig=True)))
    for its in (1, 15, 16, 17, 64, 100, 1024):
        out["sac_rig"].append(("%d hypotheses" % its, blob_sac(cams, *prefix(obs, match, 130), H=its, rig=True)))
    out["sac_rig"].append(("S = 3", blob_sac(cams, obs[:3], None, H=5, rig=True)))
    for ncams in (1, 4, 16):
        c, truth, o, m, moved = SC.scene(ncams, nlm=200, seed=20 + ncams)
        both("%d cameras" % ncams, c, o, m)
    for per_match in (1, 2, 16):
        c, truth, o, m, moved = SC.scene(4, nlm=40, seed=7, per_match=per_match)
        both("%d per match" % per_match, c, o, m)
        if per_match == 1:
            both("no match array", c, o, None)
    c, truth, o, m, moved = SC.scene(4, nlm=120, seed=31)
    cam, uv, octave, pts = PC.arrays(o)
    new = pts + np.random.default_rng(3).normal(scale=0.002, size=pts.shape)
    out["sac"].append(("before the points move", blob_sac(c, o, m)))
    out["sac"].append(("after", blob_sac(c, [(x[0], x[1], x[2], x[3], new[i].tolist()) for i, x in enumerate(o)], m)))
    rig, o, seed, sc, model = test_sac_cpu.threshold_rows(mc)
    out["sac"].append(("threshold = the score", blob_sac(rig, o, None, threshold=sc, H=1, seed=seed)))
    out["sac"].append(("the next double", blob_sac(rig, o, None, threshold=S.next_up(sc), H=1, seed=seed)))
    out["sac"].append(("64 hypotheses on the rows", blob_sac(rig, o, None, threshold=S.next_up(sc), H=64, seed=seed)))
    both("S = 4", PC.flat_rig(), SC.square(), None, threshold=1e-9)
    out["sac"].append(("S = 3", blob_sac(PC.flat_rig(), SC.square()[:3], None, H=5)))
    for ncams in (1, 4):
        c, truth, o, m, moved = SC.scene(ncams, nlm=300, seed=40 + ncams, per_match=2)
        out["sac"].append(("the refinement's scene, %d cameras" % ncams, blob_sac(c, o, m)))
    c, truth, o, m, moved = SC.scene(4, nlm=60, seed=9, moved=0.0)
    o = [(x[0], PC.f32(x[1] + 5.0) if i % 9 == 4 and i < 72 else x[1], x[2], 0, x[4]) for i, x in enumerate(o)]
    out["sac"].append(("a match the refinement culls", blob_sac(c, o, m, threshold=1.0 - math.cos(16.0 / 500.0))))
    c, truth, o, m, moved = SR.thin_scene(16)
    out["sac_rig"].append(("16 x 3", blob_sac(c, o, m, rig=True)))
    c, truth, o, m, moved = SR.thin_scene(4, per_cam=1, moved=0.0, noise=0.0)
    out["sac_rig"].append(("one per camera", blob_sac(c, o, None, rig=True)))
    c, truth, o, m, moved = SC.scene(4, nlm=300, seed=44, per_match=2)
    out["sac_rig"].append(("the refinement's scene", blob_sac(c, o, m, rig=True)))
    return {k: [(name, b) for name, b in v if b is not None] for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# the back end's and mapping's programs
# ---------------------------------------------------------------------------------------------------------------------------
def _poses(poses):
    return np.array([p[0] for p in poses], np.float64).tobytes() + np.array([p[1] for p in poses], np.float64).tobytes()


def blob_ba(sc, max_iterations=25):
    """test_ba_sanitize.cpp's problem of a scene of ba_cases.py, or None without a landmark or an observation"""
    import ba_cases as BC
    if not sc["obs"] or not sc["pts"]:
        return None
    kf, cam, olm, uv, octave = BC.arrays(sc["obs"])
    blob = struct.pack("<6i", len(sc["poses"]), len(sc["cams"]), len(sc["pts"]), len(kf), len(sc["sigma"]), max_iterations)
    blob += np.array(sc["sigma"], np.float64).tobytes() + _cams(sc["cams"]) + _poses(sc["poses"])
    blob += np.array(sc["fixed"], np.uint8).tobytes() + np.array(sc["pts"], np.float64).tobytes()
    return blob + kf.tobytes() + cam.tobytes() + olm.tobytes() + uv.tobytes() + octave.tobytes()


def blob_retri(sc, rank_tol=1.0, landmark_distance_threshold=-1.0, dynamic_outlier_threshold=-1.0, max_diff=5.0):
    """test_retri_sanitize.cpp's problem of a scene of retri_cases.py (the program runs in apply mode)"""
    import retri_cases as RC
    if not sc["obs"] or not sc["pts"]:
        return None
    kf, cam, olm, uv = RC.arrays(sc["obs"])
    blob = struct.pack("<4i4d", len(sc["poses"]), len(sc["cams"]), len(sc["pts"]), len(kf), rank_tol, landmark_distance_threshold,
                       dynamic_outlier_threshold, max_diff)
    blob += _cams(sc["cams"]) + _poses(sc["poses"]) + np.array(sc["moved"], np.uint8).tobytes() + np.array(sc["pts"], np.float64).tobytes()
    return blob + kf.tobytes() + cam.tobytes() + olm.tobytes() + uv.tobytes()


def blob_pose(cams, init, obs, inv_sigma2=None, max_iterations=25):
    """test_pose_sanitize.cpp's problem of the arguments of pose_cases.refine, or None without an observation"""
    import pose_cases as PC
    if not obs:
        return None
    inv_sigma2 = PC.INV_SIGMA2 if inv_sigma2 is None else inv_sigma2
    cam, uv, octave, pts = PC.arrays(obs)
    blob = struct.pack("<4i", len(cams), len(obs), len(inv_sigma2), max_iterations) + np.array(inv_sigma2, np.float64).tobytes() + _cams(cams)
    return blob + _poses([init]) + cam.tobytes() + uv.tobytes() + octave.tobytes() + pts.tobytes()


def _frame(fr):
    out = np.ascontiguousarray(fr["match_index"], np.int32).tobytes() + np.ascontiguousarray(fr["proj"], np.float64).tobytes()
    out += np.ascontiguousarray(fr["centre_w"], np.float64).tobytes() + np.array([len(k) for k in fr["kps"]], np.int32).tobytes()
    for k in fr["kps"]:
        out += np.stack([k["x"], k["y"]], axis=1).astype(np.float32).tobytes() + k["octave"].astype(np.int32).tobytes()
    return out


def blob_neigh(sc):
    """test_mapping_sanitize.cpp's problem of a scene of mapping_cases.py (the points of the neighbours' landmarks from the
    scene's store), or None without a neighbour"""
    if not sc["neigh"]:
        return None
    f64 = lambda a: np.ascontiguousarray(a, np.float64).tobytes()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()
    frame = lambda fr: f64(fr["twc"]) + _frame(fr) + i32(fr["lids"])
    blob = struct.pack("<5i", sc["ncams"], len(sc["neigh"]), len(sc["inv_sigma2"]), sc["next_lid"], len(sc["cur"]["match_index"]))
    blob += f64(sc["K"]) + np.ascontiguousarray(sc["inv_sigma2"], np.float32).tobytes() + f64(sc["Rcw"]) + f64(sc["tcw"]) + frame(sc["cur"])
    for fr, F, m in zip(sc["neigh"], sc["F21"], sc["matches"]):
        m = np.asarray(m, np.int32).reshape(-1, 2)
        blob += struct.pack("<2i", len(fr["match_index"]), len(m)) + frame(fr)
        blob += b"".join(f64(sc["store"][int(l)]) for l in fr["lids"] if l != -1) + f64(F) + i32(m[:, 0]) + i32(m[:, 1])
    return blob


def blob_init(sc):
    """test_init_sanitize.cpp's problem of a scene of init_cases.py, or None where the call ends before its loop (no match, no
    baseline)"""
    import init_ref as IR
    n = len(sc["matches"])
    if not n or not IR.baseline_ok(sc["t"], sc["min_baseline"]):
        return None
    blob = np.array([sc["ncams"], n, len(sc["inv_sigma2"]), sc["next_lid"], len(sc["prev"]["match_index"]), len(sc["cur"]["match_index"])],
                    np.int32).tobytes()
    for a in (sc["R"], sc["t"], sc["body"], sc["K"]):
        blob += np.ascontiguousarray(a, np.float64).tobytes()
    blob += np.ascontiguousarray(sc["inv_sigma2"], np.float32).tobytes() + sc["matches"].astype(np.int32).tobytes()
    return blob + np.asarray(sc["flags"]).astype(np.uint8).tobytes() + _frame(sc["cur"]) + _frame(sc["prev"])


def blob_new(sc):
    """test_mapping_new_sanitize.cpp's scene file of a scene of mapping_new_cases.py: the program runs every match it is given,
    so the matches the walk skips (a current feature that has a landmark, on entry or from an earlier match) are left out"""
    lids, keep = sc["cur"]["lids"].copy(), []
    for q, t in np.asarray(sc["matches"]).reshape(-1, 2).tolist():
        if lids[t] == -1:
            keep.append((q, t))
            lids[t] = 0
    if not keep:
        return None
    num = lambda a: " ".join(repr(float(x)) for x in np.asarray(a, np.float64).reshape(-1))
    out = ["%d %d" % (sc["ncams"], len(sc["inv_sigma2"])), num(sc["K"]), num(sc["inv_sigma2"])]
    for fr in (sc["cur"], sc["prev"]):
        out.append(num(fr["twc"]))
        for c in range(sc["ncams"]):
            out.append(num(fr["proj"][c]) + " " + num(fr["centre_w"][c]))
        for kps in fr["kps"]:
            out.append("%d %s" % (len(kps), " ".join("%r %r %d" % (float(k["x"]), float(k["y"]), k["octave"]) for k in kps)))
        out.append("%d" % len(fr["match_index"]))
        out.append(" ".join(str(int(v)) for v in np.asarray(fr["match_index"]).reshape(-1)))
    out.append("%d" % len(keep))
    out.append(" ".join("%d %d" % m for m in keep))
    return ("\n".join(out) + "\n").encode()


def backend_hostile():
    """-> {program: [(name, problem)]}: the rows of tests/hostile_backend_cases.py that these programs can read"""
    import hostile_backend_cases as HB
    out = {k: [] for k in BACKEND_PROGRAMS}
    for name, sc, kw in HB.ba_rows():
        out["ba"].append((name, blob_ba(sc, kw.get("max_iterations", HB.BA_ITERATIONS))))
    for name, sc, kw in HB.retri_rows():
        out["retri"].append((name, blob_retri(sc, **kw)))
    for name, cams, init, obs, kw in HB.pose_rows():
        out["pose"].append((name, blob_pose(cams, init, obs, **kw)))
    for name, sc, kw in HB.init_rows():
        out["init"].append((name, blob_init(sc)))
    for name, sc, kw in HB.new_rows():
        out["new"].append((name, blob_new(sc)))
    for name, sc, kw in HB.neigh_rows():
        out["neigh"].append((name, blob_neigh(sc)))
    return {k: [(name, b) for name, b in v if b is not None] for k, v in out.items()}


def backend_existing():
    """-> {program: [(name, problem)]}: what tests/test_gpu_{ba,retri,init,mapping_new}.py hand their calls (a call that launches
    nothing has no problem file; the hooks' hand-built cases give the point, which these programs compute)"""
    import ba_cases as BC
    import init_cases as Ic
    import mapping_cases as Mc
    import mapping_new_cases as Nc
    import pose_cases as PC
    import retri_cases as RC
    import test_retri_cpu as TR
    out = {k: [] for k in BACKEND_PROGRAMS}
    # ---- test_gpu_ba.py
    add = lambda name, sc, its=25: out["ba"].append((name, blob_ba(sc, its)))
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        add("%d landmarks" % n, BC.scene(nlm=n, seed=30 + n % 7, max_views=3), 3 if n == 1025 else 25)
    for nkf in (1, 2, 3, 16):
        add("%d keyframes" % nkf, BC.scene(nkf=nkf, nlm=40, nfixed={1: 0, 2: 1, 3: 1, 16: 2}[nkf], seed=40 + nkf, spacing=0.3 if nkf < 16 else 0.1),
            4 if nkf == 16 else 25)
    for ncams in (1, 4, 16):
        add("%d cameras" % ncams, BC.scene(ncams=ncams, nlm=60, seed=50 + ncams, skew=0.2))
    for with_nan in (True, False):
        for extra in ((), (1,)):
            add("z and Huber rows", BC.hand_scene(PC.z_rows(with_nan) + BC.huber_rows(1.0), fixed=not extra, extra_kf=extra))
    for sg in (1.0, 0.25):
        add("Huber rows", BC.hand_scene(BC.huber_rows(sg), sigma=(sg,)))
    rows, sigma, flags = BC.chi2_rows()
    add("chi2 rows", BC.hand_scene(rows, sigma=sigma))
    for name, sc, check in BC.degenerate():
        add(name, sc)
    for its in (1, 100):
        add("max_iterations %d" % its, BC.scene(nlm=30, seed=21), its)
    sc = BC.scene(nlm=50, seed=23)
    add("before the points move", sc)
    add("after", dict(sc, pts=(np.array(sc["pts"]) + np.random.default_rng(3).normal(scale=0.02, size=(len(sc["pts"]), 3))).tolist()))
    add("the timing's scene", BC.scene(nlm=100, seed=24))
    # ---- test_gpu_retri.py
    add = lambda name, sc, **kw: out["retri"].append((name, blob_retri(sc, **kw)))
    add("view counts", RC.synth(17, 16, RC.VIEW_COUNTS * 2, seed=60, skew=0.1))
    for n in RC.LANDMARK_COUNTS:
        add("%d landmarks" % n, RC.synth(6, 2, [2 + j % 4 for j in range(n)], seed=70 + n, moved=[k % 3 == 0 for k in range(6)]))
    for nkf in (1, 17, 1024):
        used = {1: [0], 17: [2, 9, 16], 1024: [3, 500, 1023]}[nkf]
        add("%d keyframes" % nkf, RC.synth(nkf, 4, [min(v, 4 * len(used)) for v in (1, 2, 3, 4, 5, 6, 4, 3)], seed=80 + nkf % 7, used_kfs=used,
                                           moved=[k == used[-1] for k in range(nkf)]))
    for ncams in (1, 4, 16):
        add("%d cameras" % ncams, RC.synth(5, ncams, [2 + j % 4 for j in range(20)], seed=90 + ncams, skew=0.3 if ncams == 4 else 0.0))
    add("exact scene", RC.exact_scene(pt=(3.0, 4.0, 0.0)))
    for max_diff in (5.0, math.nextafter(5.0, 10.0), 0.0, math.inf):
        add("max_diff", RC.exact_scene(pt=(3.0, 4.0, 0.0)), max_diff=max_diff)
    add("NaN point", RC.exact_scene(pt=(float("nan"), 0.0, 0.0)), max_diff=math.nextafter(5.0, 10.0))
    for extra in (RC.AT_ORIGIN, RC.AT_ORIGIN_MINUS):
        add("z of zero", RC.exact_scene(extra=[extra]))
    sc = RC.synth(4, 2, [3, 6], seed=7)
    want = RC.ref(sc, detail=True)
    for j in (0, 1):
        for tol in (want["s3"][j], math.nextafter(want["s3"][j], 0.0), math.nextafter(want["s3"][j], math.inf)):
            add("rank_tol at sqrt(lambda_3)", sc, rank_tol=tol)
        for thr in (want["emax"][j], math.nextafter(want["emax"][j], 0.0)):
            add("outlier threshold at the largest error", sc, dynamic_outlier_threshold=thr)
    add("the apply scene", TR.apply_scene())
    add("apply writes the point", RC.synth(4, 2, [3, 4, 5, 2] * 20, seed=13))
    add("the timing's scene", RC.synth(4, 2, [3] * 100, seed=14))
    sc = BC.scene(nlm=60, seed=21)
    add("a bundle adjustment's scene", RC.from_ba(sc))
    add("a bundle adjustment's scene, thresholds on", RC.from_ba(sc), landmark_distance_threshold=50.0, dynamic_outlier_threshold=3.0)
    # ---- test_gpu_pose.py
    add = lambda name, *a, **kw: out["pose"].append((name, blob_pose(*a, **kw)))
    cams, truth, init, obs, moved = PC.scene(4, nlm=280, seed=9)
    for n in (1, 5, 6, 63, 64, 65, 255, 256, 257, 1025, 2, 3):
        add("%d observations" % n, cams, init, obs[:n])
    for its in (1, 100):
        add("max_iterations %d" % its, cams, init, obs[:130], max_iterations=its)
    bad = ([row[:] for row in init[0]], init[1][:])
    bad[0][1][2] = float("nan")
    add("a NaN initial pose", cams, bad, obs[:70])
    for ncams in (1, 4, 16):
        c, truth, i0, o, moved = PC.scene(ncams, nlm=max(20, 160 // ncams), seed=20 + ncams)
        add("%d cameras" % ncams, c, i0, o)
    for with_nan in (True, False):
        add("z and Huber rows", PC.flat_rig(), PC.IDENT, PC.z_rows(with_nan) + PC.huber_rows())
    add("Huber rows", PC.flat_rig(), PC.IDENT, PC.huber_rows())
    o, inv, flags = PC.chi2_rows()
    add("chi2 rows", PC.flat_rig(), PC.IDENT, o, inv_sigma2=inv)
    add("an exact observation", PC.flat_rig(), PC.IDENT, [(0, 3.0, 4.0, 0, [3.0, 4.0, 1.0])])
    add("all behind the rig", PC.flat_rig(), PC.IDENT, [(c, kx, ky, o_, [-v for v in X]) for c, kx, ky, o_, X in PC.z_rows(False)[:6]])
    # ---- test_gpu_init.py
    big = Ic.scene(4, n=1100, seed=3)
    for third in (False, True):
        for n in (1, 51, 63, 64, 65, 255, 256, 257, 1025):
            out["init"].append(("%d matches" % n, blob_init(Ic.cut(big, n, third))))
    for ncams in (1, 4, 8):
        out["init"].append(("%d cameras" % ncams, blob_init(Ic.scene(ncams))))
    # ---- test_gpu_mapping_new.py
    for n in (1, 63, 64, 65, 256, 257):
        out["new"].append(("%d matches" % n, blob_new(Nc.scene(4, n=n, seed=n + 1))))
    for ncams in (1, 4, 8):
        out["new"].append(("%d cameras" % ncams, blob_new(Nc.scene(ncams))))
    # ---- test_gpu_mapping.py: its scenes (the gate cases are a hook's: the point is given)
    add = lambda name, sc: out["neigh"].append((name, blob_neigh(sc)))
    for n in (1, 63, 64, 65, 256, 257):
        add("%d matches" % n, Mc.scene(4, sizes=(n,), seed=n + 1, zero_f=None))
    for sizes in ((257,), (100, 157), (60, 0, 97, 50, 50)):
        sc = Mc.scene(4, sizes=sizes, seed=11, zero_f=None)
        if len(sizes) == 5:
            sc["neigh"][3]["twc"] = sc["cur"]["twc"].copy()
        add("segments %s" % (sizes,), sc)
    add("the random scene", Mc.scene(4, sizes=(300, 300, 300), seed=3))
    rng = np.random.default_rng(4)     # (test_view_counts_in_one_call's scene: 2 .. 16 views)
    Ks, rigT = Mc.make_rig(8, rng)
    cur = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(0.02, -0.01, 0.03), np.zeros(3)), rigT), Ks)
    nb = Mc.FrameBuilder(Mc.frame_geometry(Mc.T4(Mc.rot(-0.03, 0.05, 0.0), np.array([1.1, 0.05, -0.1])), rigT), Ks)
    nb.add(np.array([0.0, 0.0, 5.0]), [0], rng, lid=900)
    ms = []
    for i in range(150):
        a, b = [(1, 1), (2, 1), (2, 2), (4, 4), (8, 8)][i % 5]
        X = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 15)])
        ms.append((nb.add(X, sorted(rng.choice(8, a, replace=False).tolist()), rng), cur.add(X, sorted(rng.choice(8, b, replace=False).tolist()), rng)))
    F = np.array([[Mc.fundamental(cur.g["full"][cc], nb.g["full"][cn], Ks[cc], Ks[cn]) for cn in range(8)] for cc in range(8)])
    Tcw = np.linalg.inv(cur.g["pose"])
    add("view counts", dict(ncams=8, K=np.array(Ks), inv_sigma2=Mc.INV_SIGMA2, cur=cur.done(), neigh=[nb.done()], F21=[F],
                            store={900: np.array([0.0, 0.0, 5.0])}, matches=[np.array(ms, np.int32)], Rcw=Tcw[:3, :3], tcw=Tcw[:3, 3], next_lid=0))
    return {k: [(name, b) for name, b in v if b is not None] for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# build, run, read
# ---------------------------------------------------------------------------------------------------------------------------
def build(tmp, programs=PROGRAMS):
    """the programs, each in a directory of its own under tmp (its .gcno and .gcda live there) -> {program: directory}"""
    dirs = {}
    for prog, src in programs.items():
        d = os.path.join(tmp, prog)
        os.makedirs(d)
        subprocess.check_call(["g++"] + FLAGS + ["-c", os.path.join(ROOT, "tests", "cpp", src), "-o", "prog.o"], cwd=d)
        subprocess.check_call(["g++", "--coverage", "prog.o", "-o", "prog"], cwd=d)
        dirs[prog] = d
    return dirs


def run(dirs, inputs):
    for prog, problems in inputs.items():
        d = dirs[prog]
        for name, blob in problems:
            with open(os.path.join(d, "in.bin"), "wb") as f:
                f.write(blob)
            more, says = CALLS.get(prog, (["out.bin"], "bad=0"))
            got = subprocess.run([os.path.join(d, "prog"), "in.bin"] + more, cwd=d, capture_output=True, text=True, timeout=600)
            ran = says in got.stdout if says is not None else not got.stderr and \
                (os.path.getsize(os.path.join(d, "out.bin")) > 0 if more else got.stdout.count("\n") > 0)
            assert got.returncode == 0 and ran, (prog, name, got.returncode, got.stdout[-300:], got.stderr[-300:])


LINE = re.compile(r"^\s*([^:]+):\s*(\d+):(.*)$")
BRANCH = re.compile(r"^branch\s+(\d+)\s+(never executed|taken (\d+))(.*)$")


def read(dirs, headers=HEADERS):
    """gcov -b -c in every program's directory -> {header: {(line text, occurrence, outcome): times taken, summed over the
    programs and over the instantiations of a template}}; an outcome in code that never ran counts as not taken.  The edge
    gcov marks (throw) at a call of a function that is not noexcept is no outcome of the arithmetic and is left out"""
    taken, throws = {h: {} for h in headers}, {h: set() for h in headers}
    for prog, d in dirs.items():
        subprocess.run(["gcov", "-b", "-c", "prog.gcno"], cwd=d, check=True, capture_output=True)
        for h in headers:
            path = os.path.join(d, h + ".gcov")
            if not os.path.exists(path):
                continue
            text, per_line, thrown, cur = {}, {}, set(), None
            with open(path, errors="replace") as f:
                for row in f:
                    m = BRANCH.match(row)
                    if m and cur is not None:
                        key = (cur, int(m.group(1)))
                        per_line[key] = per_line.get(key, 0) + int(m.group(3) or 0)
                        if "(throw)" in m.group(4):
                            thrown.add(key)
                        continue
                    m = LINE.match(row)
                    if m and int(m.group(2)) > 0:
                        cur = int(m.group(2))
                        text[cur] = " ".join(m.group(3).split())
            lines = sorted(set(ln for ln, _ in per_line))
            for (ln, k), cnt in per_line.items():
                occurrence = sum(1 for other in lines if other < ln and text[other] == text[ln])
                key = (text[ln], occurrence, k)
                taken[h][key] = taken[h].get(key, 0) + cnt
                if (ln, k) in thrown:
                    throws[h].add(key)
    return {h: {k: v for k, v in taken[h].items() if k not in throws[h]} for h in headers}


def coverage(which, group="pose"):
    """which: "existing", "hostile" or "hooks"; group: "pose" (HEADERS) or "backend" (BACKEND_HEADERS, no hooks) -> read()'s dict
    after a fresh build run on that set"""
    with tempfile.TemporaryDirectory() as tmp:
        if group == "backend":
            dirs = build(tmp, BACKEND_PROGRAMS)
            run(dirs, {"existing": backend_existing, "hostile": backend_hostile}[which]())
            return read(dirs, BACKEND_HEADERS)
        dirs = build(tmp)
        run(dirs, {"existing": inputs_existing, "hostile": inputs_hostile, "hooks": inputs_hooks}[which]())
        return read(dirs)


def name_of(key):
    return "%s  [%d]%s" % (key[0], key[2], "" if key[1] == 0 else "  (occurrence %d)" % key[1])


def never(taken):
    return sorted(k for k, v in taken.items() if v == 0)


def report(results, headers=HEADERS, head=True):
    """results: {which: coverage(which)} -> the text of profiles/header_coverage.txt"""
    out = ["header_coverage.py: branch outcomes (gcov -b -c, g++ -O0 --coverage -ffp-contract=off) of the serial programs of tests/cpp.",
           "An outcome is `source line  [gcov's index on the line]`.", ""] if head else []
    for h in headers:
        for which, res in results.items():
            miss = never(res[h])
            out.append("%s, inputs %s: %d of %d outcomes taken, %d never:" % (h, which, len(res[h]) - len(miss), len(res[h]), len(miss)))
            out += ["    " + name_of(k) for k in miss]
            out.append("")
        if "existing" in results and "hostile" in results:
            e, t = results["existing"][h], results["hostile"][h]
            reached = sorted(k for k in never(e) if t.get(k, 0) > 0)
            still = sorted(k for k in never(e) if t.get(k, 0) == 0)
            out.append("%s: never taken by the existing inputs, taken by the tables (%d):" % (h, len(reached)))
            out += ["    " + name_of(k) for k in reached]
            out.append("%s: taken by neither (%d):" % (h, len(still)))
            out += ["    " + name_of(k) for k in still]
            out.append("")
            if "hooks" in results:
                k3 = results["hooks"][h]
                more = [k for k in still if k3.get(k, 0) > 0]
                out.append("%s: taken by neither, taken by the solver hooks' rows (%d):" % (h, len(more)))
                out += ["    " + name_of(k) for k in more]
                out.append("%s: taken by none of the three (%d):" % (h, len(still) - len(more)))
                out += ["    " + name_of(k) for k in still if k not in more]
                out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--inputs", choices=("existing", "hostile", "hooks", "all"), default="all")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "header_coverage.txt"))
    args = ap.parse_args()
    results = {w: coverage(w) for w in (("existing", "hostile", "hooks") if args.inputs == "all" else (args.inputs,))}
    backend = {w: coverage(w, "backend") for w in (("existing", "hostile") if args.inputs == "all" else (args.inputs,)) if w != "hooks"}
    text = report(results) + "\n" + report(backend, BACKEND_HEADERS, head=False)
    with open(args.output, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
