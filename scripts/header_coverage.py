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

writes profiles/header_coverage.txt (-o: elsewhere).  tests/test_hostile_cpu.py uses coverage() and the lists of docs/design/09n."""
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
# build, run, read
# ---------------------------------------------------------------------------------------------------------------------------
def build(tmp):
    """the five programs, each in a directory of its own under tmp (its .gcno and .gcda live there) -> {program: directory}"""
    dirs = {}
    for prog, src in PROGRAMS.items():
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
            got = subprocess.run([os.path.join(d, "prog"), "in.bin", "out.bin"], cwd=d, capture_output=True, text=True, timeout=600)
            assert got.returncode == 0 and "bad=0" in got.stdout, (prog, name, got.returncode, got.stdout, got.stderr)


LINE = re.compile(r"^\s*([^:]+):\s*(\d+):(.*)$")
BRANCH = re.compile(r"^branch\s+(\d+)\s+(never executed|taken (\d+))(.*)$")


def read(dirs):
    """gcov -b -c in every program's directory -> {header: {(line text, occurrence, outcome): times taken, summed over the
    programs and over the instantiations of a template}}; an outcome in code that never ran counts as not taken.  The edge
    gcov marks (throw) at a call of a function that is not noexcept is no outcome of the arithmetic and is left out"""
    taken, throws = {h: {} for h in HEADERS}, {h: set() for h in HEADERS}
    for prog, d in dirs.items():
        subprocess.run(["gcov", "-b", "-c", "prog.gcno"], cwd=d, check=True, capture_output=True)
        for h in HEADERS:
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
    return {h: {k: v for k, v in taken[h].items() if k not in throws[h]} for h in HEADERS}


def coverage(which):
    """which: "existing", "hostile" or "hooks" -> read()'s dict after a fresh build run on that set"""
    with tempfile.TemporaryDirectory() as tmp:
        dirs = build(tmp)
        run(dirs, {"existing": inputs_existing, "hostile": inputs_hostile, "hooks": inputs_hooks}[which]())
        return read(dirs)


def name_of(key):
    return "%s  [%d]%s" % (key[0], key[2], "" if key[1] == 0 else "  (occurrence %d)" % key[1])


def never(taken):
    return sorted(k for k, v in taken.items() if v == 0)


def report(results):
    """results: {which: coverage(which)} -> the text of profiles/header_coverage.txt"""
    out = ["header_coverage.py: branch outcomes (gcov -b -c, g++ -O0 --coverage -ffp-contract=off) of the serial programs of tests/cpp.",
           "An outcome is `source line  [gcov's index on the line]`.", ""]
    for h in HEADERS:
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
    text = report(results)
    with open(args.output, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
