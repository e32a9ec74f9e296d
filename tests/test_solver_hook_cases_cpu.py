"""The tables of solver_hook_cases.py held to their own claims on the host hooks alone, without a GPU: what each table contains,
that a row built for an outcome takes it, that the rows named for a rejected root between two kept ones are what
tests/cpp/ess_roots.cpp prints, that each rig row named for a root has exactly that, and which branch outcomes of the shared
headers the rows no scene can hold take (scripts/header_coverage.py, its third input set).

test_gpu_solver_hooks.py runs the same tables on the device twins of the hooks."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import ess_cases as EC
import hostile_cases as HC
import sac_cases as SC
import solver_hook_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


_HOST = {}


def host(mc, solver):
    if solver not in _HOST:
        table, run, _ = H.SOLVERS[solver]
        _HOST[solver] = (table(), run(mc, table()))
    return _HOST[solver]


def by_name(mc, solver):
    rows, res = host(mc, solver)
    return {r[0]: (i, r) for i, r in enumerate(rows)}, res


def header_coverage():
    spec = importlib.util.spec_from_file_location("header_coverage", os.path.join(ROOT, "scripts", "header_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("solver", sorted(H.SOLVERS))
def test_what_a_table_contains(mc, solver):
    """the CPU suite's seeded cases in full, a problem per complete sample of every hostile row, the rows no scene holds; cuts
    that hold both kinds of row; and the host hook's result in the form the device's is compared in: the models first, zero
    behind the count, the same bytes on a second call"""
    rows, res = host(mc, solver)
    seeded = sum(1 for r in rows if not r[1])
    assert seeded == {"ess": 4000, "sac": 4000, "rig": 12000, "rel": 12000, "align": 5360}[solver]
    cut = sum(1 for r in rows if r[1] and re.search(r", h \d+$", r[0]))
    tables = {"ess": HC.ess_rows, "sac": HC.sac_rows, "rig": HC.sac_rows, "rel": HC.rel_rows, "align": HC.align_rows}[solver]()
    assert 0 < cut <= len(tables) * HC.H and (cut == len(tables) * HC.H or solver in ("sac", "rig"))   # (incomplete samples have no problem)
    for name in names_of(tables):
        assert solver in ("sac", "rig") or "%s, h %d" % (name, HC.H - 1) in H.names(rows)
    order = H.mixed(rows)
    assert sorted(order) == list(range(len(rows)))
    for n in H.CUTS[1:]:
        assert 0 < sum(1 for i in order[:n] if rows[i][1]) < n
    count, models = res[0], res[1]
    assert count.min() >= 0 and count.max() <= models.shape[1] if models.ndim == 3 else count.max() <= 1
    for i in range(len(rows)):
        m = models[i].reshape(models.shape[1], -1) if models.ndim == 3 else models[i].reshape(1, -1)
        assert not m[count[i]:].any() and np.isfinite(m).all(), rows[i][0]
        assert solver == "align" or m[:count[i]].any(axis=1).all(), rows[i][0]
    again = H.SOLVERS[solver][1](mc, rows[-300:])
    assert H.same(again, H.take(res, list(range(len(rows) - 300, len(rows))))) == []


def names_of(rows):
    return [r[0] for r in rows]


def test_rows_built_for_an_outcome_take_it(mc):
    at, res = by_name(mc, "sac")
    count = res[0]
    for name in ("by hand 0", "by hand 1", "two coincident", "three coincident", "collinear points", "points at the origin", "points times 1e+165",
                 "points times 1e-165", "keypoints times 1e+36", "NaN at point number 4", "inf at keypoint number 0"):
        assert count[at[name][0]] == 0, name
    # (the seeded case's camera sits off the body's origin: its problem does not scale with the points, so no scale keeps a pose)
    assert count[at["points times 1e-155"][0]] == 0
    # the biquadratic quartic: a sample of "half the rows one observation" that holds one point twice among its first three
    twice = [r for r in host(mc, "sac")[0] if r[0].startswith("half the rows one observation") and len(set(map(tuple, r[5]))) < 3]
    assert twice and all(count[at[r[0]][0]] == 0 for r in twice)
    at, res = by_name(mc, "rig")
    count, mask, best = res[0], res[3], res[4]
    twice = [r for r in host(mc, "rig")[0] if r[0].startswith("half the rows one observation") and len(set(map(tuple, r[5][:3]))) < 3]
    assert twice and all(count[at[r[0]][0]] == 0 for r in twice)
    for name in ("by hand 0", "by hand 1", "three coincident", "points at the origin", "NaN at point number 0", "inf at keypoint number 3"):
        assert count[at[name][0]] == 0 and mask[at[name][0]] == 0 and best[at[name][0]] == -1, name
    for name in ("three observations in one camera", "three observations in three cameras", "every camera at the body's origin"):
        i = at[name][0]
        assert count[i] >= 1 and best[i] >= 0 and mask[i] >> best[i] & 1, name
    # a NaN at the fourth observation: the roots keep their poses and none wins
    i, j = at["NaN at the fourth point, number 1"][0], at["the fourth is the first again"][0]
    assert count[i] == count[j] > 0 and mask[i] == mask[j] and best[i] == -1 and best[j] >= 0
    assert res[1][i].tobytes() == res[1][j].tobytes() and not res[5][i].any()
    # the central rig's problem scales with its points: a model at 1e-155, none at 1e-165 (hostile_cases.py's edge)
    assert count[at["every camera at the body's origin, points times 1e-155"][0]] > 0
    assert count[at["every camera at the body's origin, points times 1e-165"][0]] == 0
    at, res = by_name(mc, "rel")
    for name in ("a rig of one camera, outward, 0", "a rig of one camera, flat, 23", "all 17 in camera 0, pure translation", "seventeen coincident",
                 "collinear in both images, all in camera 0", "all at the image's origin, all in camera 0",   # (one camera: no scale)
                 "keypoints times 1e+200, as doubles", "NaN in match 8, column 4", "inf in match 16, column 1"):
        assert res[0][at[name][0]] == 0, name
    at, res = by_name(mc, "ess")
    for name in ("three coincident", "five coincident", "all at the principal point", "NaN at number 0", "inf at number 19", "-inf at number 7",
                 "keypoints times 1e+200, as doubles"):
        assert res[0][at[name][0]] == 0, name
    at, res = by_name(mc, "align")
    valid, gap = res[0], res[3]
    for name in ("collinear triple", "collinear as float triple", "coincident triple", "two coincident of three", "all at the origin",
                 "a member mask of 0 of 300", "a member mask of 1 of 300", "a member mask of 2 of 300", "0 pairs, all members", "1 pairs, all members",
                 "2 pairs, all members", "times 1e+158", "times 1e+200", "times 1e-200", "NaN in frame 1, number 0", "inf in frame 2, number 8"):
        assert valid[at[name][0]] == 0 and not gap[at[name][0]] > 1e-12, name
    for name in ["a member mask of 3 of 300", "times 1e-158", "a reflection"] + ["%d pairs%s" % (k, s) for k in H.ALIGN_COUNTS
                                                                                 for s in ("", ", every third a member", ", the last three members")
                                                                                 if (k, s) != (3, ", every third a member")]:
        assert valid[at[name][0]] == 1 and gap[at[name][0]] > 1e-12, name
    assert valid[at["3 pairs, every third a member"][0]] == 0      # (one member)
    i = at["a reflection"][0]
    assert abs(np.linalg.det(res[1][i].reshape(3, 3)) - 1.0) < 1e-12      # (a proper rotation whatever the data)
    a, b = at["a member set of 600"][0], at["a member set of 600, NaN outside it"][0]
    assert valid[a] == 1 and all(x[a].tobytes() == x[b].tobytes() for x in res)


def test_the_rows_with_a_rejected_root_between_two_kept_ones(mc, tmp_path):
    """H.ESS_BETWEEN is what tests/cpp/ess_roots.cpp prints on the hostile tables, hypothesis by hypothesis; on each of its rows
    the host hook's z list has the pattern's count and ascends; the patterns of section 9n are among them"""
    exe = str(tmp_path / "ess_roots")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ess_roots.cpp"), "-o", exe])
    C = header_coverage()
    found = []
    for name, matches, kw in HC.ess_rows():
        (tmp_path / "in.bin").write_bytes(C.blob_ess(matches, max_iterations=HC.H, **kw))
        out = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=300, check=True).stdout.split("\n")
        kept = [ln.split()[1] for ln in out if ln]
        found += [("%s, h %d" % (name, h), k) for h, k in enumerate(kept) if re.search("10+1", k)]
    assert tuple(found) == H.ESS_BETWEEN
    assert {"100111", "100001", "1010"} <= set(k for _, k in found)
    at, res = by_name(mc, "ess")
    for name, pattern in H.ESS_BETWEEN:
        i = at[name][0]
        z = res[2][i][:res[0][i]].tolist()
        assert res[0][i] == pattern.count("1") and z == sorted(z) and len(set(z)) == len(z), name


def test_each_rig_row_named_for_a_root_has_exactly_that(mc):
    at, res = by_name(mc, "rig")
    count, mask, best = res[0], res[3], res[4]
    for k in range(4):
        assert len(H.RIG_BEST[k]) >= 1 and len(H.RIG_ONLY[k]) >= 1
        for seed, i in H.RIG_BEST[k]:
            j = at["the winner is root %d (seed %d, %d)" % (k, seed, i)][0]
            assert best[j] == k and count[j] >= 2 and mask[j] >> k & 1
            slot = bin(mask[j] & ((1 << k) - 1)).count("1")      # (root k's place in the compacted list)
            assert res[1][j][slot].tobytes() == res[5][j].tobytes() and res[2][j][slot].tobytes() == res[6][j].tobytes()
        for seed, i in H.RIG_ONLY[k]:
            j = at["the only pose is root %d (seed %d, %d)" % (k, seed, i)][0]
            assert mask[j] == 1 << k and count[j] == 1 and best[j] == k
            assert res[1][j][0].tobytes() == res[5][j].tobytes()
    # the search finds the same within its first 128 problems
    found_best, found_only, seen, masks = H.rig_search(mc, limit=128)
    assert found_best == H.RIG_BEST and found_only == H.RIG_ONLY and seen == 128


def test_the_hooks_agree_with_the_three_observation_hooks(mc):
    """mcorb_host_sac_rig_roots' list is mcorb_sac_solve_rig's on the first three observations, on every row"""
    rows, res = host(mc, "rig")
    step = 37
    for i in range(0, len(rows), step):
        name, hostile, cams, ci, uv, X = rows[i]
        poses = mc.sac_solve_rig(H.view_of(mc, cams), ci[:3], uv[:3], X[:3])
        assert len(poses) == res[0][i], name
        for k, (R, t) in enumerate(poses):
            assert R.tobytes() == res[1][i][k].tobytes() and t.tobytes() == res[2][i][k].tobytes(), name


def test_the_rig_hooks_winner_is_the_estimators(mc):
    """mcorb_host_sac_rig_roots walks the roots by hand; what the estimator runs is sac_model_rig with SacDisambiguate, which the
    CPU suite holds to sac_rig_ref.model on the bits.  On every row of the rig table the hook's winning pose is that
    restatement's pick from mcorb_sac_solve_rig's list by the fourth observation's score, or zero where it picks none"""
    import struct
    import sac_rig_cases as SRC
    import sac_rig_ref as SR
    rows, res = host(mc, "rig")
    solvers, none = {}, 0
    for i, (name, hostile, cams, ci, uv, X) in enumerate(rows):
        if id(cams) not in solvers:
            solvers[id(cams)] = SRC.solver_of(mc, cams)
        obs = [(c, p[0], p[1], 0, x) for c, p, x in zip(ci, uv, X)]
        want = SR.model(cams, obs, [0, 1, 2, 3], solvers[id(cams)])
        if want is None:
            none += 1
            assert res[4][i] == -1 and not res[5][i].any() and not res[6][i].any(), name
        else:
            assert res[4][i] >= 0, name
            assert res[5][i].tobytes() == struct.pack("<9d", *[v for row in want[0] for v in row]), name
            assert res[6][i].tobytes() == struct.pack("<3d", *want[1]), name
    assert 0 < none < len(rows)


def test_the_rows_no_scene_holds_on_the_headers_branch_outcomes():
    """scripts/header_coverage.py's third input set runs, and the committed reading names it.  needs g++ and gcov"""
    C = header_coverage()
    hooks = C.coverage("hooks")
    for h in C.HEADERS:
        assert sum(1 for v in hooks[h].values() if v > 0) > 0, h
    committed = open(os.path.join(ROOT, "profiles", "header_coverage.txt")).read()
    assert "inputs hooks" in committed and "taken by none of the three" in committed
