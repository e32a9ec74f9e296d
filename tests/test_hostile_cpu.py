"""The pose RANSACs on degenerate and hostile inputs, without a GPU: on every row of the tables of hostile_cases.py the host-only
store == the restatement (ess_ref.py, rel_ref.py, align_ref.py, sac_ref.py, sac_rig_ref.py) with the family's own same / same_counts
helpers -- doubles as raw bytes, no tolerance, no excluded row.  The tables themselves are held to what they are for: each has a
row that ends NO_MODEL after a launch, an OK row whose models come from degenerate samples, an OK row with non-finite inputs, and
essential_pose's has a hypothesis with a rejected root between two kept ones.  And the branch outcomes of the shared headers that
docs/design/09n_hostile_inputs.md lists as reached by the tables are taken by them (scripts/header_coverage.py: g++ -O0
--coverage and gcov on the stand-alone serial programs, no sanitizer), the list of outcomes nothing reaches has not grown.

test_gpu_hostile.py runs the same rows on a device store."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
import ess_cases as EC
import ess_ref as ER
import hostile_cases as HC
import kfdb_cases as K
import rel_cases as RC
import rel_ref as RR
import sac_cases as SC
import sac_ref as S
import sac_rig_cases as SRC
import sac_rig_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = os.path.join(ROOT, "docs", "design", "09n_hostile_inputs.md")


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lm(mc):
    return mc.LocalMap(mc.ORBVocabulary(device=-1).create(**K.vocabulary()), device=-1, max_landmarks=4096, max_candidates=1024)


def names(rows):
    return [r[0] for r in rows]


# ---------------------------------------------------------------------------------------------------------------------------
# one launch of a row on a store against the restatement -> the restatement (test_gpu_hostile.py uses these on both stores)
# ---------------------------------------------------------------------------------------------------------------------------
_REF = {}


def ess_ref(mc, row, seed=0):
    name, matches, kw = row
    if ("ess", name, seed) not in _REF:
        _REF["ess", name, seed] = ER.ransac(EC.CAM, matches, EC.solver_of(mc), max_iterations=HC.H, seed=seed, **kw)
    return _REF["ess", name, seed]


def ess_check(mc, lm, row, who, seed=0):
    ref = ess_ref(mc, row, seed)
    got = EC.run(mc, lm, row[1], max_iterations=HC.H, seed=seed, **row[2])
    EC.same(got, ref, "%s: %s" % (row[0], who))
    EC.same_counts(lm, ref, "%s: %s" % (row[0], who))
    return got, ref


def rel_ref(mc, row, seed=0):
    name, cams, matches, kw = row
    if ("rel", name, seed) not in _REF:
        _REF["rel", name, seed] = RR.ransac(cams, matches, kw.get("threshold", RC.THRESHOLD), RC.solver_of(mc, cams), HC.H, seed)
    return _REF["rel", name, seed]


def rel_check(mc, lm, row, who, seed=0):
    name, cams, matches, kw = row
    ref = rel_ref(mc, row, seed)
    got = RC.run(mc, lm, cams, matches, kw.get("threshold", RC.THRESHOLD), HC.H, seed)
    RC.same(got, ref, "%s: %s" % (name, who))
    RC.same_counts(lm, ref, "%s: %s" % (name, who))
    return got, ref


def align_ref(mc, row, mode, seed=0):
    name, p1, p2, kw = row
    if ("align", name, mode, seed) not in _REF:
        _REF["align", name, mode, seed] = AC.ref(mc, p1, p2, mode=mode, max_iterations=HC.H, seed=seed, **kw)
    return _REF["align", name, mode, seed]


def align_check(mc, lm, row, mode, who, seed=0, lids1=None):
    name, p1, p2, kw = row
    want = align_ref(mc, row, mode, seed)
    got = AC.run(mc, lm, p1, p2, mode=mode, lids1=lids1, max_iterations=HC.H, seed=seed, **kw)
    AC.same(got, want, "%s, mode %d: %s" % (name, mode, who))
    if mode == AR.SAC:
        AC.same_counts(lm, want, "%s: %s" % (name, who))
    return got, want


def sac_ref(mc, row, solver, seed=0):
    name, cams, obs, match, kw = row
    if ("sac", name, solver, seed) not in _REF:
        thr = kw.get("threshold", SC.THRESHOLD)
        _REF["sac", name, solver, seed] = S.ransac(cams, obs, thr, SC.solver_of(mc, cams), match, HC.H, seed) if solver == "central" else \
            SR.ransac(cams, obs, thr, SRC.solver_of(mc, cams), match, HC.H, seed)
    return _REF["sac", name, solver, seed]


def sac_check(mc, lm, row, solver, who, seed=0, forms=("pts", "lids")):
    name, cams, obs, match, kw = row
    ref = sac_ref(mc, row, solver, seed)
    got = []
    for form in forms:
        what = "%s, %s, %s: %s" % (name, solver, form, who)
        got.append(SRC.run(mc, lm, cams, obs, solver, kw.get("threshold", SC.THRESHOLD), match, HC.H, seed, form=form))
        SC.same_plain(got[-1], ref, what)
        count, valid = lm.last_ransac_counts()
        assert valid.tolist() == [m is not None for m in ref["models"]], (what, "models")
        assert count.tolist() == [c or 0 for c in ref["counts"]], (what, "counts")
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------------
# the host-only store == the restatement on every row
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", HC.ess_rows(), ids=names(HC.ess_rows()))
def test_essential_pose(mc, lm, row):
    ess_check(mc, lm, row, "host-only store")


@pytest.mark.parametrize("row", HC.rel_rows(), ids=names(HC.rel_rows()))
def test_relative_pose(mc, lm, row):
    rel_check(mc, lm, row, "host-only store")


@pytest.mark.parametrize("mode", [AR.SAC, AR.ALL])
@pytest.mark.parametrize("row", HC.align_rows(), ids=names(HC.align_rows()))
def test_align_pose(mc, lm, row, mode):
    align_check(mc, lm, row, mode, "host-only store")


@pytest.mark.parametrize("solver", ["central", "rig"])
@pytest.mark.parametrize("row", HC.sac_rows(), ids=names(HC.sac_rows()))
def test_ransac_pose(mc, lm, row, solver):
    sac_check(mc, lm, row, solver, "host-only store")


@pytest.mark.parametrize("seed", HC.SEEDS)
def test_seeds_above_32_bits(mc, lm, seed):
    """the well-posed row of every call with seeds whose upper half decides the draws: the samples differ from those of the
    lower half alone"""
    got, ref = ess_check(mc, lm, HC.ess_rows()[0], "host-only store", seed)
    assert ref["status"] == ER.OK and ref["samples"] != ess_ref(mc, HC.ess_rows()[0], seed & 0xFFFFFFFF)["samples"]
    got, ref = rel_check(mc, lm, HC.rel_rows()[0], "host-only store", seed)
    assert ref["status"] == RR.OK and ref["samples"] != rel_ref(mc, HC.rel_rows()[0], seed & 0xFFFFFFFF)["samples"]
    got, want = align_check(mc, lm, HC.align_rows()[0], AR.SAC, "host-only store", seed)
    assert want["status"] == AR.OK and want["samples"] != align_ref(mc, HC.align_rows()[0], AR.SAC, seed & 0xFFFFFFFF)["samples"]
    for solver in ("central", "rig"):
        got, ref = sac_check(mc, lm, HC.sac_rows()[0], solver, "host-only store", seed)
        assert ref["status"] == S.OK and ref["samples"] != sac_ref(mc, HC.sac_rows()[0], solver, seed & 0xFFFFFFFF)["samples"]


# ---------------------------------------------------------------------------------------------------------------------------
# what the tables are for, on the restatement alone
# ---------------------------------------------------------------------------------------------------------------------------
def finite_row(values):
    return bool(np.isfinite(np.asarray(values, np.float64)).all())


def table_conditions(refs, inputs_finite, degenerate, OK, NO_MODEL):
    """refs: {row name: restatement}; inputs_finite: {row name: bool}; degenerate: the rows whose every sample is degenerate by
    construction"""
    assert any(r["status"] == NO_MODEL for r in refs.values()), "no row ends NO_MODEL after a launch"
    assert any(refs[k]["status"] == OK and refs[k]["n_models"] > 0 for k in degenerate), "no OK row with models of degenerate samples"
    assert any(r["status"] == OK and not inputs_finite[k] for k, r in refs.items()), "no OK row with non-finite inputs"


def test_the_tables_hold_what_they_are_for(mc):
    """per call: a NO_MODEL row (a launch: the row has 64 matches), an OK row whose models all come from degenerate samples --
    zero motion and pure rotation have no essential matrix, a rig that did not move no 17-point solution, points on one plane or
    three points repeated a fit from (nearly) collinear triples, a repeated observation a three-point problem with two equal
    points --, an OK row with non-finite inputs"""
    rows = HC.ess_rows()
    assert all(len(r[1]) == HC.N for r in rows)
    table_conditions({r[0]: ess_ref(mc, r) for r in rows}, {r[0]: finite_row(r[1]) for r in rows}, ("zero motion", "pure rotation"), ER.OK,
                     ER.NO_MODEL)
    rows = HC.rel_rows()
    assert all(len(r[2]) == HC.N and len(r[1]) == HC.NCAMS_REL for r in rows)
    table_conditions({r[0]: rel_ref(mc, r) for r in rows}, {r[0]: finite_row([m[1:3] + m[4:6] for m in r[2]]) for r in rows},
                     ("zero motion", "every keypoint at the principal point"), RR.OK, RR.NO_MODEL)
    rows = HC.align_rows()
    assert all(len(r[1]) == len(r[2]) == HC.N for r in rows)
    for mode in (AR.SAC, AR.ALL):
        refs = {r[0]: align_ref(mc, r, mode) for r in rows}
        assert any(w["status"] == AR.NO_MODEL for w in refs.values())
        assert refs["three points repeated"]["status"] == AR.OK and refs["on a plane"]["status"] == AR.OK
    sac = {r[0]: align_ref(mc, r, AR.SAC) for r in rows}
    assert 0 < sac["three points repeated"]["n_models"] < HC.H      # (the collinear and coincident samples among them have none)
    assert sac["inf and NaN rows"]["status"] == AR.OK and not finite_row(rows[names(rows).index("inf and NaN rows")][1])
    rows = HC.sac_rows()
    assert all(len(S.consensus(r[2], r[3])[0]) == HC.N and len(r[1]) == HC.NCAMS_SAC for r in rows)
    for solver in ("central", "rig"):
        table_conditions({r[0]: sac_ref(mc, r, solver) for r in rows},
                         {r[0]: finite_row([[o[1], o[2]] + list(o[4]) for o in r[2]]) for r in rows}, ("half the rows one observation",), S.OK,
                         S.NO_MODEL)
        ref = sac_ref(mc, rows[names(rows).index("half the rows one observation")], solver)
        # (samples that hold observation 0 twice, under two indices, are among those that ran)
        assert any(sum(1 for i in s if i >= 0 and i % 2 == 0) >= 2 for s in ref["samples"])


def test_the_scale_rows_are_at_the_edge(mc):
    """the rows scaled down until the squares of the lengths are subnormal still end OK, and a little further down they would
    not: the scale is at the edge, found on the restatement"""
    rows = {r[0]: r for r in HC.align_rows()}
    assert align_ref(mc, rows["times 1e-158, the limits too"], AR.SAC)["status"] == AR.OK
    assert align_ref(mc, rows["times 1e-200"], AR.SAC)["status"] == AR.NO_MODEL
    p1 = rows["times 1e-158, the limits too"][1]
    d = p1[0] - p1[1]
    assert 0.0 < float(d @ d) < 2.3e-308
    rows = {r[0]: r for r in HC.sac_rows()}
    for solver in ("central", "rig"):
        ref = sac_ref(mc, rows["central rig, points times 1e-160"], solver)
        assert ref["status"] == S.OK and 0 < ref["n_models"] < HC.H
        assert sac_ref(mc, rows["every camera at the body's origin"], solver)["n_models"] == HC.H


# ---------------------------------------------------------------------------------------------------------------------------
# essential_pose: a rejected root between two kept ones
# ---------------------------------------------------------------------------------------------------------------------------
def header_coverage():
    spec = importlib.util.spec_from_file_location("header_coverage", os.path.join(ROOT, "scripts", "header_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_a_rejected_root_between_two_kept_ones(mc, lm, tmp_path):
    """tests/cpp/ess_roots.cpp walks ess_solve5's steps and says which real roots gave a model.  Its count of kept roots is the
    read-back's count of valid slots and ess_solve's count of roots for every hypothesis of every row; and in at least one
    hypothesis of the table a rejected root lies between two kept ones: the lanes of k_ess_hypotheses that hold nothing are
    then in the middle of the compaction, not at its end"""
    exe = str(tmp_path / "ess_roots")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "mc-slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ess_roots.cpp"), "-o", exe])
    H = header_coverage()
    between = []
    for row in HC.ess_rows():
        name, matches, kw = row
        (tmp_path / "in.bin").write_bytes(H.blob_ess(matches, max_iterations=HC.H, **kw))
        out = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=300, check=True).stdout.split("\n")
        kept = [ln.split()[1] for ln in out if ln]
        assert len(kept) == HC.H
        EC.run(mc, lm, matches, max_iterations=HC.H, **kw)
        count, valid, models = lm.last_essential_counts()
        ref = ess_ref(mc, row)
        for h, k in enumerate(kept):
            assert k.count("1") == int(valid[10 * h:10 * h + 10].sum()) == ref["roots"][h], (name, h, k)
            assert valid[10 * h:10 * h + 10].tolist() == [c < k.count("1") for c in range(10)], (name, h)
            if ref["roots"][h]:
                smp = ref["samples"][h]
                z = mc.ess_solve(EC.to_cam(mc), [matches[i][0:2] for i in smp], [matches[i][2:4] for i in smp], with_roots=True)[1]
                assert len(z) == k.count("1") and z == sorted(z), (name, h)
            if re.search("10+1", k):
                between.append((name, h, k))
    print("%d hypotheses with a rejected root between two kept ones, e.g. %s" % (len(between), between[:4]))
    assert between


# ---------------------------------------------------------------------------------------------------------------------------
# the branch outcomes of the shared headers
# ---------------------------------------------------------------------------------------------------------------------------
def doc_lists(path=DOC):
    """a design note in the format of docs/design/09n_hostile_inputs.md -> {(header, list name): [outcome name]}: an outcome is an
    indented line `source line  [k]`, in the last list followed by `  -- ` and the reason"""
    out, cur = {}, None
    with open(path) as f:
        for row in f:
            m = re.match(r"^\*\*(mcorb_\w+\.h): (unreached by the existing inputs|reached by the tables|still unreached)\*\*", row)
            if m:
                cur = (m.group(1), m.group(2))
                out[cur] = []
            elif row.startswith("    ") and row.strip() and cur is not None:
                name, _, reason = row.strip().partition("  -- ")
                assert cur[1] != "still unreached" or reason.strip(), ("no reason", row)
                out[cur].append(name)
            elif row.strip():
                cur = None
    return out


def hold_the_lists(H, lists, headers, hostile, existing):
    """the three lists of every header against the two readings: every "reached" outcome is taken by the tables, nothing taken by
    neither is missing from "still unreached", and the three lists are consistent"""
    for h in headers:
        for k in ("unreached by the existing inputs", "reached by the tables", "still unreached"):
            assert (h, k) in lists, (h, k)
        by_name = {H.name_of(key): key for key in hostile[h]}
        for name in lists[h, "reached by the tables"]:
            assert name in by_name, (h, "no such outcome", name)
            assert hostile[h][by_name[name]] > 0, (h, "the tables no longer take", name)
            assert name in lists[h, "unreached by the existing inputs"], (h, name)
        never = set(H.name_of(key) for key in hostile[h] if hostile[h][key] == 0 and existing[h].get(key, 0) == 0)
        assert never <= set(lists[h, "still unreached"]), (h, "reached by nothing and not listed", sorted(never - set(lists[h, "still unreached"])))
        assert set(lists[h, "reached by the tables"]) | set(lists[h, "still unreached"]) == set(lists[h, "unreached by the existing inputs"]), h


def test_the_headers_branch_outcomes(tmp_path):
    """needs g++ and gcov, as the sanitizer tests of the family need g++: fails without them"""
    H = header_coverage()
    hold_the_lists(H, doc_lists(), H.HEADERS, H.coverage("hostile"), H.coverage("existing"))
    committed = os.path.join(ROOT, "profiles", "header_coverage.txt")
    assert os.path.exists(committed) and "taken by neither" in open(committed).read()
