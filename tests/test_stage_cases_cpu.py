"""The stage matrix's coverage claim, checked without a GPU: stage_cases.CASES reach every launch variant of CHECKLIST (by the
restated launch arithmetic), and the oracle's output on their images has the properties that make the GPU comparison of
test_gpu_stages.py mean something (candidates in the narrow tail cells, none in skipped ones, every candidate kept at the large
budget, cells with more than 64 candidates, responses of 254, empty images).  The pyramid expectation is cross-checked through
a second path of the oracle (resize_linear of the previous level)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import stage_cases as S

ALL_TAGS = {c.name: S.tags(c) for c in S.CASES}


@pytest.mark.parametrize("tag", S.CHECKLIST)
def test_checklist_item_is_reached(tag):
    assert any(tag in t for t in ALL_TAGS.values()), "no case of stage_cases.CASES reaches %r any more" % tag


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_every_case_is_needed_and_within_the_size_limit(case):
    """each case carries a tag no other case does (else it is redundant and goes), and it is the tag written beside it"""
    assert case.W * case.H <= S.MAX_PIXELS
    own = S.OWN_TAG[case.name]
    assert own in ALL_TAGS[case.name], "%s no longer reaches %r: %s" % (case.name, own, sorted(ALL_TAGS[case.name]))
    others = [o.name for o in S.CASES if o is not case and own in ALL_TAGS[o.name]]
    assert not others, "%s: %r is also reached by %s" % (case.name, own, others)


def test_case_table_is_complete():
    assert sorted(S.OWN_TAG) == sorted(c.name for c in S.CASES) and len(S.CASE_BY_NAME) == len(S.CASES)
    assert not set(S.UNREACHABLE) & set(S.CHECKLIST)
    assert len(S.CONTENTS) == 10 and S.CONTENT_NAMES[:2] == ["noise", "binary"]
    i = S.CONTENT_NAMES.index("flat")
    assert S.CONTENT_NAMES[i - 1] in S.DENSE_CONTENTS and S.CONTENT_NAMES[i + 1] in S.DENSE_CONTENTS


def test_unreachable_item_really_is():
    """no image within the size limit has a last cell row that the reference's `iniY >= maxBorderY - 3` rule skips: scan every
    height up to the limit at the narrowest width whose nIni is still 1"""
    for h in range(67, 1400):
        mby, span, n = S._axis(h)
        cell = -(-span // n)
        state = S._cells_1d(mby, n, cell, 3)[-1][3]
        if state in ("skipped", "beyond"):
            w_min = next(w for w in range(67, 4000) if int(np.floor(float(np.float32(w - 32) / np.float32(span)) + 0.5)) >= 1)
            assert w_min * h > S.MAX_PIXELS, "%dx%d reaches a skipped last row within the limit: add it" % (w_min, h)


def test_compact_forms_reached():
    """k_compact's four forms: 512 / 1024 threads by batch size (ten contents, or the first two), four table copies or one by
    the bucket count of the budget (launch_compact)"""
    forms = set()
    for c in S.CASES:
        for n in S.budgets(c):
            ex = S.oracle_extractor(c, n)
            g = S.geometry(c.W, c.H, c.nlevels, c.scale, quotas=ex.tables()["quota"])
            forms |= {(S.compact_threads(nimg), g["job"]["compact_copies"]) for nimg in (len(S.CONTENTS), 2)}
    assert forms == {(512, 4), (512, 1), (1024, 4), (1024, 1)}


@functools.lru_cache(maxsize=1)
def _stages(name):
    case = S.CASE_BY_NAME[name]
    ex = S.oracle_extractor(case, S.budgets(case)[0])
    return {cn: S.oracle_stages(ex, img) for cn, img in zip(S.CONTENT_NAMES, S.images(case))}


def _cand_cells(L, cand):
    x, y, _ = cand
    return ((y - 3) // L["hCell"]) * L["nCols"] + (x - 3) // L["wCell"]


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_oracle_conditions(case):
    st = _stages(case.name)
    geo = S.geometry(case.W, case.H, case.nlevels, case.scale)
    th = (case.ini_th, case.min_th)
    # level l of the extractor == resize_linear(level l - 1): the pyramid expectation through a second path
    for cn, s in st.items():
        for l in range(1, case.nlevels):
            h, w = s["level"][l].shape
            assert (w, h) == (geo["levels"][l]["w"], geo["levels"][l]["h"])
            d = S.diff_plane(s["level"][l], O.resize_linear(s["level"][l - 1], w, h))
            assert d is None, "%s %s: level %d is not resize_linear of level %d: %s" % (case.name, cn, l, l - 1, d)
    # the flat image and the (255, 255) case: nothing anywhere
    for cn, s in st.items():
        if cn == "flat" or th == (255, 255):
            assert [len(c[0]) for c in s["cand"]] == [0] * case.nlevels and len(s["kps"]) == 0, (case.name, cn)
    if th == (255, 255):
        return
    if th == (254, 254):
        r = np.concatenate([c[2] for c in st["binary"]["cand"]])
        assert len(r) > 50 and (r == 254).all(), "binary content at (254, 254): %d candidates, responses %s" % (len(r), np.unique(r))
        return
    # binary content: responses reach 254
    assert max(int(c[2].max()) for c in st["binary"]["cand"] if len(c[2])) == 254
    # the flat image's neighbours in the batch are dense
    for cn in S.DENSE_CONTENTS:
        assert len(st[cn]["cand"][0][0]) >= 4 * geo["levels"][0]["nCols"] * geo["levels"][0]["nRows"], (case.name, cn)
    noise = st["noise"]["cand"]
    # k_compact's extra trips: a cell with more than 64 candidates
    assert max(int(np.bincount(_cand_cells(L, noise[L["level"]])).max()) for L in geo["levels"]) > 64
    # tail cells: candidates where the arithmetic says the last cell evaluates 1 to 3 columns (rows), none where it is off
    for L in geo["levels"]:
        for axis, span, (ini, roi, ev, state) in ((0, L["W0"], L["last_col"]), (1, L["H0"], L["last_row"])):
            v = noise[L["level"]][axis]
            first = ini + 3 - S.MIN_BORDER        # the first coordinate only the last cell evaluates
            tail = v[v >= first]
            what = "%s level %d %s: last cell at %d, ROI %d, %s" % (case.name, L["level"], "xy"[axis], ini, roi, state)
            if state == "on":
                assert len(tail) > 0 and tail.max() == span - 4 and tail.min() >= span - 3 - ev, "%s: %s" % (what, np.unique(tail))
                if ev <= 3:
                    assert v.max() == span - 4 and len(np.unique(tail)) <= ev
            else:
                assert len(tail) == 0, "%s: candidates at %s" % (what, np.unique(tail))
                assert v.max() == span - 4    # (the cell before it reaches to the border: its ROI is six pixels longer)
    # every candidate kept at the large budget: the feature comparison then checks every descriptor FAST can ask for
    if S.keep_all(case):
        for cn in S.KEEP_ALL_CONTENTS:
            total = sum(len(c[0]) for c in st[cn]["cand"])
            assert len(st[cn]["kps"]) == total, "%s %s: %d of %d candidates kept at %d features" % (
                case.name, cn, len(st[cn]["kps"]), total, S.KEEP_ALL)
