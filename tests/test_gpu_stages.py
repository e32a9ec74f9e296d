"""Every extraction stage against the oracle, tolerance zero, on the stage matrix of stage_cases.py: small images whose level
geometry steers k_resize, k_fast_cells, k_compact, k_blur and the descriptor kernels into each of their shape-dependent
variants (test_stage_cases_cpu.py proves which).  Per image and level: every pyramid pixel, every blurred pixel, the FAST
candidate list (x, y, response) in vToDistributeKeys order; per image: monoIndex, every keypoint field, every descriptor byte.
At the keep-all budget the oracle keeps every candidate, so the descriptor of every candidate FAST emits is compared, the ones
in the narrow tail cells included.  A failure names the case, the content, the level and the first differing element."""
import functools

import numpy as np
import pytest

import limits_ref as R
import stage_cases as S

pytestmark = pytest.mark.gpu

BUDGETED = [(c, n) for c in S.CASES for n in S.budgets(c)]
KEEP_ALL_CASES = [c for c in S.CASES if S.keep_all(c)]


def _id(v):
    return v.name if isinstance(v, S.Case) else "n%d" % v


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@functools.lru_cache(maxsize=2)
def _expected(name, nfeatures, orientation=0):
    """the oracle's stages of every content of a case, computed once and shared by the jobs compared with it (read only)"""
    case = S.CASE_BY_NAME[name]
    ex = S.oracle_extractor(case, nfeatures, orientation)
    return [S.oracle_stages(ex, img) for img in S.images(case)]


def _rig(mc, case, nimg, nfeatures, **kw):
    return mc.Rig(1, case.W, case.H, max_frames=nimg, nslots=1, nfeatures=nfeatures, scale_factor=case.scale, nlevels=case.nlevels,
                  ini_th_fast=case.ini_th, min_th_fast=case.min_th, **kw)


def _run(rig, imgs):
    rig.upload(imgs)
    rig.extract(len(imgs))


def _check_geometry(rig, case):
    """the restated launch arithmetic describes the launches that ran"""
    geo = S.geometry(case.W, case.H, case.nlevels, case.scale)
    info = rig.info()
    got = dict(sizes=[rig.level_size(l) for l in range(case.nlevels)], cells=info["cells"], cell_cap=info["cell_cap"],
               nlevels=info["nlevels"], tiles=info["tiles"])
    want = dict(sizes=[(L["w"], L["h"]) for L in geo["levels"]], cells=geo["job"]["cells"], cell_cap=geo["job"]["cell_cap"],
                nlevels=case.nlevels, tiles=geo["job"]["tiles"])
    assert got == want, "%s: the library's geometry %s is not the restatement's %s" % (case.name, got, want)


def _compare(rig, case, what, exp, with_features=True):
    """images 0 .. len(exp) - 1 of the rig's last job against the expectation; one assertion with every image's first differences"""
    msgs = []
    for m, e in enumerate(exp):
        msgs += ["%s, image %d (%s): %s" % (what, m, S.CONTENT_NAMES[m], d) for d in S.diff_image(rig, m, e, with_features)]
    assert not msgs, "%s [select_fallbacks %d]: %d differences from the oracle\n%s" % (
        case.name, rig.select_fallbacks(), len(msgs), "\n".join(msgs[:12]))


@pytest.mark.parametrize("case,nfeatures", BUDGETED, ids=_id)
def test_stages_match_oracle(mc, case, nfeatures):
    """One job over the ten contents (512-thread k_compact, copied results) and one over the first two (1024 threads,
    host-mapped results).  The flat image lies between two dense ones of the batch and must come back empty."""
    imgs, exp = S.images(case), _expected(case.name, nfeatures)
    kw = dict(selection=2) if nfeatures == 300 else {}
    for nimg in (len(imgs), 2):
        rig = _rig(mc, case, nimg, nfeatures, **kw)
        try:
            if nfeatures == 300:
                assert rig.select_mode() == "gpu", "%s: selection=2 at 300 features runs on the %s" % (case.name, rig.select_mode())
            _check_geometry(rig, case)
            _run(rig, imgs[:nimg])
            what = "%d features, batch of %d" % (nfeatures, nimg)
            _compare(rig, case, what, exp[:nimg])
            if nimg > 2:
                m = S.CONTENT_NAMES.index("flat")
                ncand = [len(rig.candidates(m, l)[0]) for l in range(case.nlevels)]
                assert ncand == [0] * case.nlevels and len(rig.features(m)[1]) == 0, \
                    "%s, %s: the flat image between two dense ones has candidates per level %s, %d keypoints [select_fallbacks %d]" % (
                        case.name, what, ncand, len(rig.features(m)[1]), rig.select_fallbacks())
            print("[stages] %s %s: select_mode %s, select_fallbacks %d" % (case.name, what, rig.select_mode(), rig.select_fallbacks()))
        finally:
            rig.close()


@pytest.mark.parametrize("case", KEEP_ALL_CASES, ids=_id)
def test_plane_descriptor_path_matches_oracle(mc, monkeypatch, case):
    """MCORB_BLUR_PLANES=1 at rig creation: k_blur over whole levels with the job and k_describe on the planes, instead of
    k_describe_fused; every candidate's descriptor at the keep-all budget"""
    monkeypatch.setenv("MCORB_BLUR_PLANES", "1")
    imgs, exp = S.images(case), _expected(case.name, S.KEEP_ALL)
    rig = _rig(mc, case, len(imgs), S.KEEP_ALL)
    try:
        _run(rig, imgs)
        _compare(rig, case, "blur planes, %d features" % S.KEEP_ALL, exp)
    finally:
        rig.close()


# (case, budget) whose k_compact runs four table copies by default: the knob changes the launch
ONE_COPY = [("99x97_l1", S.KEEP_ALL), ("1083x100_l1", 300)]


@pytest.mark.parametrize("name,nfeatures", ONE_COPY, ids=["%s-n%d" % j for j in ONE_COPY])
def test_compact_one_copy_matches_oracle(mc, monkeypatch, name, nfeatures):
    """MCORB_COMPACT_ONE_COPY=1 at rig creation: k_compact with one copy of its bucket tables in LDS, at both workgroup sizes"""
    case = S.CASE_BY_NAME[name]
    quotas = S.oracle_extractor(case, nfeatures).tables()["quota"]
    assert S.geometry(case.W, case.H, case.nlevels, case.scale, quotas=quotas)["job"]["compact_copies"] == S.COMPACT_COPIES
    monkeypatch.setenv("MCORB_COMPACT_ONE_COPY", "1")
    imgs, exp = S.images(case), _expected(name, nfeatures)
    for nimg in (len(imgs), 2):
        rig = _rig(mc, case, nimg, nfeatures)
        try:
            _run(rig, imgs[:nimg])
            _compare(rig, case, "one table copy, %d features, batch of %d" % (nfeatures, nimg), exp[:nimg])
        finally:
            rig.close()


@pytest.mark.parametrize("name", ["99x97_l1", "308x116_l2", "1083x100_l1"])
def test_orientation_mode_matches_oracle_and_restatement(mc, name):
    """orientation = 1 at the keep-all budget: stages and keypoints (angles included) equal the oracle's; descriptors equal
    computeOrbDescriptor restated with double-rounded cos / sin (what k_describe_oriented computes) on the job's own blurred
    planes and level keypoints"""
    case = S.CASE_BY_NAME[name]
    imgs, exp = S.images(case), _expected(name, S.KEEP_ALL, 1)
    rig = _rig(mc, case, len(imgs), S.KEEP_ALL, orientation=1)
    try:
        _run(rig, imgs)
        _compare(rig, case, "orientation mode", exp, with_features=False)
        scale = mc.get_tables(rig.params)["scale"]
        for m, e in enumerate(exp):
            what = "%s, orientation mode, image %d (%s)" % (name, m, S.CONTENT_NAMES[m])
            mono, k, d = rig.features(m)
            diff = S.diff_features((mono, k, e["desc"]), (e["mono"], e["kps"], e["desc"]))   # keypoints only
            assert diff is None, "%s: %s" % (what, diff)
            for l in range(case.nlevels):
                sel = k["octave"] == l
                kl = k[sel]
                lx = np.rint(kl["x"].astype(np.float64) / float(scale[l])).astype(np.float32)   # level coordinates are integers
                ly = np.rint(kl["y"].astype(np.float64) / float(scale[l])).astype(np.float32)
                assert np.array_equal(lx, e["level_kps"][l]["x"]) and np.array_equal(ly, e["level_kps"][l]["y"]), what
                restated = R.describe_restated(rig.level(m, l, blurred=True), lx, ly, kl["angle"], R.trig_double)
                bad = R.first_diff(d[sel], restated)
                assert bad is None, "%s: descriptor of level %d keypoint (%g, %g), angle %r, differs from the restatement: %s / %s" % (
                    what, l, lx[bad], ly[bad], float(kl["angle"][bad]), d[sel][bad].tobytes().hex(), restated[bad].tobytes().hex())
    finally:
        rig.close()
