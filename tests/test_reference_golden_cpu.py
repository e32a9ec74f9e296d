"""The oracle against RECORDED results of the reference binary (tests/golden/ref_*.npz, written by
tests/golden/make_ref_golden.py where oracle/_ref/libmcslam_ref_orb.so exists): the reference's own ORBextractor.cpp, compiled
unchanged against the stand-in cv:: types of oracle/refcv.  Needs no binary and never skips.

Pinned by this: the reference's own logic (tables aside, everything operator() does around the primitives, DistributeOctTree,
IC_Angle, computeOrbDescriptor).  Not pinned: OpenCV's five primitives (FAST, resize, copyMakeBorder, GaussianBlur,
fastAtan2) -- the recording binary took them from the oracle (tests/ref_lib.py).  Bit for bit, no tolerance."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import ref_lib as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ref_golden as G  # noqa: E402


@pytest.mark.parametrize("name", sorted(G.EXTRACTIONS))
def test_oracle_equals_recorded_reference_extraction(name):
    spec, rec = G.EXTRACTIONS[name], G.load(name)
    nf, sf, nl, ini, mn = spec[5]
    assert np.array_equal(rec["params"], np.array(spec[5], np.float64)) and tuple(rec["lap"]) == spec[6]
    for c in range(spec[1]):
        img = G.image(spec, c)
        assert np.array_equal(G.sha1(img), rec["img_sha1_%d" % c]), "the input image is not the recorded one"
        ora = O.OracleExtractor(nf, sf, nl, ini, mn)
        got = ora(img, lap=spec[6])
        R.same_as_record("%s cam %d" % (name, c), rec, c, got, levels=[ora.level(l) for l in range(nl)],
                         bordered=[ora.level_bordered(l) for l in range(nl)], level_counts=[len(ora.level_keypoints(l)) for l in range(nl)])
    assert len(got[1]) > 0.5 * nf


def test_recorded_cases_are_what_they_are_for():
    """the clustered image drives a deep tree: more than a hundred level-0 keypoints kept inside the 80 x 80 patch, some only 2 or 3
    pixels apart, so the tree divided a 768-pixel root down to nodes of that size; the lapping case has both parts"""
    k = R.unpack_keypoints(G.load("ref_clustered_800x600_n1500_l2"), "kps_0")
    p = k[(k["octave"] == 0) & (k["x"] > 450) & (k["x"] < 530) & (k["y"] > 250) & (k["y"] < 330)]
    pts = np.stack([p["x"], p["y"]], 1)
    apart = np.abs(pts[:, None] - pts[None]).max(-1) + np.eye(len(pts)) * 99
    assert len(p) > 100 and apart.min() <= 3
    rec = G.load("ref_lapping_752x480_n600")
    assert 0 < rec["mono_0"][0] < rec["kps_0"].shape[1]


def test_oracle_equals_recorded_reference_octree():
    rec = G.load(G.OCTREE)
    n = sum(1 for k in rec if k.startswith("kept_"))
    assert n >= 5
    for i in range(n):
        x0, x1, y0, y1, N = (int(v) for v in rec["region_N_%d" % i])
        cnt, got = O.distribute_octree(rec["x_%d" % i], rec["y_%d" % i], rec["resp_%d" % i], x0, x1, y0, y1, N)
        assert cnt == len(rec["kept_%d" % i]), "stage DistributeOctTree case %d: %d keys, recorded reference %d" % (i, cnt, len(rec["kept_%d" % i]))
        R.same("DistributeOctTree case %d (recorded reference), index of every retained key in result order" % i, rec["kept_%d" % i], got)


@pytest.mark.parametrize("name", sorted(G.ROTATED))
def test_oracle_equals_recorded_reference_rotated_brief(name):
    """staged (the reference never calls IC_Angle): the recorded angles are the reference's IC_Angle at the keypoints the oracle
    keeps, the recorded bytes its computeOrbDescriptor at those angles"""
    spec, rec = G.ROTATED[name], G.load(name)
    nf, sf, nl, ini, mn = spec[5]
    img = G.image(spec, 0)
    assert np.array_equal(G.sha1(img), rec["img_sha1_0"])
    ora = O.OracleExtractor(nf, sf, nl, ini, mn, 1)
    mono, k, d = ora(img)
    lk = np.concatenate([ora.level_keypoints(l) for l in range(nl)])
    R.same_keypoints("%s, level keypoints with IC_Angle (recorded reference)" % name, R.unpack_keypoints(rec, "level_kps"), lk)
    R.same("%s, computeOrbDescriptor (recorded reference)" % name, rec["desc"], d)
    assert len(d) > 0.8 * nf and len(np.unique(lk["angle"])) > 0.5 * len(lk)


def test_reference_undefined_oracle_refuses():
    """nIni = round(width / height) < 1, a region more than twice as tall as wide: the reference divides by zero for hX and
    indexes an empty vpIniNodes.  The oracle answers -2 and the reference is never called there."""
    n, _ = O.distribute_octree(np.array([5.0]), np.array([5.0]), np.array([20.0]), 16, 216, 16, 516, 10)
    assert n == -2
    # a level too small for one 35-pixel cell (nCols or nRows = 0, ceil(width / 0)): -2 from orc_extract
    assert O.OracleExtractor(500, 1.2, 8)(np.zeros((100, 100), np.uint8))[0] == -2
