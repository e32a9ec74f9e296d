"""The pose RANSACs on degenerate and hostile inputs on a device store: every row of the tables of hostile_cases.py -- a camera
that has not moved, pure rotation, one match 64 times, collinear and coplanar points, overflowed, infinite and NaN keypoints,
inputs scaled until a product is subnormal -- in one launch each: the device store == the host-only store == the restatement on
the result record, the flags, sample, hypothesis and root, and every slot's count, valid flag and (essential_pose) model through
the last_*_counts read-backs; ransac_pose with both solvers and in both forms, align_pose in both modes.  Doubles are compared
as raw bytes, a NaN's sign and payload included where both stores give one.  64 matches, 64 hypotheses: a wave of hypotheses and
a partly filled tile.  What these rows run that the seeded scenes of the family's files do not: a rejected root in the middle of a
hypothesis' ten slots (k_ess_hypotheses compacts through LDS), a Gauss-Newton step that is refused, a leading coefficient that
is zero or NaN, quads and waves in which some lanes have no model.

And the well-posed row of each call with seeds above 2^32: the upper half of the seed reaches the kernels' draws.

test_hostile_cpu.py holds the same rows on the host-only store alone, and the tables to what they are for."""
import struct

import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
import ess_cases as EC
import hostile_cases as HC
import kfdb_cases as K
from test_hostile_cpu import align_check, ess_check, names, rel_check, sac_check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


WHO = ("device store", "host-only store")


def same_bytes(a, b, arrays, scalars, what):
    """two results of the library on the bytes"""
    for f in arrays:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, f, x, y)
    for f in scalars:
        x, y = getattr(a, f), getattr(b, f)
        assert (struct.pack("<d", x) == struct.pack("<d", y)) if isinstance(x, float) else x == y, (what, f, x, y)


def essential(mc, lms, row, seed=0):
    got = [ess_check(mc, lm, row, who, seed)[0] for lm, who in zip(lms, WHO)]
    EC.same_stores(got[0], got[1], row[0])
    slots = [lm.last_essential_counts() for lm in lms]
    for x, y in zip(*slots):
        assert x.tobytes() == y.tobytes(), row[0]


def relative(mc, lms, row, seed=0):
    got = [rel_check(mc, lm, row, who, seed)[0] for lm, who in zip(lms, WHO)]
    same_bytes(got[0], got[1], ("R", "t", "inliers"), ("status", "n_inliers", "n_matches", "best_hypothesis", "sample", "n_models"), row[0])


def align(mc, lms, row, mode, seed=0):
    got = [align_check(mc, lm, row, mode, who, seed)[0] for lm, who in zip(lms, WHO)]
    same_bytes(got[0], got[1], ("R", "t", "sac_R", "sac_t", "inliers"),
               ("mean_error", "status", "used", "n_inliers", "n_matches", "sac_n_inliers", "best_hypothesis", "sample", "n_models"), row[0])


def ransac(mc, lms, row, solver, seed=0):
    got = [sac_check(mc, lm, row, solver, who, seed)[0] for lm, who in zip(lms, WHO)]
    for a, b in zip(*got):
        same_bytes(a, b, ("R", "t", "sac_R", "sac_t", "inliers"),
                   ("status", "used", "n_inliers", "n_matches", "sac_n_inliers", "best_hypothesis", "sample", "n_models", "n_consensus"), row[0])


@pytest.mark.parametrize("row", HC.ess_rows(), ids=names(HC.ess_rows()))
def test_essential_pose(mc, lms, row):
    essential(mc, lms, row)


@pytest.mark.parametrize("row", HC.rel_rows(), ids=names(HC.rel_rows()))
def test_relative_pose(mc, lms, row):
    relative(mc, lms, row)


@pytest.mark.parametrize("mode", [AR.SAC, AR.ALL])
@pytest.mark.parametrize("row", HC.align_rows(), ids=names(HC.align_rows()))
def test_align_pose(mc, lms, row, mode):
    align(mc, lms, row, mode)


def test_align_pose_by_landmark_ids(mc, lms):
    """the rows whose frame-1 points a store can hold -- finite ones -- read from the store's landmark array on the device"""
    lids = np.arange(700, 700 + HC.N, dtype=np.int32)
    for row in HC.align_rows():
        if not np.isfinite(row[1]).all():
            continue
        for lm, who in zip(lms, WHO):
            lm.set(lids, row[1], np.zeros_like(row[1]))
            for mode in (AR.SAC, AR.ALL):
                align_check(mc, lm, row, mode, who + ", lids1", lids1=lids)


@pytest.mark.parametrize("solver", ["central", "rig"])
@pytest.mark.parametrize("row", HC.sac_rows(), ids=names(HC.sac_rows()))
def test_ransac_pose(mc, lms, row, solver):
    ransac(mc, lms, row, solver)


@pytest.mark.parametrize("seed", HC.SEEDS)
def test_seeds_above_32_bits(mc, lms, seed):
    """1 << 32, (1 << 63) + 1 and 2^64 - 1 on the well-posed row of every call, against the restatement: the job carries all 64
    bits to the device (test_hostile_cpu.py: the samples differ from those of the lower half alone)"""
    essential(mc, lms, HC.ess_rows()[0], seed)
    relative(mc, lms, HC.rel_rows()[0], seed)
    align(mc, lms, HC.align_rows()[0], AR.SAC, seed)
    for solver in ("central", "rig"):
        ransac(mc, lms, HC.sac_rows()[0], solver, seed)
