"""The back end's and mapping's calls on degenerate and hostile inputs on a device store: every row of the tables of
hostile_backend_cases.py -- a window that did not move or only rotated, every landmark one point, on the line through two camera
centres, on one plane, at a camera centre, keypoints at the principal point, repeated, given twice, overflowed, infinite and NaN,
an R that is no rotation, a NaN and an inf in each operand position, points and translations scaled until a square is subnormal
or infinite -- in one chain each: the device store == the host-only store == the restatement, with the helpers of
test_hostile_backend_cpu.py, and the two stores' results against each other on the bytes, a NaN's sign and payload included.
bundle_adjust and refine_pose run in both forms; retriangulate in report mode and, where the restatement ends a landmark in a failed
verdict, in apply mode on ids of the row's own, the store read back and compared with the twin's.  68 landmarks, observations
or matches: a full wave and a part of the next.  What these rows run that the seeded scenes of the calls' own files do not: the
minimum and the NaN-to-inf maximum of k_retri_solve's 16 lanes over non-finite z and errors, landmarks of k_ba_linearize and
k_ba_update whose pivot is not > 0 beside active ones in one wave, ba_decide on a NaN cost.

test_hostile_backend_cpu.py holds the same rows on the host-only store alone, and the tables to what they are for."""
import pytest

import hostile_backend_cases as HB
import kfdb_cases as K
import mapping_new_cases as Nc
from hostile_backend_cases import names
from test_gpu_hostile import WHO, same_bytes
from test_gpu_init import same as same_init, same_store as same_init_store
from test_hostile_backend_cpu import MAXL, ba_check, init_check, neigh_check, new_check, pose_check, retri_apply, retri_check

pytestmark = pytest.mark.gpu

NEIGH_ARRAYS = ("inliers", "verdict", "new_lid", "pt3d", "normal", "dist2", "cos_parallax", "neigh_skipped", "depth_vec", "lids_cur")


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lms(mc):
    vocs = mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    return [mc.LocalMap(voc, device=dev, max_landmarks=MAXL, max_candidates=1024) for voc, dev in zip(vocs, (0, -1))]


@pytest.mark.parametrize("row", HB.ba_rows(), ids=names(HB.ba_rows()))
def test_bundle_adjust(mc, lms, row):
    got = [ba_check(mc, lm, row, who)[0] for lm, who in zip(lms, WHO)]
    for a, b in zip(*got):
        same_bytes(a, b, ("R", "t", "pts", "inliers"), ("status", "iterations", "cost_initial", "cost_final", "n_inliers", "n_obs"), row[0])


@pytest.mark.parametrize("row", HB.retri_rows(), ids=names(HB.retri_rows()))
def test_retriangulate(mc, lms, row):
    got = [retri_check(mc, lm, row, who) for lm, who in zip(lms, WHO)]
    fields = (("pts", "diff_norm", "n_views", "verdict"), ("counts", "n_pairs", "pairs"))
    same_bytes(got[0][0], got[1][0], *fields, row[0])
    if HB.failed(got[0][1]):
        after = [retri_apply(mc, lm, row, who) for lm, who in zip(lms, WHO)]
        same_bytes(after[0][0], after[1][0], *fields, row[0] + ", apply")
        assert after[0][1] == after[1][1], (row[0], "the stores after apply")


@pytest.mark.parametrize("row", HB.pose_rows(), ids=names(HB.pose_rows()))
def test_refine_pose(mc, lms, row):
    got = [pose_check(mc, lm, row, who)[0] for lm, who in zip(lms, WHO)]
    for a, b in zip(*got):
        same_bytes(a, b, ("R", "t", "inliers"), ("status", "iterations", "cost_initial", "cost_final", "n_inliers", "n_obs"), row[0])


@pytest.mark.parametrize("row", HB.new_rows(), ids=names(HB.new_rows()))
def test_triangulate_new(mc, lms, row):
    got = [new_check(mc, lm, row, who)[0] for lm, who in zip(lms, WHO)]
    Nc.same(got[0], got[1], row[0])
    same_init_store(lms[0], lms[1], got[0].new_lid[got[0].new_lid >= 0], row[0])      # the new landmarks as the two stores hold them


@pytest.mark.parametrize("row", HB.neigh_rows(), ids=names(HB.neigh_rows()))
def test_triangulate_neighbours(mc, lms, row):
    got = [neigh_check(mc, lm, row, who)[0] for lm, who in zip(lms, WHO)]
    same_bytes(got[0], got[1], NEIGH_ARRAYS, ("n_triangulated", "next_lid"), row[0])
    for a, b in zip(got[0].lids_neigh, got[1].lids_neigh):
        assert a.tolist() == b.tolist(), row[0]
    same_init_store(lms[0], lms[1], got[0].new_lid[got[0].new_lid >= 0], row[0])      # the new landmarks as the two stores hold them


@pytest.mark.parametrize("row", HB.init_rows(), ids=names(HB.init_rows()))
def test_initialize(mc, lms, row):
    got = [init_check(mc, lm, row, who)[0] for lm, who in zip(lms, WHO)]
    same_init(got[0], got[1], row[0])
    same_init_store(lms[0], lms[1], got[0].new_lid[got[0].new_lid >= 0], row[0])
