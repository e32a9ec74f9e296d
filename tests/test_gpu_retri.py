"""The re-triangulation after the back end moved keyframes on a device store (LocalMap.retriangulate: k_retri_views and
k_retri_solve in one submission): the device store == the host-only store == the plain-Python restatement (retri_ref.py), floats
as raw bytes, no tolerance, no excluded case.  The checks are test_retri_cpu.py's, run on both stores.

On the commit before this call existed every test of this file fails (`python -m pytest -m gpu tests/test_gpu_retri.py`):
LocalMap has no retriangulate."""
import numpy as np
import pytest

import kfdb_cases as K
import retri_cases as RC
import retri_ref as R
import test_retri_cpu as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def vocs(mc):
    return mc.ORBVocabulary().create(**K.vocabulary()), mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture(scope="module")
def lms(mc, vocs):
    assert hasattr(mc.LocalMap, "retriangulate")
    return [mc.LocalMap(voc, device=dev, max_landmarks=4096, max_candidates=64) for voc, dev in zip(vocs, (0, -1))]


def test_view_counts(mc, lms):
    TC.check_view_counts(mc, lms)


@pytest.mark.parametrize("n", RC.LANDMARK_COUNTS)
def test_landmark_counts(mc, lms, n):
    TC.check_landmark_counts(mc, lms, n)


@pytest.mark.parametrize("nkf", [1, 17, 1024])
def test_keyframe_counts(mc, lms, nkf):
    TC.check_keyframe_counts(mc, lms, nkf)


@pytest.mark.parametrize("ncams", [1, 4, 16])
def test_rigs(mc, lms, ncams):
    TC.check_rigs(mc, lms, ncams)


def test_hand_rows(mc, lms):
    TC.check_hand_rows(mc, lms)


def test_thresholds_from_the_restatement(mc, lms):
    TC.check_thresholds_from_the_restatement(mc, lms)


def test_apply(mc, vocs):
    TC.check_apply(mc, lambda: mc.LocalMap(vocs[0], device=0, max_landmarks=64, max_candidates=64))


def test_apply_writes_the_hbm_point(mc, lms):
    """the gated store lands in the device store's point, and a following report reads it from there: diff_norm 0"""
    sc = RC.synth(4, 2, [3, 4, 5, 2] * 20, seed=13)
    want = RC.ref(sc)
    lids = RC.fill(lms[0], sc, first_lid=100)
    got = RC.run(mc, lms[0], sc, lids=lids, apply=True, cap=0)
    RC.same(got, want, "apply")
    assert got.counts[R.VALID_UPDATED] == 80 and got.pairs == []
    assert np.array([lms[0].get(int(l))[0] for l in lids]).tobytes() == got.pts.tobytes()
    again = RC.run(mc, lms[0], sc, lids=lids)
    assert not again.diff_norm.any() and again.pts.tobytes() == got.pts.tobytes()


def test_search_after_apply(mc, vocs):
    TC.check_search_after_apply(mc, vocs[0], 0)


def test_end_to_end(mc, lms):
    TC.check_end_to_end(mc, lms)


def test_moved_observations(mc, lms):
    TC.check_moved_observations(mc, lms)


def test_timing(mc, lms):
    """positive after a launch, unchanged by a call that launches nothing"""
    sc = RC.synth(4, 2, [3] * 100, seed=14)
    got = RC.run(mc, lms[0], sc)
    us = lms[0].last_retri_timing()
    assert got.launched and all(u > 0 for u in us)
    idle = RC.run(mc, lms[0], dict(sc, moved=[False] * 4))
    assert not idle.launched and idle.counts[R.NOT_SELECTED] == 100 and lms[0].last_retri_timing() == us
    assert lms[1].last_retri_timing() == (0.0, 0.0)
    print("retriangulate, 100 landmarks, spans in us: %s" % ", ".join("%.1f" % u for u in us))


def test_refusals_on_a_device_store(mc, lms):
    """every refusal of test_retri_cpu.py, the store read back unchanged"""
    TC.check_refusals(mc, lms[0])
