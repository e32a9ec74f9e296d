"""The slot entry of fast tracking where no GPU is needed: what mcorb_lmap_track_rig_frame refuses before it looks at a rig, on a
host-only store, and the four-kernel timing call there.

On the commit before this call existed every test of this file fails (`python -m pytest tests/test_track_rig_cpu.py`): LocalMap has
no track_rig_frame and no last_track_timing4."""
import numpy as np
import pytest

import kfdb_cases as K
import track_cases as T
from test_track_cpu import D0


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def lm(mc):
    voc = mc.ORBVocabulary(device=-1).create(**K.vocabulary())
    lm = mc.LocalMap(voc, device=-1, max_landmarks=64, max_candidates=16)
    T.fill(lm, T.flat_store([(100.0 + 3 * i, 50.0, T.desc_at(D0, i % 5)) for i in range(20)]))
    lm.voc_kept = voc
    return lm


def test_a_null_rig_is_refused_and_the_store_unchanged(mc, lm):
    L = mc._lib
    before = T.snapshot(lm, range(20))
    for ncams in (1, 4):
        view = T.to_view(mc, T.flat_view(ncams=ncams))
        for slot, frame in ((0, 0), (3, 0), (0, -1), (-1, 7)):
            err = T.expect(mc, L.E_ARG, lambda: lm.track_rig_frame(view, None, frame, list(range(10)), slot=slot))
            assert err.n_candidates == 0 and err.n_proj == [0] * ncams and err.n_match == [0] * ncams
    assert T.snapshot(lm, range(20)) == before


def test_the_arguments_are_checked_before_the_rig(mc, lm):
    """what mcorb_lmap_track refuses about the view, the ids and the gate is refused here as well, rig or no rig"""
    L = mc._lib
    view = T.to_view(mc, T.flat_view())
    T.expect(mc, L.E_ARG, lambda: lm.track_rig_frame(view, None, 0, [0, 1], max_hamming=-1))
    bad = T.to_view(mc, T.flat_view())
    bad.ncams = L.MAX_CAMS + 1
    code = L.load().mcorb_lmap_track_rig_frame(lm.h, bad, None, 0, 0, None, 0, 10000.0, 20, mc._lib.TrackOut())
    assert code == L.E_ARG


def test_timing4_on_a_host_only_store(mc, lm):
    """as last_track_timing there: the call succeeds and nothing was ever launched"""
    assert lm.last_track_timing() == (0.0, 0.0)
    assert lm.last_track_timing4() == (0.0, 0.0, 0.0, 0.0)
    xy, ds = [np.array([[100.0, 50.0]], np.float32)], [np.array([D0])]
    assert lm.track(T.to_view(mc, T.flat_view()), xy, ds, list(range(10))).n_candidates == 10
    assert lm.last_track_timing4() == (0.0, 0.0, 0.0, 0.0) and lm.last_track_timing() == (0.0, 0.0)
