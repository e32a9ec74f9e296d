"""The batched slot entry of fast tracking (LocalMap.track_rig_frames, track_rig_frames_submit, track_frames_wait) where no GPU is
needed: what a host-only store refuses before it looks at a rig, and track_frames_wait serving a pending single submission as a
batch of one.  Bit for bit, floats as raw bytes.  No GPU.

On the commit before the batch existed every test of this file fails (`python -m pytest tests/test_track_batch_cpu.py`): LocalMap
has no track_rig_frames and no track_frames_wait."""
import pytest

import kfdb_cases as K
import track_cases as T


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


@pytest.fixture(scope="module")
def voc(mc):
    return mc.ORBVocabulary(device=-1).create(**K.vocabulary())


@pytest.fixture(scope="module")
def seeded():
    return T.scene(2)


def store_of(mc, voc, store):
    lm = mc.LocalMap(voc, device=-1, max_landmarks=4096, max_candidates=1024)
    T.fill(lm, store)
    return lm


def no_counts(err):
    return not any(err.n_candidates) and not any(any(p) for p in err.n_proj) and not any(any(p) for p in err.n_match)


def test_refusals_before_the_rig_is_read(mc, voc, seeded):
    L = mc._lib
    v, store, kps, descs, lids = seeded
    lm = store_of(mc, voc, store)
    view = T.to_view(mc, v)
    watched = sorted(store)[::50]
    before = T.snapshot(lm, watched)
    assert L.TRACK_MAX_FRAMES == 32
    for nf, what in ((1, "a NULL rig"), (3, "a NULL rig, three frames"), (0, "nf = 0"), (33, "nf = 33")):
        for call in (lambda: lm.track_rig_frames([view] * nf, None, list(range(nf)), [lids] * nf),
                     lambda: lm.track_rig_frames_submit([view] * nf, None, list(range(nf)), [lids] * nf)):
            err = T.expect(mc, L.E_ARG, call)
            assert not hasattr(err, "n_candidates") or (len(err.n_candidates) == nf and no_counts(err)), what
            T.expect(mc, L.E_STATE, lambda: lm.track_frames_wait())           # nothing is pending
    assert T.snapshot(lm, watched) == before
    T.same(T.as_lists(lm.track(view, kps, descs, lids)), T.as_lists(store_of(mc, voc, store).track(view, kps, descs, lids)),
           "the store after the refusals against a fresh one")


def test_frames_wait_without_a_pending_call(mc, voc, seeded):
    lm = store_of(mc, voc, seeded[1])
    T.expect(mc, mc._lib.E_STATE, lambda: lm.track_frames_wait())
    T.expect(mc, mc._lib.E_STATE, lambda: lm.track_frames_wait())


def test_frames_wait_serves_a_single_submission(mc, voc, seeded):
    v, store, kps, descs, lids = seeded
    lm = store_of(mc, voc, store)
    view = T.to_view(mc, v)
    want = lm.track(view, kps, descs, lids)
    assert want.n_candidates == len(store) and all(len(m) for m in want.match_kp)
    lm.track_submit(view, kps, descs, lids)
    got = lm.track_frames_wait()
    assert isinstance(got, list) and len(got) == 1
    T.same(T.as_lists(got[0]), T.as_lists(want), "track_frames_wait after track_submit against track")
    assert got[0].n_candidates == want.n_candidates
    T.expect(mc, mc._lib.E_STATE, lambda: lm.track_frames_wait())             # the wait cleared it
    T.expect(mc, mc._lib.E_STATE, lambda: lm.track_wait())
