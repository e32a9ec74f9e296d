"""CPU halves of the limit tests (test_gpu_limits.py): the exact-distance descriptor builder, the float32 accept
test on every (d0, d1) pair with 0 <= d0 <= d1 <= 256, and the numpy restatement of rotated BRIEF against the
oracle.  No GPU needed."""
import numpy as np
import pytest

import limits_ref as R
import oracle_lib as O


def test_accept_case_distances_are_exact():
    for D in range(257):
        for swap in (False, True):
            q, t = R.accept_case(D, swap)
            assert q.shape == (257 - D, 32) and t.shape == (2, 32)
            d = R.popcount_dist(q, t)
            a = np.arange(257 - D)
            best, other = (1, 0) if swap else (0, 1)
            assert np.array_equal(d[:, best], a), "D %d swap %d: d0" % (D, swap)
            assert np.array_equal(d[:, other], a + D), "D %d swap %d: d1" % (D, swap)
            if D % 32 == 0:   # the popcount agrees with the oracle's DescriptorDistance
                od = [[O.descriptor_distance(q[i], t[j]) for j in range(2)] for i in range(len(q))]
                assert np.array_equal(d, np.array(od)), "D %d swap %d" % (D, swap)


def test_accept_table_has_the_deciding_pairs():
    """0.85f * 20 rounds to 17.0f: (17, 20) is rejected in float (accepted by a double or fused product); same for its multiples"""
    d1 = np.array([20, 40, 60, 80])
    d0 = np.array([17, 34, 51, 68])
    assert not R.accept_restated(d0, d1, 75.0, 0.85).any()
    assert (np.float64(np.float32(0.85)) * d1 > d0).all(), "a double product would accept them"
    # and the table holds them: D = d1 - d0 at a = d0
    for a, b in zip(d0, d1):
        q, t = R.accept_case(int(b - a))
        assert tuple(R.popcount_dist(q[a:a + 1], t)[0]) == (a, b)


@pytest.mark.parametrize("thr,ratio", R.ACCEPT_SETTINGS)
def test_oracle_accept_equals_float32_restatement_on_every_pair(thr, ratio):
    """O.bruteforce_match against the float32 restatement on the whole (d0, d1) table, both train orders"""
    nacc = 0
    for D in range(257):
        for swap in (False, True):
            q, t = R.accept_case(D, swap)
            o1, o2 = O.bruteforce_match(q, t, thr, ratio)
            r1, r2 = R.match_restated(q, t, thr, ratio)
            assert np.array_equal(o1, r1) and np.array_equal(o2, r2), \
                "D %d swap %d (%g, %g): oracle accepts %s, float32 restatement %s" % (D, swap, thr, ratio, o1.tolist(), r1.tolist())
            oi, od = O.knn2(q, t)
            ri, rd = R.knn2_restated(q, t)
            assert np.array_equal(oi, ri) and np.array_equal(od, rd), "D %d swap %d: knn2 row %s" % (D, swap, R.first_diff(oi, ri))
            nacc += len(o1)
    assert nacc > 0 or thr == 0.0


def test_knn2_restated_matches_oracle_on_random_sets():
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (700, 32), dtype=np.uint8)
    t[300] = t[299]                      # a duplicate pair: the lower index first
    q[7] = t[299]
    oi, od = O.knn2(q, t)
    ri, rd = R.knn2_restated(q, t)
    assert np.array_equal(oi, ri) and np.array_equal(od, rd)
    assert tuple(ri[7]) == (299, 300) and tuple(rd[7]) == (0, 0)


def test_brief_pattern_parses():
    P = R.brief_pattern()
    assert P.shape == (512, 2) and tuple(P[0]) == (8, -3) and tuple(P[-1]) == (0, -11)
    assert np.abs(P).max() == 13


@pytest.mark.parametrize("frame,W,H", [(4, 640, 480), (9, 640, 480), (0, 1280, 720), (2, 1280, 720)])
def test_rotated_brief_restatement_equals_oracle_bit_for_bit(frame, W, H):
    """computeOrbDescriptor restated in numpy with glibc's cosf / sinf: every row of every level equals the oracle's"""
    import mcorb
    img = mcorb.synth_rig_frame(frame, 1, 0, W, H)
    ex = O.OracleExtractor(1000, orientation=1)
    mono, k, d = ex(img)
    rows = []
    for l in range(8):
        lk = ex.level_keypoints(l)
        assert len(lk) > 0, "level %d has no keypoints" % l
        rows.append(R.describe_restated(ex.blurred(l), lk["x"], lk["y"], lk["angle"], R.trig_glibc))
    g = np.concatenate(rows)
    assert len(g) == len(d) == mono
    bad = R.first_diff(g, d)
    assert bad is None, "row %s (level %d, angle %r) differs" % (bad, k["octave"][bad], float(k["angle"][bad]))
    assert len(np.unique(np.round(k["angle"]))) > 300, "the angles must cover the circle"


def test_rotated_brief_fragile_images_hold_fragile_bits():
    """FRAGILE_IMAGES: the restatement equals the oracle on every row, and the images hold the bits that a last-bit change in
    the tap arithmetic (fma, double) would flip -- the GPU half compares k_describe_oriented with the restatement on them"""
    import mcorb
    W, H, N = R.FRAGILE_SHAPE
    ex = O.OracleExtractor(N, orientation=1)
    total = {"glibc": 0, "double": 0}
    for f, c in R.FRAGILE_IMAGES:
        mono, k, d = ex(mcorb.synth_rig_frame(f, 4, c, W, H))
        rows, nfr = [], {"glibc": 0, "double": 0}
        for l in range(8):
            lk, b = ex.level_keypoints(l), ex.blurred(l)
            rows.append(R.describe_restated(b, lk["x"], lk["y"], lk["angle"], R.trig_glibc))
            for name, trig in (("glibc", R.trig_glibc), ("double", R.trig_double)):
                nfr[name] += R.fragile_bits(b, lk["x"], lk["y"], *trig(lk["angle"]))
        bad = R.first_diff(np.concatenate(rows), d)
        assert bad is None, "frame %d cam %d row %d" % (f, c, bad)
        assert nfr["double"] >= 1, "frame %d cam %d has no fragile bit" % (f, c)
        for name in total:
            total[name] += nfr[name]
    print("fragile bits:", total)
    assert min(total.values()) >= len(R.FRAGILE_IMAGES)
