"""GPU limit tests: BruteForceMatch's accept test on every (d0, d1) pair, the k-NN key packing at its index and
distance limits, rotated BRIEF bit for bit, and the job shape bench.py times.  Tolerance zero everywhere; a failure
names the first differing row and its inputs.  CPU halves (the tables and the restatements themselves) are in
test_limits_cpu.py."""
import time

import numpy as np
import pytest

import limits_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import mcorb
    assert mcorb.device_count() >= 1, "no gfx950 device visible: the product has no CPU path"
    return mcorb


# Which k-NN epilogue a standalone call (ORBextractor.knnMatch2 / matchRatio, one camera pair) runs:
#   chunkLen = knn_chunk_len(1) = 256 and nchunks = ceil(kc / 256), where kc = roundup64(max(nq, nt, 1)) is the extractor's
#   scratch capacity -- and kc ONLY GROWS over the extractor's life (knn2_host_arrays reallocates only upward).
#   kc <= 256 -> one chunk -> k_knn2's folded epilogue; kc > 256 -> partials merged by k_knn2_finalize.
# So: a fresh extractor whose calls all stay at or below 256 descriptors per side runs the folded arm, and an extractor that
# has once seen more than 256 runs the finalize arm for every later call, small ones included.
FOLD_MAX = 256


def _extractor(mc, arm):
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    if arm == "finalize":
        rng = np.random.default_rng(99)
        ext.knnMatch2(rng.integers(0, 256, (FOLD_MAX + 1, 32), dtype=np.uint8), rng.integers(0, 256, (2, 32), dtype=np.uint8))
    return ext


def _standalone(ext, q, t, arm, thr=75.0, ratio=0.85):
    """knnMatch2 + matchRatio; on the folded arm the queries go in blocks of <= 256 so kc never grows"""
    if arm == "finalize" or len(q) <= FOLD_MAX:
        assert arm == "finalize" or len(t) <= FOLD_MAX
        i, d = ext.knnMatch2(q, t)
        m1, m2 = ext.matchRatio(q, t, thr, ratio)
        return i, d, m1, m2
    parts = [_standalone(ext, q[s:s + FOLD_MAX], t, arm, thr, ratio) for s in range(0, len(q), FOLD_MAX)]
    off = np.cumsum([0] + [FOLD_MAX] * (len(parts) - 1))
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] + o for p, o in zip(parts, off)]).astype(np.uint32), np.concatenate([p[3] for p in parts]))


def _accept_msg(what, q, t, thr, ratio, gi, gd, g1, ref1):
    d = R.popcount_dist(q, t)
    acc_g, acc_r = set(g1.tolist()), set(ref1.tolist())
    rows = sorted(acc_g ^ acc_r)
    if rows:
        a = rows[0]
        return "%s (thr %g, ratio %r): query %d, distances %s, GPU row idx %s dist %s accepts=%d, expected accept=%d" % (
            what, thr, ratio, a, d[a].tolist(), gi[a].tolist(), gd[a].tolist(), a in acc_g, a in acc_r)
    return "%s (thr %g, ratio %r): same accepted queries, different train indices" % (what, thr, ratio)


# --------------------------------------------------------------------------------------------
# A. the accept test on every (d0, d1) pair with 0 <= d0 <= d1 <= 256
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["fold", "finalize"])
def test_accept_table_standalone(mc, arm):
    t_start = time.time()
    ext = _extractor(mc, arm)
    nacc = 0
    for D in range(257):
        for swap in (False, True):
            q, t = R.accept_case(D, swap)
            ri, rd = R.knn2_restated(q, t)
            gi, gd, _, _ = _standalone(ext, q, t, arm)
            bad = R.first_diff(np.hstack([gi, gd]), np.hstack([ri, rd]))
            assert bad is None, "D %d swap %d query %s: GPU %s %s, expected %s %s" % (
                D, swap, bad, gi[bad].tolist(), gd[bad].tolist(), ri[bad].tolist(), rd[bad].tolist())
            for thr, ratio in R.ACCEPT_SETTINGS:
                g1, g2 = _standalone(ext, q, t, arm, thr, ratio)[2:]
                r1, r2 = R.match_restated(q, t, thr, ratio)
                assert np.array_equal(g1, r1) and np.array_equal(g2, r2), \
                    _accept_msg("D %d swap %d %s" % (D, swap, arm), q, t, thr, ratio, gi, gd, g1, r1)
                nacc += len(g1)
    assert nacc > 10000
    ext.close()
    print("[limits] accept table standalone %s: %.1f s" % (arm, time.time() - t_start))


@pytest.mark.parametrize("arm", ["fold", "finalize"])
def test_accept_table_rig_match_sets(mc, arm):
    """The same table through DescriptorBlock + Rig.match_sets / pairknn2 / pairlist.  Set 0 = query a has the last a bits
    set (a = 0 .. 256); set 1 + 2D + swap = the two trains of D.  knn_chunk_len: more than 48 pairs with kcap <= 4096 is one
    chunk (folded epilogue); at most 12 pairs with kcap > 256 is chunkLen 256 over kcap 384 (k_knn2_finalize)."""
    t_start = time.time()
    rig = mc.Rig(4, 640, 480, max_frames=13, nslots=1, nfeatures=300)   # <= 78 pairs and 52 distinct sets per job
    assert 256 < rig.kcap <= 4096, rig.kcap
    qb = np.zeros((257, 256), np.uint8)
    for a in range(257):
        qb[a, 256 - a:] = 1
    Q = R.bits_desc(qb)
    trains = [R.accept_case(D, swap)[1] for D in range(257) for swap in (False, True)]
    blk = mc.DescriptorBlock(1 + len(trains), rig.kcap)
    blk.upload(0, Q)
    for k, t in enumerate(trains):
        blk.upload(1 + k, t)
    expect = [R.knn2_restated(Q, t) for t in trains]
    per_job = 51 if arm == "fold" else 12
    assert (per_job > 48) == (arm == "fold") and per_job + 1 <= 52
    jobs = []
    for s in range(0, len(trains), per_job):
        s = min(s, len(trains) - per_job)   # the last job overlaps the one before: every job keeps its pair count
        jobs.append(list(range(s, s + per_job)))
    nacc = 0
    for thr, ratio in R.ACCEPT_SETTINGS:
        for job in jobs:
            rig.match_sets(blk, [[0, 1 + k] for k in job], dist_thresh=thr, ratio=ratio)
            for p, k in enumerate(job):
                D, swap = divmod(k, 2)
                gi, gd = rig.pairknn2(p)
                ri, rd = expect[k]
                bad = R.first_diff(np.hstack([gi, gd]), np.hstack([ri, rd]))
                assert bad is None, "%s D %d swap %d query %s: GPU %s %s, expected %s %s" % (
                    arm, D, swap, bad, gi[bad].tolist(), gd[bad].tolist(), ri[bad].tolist(), rd[bad].tolist())
                g1, g2 = rig.pairlist(p)
                r1, r2 = R.match_restated(Q, trains[k], thr, ratio)
                assert np.array_equal(g1, r1) and np.array_equal(g2, r2), \
                    _accept_msg("rig %s D %d swap %d" % (arm, D, swap), Q, trains[k], thr, ratio, gi, gd, g1, r1)
                nacc += len(g1)
    assert nacc > 10000
    blk.close()
    rig.close()
    print("[limits] accept table rig %s: %.1f s" % (arm, time.time() - t_start))


# --------------------------------------------------------------------------------------------
# B. k-NN at the index and distance limits (standalone knnMatch2 / matchRatio against the oracle)
# --------------------------------------------------------------------------------------------
def _check_vs_oracle(ext, q, t, what, arm="finalize", thr=75.0, ratio=0.85):
    gi, gd, g1, g2 = _standalone(ext, q, t, arm, thr, ratio)
    oi, od = O.knn2(q, t)
    bad = R.first_diff(np.hstack([gi, gd]), np.hstack([oi, od]))
    assert bad is None, "%s: query %s: GPU idx %s dist %s, oracle idx %s dist %s (nq %d, nt %d)" % (
        what, bad, gi[bad].tolist(), gd[bad].tolist(), oi[bad].tolist(), od[bad].tolist(), len(q), len(t))
    o1, o2 = O.bruteforce_match(q, t, thr, ratio)
    assert np.array_equal(g1, o1) and np.array_equal(g2, o2), _accept_msg(what, q, t, thr, ratio, gi, gd, g1, o1) \
        if len(q) * len(t) <= 2e7 else "%s: accepted pairs differ (%d vs %d)" % (what, len(g1), len(o1))
    return gi, gd, g1


def _near_copies(rng, src, n, maxflip=40, rows=None):
    """n noisy copies of rows of src (random rows, or the given ones; 0 .. maxflip bits flipped), and the rows they came from"""
    rows = rng.integers(0, len(src), n) if rows is None else np.asarray(rows)
    out = src[rows].copy()
    bits = np.unpackbits(out, axis=1)
    for i in range(len(rows)):
        k = int(rng.integers(0, maxflip + 1))
        bits[i, rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits, axis=1), rows


@pytest.mark.parametrize("nt", [255, 256, 257, 8191, 8192, 8193, 16385, 32768, 32769, 65535])
def test_knn2_train_index_limits(mc, nt):
    """~300 queries (half of them noisy copies of trains, the last trains and chunk-boundary neighbours among them) against nt
    trains: the 16-bit train index and the 13-bit in-chunk index across every chunk boundary up to the 65535 limit"""
    t_start = time.time()
    rng = np.random.default_rng(nt)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    nq = 250 if nt <= FOLD_MAX else 300           # nt <= 256: the folded epilogue on a fresh extractor
    arm = "fold" if nt <= FOLD_MAX else "finalize"
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    special = [i for i in (0, 255, 256, 4095, 4096, 8191, 8192, 16384, 32767, 32768, nt - 2, nt - 1) if i < nt]
    qc, _ = _near_copies(rng, t, 0, rows=np.repeat(special, 4))
    qn, _ = _near_copies(rng, t, nq // 2 - len(qc))
    q = np.concatenate([qc, qn, rng.integers(0, 256, (nq - len(qc) - len(qn), 32), dtype=np.uint8)])
    q = q[rng.permutation(len(q))]
    gi, gd, g1 = _check_vs_oracle(ext, q, t, "nt %d" % nt, arm)
    assert set(special) <= set(gi[:, 0].tolist()) and len(g1) > 50
    ext.close()
    print("[limits] nt %d: %.2f s" % (nt, time.time() - t_start))


def test_knn2_query_index_limit(mc):
    """65535 queries against 300 trains: 256 query blocks, accepted-pair list entries with query indices up to 65534 (q << 16)"""
    rng = np.random.default_rng(7)
    t = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (65535, 32), dtype=np.uint8)
    pos = np.concatenate([rng.choice(65535, 2000, replace=False), [0, 255, 256, 8191, 8192, 32767, 32768, 65533, 65534]])
    q[pos], _ = _near_copies(rng, t, len(pos))
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    gi, gd, g1 = _check_vs_oracle(ext, q, t, "nq 65535")
    assert g1.max() == 65534 and len(g1) > 1000
    ext.close()


def test_knn2_duplicates_across_chunk_boundaries(mc):
    """equal trains at 255/256, 8191/8192, 32767/32768 and at the last index 65534 (with 65533): a query equal to them gets
    the lower index first, both at distance 0"""
    rng = np.random.default_rng(11)
    t = rng.integers(0, 256, (65535, 32), dtype=np.uint8)
    pairs = [(255, 256), (8191, 8192), (32767, 32768), (65533, 65534), (0, 65534)]
    qs = []
    for lo, hi in pairs[:4]:
        t[hi] = t[lo]
        qs.append(t[lo].copy())
    q = np.concatenate([np.stack(qs), rng.integers(0, 256, (300, 32), dtype=np.uint8)])
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    gi, gd, _ = _check_vs_oracle(ext, q, t, "duplicates")
    for k, (lo, hi) in enumerate(pairs[:4]):
        assert tuple(gi[k]) == (lo, hi) and tuple(gd[k]) == (0, 0), "query %d: %s %s" % (k, gi[k], gd[k])
    # the last index duplicated from the first: (0, 65534), the widest index gap
    t2 = t.copy()
    t2[65534] = t2[0]
    gi, gd, _ = _check_vs_oracle(ext, t2[:1], t2, "duplicate of index 0 at 65534")
    assert tuple(gi[0]) == (0, 65534) and tuple(gd[0]) == (0, 0)
    ext.close()


@pytest.mark.parametrize("arm", ["fold", "finalize"])
def test_knn2_distance_256(mc, arm):
    """the +2^20 key offset that keeps distance 256 non-negative: 256 as the best (one train), as the second, and as both
    (every train a complement: nt = 2 and, on the finalize arm, nt = 300 over two chunks)"""
    rng = np.random.default_rng(13)
    ext = _extractor(mc, arm)
    q = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    c0 = ~q[0]
    near = q[0].copy()
    near[3] ^= 0x11
    cases = {"best": (np.stack([c0]), (0, -1), (256, -1)),
             "second": (np.stack([near, c0]), (0, 1), (2, 256)),
             "second swapped": (np.stack([c0, near]), (1, 0), (2, 256)),
             "both": (np.stack([c0, c0]), (0, 1), (256, 256))}
    if arm == "finalize":
        cases["both, 300 trains"] = (np.repeat(c0[None], 300, 0), (0, 1), (256, 256))
    for name, (t, ei, ed) in cases.items():
        for thr, ratio in ((75.0, 0.85), (256.0, 1.0)):
            gi, gd, _ = _check_vs_oracle(ext, q, t, "distance 256, %s, %s" % (name, arm), arm, thr, ratio)
            assert tuple(gi[0]) == ei and tuple(gd[0]) == ed, "%s: %s %s" % (name, gi[0], gd[0])
    # and as query: the complement of a train set's member is 256 from it, in a set with both near and far trains
    t = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    _check_vs_oracle(ext, np.concatenate([~t[:50], t[50:60]]), t, "complement queries, %s" % arm, arm)
    ext.close()


def test_knn2_refuses_65536_and_recovers(mc):
    rng = np.random.default_rng(17)
    ext = mc.ORBextractor(1000, 1.2, 8, 20, 7)
    small_q = rng.integers(0, 256, (100, 32), dtype=np.uint8)
    small_t = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    small_q[:50], _ = _near_copies(rng, small_t, 50)
    big = np.zeros((65536, 32), np.uint8)
    for args in ((big, small_t), (small_q, big)):
        for fn in (ext.knnMatch2, ext.matchRatio):
            with pytest.raises(mc.McorbError) as e:
                fn(*args)
            assert e.value.code == mc.E_ARG, e.value
    _check_vs_oracle(ext, small_q, small_t, "after the refused calls")
    ext.close()


# --------------------------------------------------------------------------------------------
# C. rotated BRIEF bit for bit
# --------------------------------------------------------------------------------------------
def _restated_rows(ora, trig):
    rows, kps = [], []
    for l in range(8):
        lk = ora.level_keypoints(l)
        rows.append(R.describe_restated(ora.blurred(l), lk["x"], lk["y"], lk["angle"], trig))
        kps.append(lk)
    return np.concatenate(rows), np.concatenate(kps)


def _check_rotated(what, ora_out, gpu_out, restated, level_kps):
    (m1, k1, d1), (m2, k2, d2) = ora_out, gpu_out
    assert m1 == m2 and len(k1) == len(k2) == len(restated), "%s: keypoint counts" % what
    for f in k1.dtype.names:
        assert np.array_equal(k1[f], k2[f]), "%s: keypoint field %s" % (what, f)
    bad = R.first_diff(d2, restated)
    if bad is not None:
        ang = np.float32(k2["angle"][bad])
        rad = R._rad([ang])
        cd, sd = R.trig_double([ang])
        cg, sg = R.trig_glibc([ang])
        pytest.fail("%s: row %d (level %d, level x %r y %r, angle %r = 0x%08x, rad 0x%08x) differs from the restatement: "
                    "cos/sin double-rounded 0x%08x/0x%08x, glibc 0x%08x/0x%08x" % (
                        what, bad, k2["octave"][bad], float(level_kps["x"][bad]), float(level_kps["y"][bad]), float(ang),
                        ang.view(np.uint32), rad[0].view(np.uint32), cd[0].view(np.uint32), sd[0].view(np.uint32),
                        cg[0].view(np.uint32), sg[0].view(np.uint32)))
    ndiff = int((~np.all(d1 == d2, axis=1)).sum())
    print("[limits] %s: %d rows, GPU == restatement on all; oracle (glibc cosf/sinf) differs from the GPU on %d" % (what, len(d2), ndiff))


@pytest.mark.parametrize("frame,W,H,N", [(4, 640, 480, 1000), (9, 640, 480, 1000), (0, 1280, 720, 2000), (2, 1280, 720, 2000)])
def test_rotated_brief_extractor_bit_for_bit(mc, frame, W, H, N):
    img = mc.synth_rig_frame(frame, 1, 0, W, H)
    ext = mc.ORBextractor(N, 1.2, 8, 20, 7, orientation=mc.ORIENT_IC_ANGLE)
    ora = O.OracleExtractor(N, orientation=1)
    ref = ora(img)
    restated, lk = _restated_rows(ora, R.trig_double)
    _check_rotated("extractor %dx%d frame %d" % (W, H, frame), ref, ext(img), restated, lk)
    ext.close()


@pytest.mark.parametrize("W,H,C,F,N", [(640, 480, 2, 2, 1000), (1280, 720, 2, 2, 2000)])
def test_rotated_brief_rig_batch_bit_for_bit(mc, W, H, C, F, N):
    rig = mc.Rig(C, W, H, F, 1, nfeatures=N, orientation=1)
    imgs = [mc.synth_rig_frame(30 + f, C, c, W, H) for f in range(F) for c in range(C)]
    rig.upload(imgs)
    rig.process(F)
    ora = O.OracleExtractor(N, orientation=1)
    for m, img in enumerate(imgs):
        ref = ora(img)
        restated, lk = _restated_rows(ora, R.trig_double)
        _check_rotated("rig %dx%d image %d" % (W, H, m), ref, rig.features(m), restated, lk)
    rig.close()


def test_rotated_brief_fragile_images_bit_for_bit(mc):
    """FRAGILE_IMAGES in one batched orientation-mode job at 8000 features: every descriptor equals the restatement with
    double-rounded cos / sin, computed from the job's own keypoints (level coordinates recovered from the scaled ones) and
    blurred levels -- including the few bits that an fma or a double evaluation of one tap would flip"""
    W, H, N = R.FRAGILE_SHAPE
    imgs = [mc.synth_rig_frame(f, 4, c, W, H) for f, c in R.FRAGILE_IMAGES]
    rig = mc.Rig(4, W, H, len(imgs) // 4, 1, nfeatures=N, orientation=1)
    rig.upload(imgs)
    rig.extract(len(imgs))
    scale = mc.get_tables(rig.params)["scale"]
    nfragile = 0
    for m, (f, c) in enumerate(R.FRAGILE_IMAGES):
        _, k, d = rig.features(m)
        assert len(k) > 7900
        for l in range(8):
            sel = k["octave"] == l
            kl = k[sel]
            lx = np.rint(kl["x"].astype(np.float64) / float(scale[l])).astype(np.float32)   # level coordinates are integers
            ly = np.rint(kl["y"].astype(np.float64) / float(scale[l])).astype(np.float32)
            if l:
                assert np.array_equal(lx * scale[l], kl["x"]) and np.array_equal(ly * scale[l], kl["y"])
            b = rig.level(m, l, blurred=True)
            restated = R.describe_restated(b, lx, ly, kl["angle"], R.trig_double)
            bad = R.first_diff(d[sel], restated)
            if bad is not None:
                ang = np.float32(kl["angle"][bad])
                cd, sd = R.trig_double([ang])
                pytest.fail("frame %d cam %d level %d keypoint (%g, %g) angle %r = 0x%08x: GPU descriptor differs from the restatement; "
                            "double-rounded cos/sin 0x%08x/0x%08x" % (f, c, l, lx[bad], ly[bad], float(ang), ang.view(np.uint32),
                                                                       cd[0].view(np.uint32), sd[0].view(np.uint32)))
            nfragile += R.fragile_bits(b, lx, ly, *R.trig_double(kl["angle"]))
    print("[limits] fragile images: %d fragile bits" % nfragile)
    assert nfragile >= len(R.FRAGILE_IMAGES)
    rig.close()


# --------------------------------------------------------------------------------------------
# D. the job shape bench.py times: 4 slots x 128 four-camera 1280x720 frames at 2000 features
# --------------------------------------------------------------------------------------------
BENCH_C, BENCH_W, BENCH_H, BENCH_N, BENCH_F, BENCH_S = 4, 1280, 720, 2000, 128, 4
PAIRS = [(i, j) for i in range(BENCH_C) for j in range(i + 1, BENCH_C)]


def _frame_id(slot, f):
    return 500 + slot * BENCH_F + f


def _frame_outputs(rig, f, slot=0):
    feats = [rig.features(f * BENCH_C + c, slot=slot) for c in range(BENCH_C)]
    knn = [rig.pair_knn2(f, i, j, slot=slot) for i, j in PAIRS]
    mat = [rig.pair_matches(f, i, j, slot=slot) for i, j in PAIRS]
    return feats, knn, mat, rig.tracks(f, slot=slot)


def _same_outputs(a, b, what):
    (fa, ka, ma, ta), (fb, kb, mb, tb) = a, b
    for c in range(BENCH_C):
        (m1, k1, d1), (m2, k2, d2) = fa[c], fb[c]
        assert m1 == m2 and len(k1) == len(k2), "%s cam %d: monoIndex / keypoint count %d/%d vs %d/%d" % (what, c, m1, len(k1), m2, len(k2))
        for fld in k1.dtype.names:
            bad = R.first_diff(k1[fld], k2[fld])
            assert bad is None, "%s cam %d keypoint %s field %s: %r vs %r" % (what, c, bad, fld, k1[bad], k2[bad])
        bad = R.first_diff(d1, d2)
        assert bad is None, "%s cam %d descriptor row %s" % (what, c, bad)
    for p, (i, j) in enumerate(PAIRS):
        bad = R.first_diff(np.hstack(ka[p]), np.hstack(kb[p]))
        assert bad is None, "%s pair (%d, %d) knn row %s: %s vs %s" % (what, i, j, bad, np.hstack(ka[p])[bad], np.hstack(kb[p])[bad])
        assert np.array_equal(ma[p][0], mb[p][0]) and np.array_equal(ma[p][1], mb[p][1]), "%s pair (%d, %d) accepted pairs" % (what, i, j)
    assert ta[1] == tb[1] and ta[0].shape == tb[0].shape, "%s tracks: %d/%d vs %d/%d" % (what, len(ta[0]), ta[1], len(tb[0]), tb[1])
    bad = R.first_diff(ta[0], tb[0])
    assert bad is None, "%s track %s: %s vs %s" % (what, bad, ta[0][bad], tb[0][bad])


def test_bench_job_shape(mc):
    """Rig(4, 1280, 720, max_frames=128, nslots=4, nfeatures=2000), bench.py's default (IMAGES_PER_LAUNCH = 512, S = 4): one
    k_knn2 launch of 768 pairs per job.  Every frame of every slot equals a one-frame rig on the same device; a seeded sample
    of >= 6 frames per slot (first and last included) equals the oracle on features, all 6 pairs' k-NN tables and accepted
    pairs, and the tracks.  With GPU selection and with host selection."""
    t_start = time.time()
    rigs = {m: mc.Rig(BENCH_C, BENCH_W, BENCH_H, max_frames=BENCH_F, nslots=BENCH_S, nfeatures=BENCH_N, selection=sel)
            for m, sel in (("gpu", 2), ("host", 1))}
    for m, rig in rigs.items():
        assert rig.select_mode() == m
    for s in range(BENCH_S):   # distinct frames in every slot
        imgs = [mc.synth_rig_frame(_frame_id(s, f), BENCH_C, c, BENCH_W, BENCH_H) for f in range(BENCH_F) for c in range(BENCH_C)]
        for rig in rigs.values():
            rig.upload(imgs, slot=s)
        del imgs
    for m in ("gpu", "host"):   # one mode at a time: all four slots submitted, then all waited on
        for s in range(BENCH_S):
            rigs[m].process_submit(BENCH_F, slot=s)
        for s in range(BENCH_S):
            rigs[m].process_wait(slot=s)
    t_jobs = time.time()
    rng = np.random.default_rng(2026)
    sample = {s: sorted({0, BENCH_F - 1} | set(rng.choice(np.arange(1, BENCH_F - 1), 4, replace=False).tolist())) for s in range(BENCH_S)}
    one = mc.Rig(BENCH_C, BENCH_W, BENCH_H, 1, 1, nfeatures=BENCH_N)
    ora = O.OracleExtractor(BENCH_N)
    n_oracle = 0
    for s in range(BENCH_S):
        for f in range(BENCH_F):
            imgs = [mc.synth_rig_frame(_frame_id(s, f), BENCH_C, c, BENCH_W, BENCH_H) for c in range(BENCH_C)]
            one.upload(imgs)
            one.process(1)
            ref = _frame_outputs(one, 0)
            for m, rig in rigs.items():
                _same_outputs(ref, _frame_outputs(rig, f, slot=s), "%s selection, slot %d frame %d vs the one-frame rig" % (m, s, f))
            if f in sample[s]:
                feats = [ora(im) for im in imgs]
                descs = [d for _, _, d in feats]
                knn = [O.knn2(descs[i], descs[j]) for i, j in PAIRS]
                mat = [O.bruteforce_match(descs[i], descs[j]) for i, j in PAIRS]
                _same_outputs((feats, knn, mat, O.intra_matches(descs)), ref, "slot %d frame %d: oracle vs GPU" % (s, f))
                assert min(len(d) for d in descs) > 1900 and len(ref[3][0]) > 1000
                n_oracle += 1
    assert n_oracle >= 6 * BENCH_S
    assert sum(rigs["gpu"].select_fallbacks(slot=s) for s in range(BENCH_S)) == 0
    one.close()
    for rig in rigs.values():
        rig.close()
    print("[limits] bench job shape: jobs %.1f s, checks %.1f s" % (t_jobs - t_start, time.time() - t_jobs))
