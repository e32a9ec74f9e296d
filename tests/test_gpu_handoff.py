"""The code that puts pixels into level 0 (mcorb_upload.cpp, k_stage_f32, k_remap_u8, the padded device maps of
Rig::set_image_undistortion) at the shapes and values the other files leave out, every comparison with ==:

(a) k_stage_f32 on the whole value set of tests/handoff_ref.py (every u / 255, all 255 rounding ties and their ulp neighbours,
    negatives, values above 1, a denormal, products an int cannot hold) against the numpy restatement, 1 and 3 channels, tight
    and with a padded caller stride, into the pyramid (pitch 64-aligned) and into the raw planes of a rectified rig (pitch w);
(b) mcorb_rig_upload_u8 with a padded caller stride on its three paths (one image, the pipelined quarters of 2..8 images, the
    pool copy above), with and without image undistortion;
(c) the rectified hand-off at w % 4 in {1, 2, 3}: k_remap_u8's tail stores, its byte-wise pass-through, the zero-padded device
    maps, nimg < ncams and a ragged last frame, against tests/undistort_image_ref.py.
The rigs are the smallest the geometry takes with 4 levels; 323 is wider than one 256-lane block of k_stage_f32."""
import ctypes as C

import numpy as np
import pytest

import handoff_ref as HR
import oracle_lib as O
import undistort_image_ref as R
from test_gpu_undistort_image import (DISTS, check_planes, expected_level0, frames, job_results, ref_maps, same_results,
                                      set_all, upload_form)

pytestmark = pytest.mark.gpu

SIZES = [(161, 120), (162, 121), (163, 123), (323, 243)]
SIZE_IDS = ["%dx%d" % s for s in SIZES]
NFEAT, NLEVELS = 300, 4
SMALL_BATCH = 8            # kSmallBatch (mcorb_engine.h): upload_u8 pipelines 2..8 images and hands more to the pool
PINCUSHION, BARREL, RATIONAL = DISTS[1], DISTS[0], DISTS[2]
SENTINEL = 0xEE


@pytest.fixture(scope="module")
def mc():
    import mcorb
    return mcorb


def make_rig(mc, ncams, W, H, max_frames=1):
    return mc.Rig(ncams, W, H, max_frames, 1, nfeatures=NFEAT, nlevels=NLEVELS)


def test_sizes_are_accepted_and_unaligned(mc):
    """the geometry takes every size with 4 levels (a CPU computation); w % 4 covers 1, 2, 3; 323 needs a second block of 256
    lanes and is no multiple of 64; the heights make upload_u8's quarter split H q / 4 uneven"""
    p = mc.default_params(nfeatures=NFEAT, nlevels=NLEVELS)
    six = np.zeros((NLEVELS, 6), np.int32)
    for w, h in SIZES:
        assert mc._lib.load().mcorb_host_geometry(C.byref(p), w, h, six.ctypes.data) == 0, (w, h)
        assert (six[0, 0], six[0, 1]) == (w, h) and w % 4 != 0 and w % 64 != 0
    assert {w % 4 for w, _ in SIZES} == {1, 2, 3} and any(w > 256 and w % 4 == 3 for w, _ in SIZES)
    assert any(h % 4 for _, h in SIZES)


def assert_same_features(ref, got, what):
    (m1, k1, d1), (m2, k2, d2) = ref, got
    assert m1 == m2 and len(k1) == len(k2), "%s: monoIndex %d / %d, %d / %d keypoints" % (what, m1, m2, len(k1), len(k2))
    for f in k1.dtype.names:
        assert np.array_equal(k1[f], k2[f]), "%s: keypoint field %s differs" % (what, f)
    assert np.array_equal(d1, d2), "%s: descriptors differ" % what


# -- (a) k_stage_f32 on the value set ---------------------------------------------------------------------------------------------
_VALUES = {}


def value_case(W, H, ch):
    """(images, expected planes) of a batch of two: the value image, and the same rolled down by one row so that the second image
    differs from the first; computed once per shape and left unchanged"""
    key = (W, H, ch)
    if key not in _VALUES:
        a = HR.value_image(W, H, ch)
        b = np.ascontiguousarray(np.roll(a, 1, axis=0))
        imgs = [a, b]
        want = [HR.stage_f32(im) for im in imgs]
        for x in imgs + want:
            x.setflags(write=False)
        _VALUES[key] = (imgs, want)
    return _VALUES[key]


def upload_f32_strided(rig, imgs, pad_floats):
    """mcorb_rig_upload_f32 through the C ABI with stride_bytes = (W ch + pad) 4; the padding holds 1e10, which stages to 0 and
    occurs in no row of its own length"""
    bufs = []
    for im in imgs:
        h, w = im.shape[:2]
        ch = 1 if im.ndim == 2 else im.shape[2]
        buf = np.full((h, w * ch + pad_floats), 1e10, np.float32)
        buf[:, :w * ch] = im.reshape(h, w * ch)
        bufs.append(buf)
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    st = rig.L.mcorb_rig_upload_f32(rig.h_rig, 0, ptrs, len(bufs), bufs[0].strides[0], ch)
    assert st == 0, rig.L.mcorb_last_error()


def assert_planes(got, want, src, what):
    bad = np.argwhere(got != want)
    if bad.size:
        y, x = bad[0]
        cols = np.bincount(bad[:, 1] & 3, minlength=4).tolist()
        raise AssertionError("%s: %d pixels differ (by column mod 4: %s), first at row %d col %d: input %r gives %d, expected %d"
                             % (what, len(bad), cols, y, x, src[y, x], got[y, x], want[y, x]))


@pytest.mark.parametrize("pad", [0, 5], ids=["tight", "padded"])
@pytest.mark.parametrize("ch", [1, 3], ids=["f32c1", "f32c3"])
@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_f32_value_set_into_level0_and_raw_planes(mc, W, H, ch, pad):
    imgs, want = value_case(W, H, ch)
    # a plain rig: k_stage_f32 writes level 0 (launch_stage_f32)
    rig = make_rig(mc, 2, W, H)
    if pad:
        upload_f32_strided(rig, imgs, pad)
    else:
        rig.upload(imgs)
    for m in range(2):
        assert_planes(rig.level(m, 0), want[m], imgs[m], "level 0 of image %d" % m)
    rig.close()
    # a rectified rig: k_stage_f32 writes the raw planes (launch_stage_f32_raw, pitch w); camera 0 is then copied through
    rig = make_rig(mc, 2, W, H)
    set_all(rig, W, H, [None, BARREL])
    if pad:
        upload_f32_strided(rig, imgs, pad)
    else:
        rig.upload(imgs)
    for m in range(2):
        assert_planes(rig.raw_image(m), want[m], imgs[m], "raw plane of image %d" % m)
    check_planes(rig, want, W, H, [None, BARREL])
    rig.close()


def test_single_camera_extractor_takes_the_same_kernel(mc):
    """mcorb_extract_f32 is upload_f32 of a one-camera rig: level 0 of the value image, and the job on it equals the oracle's"""
    W, H = SIZES[2]
    imgs, want = value_case(W, H, 3)
    ext = mc.ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    got = ext(imgs[0])
    assert_planes(ext.pyramid_level(0), want[0], imgs[0], "level 0")
    ref = O.OracleExtractor(NFEAT, 1.2, NLEVELS)(want[0])
    assert_same_features(ref, got, "the extractor")
    ext.close()


# -- (b) u8 uploads with a padded caller stride -----------------------------------------------------------------------------------
def padded_u8(imgs, pad):
    """the images without the sentinel value, inside buffers of row stride W + pad whose padding is the sentinel"""
    clean, bufs = [], []
    for im in imgs:
        im = np.where(im == SENTINEL, SENTINEL - 1, im).astype(np.uint8)
        buf = np.full((im.shape[0], im.shape[1] + pad), SENTINEL, np.uint8)
        buf[:, :im.shape[1]] = im
        clean.append(im)
        bufs.append(buf)
    return clean, bufs


@pytest.mark.parametrize("rectified", [0, 1], ids=["plain", "rectified"])
@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_u8_upload_with_a_padded_stride_on_all_three_paths(mc, W, H, rectified):
    Cn, F = 3, 3
    assert Cn * F == SMALL_BATCH + 1
    dists = [PINCUSHION, None, BARREL] if rectified else [None] * Cn
    rig = make_rig(mc, Cn, W, H, F)
    set_all(rig, W, H, dists)
    for job, nimg in enumerate((1, 2, SMALL_BATCH, SMALL_BATCH + 1)):
        imgs, bufs = padded_u8(frames(mc, F, Cn, W, H, f0=4 + 3 * job)[:nimg], 13)
        ptrs = (C.c_void_p * nimg)(*[b.ctypes.data for b in bufs])
        st = rig.L.mcorb_rig_upload_u8(rig.h_rig, 0, ptrs, nimg, W + 13)
        assert st == 0, rig.L.mcorb_last_error()
        if rectified:
            check_planes(rig, imgs, W, H, dists)
        else:
            for m, im in enumerate(imgs):
                assert_planes(rig.level(m, 0), im, im, "%d images: level 0 of image %d" % (nimg, m))
    rig.close()


# -- (c) the rectified hand-off at unaligned widths -------------------------------------------------------------------------------
def check_maps(rig, W, H, dists):
    for c, d in enumerate(dists):
        if d is None:
            continue
        m1, m2 = rig.undistort_map(c)
        r1, r2 = ref_maps(W, H, c, d)
        assert np.array_equal(m1, r1) and np.array_equal(m2, r2), "camera %d's map" % c


@pytest.mark.parametrize("form", ["u8", "staged", "f32c1", "f32c3"])
@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_rectified_level0_after_each_upload_form(mc, W, H, form):
    """a strong pincushion (taps outside the plane: the border's zeros come in) and a barrel"""
    dists = [PINCUSHION, BARREL]
    rig = make_rig(mc, 2, W, H)
    set_all(rig, W, H, dists)
    check_maps(rig, W, H, dists)
    raws = upload_form(rig, form, frames(mc, 1, 2, W, H, f0=2))
    assert R.remap(raws[0], *ref_maps(W, H, 0, PINCUSHION))[1] > 0, "no tap of the pincushion camera falls outside the plane"
    check_planes(rig, raws, W, H, dists)
    rig.close()


@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_unset_camera_is_copied_through_byte_wise(mc, W, H):
    """camera 1 left unset between two rectified ones: mode 0 of the same launch, byte-wise because w is no multiple of 4"""
    dists = [PINCUSHION, None, BARREL]
    rig = make_rig(mc, 3, W, H)
    set_all(rig, W, H, dists)
    assert [rig.image_undistortion_active(c) for c in range(3)] == [True, False, True]
    imgs = frames(mc, 1, 3, W, H, f0=6)
    rig.upload(imgs)
    check_planes(rig, imgs, W, H, dists)
    assert np.array_equal(rig.level(1, 0), imgs[1])
    rig.close()


@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_fewer_images_than_cameras_and_a_ragged_last_frame(mc, W, H):
    """nimg = 1 on a 3-camera rig (grid.y = min(ncams, nimg)), then nimg = 2 C + 1"""
    Cn = 3
    dists = [PINCUSHION, BARREL, RATIONAL]
    rig = make_rig(mc, Cn, W, H, 3)
    set_all(rig, W, H, dists)
    check_maps(rig, W, H, dists)
    for nimg, f0 in ((1, 9), (2 * Cn + 1, 12)):
        imgs = frames(mc, 3, Cn, W, H, f0=f0)[:nimg]
        rig.upload(imgs)
        check_planes(rig, imgs, W, H, dists)
    rig.close()


@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_whole_job_on_an_unaligned_level0(mc, W, H):
    """the later stages on a level 0 whose width is no multiple of 4: the rectified rig's job equals the job of a plain rig fed
    the remapped planes, and that one equals the oracle's extraction and matching"""
    Cn = 3
    dists = [PINCUSHION, BARREL, None]
    rig, plain = make_rig(mc, Cn, W, H), make_rig(mc, Cn, W, H)
    set_all(rig, W, H, dists)
    imgs = frames(mc, 1, Cn, W, H, f0=3)
    want = [expected_level0(im, W, H, c, dists[c]) for c, im in enumerate(imgs)]
    rig.upload(imgs)
    plain.upload(want)
    for r in (rig, plain):
        r.process(1)
    a, b = job_results(rig, 1, Cn, False), job_results(plain, 1, Cn, False)
    same_results(a, b)
    ex = O.OracleExtractor(NFEAT, 1.2, NLEVELS)
    descs = []
    for c in range(Cn):
        mono, k, d = ex(want[c])
        assert len(k) > 20, "camera %d: %d keypoints say nothing" % (c, len(k))
        assert_same_features((mono, k, d), rig.features(c), "camera %d" % c)
        descs.append(d)
    tr, mg = rig.tracks(0)
    otr, omg = O.intra_matches(descs)
    assert np.array_equal(tr, otr) and mg == omg
    for r in (rig, plain):
        r.close()
