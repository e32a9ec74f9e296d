"""ctypes binding of oracle/_ref/libmcslam_ref_orb.so: the reference's own ORBextractor.cpp, compiled unchanged against the
stand-in cv:: types of oracle/refcv (oracle/ref_orb_shim.cpp, `make -C oracle ref`), plus the bit-for-bit comparison helpers
the reference tests share.

What a comparison against this binary pins: the reference's own logic.  What it does not: OpenCV's five primitives (FAST,
resize, copyMakeBorder, GaussianBlur, fastAtan2), which the stand-in forwards to the oracle's restatements.
Test infrastructure only."""
import ctypes as C
import hashlib
import os

import numpy as np

import oracle_lib as O

REF_SO = os.path.join(O.ORACLE_DIR, "_ref", "libmcslam_ref_orb.so")
SKIP_REASON = ("oracle/_ref/libmcslam_ref_orb.so is absent: it is built from the reference's ORBextractor.cpp by `make -C oracle ref` "
               "(build() runs it) where the reference checkout exists, and travels from there")

_f32p, _ip, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
_lib = None


def available():
    return os.path.exists(REF_SO)


def lib():
    global _lib
    if _lib is None:
        O.lib()   # builds the oracle library the shim links against
        L = C.CDLL(REF_SO)
        L.ref_create.restype = C.c_void_p
        L.ref_create.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
        L.ref_destroy.argtypes = [C.c_void_p]
        L.ref_tables.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, _f32p, _ip, _ip, _ip]
        L.ref_table_sizes.argtypes = [C.c_void_p, _ip, _ip]
        L.ref_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, _ip]
        for name in ("ref_level_bordered", "ref_level_blurred"):
            f = getattr(L, name)
            f.restype = C.c_void_p
            f.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip]
        L.ref_compute_keypoints.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.ref_level_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.ref_distribute.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int]
        L.ref_ic_angle.argtypes = [C.c_void_p, C.c_int, _f32p, _f32p, C.c_int, _f32p]
        L.ref_orb_descriptor.argtypes = [C.c_void_p, C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_void_p]
        L.ref_descriptor_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ref_get_matches_dist_ratio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _u32p, C.c_int, C.c_void_p, C.c_int, _u32p, C.c_int,
                                                 C.c_double, _u32p, _u32p, _ip]
        _lib = L
    return _lib


def _f(a):
    return np.ascontiguousarray(a, np.float32)


class RefExtractor:
    """The reference's ORBextractor object (ORBextractor.h:43-116) behind the shim."""

    def __init__(self, nfeatures=2000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
        self.L = lib()
        self.nlevels, self.nfeatures = nlevels, nfeatures
        self.h = self.L.ref_create(nfeatures, scale_factor, nlevels, ini_th, min_th)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ref_destroy(self.h)
            self.h = None

    def tables(self):
        n = self.nlevels
        sc, isc, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
        q, um, pat = np.zeros(n, np.int32), np.zeros(16, np.int32), np.zeros(1024, np.int32)
        self.L.ref_tables(self.h, O._ptr(sc, _f32p), O._ptr(isc, _f32p), O._ptr(s2, _f32p), O._ptr(is2, _f32p), O._ptr(q, _ip),
                          O._ptr(um, _ip), O._ptr(pat, _ip))
        nu, npat = C.c_int(), C.c_int()
        nl = self.L.ref_table_sizes(self.h, C.byref(nu), C.byref(npat))
        return dict(scale=sc, inv_scale=isc, sigma2=s2, inv_sigma2=is2, quota=q, umax=um, pattern=pat,
                    sizes=np.array([nl, nu.value, npat.value], np.int32))

    def __call__(self, img, lap=(0, 0), cap=None):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape
        cap = cap or (self.nfeatures + 64 * self.nlevels)
        kps, desc, n = np.zeros(cap, O.KP_DTYPE), np.zeros((cap, 32), np.uint8), C.c_int()
        mono = self.L.ref_extract(self.h, O._ptr(img), w, h, img.strides[0], lap[0], lap[1], O._ptr(kps), O._ptr(desc), cap, C.byref(n))
        assert mono != -3, "cap %d too small for %d keypoints" % (cap, n.value)
        return mono, kps[:n.value].copy(), desc[:n.value].copy()

    def _plane(self, fn, level):
        w, h, s = C.c_int(), C.c_int(), C.c_int()
        p = fn(self.h, level, C.byref(w), C.byref(h), C.byref(s))
        buf = (C.c_uint8 * (s.value * h.value)).from_address(p)
        return np.ctypeslib.as_array(buf).reshape(h.value, s.value)[:, :w.value].copy()

    def level_bordered(self, level):
        """mvImagePyramid[level] with its 19-pixel border (the matrix the view lies in)"""
        return self._plane(self.L.ref_level_bordered, level)

    def blurred(self, level):
        return self._plane(self.L.ref_level_blurred, level)

    def compute_keypoints(self, img):
        """ComputePyramid + ComputeKeyPointsOctTree: allKeypoints per level, level coordinates"""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        self.L.ref_compute_keypoints(self.h, O._ptr(img), img.shape[1], img.shape[0], img.strides[0])
        out = []
        for l in range(self.nlevels):
            k = np.zeros(self.nfeatures * 4 + 4096, O.KP_DTYPE)
            n = self.L.ref_level_keypoints(self.h, l, O._ptr(k), len(k))
            assert n <= len(k)
            out.append(k[:n].copy())
        return out

    def distribute(self, x, y, resp, minX, maxX, minY, maxY, N):
        x, y, resp = _f(x), _f(y), _f(resp)
        out = np.zeros(len(x) + 8, np.int32)
        n = self.L.ref_distribute(self.h, O._ptr(x, _f32p), O._ptr(y, _f32p), O._ptr(resp, _f32p), len(x), minX, maxX, minY, maxY, N,
                                  O._ptr(out, _ip), len(out))
        return n, out[:n].copy()

    def ic_angle(self, level, x, y):
        x, y = _f(x), _f(y)
        a = np.zeros(len(x), np.float32)
        self.L.ref_ic_angle(self.h, level, O._ptr(x, _f32p), O._ptr(y, _f32p), len(x), O._ptr(a, _f32p))
        return a

    def orb_descriptor(self, level, x, y, angle):
        x, y, angle = _f(x), _f(y), _f(angle)
        d = np.zeros((len(x), 32), np.uint8)
        self.L.ref_orb_descriptor(self.h, level, O._ptr(x, _f32p), O._ptr(y, _f32p), O._ptr(angle, _f32p), len(x), O._ptr(d))
        return d

    def descriptor_distance(self, a, b):
        a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        return self.L.ref_descriptor_distance(self.h, O._ptr(a), O._ptr(b))

    def get_matches_dist_ratio(self, A, iA, B, iB, ratio=0.85, book=0):
        A = np.ascontiguousarray(A, np.uint8).reshape(-1, 32)
        B = np.ascontiguousarray(B, np.uint8).reshape(-1, 32)
        iA, iB = np.ascontiguousarray(iA, np.uint32), np.ascontiguousarray(iB, np.uint32)
        mA, mB, bk = np.zeros(len(iA) + 1, np.uint32), np.zeros(len(iA) + 1, np.uint32), C.c_int(book)
        n = self.L.ref_get_matches_dist_ratio(self.h, O._ptr(A), len(A), O._ptr(iA, _u32p), len(iA), O._ptr(B), len(B), O._ptr(iB, _u32p),
                                              len(iB), ratio, O._ptr(mA, _u32p), O._ptr(mB, _u32p), C.byref(bk))
        return mA[:n].copy(), mB[:n].copy(), bk.value


# ---------------------------------------------------------------------------------------------------------------------
# bit-for-bit comparison: floats as their 32-bit patterns, the first differing element named with its stage
# ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same(stage, want, got):
    """want: what the reference gave; got: the implementation under test.  Raises AssertionError naming the stage and the first
    differing element."""
    want, got = np.asarray(want), np.asarray(got)
    assert want.shape == got.shape and want.dtype == got.dtype, "stage %s: shape/dtype %s %s, reference %s %s" % (
        stage, got.shape, got.dtype, want.shape, want.dtype)
    bw, bg = bits(want), bits(got)
    if not np.array_equal(bw, bg):
        i = np.argwhere(bw != bg)[0]
        t = tuple(int(v) for v in i)
        raise AssertionError("stage %s: first difference at %s: reference %r, got %r (%d of %d elements differ)" % (
            stage, t, want[t], got[t], int((bw != bg).sum()), bw.size))


def same_keypoints(stage, want, got):
    assert len(want) == len(got), "stage %s: %d keypoints, reference %d" % (stage, len(got), len(want))
    for f in O.KP_DTYPE.names:
        same("%s, KeyPoint field %s" % (stage, f), want[f], got[f])


def same_extraction(tag, want, got):
    """(monoIndex, keypoints, descriptors) of operator()"""
    assert want[0] == got[0], "stage %s, operator() monoIndex: %d, reference %d" % (tag, got[0], want[0])
    same_keypoints("%s, operator() keypoints" % tag, want[1], got[1])
    same("%s, operator() descriptors" % tag, want[2], got[2])


def compare_whole_extractor(tag, img, params=(2000, 1.2, 8, 20, 7), lap=(0, 0)):
    """orc_extract against the reference's operator(): monoIndex, every KeyPoint field, every descriptor byte, every bordered
    pyramid plane, the per-level keypoints of ComputeKeyPointsOctTree.  Returns the reference's (mono, kps, desc)."""
    nf, sf, nl, ini, mn = params
    ora, ref = O.OracleExtractor(nf, sf, nl, ini, mn), RefExtractor(nf, sf, nl, ini, mn)
    cap = nf + 64 * nl + 4096
    got = ora(img, lap=lap, cap=cap)
    assert got[0] >= 0, "%s: the oracle refuses (%d); the reference must not be called where it is undefined" % (tag, got[0])
    want = ref(img, lap=lap, cap=cap)
    for l in range(nl):
        same("%s, ComputePyramid level %d (bordered plane)" % (tag, l), ref.level_bordered(l), ora.level_bordered(l))
    same_extraction(tag, want, got)
    lk = ref.compute_keypoints(img)
    for l in range(nl):
        same_keypoints("%s, ComputeKeyPointsOctTree level %d" % (tag, l), lk[l], ora.level_keypoints(l))
    return want


def staged_rotated_brief(tag, img, params=(2000, 1.2, 8, 20, 7)):
    """The reference never calls IC_Angle (ORBextractor.cpp:475), so the rotated mode is staged: for every keypoint the oracle
    keeps at orientation = 1, the reference's IC_Angle on the reference's own pyramid level equals the oracle's angle, and the
    reference's computeOrbDescriptor at that angle on the reference's blurred level equals the oracle's 32 bytes.
    Returns (per-level keypoints with angles, descriptors) as the reference gave them."""
    nf, sf, nl, ini, mn = params
    ora, ref = O.OracleExtractor(nf, sf, nl, ini, mn, 1), RefExtractor(nf, sf, nl, ini, mn)
    mono, k, d = ora(img, cap=nf + 64 * nl + 4096)
    assert mono == len(k)          # no lapping area: rows are in level order
    lk = ref.compute_keypoints(img)
    row, out_k, out_d = 0, [], []
    for l in range(nl):
        ok = ora.level_keypoints(l)
        for f in ("x", "y", "size", "response", "octave", "class_id"):
            same("%s, ComputeKeyPointsOctTree level %d, KeyPoint field %s" % (tag, l, f), lk[l][f], ok[f])
        ang = ref.ic_angle(l, ok["x"], ok["y"])
        same("%s, IC_Angle level %d" % (tag, l), ang, ok["angle"])
        dd = ref.orb_descriptor(l, ok["x"], ok["y"], ang)
        same("%s, computeOrbDescriptor level %d" % (tag, l), dd, d[row:row + len(ok)])
        if len(ok):
            same("%s, blurred level %d" % (tag, l), ref.blurred(l), ora.blurred(l))
        row += len(ok)
        kk = lk[l].copy()
        kk["angle"] = ang
        out_k.append(kk)
        out_d.append(dd)
    assert row == len(k)
    return out_k, np.concatenate(out_d) if out_d else np.zeros((0, 32), np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# recorded results of the reference binary (tests/golden/ref_*.npz, written by tests/golden/make_ref_golden.py)
# ---------------------------------------------------------------------------------------------------------------------
def pack_keypoints(out, key, k):
    """the keypoints' bit patterns, losslessly, in a form that compresses: field after field, four byte planes per 32-bit value"""
    out[key] = np.concatenate([np.ascontiguousarray(k[f]).view(np.uint8).reshape(-1, 4).T for f in O.KP_DTYPE.names])


def unpack_keypoints(data, key):
    planes = data[key]
    k = np.zeros(planes.shape[1], O.KP_DTYPE)
    for i, f in enumerate(O.KP_DTYPE.names):
        k[f] = np.ascontiguousarray(planes[4 * i:4 * i + 4].T).view(O.KP_DTYPE[f]).ravel()
    return k


def same_as_record(tag, rec, cam, got, levels=None, bordered=None, level_counts=None):
    """got = (monoIndex, keypoints, descriptors) of camera `cam` against the recorded reference result; levels / bordered: the
    implementation's pyramid planes (without / with the 19-pixel border), compared through the recorded checksums"""
    want = (int(rec["mono_%d" % cam][0]), unpack_keypoints(rec, "kps_%d" % cam), rec["desc_%d" % cam])
    same_extraction("%s (recorded reference)" % tag, want, got)
    for what, planes in (("level_sha1", levels), ("bordered_sha1", bordered)):
        for l, p in enumerate(planes or []):
            digest = np.frombuffer(hashlib.sha1(np.ascontiguousarray(p).tobytes()).digest(), np.uint8)
            assert np.array_equal(digest, rec["%s_%d" % (what, cam)][l]), "stage %s, ComputePyramid level %d (%s): plane differs from the recorded reference" % (tag, l, what)
    if level_counts is not None:
        same("%s, ComputeKeyPointsOctTree keypoints per level (recorded reference)" % tag, rec["level_count_%d" % cam], np.asarray(level_counts, np.int32))
