"""mc-slam_amd -- MI355X-native multi-camera ORB front-end (host-side mirror).

Python mirrors of the reference interfaces this path replaces, all thin wrappers
over the C ABI of libmcorb.so (include/mcorb.h):

  ORBextractor        MCSlam/include/MCSlam/ORBextractor.h:43-116
  MultiCameraFrame    MCSlam/include/MCSlam/MultiCameraFrame.h:59-92 (extract + intra-rig match members)
  Rig                 batch/async engine underneath (cameras x frames per launch)

The directory name is not a Python identifier; import it with
``importlib.import_module("mc-slam_amd")`` or through the ``mcorb`` shim at the
repository root.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (E_ARG, E_CAP, E_EMPTY, E_HIP, E_NODEVICE, E_OVERFLOW, E_SIZE, E_STATE, INIT_BASELINE, INIT_DONE, INIT_FEW,
                   INIT_MAX_MATCHES, INIT_PARALLAX, KP_DTYPE, OBS_RECORD, OBS_UPDATE, OK, ORIENT_IC_ANGLE, ORIENT_NONE, McorbError, Params, default_params)
from .synth import synth_rig_frame, synth_rig_frame_numpy

TH_HIGH = 100   # ORBextractor.h:26
TH_LOW = 75     # ORBextractor.h:27
HISTO_LENGTH = 30


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def device_count():
    return _lib.load().mcorb_device_count()


def get_tables(params):
    """Scale tables + per-level quotas (ORBextractor.cpp:413-444)."""
    n = params.nlevels
    sc, isc, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
    q = np.zeros(n, np.int32)
    _lib.check(_lib.load().mcorb_get_tables(C.byref(params), sc.ctypes.data, isc.ctypes.data, s2.ctypes.data,
                                            is2.ctypes.data, q.ctypes.data))
    return dict(scale=sc, inv_scale=isc, sigma2=s2, inv_sigma2=is2, quota=q)


def hamming256(a, b):
    """ORBextractor::DescriptorDistance (ORBextractor.cpp:1202-1218)."""
    a, b = _u8(a).reshape(32), _u8(b).reshape(32)
    return _lib.load().mcorb_hamming256(a.ctypes.data, b.ctypes.data)


def representative_desc(descs):
    """MultiCameraFrame::computeRepresentativeDesc (MultiCameraFrame.cpp:530-567): index of the chosen row."""
    d = _u8(descs).reshape(-1, 32)
    r = _lib.load().mcorb_representative_desc(d.ctypes.data, len(d))
    if r < 0:
        _lib.check(r)
    return r


class Rig:
    """One engine per GPU: `ncams` cameras of w x h, up to `max_frames` rig frames per batch."""

    def __init__(self, ncams, width, height, max_frames=1, nslots=1, params=None, **kw):
        self.L = _lib.load()
        self.params = params if params is not None else default_params(**kw)
        self.ncams, self.w, self.h, self.max_frames, self.nslots = ncams, width, height, max_frames, nslots
        h = C.c_void_p()
        _lib.check(self.L.mcorb_rig_create(C.byref(self.params), ncams, width, height, max_frames, nslots, C.byref(h)))
        self.h_rig = h
        self.kcap = self.L.mcorb_rig_kcap(h)
        self.nlevels = self.params.nlevels

    def close(self):
        if getattr(self, "h_rig", None):
            self.L.mcorb_rig_destroy(self.h_rig)
            self.h_rig = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- staging ------------------------------------------------------------
    def upload(self, images, slot=0):
        """images: list of HxW uint8 arrays (u8 fast path) or float32 [0,1] HxW / HxWx3 (reference format)."""
        first = np.asarray(images[0])
        if first.dtype == np.uint8:
            arrs = [_u8(im) for im in images]
            for a in arrs:
                if a.shape != (self.h, self.w):
                    raise ValueError("image shape %s != (%d,%d)" % (a.shape, self.h, self.w))
            ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
            _lib.check(self.L.mcorb_rig_upload_u8(self.h_rig, slot, ptrs, len(arrs), self.w))
        else:
            arrs = [np.ascontiguousarray(im, dtype=np.float32) for im in images]
            ch = 1 if arrs[0].ndim == 2 else arrs[0].shape[2]
            ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
            _lib.check(self.L.mcorb_rig_upload_f32(self.h_rig, slot, ptrs, len(arrs), arrs[0].strides[0], ch))
        return len(arrs)

    # -- extraction ---------------------------------------------------------
    def staging(self, m, slot=0):
        """The slot's pinned staging plane of image m as a writable (H, W) uint8 array (zero-copy hand-off)."""
        ptr, stride = C.c_void_p(), C.c_int()
        _lib.check(self.L.mcorb_rig_staging(self.h_rig, slot, m, C.byref(ptr), C.byref(stride)))
        buf = (C.c_uint8 * (self.h * stride.value)).from_address(ptr.value)
        return np.frombuffer(buf, np.uint8).reshape(self.h, stride.value)[:, :self.w]

    def upload_staged(self, nimg, slot=0):
        _lib.check(self.L.mcorb_rig_upload_staged(self.h_rig, slot, nimg))

    def extract(self, nimg, slot=0, lap=(0, 0)):
        _lib.check(self.L.mcorb_rig_extract(self.h_rig, slot, nimg, lap[0], lap[1]))

    def extract_submit(self, nimg, slot=0, lap=(0, 0)):
        _lib.check(self.L.mcorb_rig_extract_submit(self.h_rig, slot, nimg, lap[0], lap[1]))

    def extract_wait(self, slot=0):
        _lib.check(self.L.mcorb_rig_extract_wait(self.h_rig, slot))

    def process_submit(self, nframes, slot=0, lap=(0, 0), dist_thresh=75.0, ratio=0.85):
        _lib.check(self.L.mcorb_rig_process_submit(self.h_rig, slot, nframes, lap[0], lap[1], dist_thresh, ratio))

    def process(self, nframes, slot=0, lap=(0, 0), dist_thresh=75.0, ratio=0.85):
        """extract + intra-rig match, synchronously on the calling thread."""
        _lib.check(self.L.mcorb_rig_process(self.h_rig, slot, nframes, lap[0], lap[1], dist_thresh, ratio))

    def process_wait(self, slot=0):
        _lib.check(self.L.mcorb_rig_process_wait(self.h_rig, slot))

    def features(self, m, slot=0):
        n = self.L.mcorb_rig_num_keypoints(self.h_rig, slot, m)
        if n < 0:
            _lib.check(n)
        kps = np.zeros(n, KP_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        nn, mono = C.c_int(), C.c_int()
        _lib.check(self.L.mcorb_rig_get_features(self.h_rig, slot, m, kps.ctypes.data, desc.ctypes.data, n,
                                                 C.byref(nn), C.byref(mono)))
        return mono.value, kps, desc

    # -- UndistortKeyPoints (MultiCameraFrame.cpp:300-347), on the device inside every job -------------------------------
    def set_undistortion(self, cam, K=None, dist=None):
        """camconfig_.K_mats_[cam] (3x3) and dist_coeffs_[cam] (4, 5, 8 or 12 values) as CV_64F; dist None or empty clears"""
        if dist is None or len(np.ravel(dist)) == 0:
            _lib.check(self.L.mcorb_rig_set_undistortion(self.h_rig, cam, None, None, 0))
            return
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        d = np.ascontiguousarray(dist, np.float64).ravel()
        _lib.check(self.L.mcorb_rig_set_undistortion(self.h_rig, cam, K.ctypes.data, d.ctypes.data, d.size))

    # -- the RECTIFY branch of setData (MultiCameraFrame.cpp:123-136): cv::undistort of every image, on the device at the hand-off --
    def set_image_undistortion(self, cam, K=None, dist=None):
        """camconfig_.K_mats_[cam] (3x3) and dist_coeffs_[cam] (4, 5, 8 or 12 values) as CV_64F; dist None or empty clears.  From
        then on every upload() / upload_staged() leaves cv::undistort(img, K, dist) of this camera's images in level 0.  Excludes
        set_undistortion (a rectified rig copies its keypoints)."""
        if dist is None or len(np.ravel(dist)) == 0:
            _lib.check(self.L.mcorb_rig_set_image_undistortion(self.h_rig, cam, None, None, 0))
            return
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        d = np.ascontiguousarray(dist, np.float64).ravel()
        _lib.check(self.L.mcorb_rig_set_image_undistortion(self.h_rig, cam, K.ctypes.data, d.ctypes.data, d.size))

    def image_undistortion_active(self, cam):
        v = self.L.mcorb_rig_image_undistortion_active(self.h_rig, cam)
        if v < 0:
            _lib.check(v)
        return bool(v)

    def undistort_map(self, cam):
        """(map1 (H, W, 2) int16, map2 (H, W) uint16) of a camera with image undistortion set, as built on the host (test hook)"""
        m1 = np.zeros((self.h, self.w, 2), np.int16)
        m2 = np.zeros((self.h, self.w), np.uint16)
        _lib.check(self.L.mcorb_rig_get_undistort_map(self.h_rig, cam, m1.ctypes.data, m2.ctypes.data, self.w * self.h))
        return m1, m2

    def raw_image(self, m, slot=0):
        """the plane of image m as uploaded, before cv::undistort (test hook)"""
        out = np.zeros((self.h, self.w), np.uint8)
        _lib.check(self.L.mcorb_rig_get_raw_image(self.h_rig, slot, m, out.ctypes.data, self.w))
        return out

    # -- transform() and computeIntraMatches(matches, words_) inside every extraction job -------------------------------------
    def set_vocabulary(self, voc, levelsup=4, match=True, max_neighbor_ratio=0.85):
        """Bind an ORBVocabulary (None unbinds): every later extraction job also runs transform(desc, BowVector, FeatureVector,
        levelsup) of every image and, with match, computeIntraMatches(matches, words_) of every frame, on the device in the same
        submission.  Read them with bow_transforms / bow_tracks.  The vocabulary is kept alive while it is bound."""
        if voc is None or voc.h is None:
            _lib.check(self.L.mcorb_rig_set_vocabulary(self.h_rig, None, 0, 0.0, 0))
            self._bow_voc = None
            return
        flags = _lib.BOW_TRANSFORM | (_lib.BOW_MATCH if match else 0)
        _lib.check(self.L.mcorb_rig_set_vocabulary(self.h_rig, voc.h, levelsup, max_neighbor_ratio, flags))
        self._bow_voc = voc

    def bow_transforms(self, img0, nimg, slot=0):
        """the last job's transform() of images [img0, img0 + nimg) -> list of (BowVector, FeatureVector), as
        ORBVocabulary.transform_rig_images returns them"""
        return _read_transforms(self, img0, nimg, slot)

    def bow_tracks(self, frame0, nframes, slot=0):
        """the last job's computeIntraMatches(matches, words_) of frames [frame0, frame0 + nframes) -> list of
        (tracks, n_rays, words), as ORBVocabulary.match_rig_frames returns them"""
        return _read_tracks(self, frame0, nframes, slot)

    # -- obtainLfFeatures + the LF set's transform inside every extraction job -------------------------------------------------
    def set_lf(self, K_mats, R_mats, t_mats, total_feats=3000):
        """camconfig_ K / R / t per camera: from now on every job of a vocabulary bound with match=True also runs obtainLfFeatures
        on its BoW-guided tracks (words_ all 1, no segmentation masks) and the LF set's transform (FrontEnd.cpp:1009-1024).  Read
        them with lf_features / lf_bow.  K_mats = None unbinds."""
        if K_mats is None:
            _lib.check(self.L.mcorb_rig_set_lf(self.h_rig, None, 0))
            return
        _lib.check(self.L.mcorb_rig_set_lf(self.h_rig, _cameras(self.ncams, K_mats, R_mats, t_mats), total_feats))

    def lf_features(self, frame, slot=0):
        """the last job's obtainLfFeatures of one frame -> (features as obtain_lf_features returns them, intramatch_size,
        mono_size, words_fil)"""
        n, ni, nm, nw = (C.c_int() for _ in range(4))
        st = self.L.mcorb_rig_get_lf_features(self.h_rig, slot, frame, None, 0, C.byref(n), C.byref(ni), C.byref(nm), None, 0, C.byref(nw))
        if st != E_CAP:
            _lib.check(st)
        out = np.empty(max(n.value, 1), _lib.LF_DTYPE)
        wf = np.zeros(max(nw.value, 1), np.uint32)
        _lib.check(self.L.mcorb_rig_get_lf_features(self.h_rig, slot, frame, out.ctypes.data, len(out), C.byref(n), C.byref(ni), C.byref(nm),
                                                    wf.ctypes.data, len(wf), C.byref(nw)))
        return out[:n.value].copy(), ni.value, nm.value, wf[:nw.value].copy()

    def lf_bow(self, frame, slot=0):
        """the last job's lfBoW / lfFeatVec of one frame -> (BowVector as (ids, values), FeatureVector as {node: features})"""
        n = C.c_int()
        st = self.L.mcorb_rig_get_lf_features(self.h_rig, slot, frame, None, 0, C.byref(n), None, None, None, 0, None)
        if st != E_CAP:
            _lib.check(st)
        return _read_transform_lists(lambda *a: self.L.mcorb_rig_get_lf_bow(self.h_rig, slot, frame, *a), n.value)

    def undistortion_active(self, cam):
        """True if the reference would call cv::undistortPoints for this camera (set, and not passed by its zero test)"""
        v = self.L.mcorb_rig_undistortion_active(self.h_rig, cam)
        if v < 0:
            _lib.check(v)
        return bool(v)

    def features_undist(self, m, slot=0):
        """image_kps_undist of image m: the keypoint records with pt undistorted (raw for cameras that are not)"""
        n = self.L.mcorb_rig_num_keypoints(self.h_rig, slot, m)
        if n < 0:
            _lib.check(n)
        kps = np.zeros(n, KP_DTYPE)
        nn = C.c_int()
        _lib.check(self.L.mcorb_rig_get_features_undist(self.h_rig, slot, m, kps.ctypes.data, n, C.byref(nn)))
        return kps

    # -- matching -----------------------------------------------------------
    def match(self, nframes, slot=0, dist_thresh=75.0, ratio=0.85):
        _lib.check(self.L.mcorb_rig_match(self.h_rig, slot, nframes, dist_thresh, ratio))

    def pair_matches(self, frame, i, j, slot=0):
        i1 = np.zeros(self.kcap, np.uint32)
        i2 = np.zeros(self.kcap, np.uint32)
        n = C.c_int()
        _lib.check(self.L.mcorb_rig_get_pair_matches(self.h_rig, slot, frame, i, j, i1.ctypes.data, i2.ctypes.data,
                                                     self.kcap, C.byref(n)))
        return i1[:n.value].copy(), i2[:n.value].copy()

    def pair_knn2(self, frame, i, j, slot=0):
        idx = np.zeros((self.kcap, 2), np.int32)
        dist = np.zeros((self.kcap, 2), np.int32)
        n = C.c_int()
        _lib.check(self.L.mcorb_rig_get_pair_knn2(self.h_rig, slot, frame, i, j, idx.ctypes.data, dist.ctypes.data,
                                                  self.kcap, C.byref(n)))
        return idx[:n.value].copy(), dist[:n.value].copy()

    def tracks(self, frame, slot=0):
        cap = self.kcap * self.ncams
        tr = np.full((cap, self.ncams), -1, np.int32)
        n, mg = C.c_int(), C.c_int()
        _lib.check(self.L.mcorb_rig_get_tracks(self.h_rig, slot, frame, tr.ctypes.data, cap, C.byref(n), C.byref(mg)))
        return tr[:n.value].copy(), mg.value

    def tracks_epipolar(self, frame, F, kps_undist=None, slot=0):
        """computeIntraMatches(matches, old=true): F is (npairs, 3, 3) float64 in pair order (0,1),(0,2).."""
        npairs = self.ncams * (self.ncams - 1) // 2
        F = np.ascontiguousarray(F, np.float64).reshape(npairs, 3, 3)
        kp_ptrs = None
        if kps_undist is not None:
            keep = [np.ascontiguousarray(k, KP_DTYPE) for k in kps_undist]
            kp_ptrs = (C.c_void_p * self.ncams)(*[k.ctypes.data for k in keep])
        cap = self.kcap * self.ncams
        tr = np.full((cap, self.ncams), -1, np.int32)
        n, mg = C.c_int(), C.c_int()
        _lib.check(self.L.mcorb_rig_get_tracks_epipolar(self.h_rig, slot, frame, F.ctypes.data, kp_ptrs, tr.ctypes.data, cap,
                                                        C.byref(n), C.byref(mg)))
        return tr[:n.value].copy(), mg.value

    # -- intermediates (parity tests) -----------------------------------------
    def obtain_lf_features(self, frame, tracks, K_mats, R_mats, t_mats, words=None, seg_masks=None, kps_undist=None,
                           total_feats=3000, slot=0):
        """FrontEnd::obtainLfFeatures (FrontEnd.cpp:213-593) for one frame of the slot: returns (features as a structured
        array [match_index, uv_ref, mono, n_rays, point3d, desc], intramatch_size, mono_size, words_fil)."""
        Cn = self.ncams
        tracks = np.ascontiguousarray(tracks, np.int32).reshape(-1, Cn)
        cams = (_lib.Camera * Cn)()
        for c in range(Cn):
            K = np.asarray(K_mats[c], np.float64).reshape(3, 3)
            Rt = np.hstack([np.asarray(R_mats[c], np.float64).reshape(3, 3), np.asarray(t_mats[c], np.float64).reshape(3, 1)])   # build_Rt
            cams[c].K[:] = K.ravel().tolist()
            cams[c].Rt[:] = Rt.ravel().tolist()
        keep, segp, stride = [], None, 0
        if seg_masks is not None:
            segp = (C.c_void_p * Cn)()
            for c in range(Cn):
                if seg_masks[c] is not None:
                    a = np.ascontiguousarray(seg_masks[c], np.float32)
                    assert stride in (0, a.shape[1]), "all segmentation masks must share one row stride"
                    keep.append(a)
                    segp[c] = a.ctypes.data
                    stride = a.shape[1]
        undp = None
        if kps_undist is not None:
            undp = (C.c_void_p * Cn)()
            for c in range(Cn):
                a = np.ascontiguousarray(kps_undist[c], _lib.KP_DTYPE)
                keep.append(a)
                undp[c] = a.ctypes.data
        wp = None
        if words is not None:
            words = np.ascontiguousarray(words, np.uint32)
            assert len(words) >= len(tracks)
            wp = words.ctypes.data
        cap = max(total_feats, len(tracks)) + 1     # intramatch_size <= tracks, and the mono fill stops at total_feats
        out = np.empty(cap, _lib.LF_DTYPE)
        wf = np.zeros(len(tracks) + 1, np.uint32)
        n, ni, nm, nw = (C.c_int() for _ in range(4))
        _lib.check(self.L.mcorb_rig_obtain_lf_features(self.h_rig, slot, frame, tracks.ctypes.data, len(tracks), wp, cams, segp, stride, undp,
                                                       total_feats, out.ctypes.data, cap, C.byref(n), C.byref(ni), C.byref(nm),
                                                       wf.ctypes.data, len(wf), C.byref(nw)))
        return out[:n.value].copy(), ni.value, nm.value, wf[:nw.value].copy()

    def obtain_lf_features_frames(self, frame0, tracks_per_frame, K_mats, R_mats, t_mats, words_per_frame=None, seg_masks=None,
                                  kps_undist=None, total_feats=3000, slot=0):
        """obtainLfFeatures for frames [frame0, frame0 + len(tracks_per_frame)) of the slot in ONE call (one worker-pool task per
        frame).  seg_masks / kps_undist: lists indexed frame * ncams + cam (None entries allowed for masks).  Returns a list of
        (features, intramatch_size, mono_size, words_fil), one per frame."""
        Cn, F = self.ncams, len(tracks_per_frame)
        trs = [np.ascontiguousarray(t, np.int32).reshape(-1, Cn) for t in tracks_per_frame]
        nt = np.array([len(t) for t in trs], np.int32)
        tracks = np.ascontiguousarray(np.concatenate(trs) if nt.sum() else np.zeros((0, Cn), np.int32))
        cams = (_lib.Camera * Cn)()
        for c in range(Cn):
            K = np.asarray(K_mats[c], np.float64).reshape(3, 3)
            Rt = np.hstack([np.asarray(R_mats[c], np.float64).reshape(3, 3), np.asarray(t_mats[c], np.float64).reshape(3, 1)])
            cams[c].K[:] = K.ravel().tolist()
            cams[c].Rt[:] = Rt.ravel().tolist()
        keep, segp, stride = [], None, 0
        if seg_masks is not None:
            segp = (C.c_void_p * (F * Cn))()
            for i in range(F * Cn):
                if seg_masks[i] is not None:
                    a = np.ascontiguousarray(seg_masks[i], np.float32)
                    assert stride in (0, a.shape[1]), "all segmentation masks must share one row stride"
                    keep.append(a)
                    segp[i] = a.ctypes.data
                    stride = a.shape[1]
        undp = None
        if kps_undist is not None:
            undp = (C.c_void_p * (F * Cn))()
            for i in range(F * Cn):
                a = np.ascontiguousarray(kps_undist[i], _lib.KP_DTYPE)
                keep.append(a)
                undp[i] = a.ctypes.data
        wp = None
        if words_per_frame is not None:
            ws = [np.ascontiguousarray(w, np.uint32)[:n] for w, n in zip(words_per_frame, nt)]
            assert all(len(w) == n for w, n in zip(ws, nt)), "one word per track"
            words = np.ascontiguousarray(np.concatenate(ws) if nt.sum() else np.zeros(0, np.uint32))
            keep.append(words)
            wp = words.ctypes.data
        cap = max(total_feats, int(nt.max(initial=0))) + 1     # intramatch_size <= tracks, and the mono fill stops at total_feats
        capw = int(nt.max(initial=0)) + 1
        out = np.empty((F, cap), _lib.LF_DTYPE)
        wf = np.zeros((F, capw), np.uint32)
        n, ni, nm, nw = (np.zeros(F, np.int32) for _ in range(4))
        _lib.check(self.L.mcorb_rig_obtain_lf_features_frames(self.h_rig, slot, frame0, F, tracks.ctypes.data, nt.ctypes.data, wp, cams, segp,
                                                              stride, undp, total_feats, out.ctypes.data, cap, n.ctypes.data, ni.ctypes.data,
                                                              nm.ctypes.data, wf.ctypes.data, capw, nw.ctypes.data))
        return [(out[f, :n[f]].copy(), int(ni[f]), int(nm[f]), wf[f, :nw[f]].copy()) for f in range(F)]

    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        _lib.check(self.L.mcorb_rig_level_size(self.h_rig, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def level(self, m, level, slot=0, blurred=False):
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        fn = self.L.mcorb_rig_get_blurred if blurred else self.L.mcorb_rig_get_level
        _lib.check(fn(self.h_rig, slot, m, level, out.ctypes.data, w))
        return out

    def candidates(self, m, level, slot=0, cap=1 << 17):
        buf = np.zeros(cap, np.uint32)
        n = C.c_int()
        _lib.check(self.L.mcorb_rig_get_candidates(self.h_rig, slot, m, level, buf.ctypes.data, cap, C.byref(n)))
        p = buf[:n.value]
        return ((p >> 8) & 0xfff).astype(np.int32), (p >> 20).astype(np.int32), (p & 0xff).astype(np.int32)

    def info(self):
        o = np.zeros(8, np.int32)
        _lib.check(self.L.mcorb_rig_info(self.h_rig, o.ctypes.data))
        d = dict(zip(("kcap", "cells", "tiles", "cell_cap", "cand_cap", "bucket_total", "img_bytes", "nlevels"), (int(v) for v in o)))
        d["host_threads"] = int(self.L.mcorb_rig_host_threads(self.h_rig))
        return d

    def select_mode(self):
        """'gpu' (DistributeOctTree's list discipline in k_select: a job is one submission) or 'host' (worker pool between two GPU phases)"""
        return {1: "host", 2: "gpu"}[self.L.mcorb_rig_select_mode(self.h_rig)]

    def set_graph(self, every):
        """replay GPU-selected jobs from a captured HIP graph: 0 never, 1 always, K > 1 all but every K-th job of a slot"""
        _lib.check(self.L.mcorb_rig_set_graph(self.h_rig, every))

    def select_fallbacks(self, slot=0):
        """jobs of the slot the host stage had to redo (a level whose tree went below the GPU bucketing depth)"""
        return int(self.L.mcorb_rig_select_fallbacks(self.h_rig, slot))

    def early_reads_rejected(self, slot=0):
        """small batches: images whose early read did not match the signal word's checksum (records redone after the end event)"""
        return int(self.L.mcorb_rig_early_reads_rejected(self.h_rig, slot))

    def timing(self, slot=0):
        t = (C.c_float * 10)()
        _lib.check(self.L.mcorb_rig_last_timing(self.h_rig, slot, t))
        return dict(phase_a_us=t[0], select_us=t[1], phase_b_us=t[2], match_us=t[3], pyramid_us=t[4],
                    fast_us=t[5], compact_us=t[6], knn2_us=t[7], blur_us=t[8], describe_us=t[9])

    # -- multi-GPU plumbing ---------------------------------------------------
    def export_descriptors(self, dst_dev_ptr, nimg, slot=0):
        counts = np.zeros(nimg, np.int32)
        _lib.check(self.L.mcorb_rig_export_descriptors(self.h_rig, slot, dst_dev_ptr, counts.ctypes.data, nimg))
        return counts

    def match_external(self, desc_dev_ptr, counts, sets, slot=0, dist_thresh=75.0, ratio=0.85):
        self.match_external_submit(desc_dev_ptr, counts, sets, slot, dist_thresh, ratio)
        self.match_wait(slot)

    def match_external_submit(self, desc_dev_ptr, counts, sets, slot=0, dist_thresh=75.0, ratio=0.85):
        counts = np.ascontiguousarray(counts, np.int32)
        sets = np.ascontiguousarray(sets, np.int32).reshape(-1, self.ncams)
        self._keep = getattr(self, "_keep", {})
        self._keep[slot] = (counts, sets)          # must outlive the asynchronous job
        _lib.check(self.L.mcorb_rig_match_external_submit(self.h_rig, slot, desc_dev_ptr, counts.ctypes.data, len(counts),
                                                          sets.ctypes.data, len(sets), dist_thresh, ratio))

    def export_descriptors_dev(self, dst_dev_ptr, counts_dev_ptr, nimg, slot=0, then_stream=None):
        """Stream-ordered export: sets + int32 counts into caller device memory; `then_stream` (raw HIP stream handle)
        waits for the copies."""
        if then_stream:
            _lib.require_torch_first("export_descriptors_dev")
        _lib.check(self.L.mcorb_rig_export_descriptors_dev(self.h_rig, slot, dst_dev_ptr, counts_dev_ptr, nimg, then_stream))

    def match_external_dev_submit(self, desc_dev_ptr, counts_dev_ptr, ntotal, sets, slot=0, dist_thresh=75.0, ratio=0.85,
                                  after_stream=None):
        """External match with device-resident counts; the slot's stream waits for `after_stream` (the collective)."""
        if after_stream:
            _lib.require_torch_first("match_external_dev_submit")
        sets = np.ascontiguousarray(sets, np.int32).reshape(-1, self.ncams)
        self._keep = getattr(self, "_keep", {})
        self._keep[slot] = (sets,)                 # must outlive the asynchronous job
        _lib.check(self.L.mcorb_rig_match_external_dev_submit(self.h_rig, slot, desc_dev_ptr, counts_dev_ptr, int(ntotal),
                                                              sets.ctypes.data, len(sets), dist_thresh, ratio, after_stream))

    def match_wait(self, slot=0):
        _lib.check(self.L.mcorb_rig_match_wait(self.h_rig, slot))

    # pair-partitioned matching: explicit (query set, train set) pairs of an external block
    def match_pairs_external(self, desc_dev_ptr, counts, pair_sets, slot=0, dist_thresh=75.0, ratio=0.85):
        counts = np.ascontiguousarray(counts, np.int32)
        pair_sets = np.ascontiguousarray(pair_sets, np.int32).reshape(-1, 2)
        _lib.check(self.L.mcorb_rig_match_pairs_external(self.h_rig, slot, desc_dev_ptr, counts.ctypes.data, len(counts),
                                                         pair_sets.ctypes.data, len(pair_sets), dist_thresh, ratio))

    def match_pairs_external_dev_submit(self, desc_dev_ptr, counts_dev_ptr, ntotal, pair_sets, slot=0, dist_thresh=75.0, ratio=0.85,
                                        after_stream=None):
        if after_stream:
            _lib.require_torch_first("match_pairs_external_dev_submit")
        pair_sets = np.ascontiguousarray(pair_sets, np.int32).reshape(-1, 2)
        self._keep = getattr(self, "_keep", {})
        self._keep[slot] = (pair_sets,)            # must outlive the asynchronous job
        _lib.check(self.L.mcorb_rig_match_pairs_external_dev_submit(self.h_rig, slot, desc_dev_ptr, counts_dev_ptr, int(ntotal),
                                                                    pair_sets.ctypes.data, len(pair_sets), dist_thresh, ratio, after_stream))

    def match_sets(self, block, pair_sets, slot=0, dist_thresh=75.0, ratio=0.85):
        """knnMatch(k=2) + (dist_thresh, ratio) filter between sets of a DescriptorBlock; read with pairlist / pairknn2"""
        pair_sets = np.ascontiguousarray(pair_sets, np.int32).reshape(-1, 2)
        _lib.check(self.L.mcorb_rig_match_sets(self.h_rig, slot, block.h, pair_sets.ctypes.data, len(pair_sets), dist_thresh, ratio))

    def pairknn2(self, pair, slot=0):
        """raw knnMatch(k=2) table of pair `pair` of the last explicit-pair match -> (idx [nq][2], dist [nq][2]), -1 = absent"""
        idx, dist = np.zeros((self.kcap, 2), np.int32), np.zeros((self.kcap, 2), np.int32)
        n = C.c_int()
        _lib.check(self.L.mcorb_rig_get_pairknn2(self.h_rig, slot, pair, idx.ctypes.data, dist.ctypes.data, self.kcap, C.byref(n)))
        return idx[:n.value].copy(), dist[:n.value].copy()

    def pairlist(self, pair, slot=0):
        """accepted (query, train) indices of pair `pair` of the last explicit-pair match -> (idx1, idx2)"""
        i1, i2 = np.zeros(self.kcap, np.uint32), np.zeros(self.kcap, np.uint32)
        n = C.c_int()
        _lib.check(self.L.mcorb_rig_get_pairlist(self.h_rig, slot, pair, i1.ctypes.data, i2.ctypes.data, self.kcap, C.byref(n)))
        return i1[:n.value].copy(), i2[:n.value].copy()


class ORBextractor:
    """Mirror of the reference's ORBextractor (ORBextractor.h:43-116) over libmcorb."""

    HARRIS_SCORE, FAST_SCORE = 0, 1

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, orientation=ORIENT_NONE, device=0):
        self.L = _lib.load()
        self.params = default_params(nfeatures=nfeatures, scale_factor=scaleFactor, nlevels=nlevels,
                                     ini_th_fast=iniThFAST, min_th_fast=minThFAST, orientation=orientation,
                                     device_id=device)
        self._tables = get_tables(self.params)
        self.max_neighbor_ratio = 0.85   # ORBextractor.h:90
        h = C.c_void_p()
        _lib.check(self.L.mcorb_create(C.byref(self.params), 0, 0, C.byref(h)))
        self.h_ext = h

    def close(self):
        if getattr(self, "h_ext", None):
            self.L.mcorb_destroy(self.h_ext)
            self.h_ext = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __call__(self, image, mask=None, vLappingArea=(0, 0)):
        """operator() (ORBextractor.cpp:1085-1171): returns (monoIndex, keypoints, descriptors);
        (-1, None, None) for an empty image, as the reference returns -1.  `mask` is ignored, as in the reference."""
        if image is None or np.asarray(image).size == 0:
            return -1, None, None
        img = np.asarray(image)
        cap = self.params.nfeatures + 8 * self.params.nlevels + 64
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n, mono = C.c_int(), C.c_int()
        if img.dtype == np.uint8:
            assert img.ndim == 2, "image.type() == CV_8UC1 (ORBextractor.cpp:1094)"
            img = _u8(img)
            st = self.L.mcorb_extract(self.h_ext, img.ctypes.data, img.shape[1], img.shape[0], img.strides[0],
                                      vLappingArea[0], vLappingArea[1], kps.ctypes.data, desc.ctypes.data, cap,
                                      C.byref(n), C.byref(mono))
        else:
            img = np.ascontiguousarray(img, np.float32)
            ch = 1 if img.ndim == 2 else img.shape[2]
            st = self.L.mcorb_extract_f32(self.h_ext, img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], ch,
                                          vLappingArea[0], vLappingArea[1], kps.ctypes.data, desc.ctypes.data, cap,
                                          C.byref(n), C.byref(mono))
        if st == E_EMPTY:
            return -1, None, None
        _lib.check(st)
        return mono.value, kps[:n.value].copy(), desc[:n.value].copy()

    def pyramid_level(self, level):
        """mvImagePyramid[level] (interior) of the last call (ORBextractor.h:89)."""
        w, h = C.c_int(), C.c_int()
        _lib.check(self.L.mcorb_get_pyramid_level(self.h_ext, level, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _lib.check(self.L.mcorb_get_pyramid_level(self.h_ext, level, out.ctypes.data, w.value, C.byref(w), C.byref(h)))
        return out

    def GetLevels(self):
        return self.params.nlevels

    def GetScaleFactor(self):
        return float(np.float32(self.params.scale_factor))

    def GetScaleFactors(self):
        return self._tables["scale"].copy()

    def GetInverseScaleFactors(self):
        return self._tables["inv_scale"].copy()

    def GetScaleSigmaSquares(self):
        return self._tables["sigma2"].copy()

    def GetInverseScaleSigmaSquares(self):
        return self._tables["inv_sigma2"].copy()

    def DescriptorDistance(self, a, b):
        return hamming256(a, b)

    def knnMatch2(self, q, t):
        """DescriptorMatcher("BruteForce-Hamming")->knnMatch(q, t, out, 2) on the GPU."""
        q, t = _u8(q).reshape(-1, 32), _u8(t).reshape(-1, 32)
        idx = np.zeros((len(q), 2), np.int32)
        dist = np.zeros((len(q), 2), np.int32)
        _lib.check(self.L.mcorb_knn2(self.h_ext, q.ctypes.data, len(q), t.ctypes.data, len(t), idx.ctypes.data,
                                     dist.ctypes.data))
        return idx, dist

    def matchRatio(self, q, t, dist_thresh=75.0, ratio=0.85):
        """BruteForceMatch's knn2 + ratio/threshold filter (MultiCameraFrame.cpp:1053-1078)."""
        q, t = _u8(q).reshape(-1, 32), _u8(t).reshape(-1, 32)
        i1 = np.zeros(len(q) + 1, np.uint32)
        i2 = np.zeros(len(q) + 1, np.uint32)
        n = C.c_int()
        _lib.check(self.L.mcorb_match_ratio(self.h_ext, q.ctypes.data, len(q), t.ctypes.data, len(t), dist_thresh,
                                            ratio, i1.ctypes.data, i2.ctypes.data, len(q), C.byref(n)))
        return i1[:n.value].copy(), i2[:n.value].copy()

    def getMatches_distRatio(self, A, i_A, B, i_B):
        """ORBextractor::getMatches_distRatio (ORBextractor.cpp:1228-1290): best / second-best search on the
        GPU k-NN kernel, the reference's one-to-one bookkeeping on the host.  Returns (i_match_A, i_match_B, BookK)."""
        A, B = _u8(A).reshape(-1, 32), _u8(B).reshape(-1, 32)
        i_A, i_B = np.asarray(i_A, np.int64), np.asarray(i_B, np.int64)
        mA, mB = [], []
        book = len(i_A) * len(i_B)
        if len(i_A) == 0 or len(i_B) == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), book
        idx, dist = self.knnMatch2(A[i_A], B[i_B])
        for a in range(len(i_A)):
            d1 = float(dist[a, 0])
            d2 = float(dist[a, 1]) if idx[a, 1] >= 0 else 1e9
            # best_dist_1 / best_dist_2 is a double division in the reference (:1264): 0 / 0 (duplicate descriptors) is NaN
            # there, the comparison is false and the feature is skipped
            if d1 <= TH_LOW and d2 > 0 and d1 / d2 <= self.max_neighbor_ratio:
                idx_B = int(i_B[idx[a, 0]])
                if idx_B not in mB:
                    mB.append(idx_B)
                    mA.append(int(i_A[a]))
                else:
                    k = mB.index(idx_B)
                    d = hamming256(A[mA[k]], B[idx_B])
                    book += 1
                    if d1 < d:
                        mA[k] = int(i_A[a])
        return np.array(mA, np.uint32), np.array(mB, np.uint32), book


def _read_transform_lists(fn, n):
    """one image's BowVector / FeatureVector through a getter of the mcorb_vocab_transform output layout"""
    cap = max(n, 1)
    ids, vals = np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
    nodes, offs, feats = np.zeros(cap, np.uint32), np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32)
    nb, nf = C.c_int(), C.c_int()
    _lib.check(fn(ids.ctypes.data, vals.ctypes.data, cap, C.byref(nb), nodes.ctypes.data, offs.ctypes.data, cap, C.byref(nf),
                  feats.ctypes.data, cap))
    bow = (ids[:nb.value].copy(), vals[:nb.value].copy())
    fv = {int(nodes[i]): feats[offs[i]:offs[i + 1]].copy() for i in range(nf.value)}
    return bow, fv


def _cameras(ncams, K_mats, R_mats, t_mats):
    """mcorb_camera per camera: K and build_Rt(R, t) (FrontEnd.cpp:224)"""
    cams = (_lib.Camera * ncams)()
    for c in range(ncams):
        K = np.asarray(K_mats[c], np.float64).reshape(3, 3)
        Rt = np.hstack([np.asarray(R_mats[c], np.float64).reshape(3, 3), np.asarray(t_mats[c], np.float64).reshape(3, 1)])
        cams[c].K[:] = K.ravel().tolist()
        cams[c].Rt[:] = Rt.ravel().tolist()
    return cams


def _read_transforms(rig, img0, nimg, slot):
    out = []
    for m in range(img0, img0 + nimg):
        n = max(rig.L.mcorb_rig_num_keypoints(rig.h_rig, slot, m), 0)
        out.append(_read_transform_lists(lambda *a, m=m: rig.L.mcorb_rig_get_transform(rig.h_rig, slot, m, *a), n))
    return out


def _read_tracks(rig, frame0, nframes, slot):
    out, cap = [], rig.kcap * rig.ncams
    for f in range(frame0, frame0 + nframes):
        tr = np.full((cap, rig.ncams), -1, np.int32)
        nr = np.zeros(cap, np.int32)
        words = np.zeros(cap, np.uint32)
        nt, nw = C.c_int(), C.c_int()
        _lib.check(rig.L.mcorb_rig_get_bow_tracks(rig.h_rig, slot, f, tr.ctypes.data, nr.ctypes.data, cap, C.byref(nt),
                                                  words.ctypes.data, cap, C.byref(nw)))
        out.append((tr[:nt.value].copy(), nr[:nt.value].copy(), words[:nw.value].copy()))
    return out


class ORBVocabulary:
    """DBoW2::ORBVocabulary (MCSlam/include/MCSlam/ORBVocabulary.h:21-30) as far as this path uses it:
    loadFromTextFile + transform(features, BowVector, FeatureVector, levelsup)."""

    def __init__(self, device=0):
        self.L_ = _lib.load()
        self.device = device
        self.h = None

    def loadFromTextFile(self, filename):
        h = C.c_void_p()
        st = self.L_.mcorb_vocab_load_text(filename.encode(), self.device, C.byref(h))
        if st != OK:
            return False          # the reference returns false and the caller exits (FrontEnd.h:139-143)
        self.close()
        self.h = h
        return True

    def create(self, k, L, scoring, weighting, parent, is_leaf, desc, weight):
        parent = np.ascontiguousarray(parent, np.int32)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = _u8(desc).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, np.float64)
        h = C.c_void_p()
        _lib.check(self.L_.mcorb_vocab_create(k, L, scoring, weighting, parent.ctypes.data, is_leaf.ctypes.data,
                                              desc.ctypes.data, weight.ctypes.data, len(parent), self.device, C.byref(h)))
        self.close()
        self.h = h
        return self

    def close(self):
        if getattr(self, "h", None):
            self.L_.mcorb_vocab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        k, L, nn, nw = (C.c_int() for _ in range(4))
        _lib.check(self.L_.mcorb_vocab_info(self.h, C.byref(k), C.byref(L), C.byref(nn), C.byref(nw)))
        return dict(k=k.value, L=L.value, nodes=nn.value, words=nw.value)

    def _call(self, fn, head, n, levelsup):
        return _read_transform_lists(lambda *a: fn(*head, levelsup, *a), n)

    def transform(self, features, levelsup=4):
        """-> BowVector as (word ids ascending, values), FeatureVector as {node id: feature indices}."""
        d = _u8(features).reshape(-1, 32)
        return self._call(self.L_.mcorb_vocab_transform, (self.h, d.ctypes.data, len(d)), len(d), levelsup)

    def match_rig_frame(self, rig, frame=0, slot=0, levelsup=4, max_neighbor_ratio=0.85):
        """computeIntraMatches(matches, words_) (MultiCameraFrame.cpp:586-943): (tracks, n_rays, words)."""
        cap = rig.kcap * rig.ncams
        tr = np.full((cap, rig.ncams), -1, np.int32)
        nr = np.zeros(cap, np.int32)
        words = np.zeros(cap, np.uint32)
        nt, nw = C.c_int(), C.c_int()
        _lib.check(self.L_.mcorb_rig_match_bow(rig.h_rig, slot, frame, self.h, levelsup, max_neighbor_ratio, tr.ctypes.data,
                                               nr.ctypes.data, cap, C.byref(nt), words.ctypes.data, cap, C.byref(nw)))
        return tr[:nt.value].copy(), nr[:nt.value].copy(), words[:nw.value].copy()

    def match_rig_frames(self, rig, frame0, nframes, slot=0, levelsup=4, max_neighbor_ratio=0.85, y_undist=None):
        """computeIntraMatches(matches, words_) for frames [frame0, frame0 + nframes) at once -> list of (tracks, n_rays, words).
        y_undist: optional list, one float32 array per image of the SLOT (index frame * ncams + cam; None entries allowed for
        images outside the range) = image_kps_undist[cam][k].pt.y, the rows the reference's |dy| < 50 gate reads."""
        ptrs, keep = None, []
        if y_undist is not None:
            arr = (C.c_void_p * len(y_undist))()
            for i, y in enumerate(y_undist):
                if y is not None:
                    a = np.ascontiguousarray(y, np.float32)
                    keep.append(a)
                    arr[i] = a.ctypes.data
            ptrs = arr
        _lib.check(self.L_.mcorb_rig_match_bow_frames(rig.h_rig, slot, frame0, nframes, self.h, levelsup, max_neighbor_ratio, ptrs))
        return _read_tracks(rig, frame0, nframes, slot)

    def transform_rig_images(self, rig, img0, nimg, slot=0, levelsup=4):
        """transform() of images [img0, img0 + nimg) of a slot in one call -> list of (BowVector, FeatureVector)."""
        _lib.check(self.L_.mcorb_rig_transform_images(rig.h_rig, slot, img0, nimg, self.h, levelsup))
        return _read_transforms(rig, img0, nimg, slot)

    def transform_rig_image(self, rig, m, slot=0, levelsup=4):
        """transform() of image m's descriptors straight from the rig's HBM buffers (MultiCameraFrame.cpp:257)."""
        n = rig.L.mcorb_rig_num_keypoints(rig.h_rig, slot, m)
        return self._call(self.L_.mcorb_rig_transform_image, (rig.h_rig, slot, m, self.h), max(n, 0), levelsup)


class ORBDatabase:
    """DBoW2's ORBDatabase as place recognition uses it (LoopCloser::callerDetectLoop, MCSlam/src/LoopCloser.cpp:59-241): add,
    query, the vocabulary's score of two stored vectors, and featureMatchesBow between two stored keyframes (mcorb_kfdb); probe
    slots hold the frames that are matched against keyframes without becoming one (tracking, relocalization).
    device >= 0: the store lives in HBM on the vocabulary's device; device = -1: a host-only database that needs no GPU."""

    def __init__(self, voc, device=0, max_entries=1024, max_words=4096, max_feats=4096):
        self.L = _lib.load()
        self.h = C.c_void_p()
        self.voc = voc   # (kept alive with the database)
        self.max_entries, self.max_words, self.max_feats = max_entries, max_words, max_feats
        _lib.check(self.L.mcorb_kfdb_create(voc.h, device, max_entries, max_words, max_feats, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.L.mcorb_kfdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _vectors(bow, fv, desc):
        """a frame's vectors as the C ABI takes them: the arrays (kept alive by the caller) and mcorb_kfdb_add's argument list"""
        ids = np.ascontiguousarray(bow[0], np.uint32)
        vals = np.ascontiguousarray(bow[1], np.float64)
        keys = sorted(fv)
        nodes = np.array(keys, np.uint32)
        offs = np.zeros(len(keys) + 1, np.int32)
        offs[1:] = np.cumsum([len(fv[k]) for k in keys])
        feats = np.concatenate([np.asarray(fv[k], np.int32).reshape(-1) for k in keys]).astype(np.int32) if keys else np.zeros(0, np.int32)
        d = _u8(desc).reshape(-1, 32)
        keep = (ids, vals, nodes, offs, feats, d)
        return keep, (ids.ctypes.data, vals.ctypes.data, len(ids), nodes.ctypes.data, offs.ctypes.data, len(keys), feats.ctypes.data,
                      d.ctypes.data, len(d))

    def add(self, bow, fv, desc):
        """bow: (word ids ascending, values); fv: {node id: feature indices}; desc: the keyframe's LF descriptors -> entry id"""
        keep, args = self._vectors(bow, fv, desc)
        e = C.c_int()
        _lib.check(self.L.mcorb_kfdb_add(self.h, *args, C.byref(e)))
        return e.value

    def add_rig_frame(self, rig, frame, slot=0):
        """lfBoW, lfFeatVec and the LF descriptors of a frame of the slot's last job (Rig.set_lf) -> entry id"""
        e = C.c_int()
        _lib.check(self.L.mcorb_kfdb_add_rig_frame(self.h, rig.h_rig, slot, frame, C.byref(e)))
        return e.value

    def size(self):
        return self.L.mcorb_kfdb_size(self.h)

    def _stored(self, get, i):
        W, F = max(self.max_words, 1), max(self.max_feats, 1)
        ids, vals = np.zeros(W, np.uint32), np.zeros(W, np.float64)
        nodes, offs, feats = np.zeros(F, np.uint32), np.zeros(F + 1, np.int32), np.zeros(F, np.int32)
        desc = np.zeros((F, 32), np.uint8)
        nb, nf, nd = C.c_int(), C.c_int(), C.c_int()
        _lib.check(get(self.h, i, ids.ctypes.data, vals.ctypes.data, W, C.byref(nb), nodes.ctypes.data, offs.ctypes.data, F, C.byref(nf),
                       feats.ctypes.data, F, desc.ctypes.data, F, C.byref(nd)))
        fv = {int(nodes[k]): feats[offs[k]:offs[k + 1]].copy() for k in range(nf.value)}
        return (ids[:nb.value].copy(), vals[:nb.value].copy()), fv, desc[:nd.value].copy()

    def entry(self, i):
        """-> (BowVector as (ids, values), FeatureVector as {node: feature indices}, descriptors) of entry i as stored"""
        return self._stored(self.L.mcorb_kfdb_get_entry, i)

    def query(self, bow, max_results, max_id=-1):
        """TemplatedDatabase::query -> (entry ids, scores), best first"""
        ids = np.ascontiguousarray(bow[0], np.uint32)
        vals = np.ascontiguousarray(bow[1], np.float64)
        cap = max(self.size(), 1)
        out_ids, out_sc = np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
        n = C.c_int()
        _lib.check(self.L.mcorb_kfdb_query(self.h, ids.ctypes.data, vals.ctypes.data, len(ids), max_results, max_id,
                                           out_ids.ctypes.data, out_sc.ctypes.data, cap, C.byref(n)))
        return out_ids[:n.value].copy(), out_sc[:n.value].copy()

    def _query_stored(self, call, sel, max_ids, max_results):
        sel = np.ascontiguousarray(sel, np.int32)
        mx = np.ascontiguousarray(max_ids, np.int32)
        assert len(sel) == len(mx)
        nq, cap = len(sel), max(self.size(), 1)
        out_ids, out_sc = np.zeros((max(nq, 1), cap), np.uint32), np.zeros((max(nq, 1), cap), np.float64)
        n = np.zeros(max(nq, 1), np.int32)
        _lib.check(call(self.h, sel.ctypes.data, mx.ctypes.data, nq, max_results, out_ids.ctypes.data, out_sc.ctypes.data, cap, n.ctypes.data))
        return [(out_ids[q, :n[q]].copy(), out_sc[q, :n[q]].copy()) for q in range(nq)]

    def query_entries(self, entries, max_ids, max_results):
        """the queries are entries of the database, all in one launch, each with its own max_id -> list of (entry ids, scores)"""
        return self._query_stored(self.L.mcorb_kfdb_query_entries, entries, max_ids, max_results)

    def score(self, a, b):
        """TemplatedVocabulary::score of the BowVectors of entries a and b"""
        s = C.c_double()
        _lib.check(self.L.mcorb_kfdb_score(self.h, a, b, C.byref(s)))
        return s.value

    def featureMatchesBow(self, best_entry, curr_entry, max_neighbor_ratio=0.85):
        """LoopCloser::featureMatchesBow -> (indices_1 into best_entry's LF set, indices_2 into curr_entry's)"""
        cap = max(self.max_feats, 1)
        i1, i2 = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        n = C.c_int()
        _lib.check(self.L.mcorb_kfdb_feature_matches(self.h, best_entry, curr_entry, max_neighbor_ratio, i1.ctypes.data, i2.ctypes.data,
                                                     cap, C.byref(n)))
        return i1[:n.value].copy(), i2[:n.value].copy()

    def timing(self):
        """microseconds of the last k_kfdb_score and k_kfdb_best2 launch (a device database)"""
        us = (C.c_float * 2)()
        _lib.check(self.L.mcorb_kfdb_last_timing(self.h, us))
        return us[0], us[1]

    # probe slots: frames held in the database's layout without being entries (the current frame of FrontEnd::trackFrame and of
    # Relocalization); no call below changes size(), an entry or a query's result
    def reserve_probes(self, nprobes):
        """allocates nprobes (1 .. 128) probe slots; once per database"""
        _lib.check(self.L.mcorb_kfdb_reserve_probes(self.h, nprobes))

    def set_probe(self, probe, bow, fv, desc):
        """add()'s arguments into probe slot `probe` (overwrites it)"""
        keep, args = self._vectors(bow, fv, desc)
        _lib.check(self.L.mcorb_kfdb_set_probe(self.h, probe, *args))

    def set_probe_rig_frame(self, probe, rig, frame, slot=0):
        """add_rig_frame()'s frame into probe slot `probe`"""
        _lib.check(self.L.mcorb_kfdb_set_probe_rig_frame(self.h, probe, rig.h_rig, slot, frame))

    def get_probe(self, probe):
        """-> (BowVector, FeatureVector, descriptors) of a probe slot as stored, like entry()"""
        return self._stored(self.L.mcorb_kfdb_get_probe, probe)

    def query_probes(self, probes, max_ids, max_results):
        """query_entries() with probe slots as the queries, all in one launch -> list of (entry ids, scores)"""
        return self._query_stored(self.L.mcorb_kfdb_query_probes, probes, max_ids, max_results)

    def score_probe(self, entry, probe):
        """TemplatedVocabulary::score of an entry's BowVector and a probe's"""
        s = C.c_double()
        _lib.check(self.L.mcorb_kfdb_score_probe(self.h, entry, probe, C.byref(s)))
        return s.value

    def probe_feature_matches(self, entry, probes, max_neighbor_ratio=0.85):
        """FrontEnd::InterMatchingBow / Relocalization::featureMatchesBow of one entry against several probes in one launch ->
        list of (indices_1 into the entry's LF set, indices_2 into the probe's)"""
        pr = np.ascontiguousarray(probes, np.int32)
        np_, cap = len(pr), max(self.max_feats, 1)
        i1, i2 = np.zeros((max(np_, 1), cap), np.uint32), np.zeros((max(np_, 1), cap), np.uint32)
        n = np.zeros(max(np_, 1), np.int32)
        _lib.check(self.L.mcorb_kfdb_probe_feature_matches(self.h, entry, pr.ctypes.data, np_, max_neighbor_ratio, i1.ctypes.data,
                                                           i2.ctypes.data, cap, n.ctypes.data))
        return [(i1[p, :n[p]].copy(), i2[p, :n[p]].copy()) for p in range(np_)]

    def probe_inter_matches_bf(self, entry, probe, lids_prev, mono_prev, p3d_prev, mono_cur, p3d_cur):
        """FrontEnd::findInterMatches of an entry (lf_prev) and a probe (lf_cur): lids_prev / mono_prev / p3d_prev (n x 3) per LF
        feature of the entry, mono_cur / p3d_cur of the probe -> (queryIdx, trainIdx, distance) of matches_z_filtered"""
        lids = np.ascontiguousarray(lids_prev, np.int32).reshape(-1)
        m1 = np.ascontiguousarray(np.asarray(mono_prev) != 0, np.uint8).reshape(-1)
        m2 = np.ascontiguousarray(np.asarray(mono_cur) != 0, np.uint8).reshape(-1)
        p1 = np.ascontiguousarray(p3d_prev, np.float64).reshape(-1, 3)
        p2 = np.ascontiguousarray(p3d_cur, np.float64).reshape(-1, 3)
        assert len(lids) == len(m1) == len(p1) and len(m2) == len(p2)
        cap = max(self.max_feats, 1)
        q, t, d = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int()
        _lib.check(self.L.mcorb_kfdb_probe_inter_matches_bf(self.h, entry, probe, lids.ctypes.data, m1.ctypes.data, p1.ctypes.data,
                                                            m2.ctypes.data, p2.ctypes.data, q.ctypes.data, t.ctypes.data, d.ctypes.data,
                                                            cap, C.byref(n)))
        return q[:n.value].copy(), t[:n.value].copy(), d[:n.value].copy()

    def probe_timing(self):
        """microseconds of the last k_kfdb_best2, many-probe launch (a device database)"""
        us = C.c_float()
        _lib.check(self.L.mcorb_kfdb_last_probe_timing(self.h, C.byref(us)))
        return us.value


class LocalMapResult:
    """what LocalMap.search returns: new_lids / cam_masks (lm_projected_cam_ids as bit masks) of the accepted landmarks in order,
    ind1 / ind2 as InterMatchingBow returns them (ind1 indexes new_lids), and matches (queryIdx, trainIdx) after the camera filter"""

    def __init__(self, new_lids, cam_masks, ind1, ind2, matches):
        self.new_lids, self.cam_masks, self.ind1, self.ind2, self.matches = new_lids, cam_masks, ind1, ind2, matches

    def cam_ids(self, i):
        """lm_projected_cam_ids[i] as the reference's list"""
        return [c for c in range(_lib.MAX_CAMS) if (int(self.cam_masks[i]) >> c) & 1]


def lmap_view(Rcw, tcw, R_mats, t_mats, K_mats, centres_w, width, height):
    """the view of LocalMap.search: rows and column of currentFrame->pose.inv(), camconfig_'s R / t / K per camera and the
    translation column of W_T_cur_vec[cam] (FrontEnd.cpp:4953-4970), im_size_"""
    v = _lib.LmapView()
    v.Rcw[:] = np.asarray(Rcw, np.float64).reshape(9).tolist()
    v.tcw[:] = np.asarray(tcw, np.float64).reshape(3).tolist()
    v.ncams, v.width, v.height = len(R_mats), int(width), int(height)
    if not 1 <= v.ncams <= _lib.MAX_CAMS or not len(t_mats) == len(K_mats) == len(centres_w) == v.ncams:
        raise ValueError("lmap_view: 1 .. %d cameras, one R, t, K and centre each" % _lib.MAX_CAMS)
    for c in range(v.ncams):
        v.cams[c].R[:] = np.asarray(R_mats[c], np.float64).reshape(9).tolist()
        v.cams[c].t[:] = np.asarray(t_mats[c], np.float64).reshape(3).tolist()
        v.cams[c].K[:] = np.asarray(K_mats[c], np.float64).reshape(9).tolist()
        v.cams[c].centre_w[:] = np.asarray(centres_w[c], np.float64).reshape(3).tolist()
    return v


def lf_mono_cam(lf):
    """mono_cur / cam_cur of LocalMap.search from mcorb_lf_feature records (Rig.lf_features): im2.mono, and the first camera whose
    matchIndex is not -1 (ii2, FrontEnd.cpp:5147-5153; -1 for a record without a view)"""
    lf = np.asarray(lf)
    seen = lf["match_index"] != -1
    cam = np.where(seen.any(axis=1), seen.argmax(axis=1), -1).astype(np.int32)
    return (lf["mono"] != 0).astype(np.uint8), cam


class MapFrameArrays:
    """one keyframe's observations for LocalMap.triangulate_neighbours (mcorb_map_frame); keeps the arrays the struct points to"""

    def __init__(self, match_index, kps_undist, centres_w, proj, twc):
        self.match_index = np.ascontiguousarray(match_index, np.int32)
        if self.match_index.ndim != 2:
            raise ValueError("map_frame: match_index is nfeat x ncams")
        nfeat, ncams = self.match_index.shape
        if not 1 <= ncams <= _lib.MAX_CAMS or not len(kps_undist) == len(centres_w) == len(proj) == ncams:
            raise ValueError("map_frame: 1 .. %d cameras, one keypoint array, centre and projection matrix each" % _lib.MAX_CAMS)
        self.kps = [np.ascontiguousarray(k, KP_DTYPE).reshape(-1) for k in kps_undist]
        self.nkps = np.array([len(k) for k in self.kps], np.int32)
        self.ptrs = (C.c_void_p * ncams)(*[k.ctypes.data for k in self.kps])
        f = self.struct = _lib.MapFrame()
        f.nfeat, f.ncams = nfeat, ncams
        f.match_index, f.kps_undist, f.nkps = self.match_index.ctypes.data, self.ptrs, self.nkps.ctypes.data
        for c in range(ncams):
            f.centre_w[c][:] = np.asarray(centres_w[c], np.float64).reshape(3).tolist()
            f.proj[c][:] = np.asarray(proj[c], np.float64).reshape(-1)[:12].tolist()
        f.twc[:] = np.asarray(twc, np.float64).reshape(3).tolist()


def map_frame(lf, kps_undist, centres_w, proj, twc):
    """the frame of LocalMap.triangulate_neighbours from mcorb_lf_feature records (Rig.lf_features; or an nfeat x ncams matchIndex
    array) and image_kps_undist per camera; centres_w: W_T_cur's translation per camera; proj: cur_T_ref * pose.inv() per camera
    (3x4 or 4x4, rows 0..2 are read); twc: the pose's translation column"""
    lf = np.asarray(lf)
    mi = lf["match_index"][:, :len(kps_undist)] if lf.dtype.names else lf
    return MapFrameArrays(mi, kps_undist, centres_w, proj, twc)


class TriangulationResult:
    """what LocalMap.triangulate_neighbours returns.  Per match, the neighbours' matches back to back (offsets[s] is neighbour s's
    first): inliers, verdict (0 landmark, 1 epipolar den == 0, 2 epipolar distance, 3 behind a camera, 4 chi-square, 5 parallax
    window, 6 a feature had a landmark already, 7 neighbour skipped), new_lid (-1: none), pt3d, normal, dist2, cos_parallax; per
    neighbour: neigh_skipped (0 used, 1 baseline gate, 2 no landmarks); depth_vec in the order the landmarks were made;
    n_triangulated; next_lid; lids_cur and lids_neigh as the call leaves them"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class NewLandmarksResult:
    """what LocalMap.triangulate_new returns.  Per match: inliers (true exactly for a new landmark), verdict (0 landmark, 3 behind a
    camera at the initial point, 4 chi-square, 5 parallax, 6 the current feature had a landmark already, 8 degenerate), new_lid
    (-1: none), pt3d, normal, dist, cos_parallax (float32), iterations, cost_initial, cost_final; depth_vec in the order the
    landmarks were made, avg_depth (their sum), n_rays_hist, n_by_verdict, n_triangulated, next_lid; lids_cur and lids_prev as the
    call leaves them"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class InitResult:
    """what LocalMap.initialize and init_cases return.  status (INIT_DONE, INIT_BASELINE, INIT_PARALLAX, INIT_FEW); per match:
    inliers (as the loop leaves them: true exactly for verdict 0), verdict (0 a landmark candidate, 3 behind a camera, 4
    chi-square, 5 cos >= 0.99998 or NaN, 9 the flag was clear on entry), new_lid (-1: none), pt3d (the stored, scaled point when
    status is INIT_DONE), normal, dist2, cos_parallax; parallax and median_scene_depth (the two medians), t_out, scaled,
    n_initial_inliers, n_parallax, n_triangulated, next_lid; lids_prev and lids_cur as the call leaves them"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _init_scalars(o):
    return dict(status=o.status, parallax=o.parallax, median_scene_depth=o.median_scene_depth, t_out=np.array(o.t_out[:]),
                n_matches=o.n_matches, n_initial_inliers=o.n_initial_inliers, n_parallax=o.n_parallax,
                n_triangulated=o.n_triangulated, scaled=bool(o.scaled), next_lid=o.next_lid)


def _map_outputs(o, cap, total, per_match, **other):
    """the output arrays of LocalMap.triangulate_neighbours, .triangulate_new and .initialize, their addresses written into the
    ctypes record o: per match inliers, verdict, new_lid, pt3d, normal (3 wide) and the call's own `per_match` (name -> dtype),
    max(cap, 1) rows each; `other`: name -> (dtype, size), max(size, 1) elements -> (the arrays by name, cut(name): the
    array's rows of the call's `total` matches, copied)"""
    spec = dict(inliers=np.uint8, verdict=np.uint8, new_lid=np.int32, **per_match)
    r = {k: np.zeros(max(cap, 1), t) for k, t in spec.items()}
    r.update(pt3d=np.zeros(3 * max(cap, 1)), normal=np.zeros(3 * max(cap, 1)))
    r.update({k: np.zeros(max(size, 1), t) for k, (t, size) in other.items()})
    for k, a in r.items():
        setattr(o, k, a.ctypes.data)
    return r, lambda k: r[k][:(3 if k in ("pt3d", "normal") else 1) * total].copy()


class LocalMap:
    """FrontEnd::searchLocalMap2 (MCSlam/src/FrontEnd.cpp:4901-5223) up to the camera-filtered matches (mcorb_lmap): a store of
    landmarks (slot = lId: pt3D, normal, the latest observation's descriptor and mono flag) and the search of a frame held in a
    probe slot of an ORBDatabase against the landmarks of its neighbouring keyframes.
    device >= 0: the store lives in HBM on the vocabulary's device; device = -1: a host-only store that needs no GPU (on a host-only
    vocabulary, searching host-only databases)."""

    def __init__(self, voc, device=0, max_landmarks=1 << 16, max_candidates=1 << 16):
        self.L = _lib.load()
        self.h = C.c_void_p()
        self.voc = voc   # (kept alive with the store)
        self.max_landmarks, self.max_candidates = max_landmarks, max_candidates
        _lib.check(self.L.mcorb_lmap_create(voc.h, device, max_landmarks, max_candidates, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.L.mcorb_lmap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _opt(a, dtype, shape):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype).reshape(shape)
        return a, a.ctypes.data

    def set(self, lids, pt3d=None, normal=None, desc=None, mono=None):
        """slots lids take pt3d / normal (n x 3), desc (n x 32) and mono (n); None keeps what the slots hold"""
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        n = len(lids)
        p, pp = self._opt(pt3d, np.float64, (n, 3))
        q, qp = self._opt(normal, np.float64, (n, 3))
        d, dp = self._opt(desc, np.uint8, (n, 32))
        m, mp = self._opt(None if mono is None else np.asarray(mono) != 0, np.uint8, (n,))
        _lib.check(self.L.mcorb_lmap_set(self.h, lids.ctypes.data, n, pp, qp, dp, mp))

    def set_desc_from_entry(self, db, entry, lids, feats, mono=None):
        """the descriptors of LF features `feats` of a database entry into slots lids (device to device on a device store)"""
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        feats = np.ascontiguousarray(feats, np.int32).reshape(-1)
        assert len(lids) == len(feats)
        m, mp = self._opt(None if mono is None else np.asarray(mono) != 0, np.uint8, (len(lids),))
        _lib.check(self.L.mcorb_lmap_set_desc_from_entry(self.h, db.h, entry, lids.ctypes.data, feats.ctypes.data, len(lids), mp))

    def get(self, lid):
        """-> (pt3D, normal, descriptor or None, mono) of a slot as stored"""
        p, q, d = np.zeros(3), np.zeros(3), np.zeros(32, np.uint8)
        mono, has = C.c_int(), C.c_int()
        _lib.check(self.L.mcorb_lmap_get(self.h, lid, p.ctypes.data, q.ctypes.data, d.ctypes.data, C.byref(mono), C.byref(has)))
        return p, q, (d if has.value else None), bool(mono.value)

    def search(self, view, neighbour_lids, matched_lids, db, probe, matched_cur, mono_cur, cam_cur, levelsup=4, max_neighbor_ratio=0.85,
               caps=None):
        """searchLocalMap2's candidates, frustum test, transform, InterMatchingBow and camera filter -> LocalMapResult.
        view: lmap_view(...); neighbour_lids: the neighbouring keyframes' lIds back to back in kfMap's order; matched_lids:
        matchedlmset; db / probe: the current frame's probe slot; matched_cur / mono_cur / cam_cur: per LF feature of the probe
        (lf_mono_cam); caps: (accepted, ind, matches) output sizes, by default what cannot be exceeded"""
        nl = np.ascontiguousarray(neighbour_lids, np.int32).reshape(-1)
        ml = np.ascontiguousarray(matched_lids, np.int32).reshape(-1)
        mc_ = np.ascontiguousarray(np.asarray(matched_cur) != 0, np.uint8).reshape(-1)
        mo = np.ascontiguousarray(np.asarray(mono_cur) != 0, np.uint8).reshape(-1)
        cc = np.ascontiguousarray(cam_cur, np.int32).reshape(-1)
        assert len(mc_) == len(mo) == len(cc)
        cap_new, cap_ind, cap_m = caps if caps is not None else (max(len(nl), 1), max(db.max_feats, 1), max(db.max_feats, 1))
        new_lids, masks = np.zeros(max(cap_new, 1), np.int32), np.zeros(max(cap_new, 1), np.uint32)
        i1, i2 = np.zeros(max(cap_ind, 1), np.uint32), np.zeros(max(cap_ind, 1), np.uint32)
        mq, mt = np.zeros(max(cap_m, 1), np.int32), np.zeros(max(cap_m, 1), np.int32)
        self.counts = nn, ni, nm = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self.L.mcorb_lmap_search(self.h, C.byref(view), nl.ctypes.data, len(nl), ml.ctypes.data, len(ml), db.h, probe,
                                            mc_.ctypes.data, mo.ctypes.data, cc.ctypes.data, levelsup, max_neighbor_ratio,
                                            new_lids.ctypes.data, masks.ctypes.data, cap_new, C.byref(nn), i1.ctypes.data, i2.ctypes.data,
                                            cap_ind, C.byref(ni), mq.ctypes.data, mt.ctypes.data, cap_m, C.byref(nm)))
        return LocalMapResult(new_lids[:nn.value].copy(), masks[:nn.value].copy(), i1[:ni.value].copy(), i2[:ni.value].copy(),
                              np.stack([mq[:nm.value], mt[:nm.value]], axis=1).copy())

    def last_timing(self):
        """(microseconds of the last k_lmap_cull launch, of the last k_kfdb_best2 launch, candidates of the last search); a device store"""
        us = (C.c_float * 2)()
        n = C.c_int()
        _lib.check(self.L.mcorb_lmap_last_timing(self.h, us, C.byref(n)))
        return us[0], us[1], n.value


    def triangulate_neighbours(self, cur, lids_cur, neigh, lids_neigh, F21, matches, K_mats, inv_sigma2, Rcw, tcw, next_lid, caps=None):
        """FrontEnd::triangulateNeighbors (FrontEnd.cpp:4856-4899) -> TriangulationResult; the new landmarks' points and normals are
        stored in their slots.  cur / neigh: map_frame(...) of the current frame and of the neighbouring keyframes in
        kfMap.rbegin() order; lids_cur / lids_neigh: their lIds (copied: the result holds the updated arrays); F21: per neighbour
        ncams x ncams x 3 x 3, index [c_cur][c_neigh]; matches: per neighbour an n x 2 array (queryIdx, trainIdx); K_mats: per
        camera; inv_sigma2: GetInverseScaleSigmaSquares(); Rcw / tcw: currentFrame->pose.inv(); caps: (matches, depth_vec) output
        sizes, by default what cannot be exceeded"""
        S, nc = len(neigh), cur.struct.ncams
        assert len(lids_neigh) == len(F21) == len(matches) == S
        lc = np.array(lids_cur, np.int32).reshape(-1)
        ln = [np.array(l, np.int32).reshape(-1) for l in lids_neigh]
        assert len(lc) == cur.struct.nfeat and all(len(l) == f.struct.nfeat for l, f in zip(ln, neigh))
        Fs = [np.ascontiguousarray(f, np.float64).reshape(nc, nc, 9) for f in F21]
        ms = [np.asarray(m_, np.int32).reshape(-1, 2) for m_ in matches]
        mq = [np.ascontiguousarray(m_[:, 0]) for m_ in ms]
        mt = [np.ascontiguousarray(m_[:, 1]) for m_ in ms]
        nm = np.array([len(m_) for m_ in ms], np.int32)
        offsets = np.concatenate([[0], np.cumsum(nm)]).astype(np.int64)
        total = int(offsets[-1])
        cap_m, cap_d = caps if caps is not None else (total, total)
        Kc = np.ascontiguousarray(K_mats, np.float64).reshape(nc, 9)
        sig = np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1)
        Rc, tc = np.ascontiguousarray(Rcw, np.float64).reshape(9), np.ascontiguousarray(tcw, np.float64).reshape(3)
        frames = (_lib.MapFrame * max(S, 1))(*[f.struct for f in neigh])
        vpp = lambda arrs: (C.c_void_p * max(S, 1))(*[a.ctypes.data for a in arrs])
        o = self.map_out = _lib.MapOut()
        o.cap_matches, o.cap_depth = cap_m, cap_d
        r, cut = _map_outputs(o, cap_m, total, dict(dist2=np.float64, cos_parallax=np.float64), neigh_skipped=(np.uint8, S),
                              depth_vec=(np.float64, cap_d))
        _lib.check(self.L.mcorb_lmap_triangulate_neighbours(self.h, C.byref(cur.struct), lc.ctypes.data, frames, vpp(ln), S, vpp(Fs),
                                                            vpp(mq), vpp(mt), nm.ctypes.data, Kc.ctypes.data, sig.ctypes.data, len(sig),
                                                            Rc.ctypes.data, tc.ctypes.data, int(next_lid), C.byref(o)))
        return TriangulationResult(inliers=cut("inliers").astype(bool), verdict=cut("verdict"), new_lid=cut("new_lid"),
                                   pt3d=cut("pt3d").reshape(-1, 3), normal=cut("normal").reshape(-1, 3), dist2=cut("dist2"),
                                   cos_parallax=cut("cos_parallax"), neigh_skipped=r["neigh_skipped"][:S].copy(),
                                   depth_vec=r["depth_vec"][:o.n_depth].copy(), n_triangulated=o.n_triangulated, next_lid=o.next_lid,
                                   lids_cur=lc, lids_neigh=ln, offsets=offsets)

    def triangulate_new(self, cur, lids_cur, prev, lids_prev, matches, K_mats, inv_sigma2, next_lid, caps=None):
        """FrontEnd::TriangulateNewLandmarks (FrontEnd.cpp:6465-6700) -> NewLandmarksResult; the new landmarks' points, normals and
        ray counts are stored in their slots.  cur / prev: map_frame(...) of the current frame and of the previous keyframe;
        lids_cur / lids_prev: their lIds (copied: the result holds the updated arrays); matches: an n x 2 array (queryIdx into
        prev, trainIdx into cur); K_mats: per camera (the skew is not read); inv_sigma2: GetInverseScaleSigmaSquares(); caps:
        (matches, depth_vec) output sizes, by default what cannot be exceeded"""
        nc = cur.struct.ncams
        lc, lp = np.array(lids_cur, np.int32).reshape(-1), np.array(lids_prev, np.int32).reshape(-1)
        assert len(lc) == cur.struct.nfeat and len(lp) == prev.struct.nfeat
        self.map_new_lids = lc, lp   # (what the call reads and writes: a refused call leaves them as they came in)
        ms = np.asarray(matches, np.int32).reshape(-1, 2)
        mq, mt = np.ascontiguousarray(ms[:, 0]), np.ascontiguousarray(ms[:, 1])
        total = len(ms)
        cap_m, cap_d = caps if caps is not None else (total, total)
        Kc = np.ascontiguousarray(K_mats, np.float64).reshape(nc, 9)
        sig = np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1)
        o = self.map_new_out = _lib.MapNewOut()
        o.cap_matches, o.cap_depth = cap_m, cap_d
        r, cut = _map_outputs(o, cap_m, total, dict(dist=np.float64, cos_parallax=np.float32, iterations=np.int32, cost_initial=np.float64,
                                                    cost_final=np.float64), depth_vec=(np.float64, cap_d))
        _lib.check(self.L.mcorb_lmap_triangulate_new(self.h, C.byref(cur.struct), lc.ctypes.data, C.byref(prev.struct), lp.ctypes.data,
                                                     mq.ctypes.data, mt.ctypes.data, total, Kc.ctypes.data, sig.ctypes.data, len(sig),
                                                     int(next_lid), C.byref(o)))
        return NewLandmarksResult(inliers=cut("inliers").astype(bool), verdict=cut("verdict"), new_lid=cut("new_lid"),
                                  pt3d=cut("pt3d").reshape(-1, 3), normal=cut("normal").reshape(-1, 3), dist=cut("dist"),
                                  cos_parallax=cut("cos_parallax"), iterations=cut("iterations"), cost_initial=cut("cost_initial"),
                                  cost_final=cut("cost_final"), depth_vec=r["depth_vec"][:o.n_depth].copy(), avg_depth=o.avg_depth,
                                  n_rays_hist=np.array(o.n_rays_hist[:], np.int32), n_by_verdict=np.array(o.n_by_verdict[:], np.int32),
                                  n_triangulated=o.n_triangulated, next_lid=o.next_lid, lids_cur=lc, lids_prev=lp)

    def initialize(self, prev, lids_prev, cur, lids_cur, R, t, cam_centre_body, matches, inliers, K_mats, inv_sigma2, next_lid,
                   min_baseline, cap=None):
        """FrontEnd::initialization from the pose between the first two rig frames to the first landmarks (FrontEnd.cpp:2633-2839)
        -> InitResult; with status INIT_DONE the landmarks' points, normals and ray counts are stored in their slots.  prev / cur:
        map_frame(...) of lf_prev (proj = prev_T_ref * lf_prev->pose.inv(), its centre_w) and of the current frame (proj =
        cur_T_ref * T.inv(); its centre_w and both twc are not read); lids_prev / lids_cur: their lIds (copied: the result holds
        the updated arrays); R, t: T; cam_centre_body: per camera the translation column of cur_T_ref.inv(); matches: an n x 2
        array (queryIdx into prev, trainIdx into cur), inter_matches then mono_matches; inliers: the estimator's flags in that
        order; min_baseline: kf_translation_threshold * 0.5; cap: the per-match output size, by default n.  The ids are refused
        (E_CAP, before anything runs) when next_lid + the number of flags set on entry exceeds max_landmarks: the most ids the
        call can give out, not the number it does give out"""
        nc = cur.struct.ncams
        lp, lc = np.array(lids_prev, np.int32).reshape(-1), np.array(lids_cur, np.int32).reshape(-1)
        assert len(lc) == cur.struct.nfeat and len(lp) == prev.struct.nfeat
        self.init_lids = lp, lc   # (what the call reads and writes: a refused call leaves them as they came in)
        ms = np.asarray(matches, np.int32).reshape(-1, 2)
        mq, mt = np.ascontiguousarray(ms[:, 0]), np.ascontiguousarray(ms[:, 1])
        total = len(ms)
        cap = total if cap is None else cap
        Kc = np.ascontiguousarray(K_mats, np.float64).reshape(nc, 9)
        sig = np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1)
        Rr, tt = np.ascontiguousarray(R, np.float64).reshape(9), np.ascontiguousarray(t, np.float64).reshape(3)
        cb = np.ascontiguousarray(cam_centre_body, np.float64).reshape(nc, 3)
        o = self.init_out = _lib.InitResultC()
        o.cap_matches = cap
        r, cut = _map_outputs(o, max(cap, total), total, dict(dist2=np.float64, cos_parallax=np.float64))
        fl = np.asarray(inliers).reshape(-1) != 0
        assert len(fl) == total
        r["inliers"][:total] = fl
        r["new_lid"][:] = -1
        _lib.check(self.L.mcorb_lmap_initialize(self.h, C.byref(prev.struct), lp.ctypes.data, C.byref(cur.struct), lc.ctypes.data,
                                                Rr.ctypes.data, tt.ctypes.data, cb.ctypes.data, mq.ctypes.data, mt.ctypes.data, total,
                                                Kc.ctypes.data, sig.ctypes.data, len(sig), int(next_lid), float(min_baseline), C.byref(o)))
        return InitResult(inliers=cut("inliers").astype(bool), verdict=cut("verdict"), new_lid=cut("new_lid"),
                          pt3d=cut("pt3d").reshape(-1, 3), normal=cut("normal").reshape(-1, 3), dist2=cut("dist2"),
                          cos_parallax=cut("cos_parallax"), lids_prev=lp, lids_cur=lc, **_init_scalars(o))

    def last_initialize_timing(self):
        """(microseconds of the last k_init_triangulate launches, of k_init_select, of k_init_put, matches launched); a device store"""
        us = (C.c_float * 3)()
        n = C.c_int()
        _lib.check(self.L.mcorb_lmap_last_initialize_timing(self.h, us, C.byref(n)))
        return us[0], us[1], us[2], n.value

    def last_triangulate_new_timing(self):
        """(microseconds of the last k_map_refine_new launches, matches launched); a device store"""
        us = (C.c_float * 1)()
        n = C.c_int()
        _lib.check(self.L.mcorb_lmap_last_triangulate_new_timing(self.h, us, C.byref(n)))
        return us[0], n.value

    def depths(self, Rcw, tcw, lids):
        """getSceneDepthStats' depthVec before its sort: z of Rcw * pt3D + tcw for the landmarks `lids`"""
        Rc, tc = np.ascontiguousarray(Rcw, np.float64).reshape(9), np.ascontiguousarray(tcw, np.float64).reshape(3)
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        z = np.zeros(max(len(lids), 1))
        _lib.check(self.L.mcorb_lmap_depths(self.h, Rc.ctypes.data, tc.ctypes.data, lids.ctypes.data, len(lids), z.ctypes.data))
        return z[:len(lids)]

    def last_triangulate_timing(self):
        """(microseconds of the last k_map_triangulate launches, of the last k_map_depth launch, matches launched, depths taken)"""
        us = (C.c_float * 2)()
        n, nd = C.c_int(), C.c_int()
        _lib.check(self.L.mcorb_lmap_last_triangulate_timing(self.h, us, C.byref(n), C.byref(nd)))
        return us[0], us[1], n.value, nd.value

    def set_rays(self, lids, n_rays):
        """n_rays of slots that are set (a caller that loads an existing map)"""
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        r = np.ascontiguousarray(n_rays, np.int32).reshape(-1)
        assert len(lids) == len(r)
        _lib.check(self.L.mcorb_lmap_set_rays(self.h, lids.ctypes.data, len(lids), r.ctypes.data))

    def observations(self, lid):
        """-> (n_rays, [(kf_id, feat), ..]) of a slot: the reference's KFs / featInds in the order they were added"""
        nr, n = C.c_int32(), C.c_int()
        code = self.L.mcorb_lmap_get_observations(self.h, lid, C.byref(nr), None, None, 0, C.byref(n))
        if code not in (_lib.OK, _lib.E_CAP):
            _lib.check(code)
        kfs, feats = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1), np.int32)
        _lib.check(self.L.mcorb_lmap_get_observations(self.h, lid, C.byref(nr), kfs.ctypes.data, feats.ctypes.data, n.value, C.byref(n)))
        return nr.value, list(zip(kfs[:n.value].tolist(), feats[:n.value].tolist()))

    def observe(self, frame, lids, feats, mode=_lib.OBS_UPDATE, db=None, entry=-1, mono=None):
        """a batch of Landmark::addLfFrame for one keyframe (GlobalMap.cpp:24-74) -> n_rays of every item's slot after it.
        frame: obs_frame(...); landmark lids[i] is seen as LF feature feats[i]; mode OBS_UPDATE (normal and n_rays change) or
        OBS_RECORD (the observation alone, for landmarks fresh from triangulate_neighbours); db / entry: the keyframe's database
        entry, whose rows become the slots' descriptors; mono: the slots' new mono flags"""
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        feats = np.ascontiguousarray(feats, np.int32).reshape(-1)
        assert len(lids) == len(feats)
        m, mp = self._opt(None if mono is None else np.asarray(mono) != 0, np.uint8, (len(lids),))
        out = np.zeros(max(len(lids), 1), np.int32)
        _lib.check(self.L.mcorb_lmap_observe(self.h, C.byref(frame.struct), lids.ctypes.data, feats.ctypes.data, len(lids), mode,
                                             db.h if db is not None else None, entry, mp, out.ctypes.data))
        return out[:len(lids)]

    def update_points(self, lids, pt_new, max_diff=5.0):
        """a batch of GlobalMap::updateLandmark (GlobalMap.cpp:162-185) -> (updated, diff_norm): a point is replaced iff
        norm(pt3D - pt_new) < max_diff"""
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        n = len(lids)
        p = np.ascontiguousarray(pt_new, np.float64).reshape(n, 3)
        upd, diff = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1))
        _lib.check(self.L.mcorb_lmap_update_points(self.h, lids.ctypes.data, n, p.ctypes.data, float(max_diff), upd.ctypes.data,
                                                   diff.ctypes.data))
        return upd[:n].astype(bool), diff[:n]

    def delete(self, lids, cap=None):
        """a batch of GlobalMap::deleteLandmark (GlobalMap.cpp:151-160) -> the dropped (kf_id, feat) pairs, in lids order and then
        observation order: the lIds entries to set to -1"""
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        n = self.delete_count = C.c_int()
        if cap is None:     # a first call without room returns the count and deletes nothing (or finds nothing to return)
            code = self.L.mcorb_lmap_delete(self.h, lids.ctypes.data, len(lids), None, None, 0, C.byref(n))
            if code == _lib.OK:
                return []
            if code != _lib.E_CAP:
                _lib.check(code)
            cap = n.value
        kfs, feats = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        _lib.check(self.L.mcorb_lmap_delete(self.h, lids.ctypes.data, len(lids), kfs.ctypes.data, feats.ctypes.data, cap, C.byref(n)))
        return list(zip(kfs[:n.value].tolist(), feats[:n.value].tolist()))

    def observers(self, lids, cap=None):
        """kfMap's keys (FrontEnd.cpp:4925-4933): the ascending, duplicate-free kf_ids that observe the landmarks `lids`"""
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        n = self.observers_count = C.c_int()
        if cap is None:
            code = self.L.mcorb_lmap_observers(self.h, lids.ctypes.data, len(lids), None, 0, C.byref(n))
            if code not in (_lib.OK, _lib.E_CAP):
                _lib.check(code)
            cap = n.value
        out = np.zeros(max(cap, 1), np.int32)
        _lib.check(self.L.mcorb_lmap_observers(self.h, lids.ctypes.data, len(lids), out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].copy()

    def last_landmark_timing(self):
        """(microseconds of the last k_lmap_observe rounds, of the last k_lmap_update rounds); a device store"""
        us = (C.c_float * 2)()
        _lib.check(self.L.mcorb_lmap_last_landmark_timing(self.h, us))
        return us[0], us[1]

    def track(self, view, kps, descs, lids, max_d2=10000.0, max_hamming=20, caps=None):
        """one frame of fast tracking (FrontEnd::startTrackingModule between the map-entry query and refinePose): Tracking::project_
        of the landmarks `lids` (the nearest map entries' l_ids back to back; -1 and repeats are skipped) into every camera of
        view = track_view(...), and Tracking::queryCurrentFrame against the frame -> TrackResult.  kps: per camera the keypoints
        (image_kps: an n x 2 float array, or keypoint records with x and y); descs: per camera n x 32 bytes; caps: (projected,
        matches) output sizes per camera, by default what cannot be exceeded; a McorbError of this call carries n_candidates,
        n_proj and n_match as the call left them"""
        f, arrays = self._track_frame(kps, descs)     # (arrays: what f points into, alive across the call)
        return self._track(f.ncams, lids, caps, lambda lids, o: self.L.mcorb_lmap_track(
            self.h, C.byref(view), C.byref(f), lids.ctypes.data, len(lids), float(max_d2), int(max_hamming), C.byref(o)))

    @staticmethod
    def _track_frame(kps, descs):
        """-> (the mcorb_track_frame of track's kps / descs, the arrays it points into)"""
        ncams = len(kps)
        if not 1 <= ncams <= _lib.MAX_CAMS or len(descs) != ncams:
            raise ValueError("track: 1 .. %d cameras, one keypoint and one descriptor array each" % _lib.MAX_CAMS)
        xy = []
        for k in kps:
            k = np.asarray(k)
            xy.append(np.ascontiguousarray(np.stack([k["x"], k["y"]], axis=1) if k.dtype.names else k, np.float32).reshape(-1, 2))
        ds = [_u8(d).reshape(-1, 32) for d in descs]
        if any(len(a) != len(d) for a, d in zip(xy, ds)):
            raise ValueError("track: a camera has another number of descriptors than keypoints")
        f = _lib.TrackFrame()
        f.ncams = ncams
        for c in range(ncams):
            f.n_kp[c], f.kp_xy[c], f.desc[c] = len(xy[c]), xy[c].ctypes.data, ds[c].ctypes.data
        return f, (xy, ds)

    def track_rig_frame(self, view, rig, frame, lids, slot=0, max_d2=10000.0, max_hamming=20, caps=None):
        """track() on frame `frame` of the last extraction job of a rig slot, read where the job left it: camera c is image
        frame * ncams + c, its keypoints image_kps (Rig.features, not the undistorted set) and its descriptors.  On a device store
        the frame does not cross PCIe.  The result and a McorbError's counts are track()'s, bit for bit what track() gives on the
        arrays Rig.features returns.  No job may be submitted on the slot during the call"""
        return self._track(view.ncams, lids, caps, lambda lids, o: self.L.mcorb_lmap_track_rig_frame(
            self.h, C.byref(view), rig.h_rig if rig is not None else None, slot, frame, lids.ctypes.data, len(lids), float(max_d2),
            int(max_hamming), C.byref(o)))

    def _track(self, ncams, lids, caps, call):
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        return self._track_one(ncams, len(lids), caps, True, lambda o, n: call(lids, o[0]))

    def _track_one(self, ncams, n_lids, caps, want_pts, call):
        """_track_outs for the single entries: the one frame's TrackResult, a McorbError's counts as those of that frame"""
        try:
            return self._track_outs(ncams, [n_lids], caps, want_pts, call)[0]
        except McorbError as e:
            if hasattr(e, "n_candidates"):
                e.n_candidates, e.n_proj, e.n_match = e.n_candidates[0], e.n_proj[0], e.n_match[0]
            raise

    def track_submit(self, view, kps, descs, lids, max_d2=10000.0, max_hamming=20, want_pts=True):
        """track() up to and excluding the wait for the device: every refusal, the candidate walk, the copy up and every launch; then
        it returns and track_wait() gives the result.  kps, descs, lids and view may be changed at once.  A host-only store runs
        the whole call here and keeps the result.  Until track_wait() every other call on the store raises MCORB_E_STATE (the
        last_*timing* calls and close() excepted); a refused submission leaves nothing pending.  want_pts=False: no match_pt"""
        f, arrays = self._track_frame(kps, descs)     # (arrays: what f points into, alive across the call)
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        _lib.check(self.L.mcorb_lmap_track_submit(self.h, C.byref(view), C.byref(f), lids.ctypes.data, len(lids), float(max_d2),
                                                  int(max_hamming), int(bool(want_pts))))
        self._submitted = (f.ncams, len(lids), bool(want_pts))

    def track_rig_frame_submit(self, view, rig, frame, lids, slot=0, max_d2=10000.0, max_hamming=20, want_pts=True):
        """track_rig_frame() as track_submit() is track(): no job may be submitted on the slot until track_wait() has returned"""
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        _lib.check(self.L.mcorb_lmap_track_rig_frame_submit(self.h, C.byref(view), rig.h_rig if rig is not None else None, slot, frame,
                                                            lids.ctypes.data, len(lids), float(max_d2), int(max_hamming),
                                                            int(bool(want_pts))))
        self._submitted = (view.ncams, len(lids), bool(want_pts))

    def track_wait(self, caps=None):
        """the TrackResult of the submitted call (match_pt None after want_pts=False); a McorbError carries the counts as track()'s
        does.  Whatever happens, nothing is pending afterwards; without a submitted call: MCORB_E_STATE"""
        ncams, n_lids, want_pts = getattr(self, "_submitted", None) or (1, 0, False)
        self._submitted = None
        n_lids = max(n_lids) if isinstance(n_lids, list) else n_lids     # (a pending batch: the call fails, MCORB_E_STATE)
        return self._track_one(ncams, n_lids, caps, want_pts, lambda o, n: self.L.mcorb_lmap_track_wait(self.h, o))

    def track_rig_frames(self, views, rig, frames, lids, slot=0, max_d2=10000.0, max_hamming=20, caps=None):
        """track_rig_frame() for len(frames) <= TRACK_MAX_FRAMES frames of the slot's last extraction job in one submission and one
        wait: frame frames[f] (any order, repeats allowed) from views[f] with the ids lids[f] -> a list of TrackResult, each bit
        for bit what track_rig_frame(views[f], rig, frames[f], lids[f]) returns.  caps: one (projected, matches) pair for every
        frame, by default what a frame cannot exceed.  A McorbError carries n_candidates, n_proj and n_match as lists with one
        entry per frame"""
        va, fa, la, first = self._track_batch(views, frames, lids)
        return self._track_outs(va[0].ncams, [len(l) for l in lids], caps, True,
                                lambda o, n: self.L.mcorb_lmap_track_rig_frames(
                                    self.h, va, rig.h_rig if rig is not None else None, slot, fa.ctypes.data, len(fa), la.ctypes.data,
                                    first.ctypes.data, float(max_d2), int(max_hamming), 1, o))

    def track_rig_frames_submit(self, views, rig, frames, lids, slot=0, max_d2=10000.0, max_hamming=20, want_pts=True):
        """track_rig_frames() as track_rig_frame_submit() is track_rig_frame(): one pending call of len(frames) frames, which
        track_frames_wait() serves; views, frames and lids may be changed at once"""
        va, fa, la, first = self._track_batch(views, frames, lids)
        _lib.check(self.L.mcorb_lmap_track_rig_frames_submit(self.h, va, rig.h_rig if rig is not None else None, slot, fa.ctypes.data,
                                                             len(fa), la.ctypes.data, first.ctypes.data, float(max_d2), int(max_hamming),
                                                             int(bool(want_pts))))
        self._submitted = (va[0].ncams, [len(l) for l in lids], bool(want_pts))

    def track_frames_wait(self, caps=None):
        """the TrackResults of the pending call, one per frame: a list of one after track_submit() / track_rig_frame_submit().  A
        McorbError carries the counts per frame.  Whatever happens, nothing is pending afterwards; without a submitted call:
        MCORB_E_STATE"""
        ncams, n_lids, want_pts = getattr(self, "_submitted", None) or (1, [0], False)
        self._submitted = None
        n_lids = n_lids if isinstance(n_lids, list) else [n_lids]
        return self._track_outs(ncams, n_lids, caps, want_pts, lambda o, n: self.L.mcorb_lmap_track_frames_wait(self.h, o, n))

    @staticmethod
    def _track_batch(views, frames, lids):
        """-> (the views as one array, frames and the concatenated ids as int32 arrays, lid_first)"""
        if not len(views) == len(frames) == len(lids):
            raise ValueError("track_rig_frames: one view and one id sequence per frame")
        va = (_lib.TrackView * max(len(views), 1))()
        for f, v in enumerate(views):
            C.memmove(C.addressof(va[f]), C.addressof(v), C.sizeof(_lib.TrackView))
        ls = [np.ascontiguousarray(l, np.int32).reshape(-1) for l in lids]
        first = np.zeros(len(ls) + 1, np.int32)
        first[1:] = np.cumsum([len(l) for l in ls])
        la = np.concatenate(ls + [np.zeros(1, np.int32)])       # (never empty: its address is passed)
        return va, np.ascontiguousarray(frames, np.int32).reshape(-1), la, first

    def _track_outs(self, ncams, n_lids, caps, want_pts, call):
        """the output arrays of a tracking call of len(n_lids) frames, call(array of mcorb_track_out, its length) -> code, and the
        TrackResult per frame (or the McorbError with the call's counts per frame)"""
        nf = len(n_lids)
        os_ = (_lib.TrackOut * max(nf, 1))()
        arrays = []
        for f in range(nf):
            cap_p, cap_m = caps if caps is not None else (n_lids[f], n_lids[f])
            n1, n2 = ncams * max(cap_p, 1), ncams * max(cap_m, 1)
            r = dict(proj_lid=np.zeros(n1, np.int32), proj_xy=np.zeros((n1, 2), np.float32), best_kp=np.zeros(n1, np.int32),
                     best_dist=np.zeros(n1, np.int32), match_kp=np.zeros(n2, np.int32), match_lid=np.zeros(n2, np.int32),
                     match_dist=np.zeros(n2, np.int32))
            if want_pts:
                r["match_pt"] = np.zeros((n2, 3))
            os_[f].cap_proj, os_[f].cap_match = cap_p, cap_m
            for k, a in r.items():
                setattr(os_[f], k, a.ctypes.data)
            arrays.append((r, cap_p, cap_m))
        code = call(os_, nf)
        n_proj, n_match = [list(os_[f].n_proj[:ncams]) for f in range(nf)], [list(os_[f].n_match[:ncams]) for f in range(nf)]
        if code != _lib.OK:
            try:
                _lib.check(code)
            except McorbError as e:     # MCORB_E_CAP for a short output comes with every count of every frame set
                e.n_candidates, e.n_proj, e.n_match = [os_[f].n_candidates for f in range(nf)], n_proj, n_match
                e.outputs = [r for r, _, _ in arrays]     # (the output arrays as the call left them: unwritten)
                raise
        res = []
        for f, (r, cap_p, cap_m) in enumerate(arrays):
            out = {k: [r[k][c * cap_p:c * cap_p + n_proj[f][c]].copy() for c in range(ncams)] for k in ("proj_lid", "proj_xy", "best_kp", "best_dist")}
            out.update({k: [r[k][c * cap_m:c * cap_m + n_match[f][c]].copy() for c in range(ncams)] if k in r else None
                        for k in ("match_kp", "match_lid", "match_dist", "match_pt")})
            res.append(TrackResult(n_candidates=os_[f].n_candidates, **out))
        return res

    def last_track_timing(self):
        """(microseconds of the last k_track_project launch, of the last k_track_match launch); a device store"""
        us = (C.c_float * 2)()
        _lib.check(self.L.mcorb_lmap_last_track_timing(self.h, us))
        return us[0], us[1]

    def last_track_timing4(self):
        """(microseconds of the last k_track_points, k_track_project, k_track_match and k_track_compact launch); k_track_points is
        0 after track(), which does not run it; a device store"""
        us = (C.c_float * 4)()
        _lib.check(self.L.mcorb_lmap_last_track_timing4(self.h, us))
        return us[0], us[1], us[2], us[3]

    def last_track_timing5(self):
        """last_track_timing4() and, last, the microseconds of the de-duplication: the clear of its table, k_track_dedup_min,
        k_track_dedup_win and k_track_dedup_emit; a device store"""
        us = (C.c_float * 5)()
        _lib.check(self.L.mcorb_lmap_last_track_timing5(self.h, us))
        return tuple(us)


    # the rig pose from 2D-3D matches (mcorb_lmap_refine_pose): OptimizePose's cost and cull around a stated Levenberg-Marquardt
    def refine_pose(self, cams, R, t, cam, uv, octave, inv_sigma2, lids=None, pts=None, max_iterations=25):
        """the pose w_T_b = (R, t) of a rig refined from observations: observation i is the keypoint uv[i] (KeyPoint::pt) of
        pyramid level octave[i] in camera cam[i] of the store's landmark lids[i] or of the point pts[i] (exactly one of the
        two).  cams: pose_cams(...) or a track_view (its cameras are the rig); inv_sigma2: GetInverseScaleSigmaSquares(), one
        per level.  Two rounds from (R, t), each followed by the chi2 > 5.991 cull -> PoseResult.  A device store runs one launch
        of k_pose_refine; a host-only store the same arithmetic serially, with the same bits"""
        cam = np.ascontiguousarray(cam, np.int32).reshape(-1)
        n = len(cam)
        uv = np.ascontiguousarray(uv, np.float32).reshape(n, 2)
        octave = np.ascontiguousarray(octave, np.int32).reshape(n)
        l, lp = self._opt(lids, np.int32, (n,))
        p, pp = self._opt(pts, np.float64, (n, 3))
        ncams, ca = _pose_cams(cams)
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        res, flags = _lib.PoseResultC(), np.zeros(max(n, 1), np.uint8)
        _lib.check(self.L.mcorb_lmap_refine_pose(self.h, n, cam.ctypes.data, uv.ctypes.data, octave.ctypes.data, lp, pp, ncams, ca,
                                                 R.ctypes.data, t.ctypes.data, C.byref(pose_params(inv_sigma2, max_iterations)),
                                                 C.byref(res), flags.ctypes.data))
        return PoseResult(res, flags[:n])

    def last_pose_timing(self):
        """microseconds of the last k_pose_refine launch of refine_pose(); a device store"""
        us = (C.c_float * 1)()
        _lib.check(self.L.mcorb_lmap_last_pose_timing(self.h, us))
        return us[0]

    # local bundle adjustment over rig keyframes and landmarks (mcorb_lmap_bundle_adjust)
    def bundle_adjust(self, cams, kf_R, kf_t, fixed, obs_kf, obs_cam, obs_lm, uv, octave, sigma, lids=None, pts=None, max_iterations=25):
        """a window of keyframes of one rig and landmarks adjusted together: keyframe k has the pose w_T_b = (kf_R[k], kf_t[k])
        and is held when fixed[k] (the fixed keyframes hold the gauge); landmark j's point is pts[j] or the store's point of
        lids[j] (exactly one of the two); observation i is the keypoint uv[i] of level octave[i] in camera obs_cam[i] of keyframe
        obs_kf[i], of landmark obs_lm[i] (an index into the call's landmark list).  cams: refine_pose's; sigma: per level what
        the back end hands Isotropic::Sigma.  The factor is the back end's projection factor with Huber at sqrt(5.991); the
        optimizer is refine_pose's Levenberg-Marquardt on the whole state, the landmarks eliminated by the Schur complement ->
        BAResult.  A device store runs a chain of kernels in one submission; a host-only store the same arithmetic serially, with
        the same bits.  The store is not written: apply update_points(lids, result.pts, ...)"""
        kf_R = np.ascontiguousarray(kf_R, np.float64)
        nkf = kf_R.size // 9
        kf_R = kf_R.reshape(nkf, 9)
        kf_t = np.ascontiguousarray(kf_t, np.float64).reshape(nkf, 3)
        fixed = np.ascontiguousarray(np.asarray(fixed).astype(bool), np.uint8).reshape(nkf)
        obs_kf = np.ascontiguousarray(obs_kf, np.int32).reshape(-1)
        n = len(obs_kf)
        obs_cam = np.ascontiguousarray(obs_cam, np.int32).reshape(n)
        obs_lm = np.ascontiguousarray(obs_lm, np.int32).reshape(n)
        uv = np.ascontiguousarray(uv, np.float32).reshape(n, 2)
        octave = np.ascontiguousarray(octave, np.int32).reshape(n)
        nlm = len(lids) if lids is not None else (np.asarray(pts).size // 3 if pts is not None else 0)
        l, lp = self._opt(lids, np.int32, (nlm,))
        p, pp = self._opt(pts, np.float64, (nlm, 3))
        ncams, ca = _pose_cams(cams)
        R_out, t_out, pts_out = np.zeros((nkf, 3, 3)), np.zeros((nkf, 3)), np.zeros((max(nlm, 1), 3))
        res, flags = _lib.BAResultC(), np.zeros(max(n, 1), np.uint8)
        _lib.check(self.L.mcorb_lmap_bundle_adjust(self.h, nkf, kf_R.ctypes.data, kf_t.ctypes.data, fixed.ctypes.data, ncams, ca, nlm, lp, pp,
                                                   n, obs_kf.ctypes.data, obs_cam.ctypes.data, obs_lm.ctypes.data, uv.ctypes.data,
                                                   octave.ctypes.data, C.byref(ba_params(sigma, max_iterations)), R_out.ctypes.data,
                                                   t_out.ctypes.data, pts_out.ctypes.data, C.byref(res), flags.ctypes.data))
        return BAResult(res, R_out, t_out, pts_out[:nlm], flags[:n])

    def last_ba_timing(self):
        """(us, launches_idle) of the last bundle_adjust() chain of a device store: us = microseconds of the copy-in with the first
        linearization, of k_ba_schur, k_ba_solve, k_ba_update and k_ba_accept of the first iteration, of all later iterations
        together and of the final pass; launches_idle: the launches that were queued behind the loop's end"""
        us, idle = (C.c_float * _lib.BA_SPANS)(), C.c_int32()
        _lib.check(self.L.mcorb_lmap_last_ba_timing(self.h, us, C.byref(idle)))
        return tuple(us), idle.value

    # re-triangulation after the back end moved keyframes (mcorb_lmap_retriangulate)
    def retriangulate(self, cams, kf_R, kf_t, moved, lids, obs_kf, obs_cam, obs_lm, uv, rank_tol=1.0, landmark_distance_threshold=-1.0,
                      dynamic_outlier_threshold=-1.0, max_diff=5.0, apply=False, cap=None):
        """the end of Backend::UpdateVariables_SmartFactors: every landmark of lids (store ids, duplicate-free) with an
        observation in a keyframe with moved[k] is triangulated again from all of its observations -- the arrays are
        bundle_adjust's, the poses those after the optimisation -- by the DLT on K [R | t] rows through a Gram matrix and Jacobi
        sweeps, then checked as triangulateSafe checks it (rank_tol; the two thresholds are off when <= 0) and put through
        updateLandmark's gate max_diff -> RetriResult.  apply=False leaves the store as it is; apply=True writes the
        VALID_UPDATED points and deletes the landmarks with a failed verdict, whose (kf_id, feat) pairs come back as delete()'s
        do (cap: room for them; None: asked for by a first call, as delete() does).  A device store runs two kernels in one
        submission; a host-only store the same arithmetic serially, with the same bits"""
        kf_R = np.ascontiguousarray(kf_R, np.float64)
        nkf = kf_R.size // 9
        kf_R = kf_R.reshape(nkf, 9)
        kf_t = np.ascontiguousarray(kf_t, np.float64).reshape(nkf, 3)
        moved = np.ascontiguousarray(np.asarray(moved).astype(bool), np.uint8).reshape(nkf)
        lids = np.ascontiguousarray(lids, np.int32).reshape(-1)
        nlm = len(lids)
        obs_kf = np.ascontiguousarray(obs_kf, np.int32).reshape(-1)
        n = len(obs_kf)
        obs_cam = np.ascontiguousarray(obs_cam, np.int32).reshape(n)
        obs_lm = np.ascontiguousarray(obs_lm, np.int32).reshape(n)
        uv = np.ascontiguousarray(uv, np.float32).reshape(n, 2)
        ncams, ca = _pose_cams(cams)
        par = _lib.RetriParams(float(rank_tol), float(landmark_distance_threshold), float(dynamic_outlier_threshold), float(max_diff),
                               RETRI_APPLY if apply else RETRI_REPORT, 0)
        pts, diff = np.zeros((max(nlm, 1), 3)), np.zeros(max(nlm, 1))
        nv, verdict = np.zeros(max(nlm, 1), np.int32), np.zeros(max(nlm, 1), np.int32)
        res = _lib.RetriResultC()

        def call(kfs, feats, room):
            return self.L.mcorb_lmap_retriangulate(self.h, nkf, kf_R.ctypes.data, kf_t.ctypes.data, moved.ctypes.data, ncams, ca, nlm,
                                                   lids.ctypes.data, n, obs_kf.ctypes.data, obs_cam.ctypes.data, obs_lm.ctypes.data,
                                                   uv.ctypes.data, C.byref(par), pts.ctypes.data, diff.ctypes.data, nv.ctypes.data,
                                                   verdict.ctypes.data, C.byref(res), kfs, feats, room)
        if cap is None:
            code = call(None, None, 0)
            if code != _lib.E_CAP or not apply:
                _lib.check(code)
                return RetriResult(res, pts[:nlm], diff[:nlm], nv[:nlm], verdict[:nlm], [])
            cap = res.n_pairs
        kfs, feats = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        _lib.check(call(kfs.ctypes.data, feats.ctypes.data, cap))
        k = res.n_pairs if apply else 0
        return RetriResult(res, pts[:nlm], diff[:nlm], nv[:nlm], verdict[:nlm], list(zip(kfs[:k].tolist(), feats[:k].tolist())))

    def last_retri_timing(self):
        """microseconds of k_retri_views and of k_retri_solve in the last retriangulate() of a device store that launched them"""
        us = (C.c_float * _lib.RETRI_SPANS)()
        _lib.check(self.L.mcorb_lmap_last_retri_timing(self.h, us))
        return tuple(us)

    # the absolute rig pose by RANSAC in front of the refinement (mcorb_lmap_ransac_pose)
    def ransac_pose(self, cams, cam, uv, octave, threshold, lids=None, pts=None, match=None, max_iterations=100, seed=0, refine=None,
                    solver="central"):
        """the pose w_T_b of a rig from observations without a predicted pose: the consensus step of
        FrontEnd::absolutePoseFromGP3P.  The observations and cams are refine_pose()'s; match: non-decreasing match indices (None:
        every observation its own match) -- the consensus set is the first observation of each match; threshold: on 1 - cos of
        the reprojection angle, sac_threshold(K[0](0, 2)) in the reference; max_iterations hypotheses, all examined; seed: of the
        draws.  refine: pose_params(...) -- the refinement over all observations from the RANSAC's pose and the reference's rule
        between the two.  solver: "central" -- a hypothesis's four samples come from one camera, which therefore needs four
        consensus observations of its own -- or "rig": the samples come from any cameras and a generalized solver works on the
        rig's rays (k_sac_hypotheses_rig), so matches spread thinly over many cameras still give a pose.  -> SacResult.  A device
        store runs k_sac_hypotheses, k_sac_score, k_sac_pick (and k_pose_refine) in one submission; a host-only store the same
        arithmetic serially, with the same bits"""
        cam = np.ascontiguousarray(cam, np.int32).reshape(-1)
        n = len(cam)
        uv = np.ascontiguousarray(uv, np.float32).reshape(n, 2)
        octave = np.ascontiguousarray(octave, np.int32).reshape(n)
        l, lp = self._opt(lids, np.int32, (n,))
        p, pp = self._opt(pts, np.float64, (n, 3))
        mt, mp = self._opt(match, np.int32, (n,))
        ncams, ca = _pose_cams(cams)
        par = _lib.SacParams()
        par.threshold, par.seed, par.max_iterations = float(threshold), int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_iterations)
        par.solver = SAC_SOLVERS[solver] if isinstance(solver, str) else int(solver)     # (a number goes through as it is, to be refused)
        res, flags = _lib.SacResultC(), np.zeros(max(n, 1), np.uint8)
        _lib.check(self.L.mcorb_lmap_ransac_pose(self.h, n, cam.ctypes.data, uv.ctypes.data, octave.ctypes.data, mp, lp, pp, ncams, ca,
                                                 C.byref(par), None if refine is None else C.byref(refine), C.byref(res),
                                                 flags.ctypes.data))
        return SacResult(res, flags[:res.n_matches], refine is not None)

    def last_ransac_timing(self):
        """((us of k_sac_hypotheses or k_sac_hypotheses_rig, k_sac_score, k_sac_pick), hypotheses) of the last ransac_pose() launch; a device store"""
        us, nh = (C.c_float * 3)(), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_ransac_timing(self.h, us, C.byref(nh)))
        return tuple(us), nh.value

    def last_ransac_counts(self):
        """test hook: (counts, has a model) of all hypotheses of the last ransac_pose() that ran any"""
        count, valid, nh = np.zeros(1024, np.int32), np.zeros(1024, np.int32), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_ransac_counts(self.h, count.ctypes.data, valid.ctypes.data, 1024, C.byref(nh)))
        return count[:nh.value], valid[:nh.value].astype(bool)

    # the relative rig pose between two frames by RANSAC on 2D-2D matches (mcorb_lmap_relative_pose)
    def relative_pose(self, cams, cam1, uv1, cam2, uv2, threshold, max_iterations=10000, seed=0):
        """the pose b1_T_b2 of a rig's second frame in its first from 2D-2D matches, without landmarks: the consensus step of
        FrontEnd::poseFromSeventeenPt and LoopCloser::checkEssentialMatrix.  Match i is the keypoint uv1[i] in camera cam1[i] of
        frame 1 and uv2[i] in camera cam2[i] of frame 2; cams: pose_cams(...) or a track_view; threshold: on the sum over both
        views of 1 - cos of the angle to the triangulated midpoint, rel_threshold(K[0](0, 2)) in the reference; max_iterations
        hypotheses of 17 matches each (1 .. REL_MAX_ITERATIONS), all examined; seed: of the draws.  -> RelResult.  A device store
        runs k_rel_hypotheses, k_rel_score and k_rel_pick in one submission; a host-only store the same arithmetic serially, with
        the same bits.  The store's landmarks are not touched"""
        return self._relative(cams, cam1, uv1, cam2, uv2, threshold, max_iterations, seed)

    def _relative(self, cams, cam1, uv1, cam2, uv2, threshold, max_iterations, seed, polish=None):
        """relative_pose, or with polish = (rounds, polish_iterations) relative_pose_polished: the arrays, the parameters, the call"""
        cam1 = np.ascontiguousarray(cam1, np.int32).reshape(-1)
        n = len(cam1)
        cam2 = np.ascontiguousarray(cam2, np.int32).reshape(n)
        uv1 = np.ascontiguousarray(uv1, np.float32).reshape(n, 2)
        uv2 = np.ascontiguousarray(uv2, np.float32).reshape(n, 2)
        ncams, ca = _pose_cams(cams)
        par = _lib.RelParams()
        par.threshold, par.seed, par.max_iterations = float(threshold), int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_iterations)
        res, flags = _lib.RelResultC(), np.zeros(max(n, 1), np.uint8)
        matches = (self.h, n, cam1.ctypes.data, uv1.ctypes.data, cam2.ctypes.data, uv2.ctypes.data, ncams, ca, C.byref(par))
        if polish is None:
            _lib.check(self.L.mcorb_lmap_relative_pose(*matches, C.byref(res), flags.ctypes.data))
            return RelResult(res, flags[:n])
        pp, rec = _lib.RelPolishParams(int(polish[0]), int(polish[1])), _lib.RelPolishC()
        _lib.check(self.L.mcorb_lmap_relative_pose_polished(*matches, C.byref(pp), C.byref(res), flags.ctypes.data, C.byref(rec)))
        return RelResult(res, flags[:n]), RelPolish(rec)

    def last_relative_timing(self):
        """((us of k_rel_hypotheses, k_rel_score, k_rel_pick), hypotheses) of the last relative_pose() launch; a device store"""
        us, nh = (C.c_float * 3)(), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_relative_timing(self.h, us, C.byref(nh)))
        return tuple(us), nh.value

    def relative_pose_polished(self, cams, cam1, uv1, cam2, uv2, threshold, max_iterations=10000, seed=0, rounds=2, polish_iterations=10):
        """relative_pose followed by the polish of the winner over its inliers: `rounds` (1 .. 2) rounds of refine_pose's
        Levenberg-Marquardt, at most polish_iterations (1 .. 100) solves each, on the residual (a - P1 / |P1|, b / |b| - P2 / |P2|)
        / sqrt(threshold) of the members; after a round all matches are scored at its result, which replaces the current pose,
        flags and count iff its count is at least the current one.  -> (RelResult, RelPolish): the result's R, t, n_inliers and
        inliers are the accepted pose's, best_hypothesis, sample and n_models the winner's.  A device store adds k_rel_fit to
        the submission; a host-only store gives the same bits"""
        return self._relative(cams, cam1, uv1, cam2, uv2, threshold, max_iterations, seed, (rounds, polish_iterations))

    def last_relative_timing4(self):
        """((us of k_rel_hypotheses, k_rel_score, k_rel_pick of the last relative call, k_rel_fit of the last polished one),
        hypotheses); a device store"""
        us, nh = (C.c_float * 4)(), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_relative_timing4(self.h, us, C.byref(nh)))
        return tuple(us), nh.value

    def last_relative_counts(self):
        """test hook: (counts, has a model) of all hypotheses of the last relative_pose() that ran any"""
        count, valid, nh = np.zeros(REL_MAX_ITERATIONS, np.int32), np.zeros(REL_MAX_ITERATIONS, np.int32), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_relative_counts(self.h, count.ctypes.data, valid.ctypes.data, REL_MAX_ITERATIONS, C.byref(nh)))
        return count[:nh.value], valid[:nh.value].astype(bool)

    # the pose of one camera between two frames by five-point RANSAC (mcorb_lmap_essential_pose)
    def essential_pose(self, cam, uv1, uv2, threshold_px=1.0, distance_thresh=50.0, max_iterations=1000, seed=0):
        """the pose c1_T_c2 of one camera's second frame in its first from 2D-2D matches, |t| = 1, without landmarks: what the
        reference takes from cv::findEssentialMat(..., RANSAC, prob, thr, mask) and cv::recoverPose in the one-camera arm of its
        bootstrap.  Match i is the keypoint uv1[i] of frame 1 and uv2[i] of frame 2; cam: pose_cams(...) or a track_view, whose
        camera 0's calibration is read; threshold_px: on the Sampson distance, in pixels (the reference's 1.0 or 0.5);
        distance_thresh: recoverPose's; max_iterations hypotheses of 5 matches each (1 .. ESS_MAX_ITERATIONS), all examined, up to
        10 models each; seed: of the draws.  -> EssentialResult, whose (R, t) and inliers LocalMap.initialize takes for a rig of
        one camera.  A device store runs k_ess_hypotheses, k_ess_score, k_ess_pick and k_ess_finish in one submission; a host-only
        store the same arithmetic serially, with the same bits.  The store's landmarks are not touched"""
        return self._essential(cam, uv1, uv2, threshold_px, distance_thresh, max_iterations, seed)

    def _essential(self, cam, uv1, uv2, threshold_px, distance_thresh, max_iterations, seed, polish=None):
        """essential_pose, or with polish = (rounds, polish_iterations) essential_pose_polished: the arrays, the parameters, the call"""
        uv1 = np.ascontiguousarray(uv1, np.float32).reshape(-1, 2)
        n = len(uv1)
        uv2 = np.ascontiguousarray(uv2, np.float32).reshape(n, 2)
        par = _lib.EssParams()
        par.threshold_px, par.distance_thresh = float(threshold_px), float(distance_thresh)
        par.seed, par.max_iterations = int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_iterations)
        res, flags = _lib.EssResultC(), np.zeros(max(n, 1), np.uint8)
        matches = (self.h, n, uv1.ctypes.data, uv2.ctypes.data, _pose_cams(cam)[1], C.byref(par))
        if polish is None:
            _lib.check(self.L.mcorb_lmap_essential_pose(*matches, C.byref(res), flags.ctypes.data))
            return EssentialResult(res, flags[:n])
        pp, rec = _lib.EssPolishParams(int(polish[0]), int(polish[1])), _lib.EssPolishC()
        _lib.check(self.L.mcorb_lmap_essential_pose_polished(*matches, C.byref(pp), C.byref(res), flags.ctypes.data, C.byref(rec)))
        return EssentialResult(res, flags[:n]), EssentialPolish(rec)

    def last_essential_timing(self):
        """((us of k_ess_hypotheses, k_ess_score, k_ess_pick, k_ess_finish), hypotheses) of the last essential_pose() launch; a
        device store"""
        us, nh = (C.c_float * 4)(), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_essential_timing(self.h, us, C.byref(nh)))
        return tuple(us), nh.value

    def essential_pose_polished(self, cam, uv1, uv2, threshold_px=1.0, distance_thresh=50.0, max_iterations=1000, seed=0, rounds=2,
                                polish_iterations=10):
        """essential_pose followed by the polish of the winner over its inliers: `rounds` (1 .. 2) rounds of refine_pose's
        Levenberg-Marquardt on five unknowns (a rotation and a move of t on the unit sphere), at most polish_iterations (1 .. 100)
        solves each, on the Sampson residual r / sqrt(a0 a0 + a1 a1 + b0 b0 + b1 b1) / thr of the members at E = [t]x R; after a round
        all matches are tested at its result (the threshold and the depth test), which replaces the current pose, E, flags and
        counts iff its n_inliers is at least the current one.  -> (EssentialResult, EssentialPolish): the result's R, t, E,
        n_ransac_inliers, n_inliers and inliers are the accepted pose's; cheirality, best_hypothesis, best_root, sample and n_models
        the winner's.  A device store adds k_ess_fit to the submission; a host-only store gives the same bits"""
        return self._essential(cam, uv1, uv2, threshold_px, distance_thresh, max_iterations, seed, (rounds, polish_iterations))

    def last_essential_timing5(self):
        """((us of k_ess_hypotheses, k_ess_score, k_ess_pick, k_ess_finish of the last essential call, k_ess_fit of the last polished
        one), hypotheses); a device store"""
        us, nh = (C.c_float * 5)(), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_essential_timing5(self.h, us, C.byref(nh)))
        return tuple(us), nh.value

    def last_essential_counts(self):
        """test hook: (counts, has a model, E 9 doubles) of all (hypothesis, root) slots of the last essential_pose() that ran
        any; slot 10 h + c is root c of hypothesis h"""
        ns = C.c_int(0)
        code = self.L.mcorb_lmap_last_essential_counts(self.h, None, None, None, 0, C.byref(ns))
        if code != E_CAP:
            _lib.check(code)
        cap = max(ns.value, 1)
        count, valid, models = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 9))
        _lib.check(self.L.mcorb_lmap_last_essential_counts(self.h, count.ctypes.data, valid.ctypes.data, models.ctypes.data, cap, C.byref(ns)))
        return count[:ns.value], valid[:ns.value].astype(bool), models[:ns.value]

    # the rig pose between two frames from 3D-3D pairs (mcorb_lmap_align_pose)
    def align_pose(self, pts2, pts1=None, lids1=None, mode="sac", threshold=0.2, inlier_dist=0.1, max_iterations=100, seed=0, refit=True):
        """the pose b1_T_b2 of a rig's second frame in its first from pairs of triangulated points: FrontEnd::poseFromPCAlignment,
        the PC_ALIGN estimator.  Pair i is pts2[i] of frame 2 and pts1[i] of frame 1, or the point of the store's landmark
        lids1[i] (exactly one of the two).  mode "all": the least-squares fit over all pairs (the reference's live code); "sac":
        max_iterations hypotheses of 3 pairs each (1 .. ALIGN_MAX_ITERATIONS), all examined, counted at `threshold` on |p1 - (R p2
        + t)|, and with refit the least-squares fit over the winner's inliers (the reference's commented code takes the winner:
        refit=False).  inlier_dist: the reference's verdict with the answer.  The defaults are the reference's values.  ->
        AlignResult.  A device store runs k_align_hypotheses, k_align_score, k_align_pick and k_align_fit ("all": k_align_fit
        alone) in one submission; a host-only store the same arithmetic serially, with the same bits.  The store's landmarks
        are not written"""
        pts2 = np.ascontiguousarray(pts2, np.float64).reshape(-1, 3)
        n = len(pts2)
        # (no pairs: one row of zeros each, so that "exactly one of pts1 and lids1" is still said by a pointer that is not NULL)
        pts2 = pts2 if n else np.zeros((1, 3))
        l, lp = self._opt(lids1 if n or lids1 is None else np.zeros(1, np.int32), np.int32, (max(n, 1),))
        p, pp = self._opt(pts1 if n or pts1 is None else np.zeros((1, 3)), np.float64, (max(n, 1), 3))
        par = _lib.AlignParams()
        par.threshold, par.inlier_dist, par.seed = float(threshold), float(inlier_dist), int(seed) & 0xFFFFFFFFFFFFFFFF
        par.max_iterations, par.refit = int(max_iterations), int(bool(refit))
        par.mode = ALIGN_MODES[mode] if isinstance(mode, str) else int(mode)     # (a number goes through as it is, to be refused)
        res, flags = _lib.AlignResultC(), np.zeros(max(n, 1), np.uint8)
        _lib.check(self.L.mcorb_lmap_align_pose(self.h, n, lp, pp, pts2.ctypes.data, C.byref(par), C.byref(res), flags.ctypes.data))
        return AlignResult(res, flags[:n])

    def last_align_timing(self):
        """((us of k_align_hypotheses, k_align_score, k_align_pick, k_align_fit), hypotheses) of the last align_pose() launches;
        mode "all" sets the last of the four only; a device store"""
        us, nh = (C.c_float * 4)(), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_align_timing(self.h, us, C.byref(nh)))
        return tuple(us), nh.value

    def last_align_counts(self):
        """test hook: (counts, has a model) of all hypotheses of the last mode-"sac" align_pose() that ran any"""
        count, valid, nh = np.zeros(ALIGN_MAX_ITERATIONS, np.int32), np.zeros(ALIGN_MAX_ITERATIONS, np.int32), C.c_int(0)
        _lib.check(self.L.mcorb_lmap_last_align_counts(self.h, count.ctypes.data, valid.ctypes.data, ALIGN_MAX_ITERATIONS, C.byref(nh)))
        return count[:nh.value], valid[:nh.value].astype(bool)

    def set_track_refine(self, inv_sigma2=None, max_iterations=25):
        """inv_sigma2 given: from now on every tracking call on the store -- track, track_rig_frame, the submit / wait pair,
        track_rig_frames -- also refines, per frame and in the same submission, the pose of the view's rig from the frame's
        de-duplicated matches (octave 0: bestMatches carry none), read with last_track_pose().  None: off, the default"""
        _lib.check(self.L.mcorb_lmap_set_track_refine(
            self.h, None if inv_sigma2 is None else C.byref(pose_params(inv_sigma2, max_iterations))))

    def last_track_pose(self, f=0):
        """the PoseResult of frame f of the last tracking call, after its wait and until the next submission: bit for bit
        refine_pose() on that frame's match_kp -> pt, match_lid and camera arrays, from pose_of_view(view).  MCORB_E_STATE when
        the call ran without set_track_refine(), is pending or never happened"""
        res = _lib.PoseResultC()
        _lib.check(self.L.mcorb_lmap_last_track_pose(self.h, f, C.byref(res), None, 0))
        flags = np.zeros(max(res.n_obs, 1), np.uint8)
        _lib.check(self.L.mcorb_lmap_last_track_pose(self.h, f, C.byref(res), flags.ctypes.data, res.n_obs))
        return PoseResult(res, flags[:res.n_obs])


class PoseResult:
    """what LocalMap.refine_pose and LocalMap.last_track_pose return: R (3 x 3), t = w_T_b after the second round; status
    (POSE_NO_OBS, POSE_NO_STEP, POSE_CONVERGED, POSE_MAX_ITER: the second round's); iterations, the solves of each round;
    cost_initial (the first round's, at the initial pose) and cost_final (the second round's); n_inliers and inliers, one bool per
    observation: False once a round's cull took it"""

    def __init__(self, res, flags):
        self.R = np.array(res.R[:], np.float64).reshape(3, 3)
        self.t = np.array(res.t[:], np.float64)
        self.status, self.iterations = res.status, (res.iterations[0], res.iterations[1])
        self.cost_initial, self.cost_final = res.cost_initial, res.cost_final
        self.n_inliers, self.n_obs = res.n_inliers, res.n_obs
        self.inliers = flags.astype(bool)


class BAResult:
    """what LocalMap.bundle_adjust returns: R (nkf x 3 x 3), t (nkf x 3) and pts (nlm x 3), the returned state; status (BA_NO_OBS,
    BA_NO_STEP, BA_CONVERGED, BA_MAX_ITER); iterations, the solves taken; cost_initial and cost_final; n_inliers and inliers, one
    bool per observation in the caller's order: False where the whitened r.r > 5.991 at the returned state"""

    def __init__(self, res, R, t, pts, flags):
        self.R, self.t, self.pts = R, t, pts
        self.status, self.iterations = res.status, res.iterations
        self.cost_initial, self.cost_final = res.cost_initial, res.cost_final
        self.n_inliers, self.n_obs = res.n_inliers, res.n_obs
        self.inliers = flags.astype(bool)


BA_NO_OBS, BA_NO_STEP, BA_CONVERGED, BA_MAX_ITER = 0, 1, 2, 3
BA_MAX_KF = 16


class RetriResult:
    """what LocalMap.retriangulate returns, per landmark of lids: pts (nlm x 3), diff_norm, n_views and verdict (RETRI_*); counts,
    the landmarks per verdict; n_pairs, the (kf_id, feat) pairs of the landmarks with a failed verdict, and pairs, those pairs
    when the call deleted them (apply=True); launched, whether the kernels ran"""

    def __init__(self, res, pts, diff_norm, n_views, verdict, pairs):
        self.pts, self.diff_norm, self.n_views, self.verdict = pts, diff_norm, n_views, verdict
        self.counts, self.n_pairs, self.launched = list(res.counts), res.n_pairs, bool(res.launched)
        self.pairs = pairs


RETRI_REPORT, RETRI_APPLY = 0, 1
(RETRI_NOT_SELECTED, RETRI_FEW_VIEWS, RETRI_VALID_UPDATED, RETRI_VALID_REJECTED, RETRI_DEGENERATE, RETRI_BEHIND, RETRI_FAR,
 RETRI_OUTLIER) = range(8)
RETRI_MAX_KF = 1024


class SacResult:
    """what LocalMap.ransac_pose returns: R (3 x 3), t = the final w_T_b; status (SAC_OK, SAC_NO_OBS, SAC_NO_MODEL); used (0: the
    RANSAC's model, 1: the refinement's result); n_inliers and inliers, one bool per match, of the answer; n_matches.  The
    RANSAC's own: sac_R, sac_t, sac_n_inliers, best_hypothesis (-1: none), sample (the winner's four observations), n_models,
    n_consensus.  refine: the refinement's PoseResult (inliers per observation are not kept), None without it"""

    def __init__(self, res, flags, refined):
        self.R = np.array(res.R[:], np.float64).reshape(3, 3)
        self.t = np.array(res.t[:], np.float64)
        self.sac_R = np.array(res.sac_R[:], np.float64).reshape(3, 3)
        self.sac_t = np.array(res.sac_t[:], np.float64)
        self.status, self.used, self.n_inliers, self.n_matches = res.status, res.used, res.n_inliers, res.n_matches
        self.sac_n_inliers, self.best_hypothesis, self.sample = res.sac_n_inliers, res.best_hypothesis, tuple(res.sample[:])
        self.n_models, self.n_consensus = res.n_models, res.n_consensus
        self.inliers = flags.astype(bool)
        self.refine = PoseResult(res.refine, np.zeros(0, np.uint8)) if refined else None


SAC_OK, SAC_NO_OBS, SAC_NO_MODEL = 0, 1, 2
SAC_SOLVER_CENTRAL, SAC_SOLVER_RIG = 0, 1
SAC_SOLVERS = {"central": SAC_SOLVER_CENTRAL, "rig": SAC_SOLVER_RIG}


class RelResult:
    """what LocalMap.relative_pose returns: R (3 x 3), t = b1_T_b2 (X_b1 = R X_b2 + t; the identity without a winner); status
    (REL_OK, REL_NO_OBS, REL_NO_MODEL); n_inliers and inliers, one bool per match; n_matches; best_hypothesis (-1: none); sample
    (the winner's 17 matches in draw order); n_models"""

    def __init__(self, res, flags):
        self.R = np.array(res.R[:], np.float64).reshape(3, 3)
        self.t = np.array(res.t[:], np.float64)
        self.status, self.n_inliers, self.n_matches = res.status, res.n_inliers, res.n_matches
        self.best_hypothesis, self.sample, self.n_models = res.best_hypothesis, tuple(res.sample[:]), res.n_models
        self.inliers = flags.astype(bool)


REL_OK, REL_NO_OBS, REL_NO_MODEL = 0, 1, 2
REL_MAX_ITERATIONS, REL_SAMPLE = 16384, 17
REL_POLISH_ROUNDS, REL_POLISH_MAX_ITERATIONS = 2, 100


class RelPolish:
    """the polish record of LocalMap.relative_pose_polished and rel_polish: R (3 x 3), t and n_inliers of the pose the polish began
    from (the RANSAC winner's); rounds_run; rounds: per round that ran a dict of n_members, iterations, status (POSE_*),
    cost_initial, cost_final, n_inliers (of all matches at the round's result) and accepted"""

    def __init__(self, rec):
        self.R = np.array(rec.R[:], np.float64).reshape(3, 3)
        self.t = np.array(rec.t[:], np.float64)
        self.n_inliers, self.rounds_run = rec.n_inliers, rec.rounds_run
        self.rounds = [dict(n_members=q.n_members, iterations=q.iterations, status=q.status, cost_initial=q.cost_initial,
                            cost_final=q.cost_final, n_inliers=q.n_inliers, accepted=bool(q.accepted))
                       for q in rec.round[:rec.rounds_run]]


class EssentialResult:
    """what LocalMap.essential_pose returns: R (3 x 3), t = c1_T_c2 (X_c1 = R X_c2 + t, |t| = 1; the identity without a winner); E
    (3 x 3), the winning model, x1^T E x2 = 0 on normalised points; status (ESS_OK, ESS_NO_OBS, ESS_NO_MODEL); n_matches;
    n_ransac_inliers, the winner's count at the threshold; n_inliers and inliers, one bool per match: those of them that pass
    the winning candidate's depth test; best_hypothesis, best_root (-1: none); sample (the winner's five matches in draw order);
    n_models; cheirality, the four candidates' counts"""

    def __init__(self, res, flags):
        self.R = np.array(res.R[:], np.float64).reshape(3, 3)
        self.t = np.array(res.t[:], np.float64)
        self.E = np.array(res.E[:], np.float64).reshape(3, 3)
        self.status, self.n_matches = res.status, res.n_matches
        self.n_ransac_inliers, self.n_inliers = res.n_ransac_inliers, res.n_inliers
        self.best_hypothesis, self.best_root, self.sample = res.best_hypothesis, res.best_root, tuple(res.sample[:])
        self.n_models, self.cheirality = res.n_models, tuple(res.cheirality[:])
        self.inliers = flags.astype(bool)


ESS_OK, ESS_NO_OBS, ESS_NO_MODEL = 0, 1, 2
ESS_MAX_ITERATIONS, ESS_SAMPLE, ESS_MAX_ROOTS = 16384, 5, 10
ESS_POLISH_ROUNDS, ESS_POLISH_MAX_ITERATIONS = 2, 100


class EssentialPolish:
    """the polish record of LocalMap.essential_pose_polished and ess_polish_run: R (3 x 3), t, E (3 x 3), n_ransac_inliers and
    n_inliers of the pose the polish began from (the RANSAC winner's); rounds_run; rounds: per round that ran a dict of n_members,
    iterations, status (POSE_*), cost_initial, cost_final, n_ransac_inliers and n_inliers (of all matches at the round's result)
    and accepted"""

    def __init__(self, rec):
        self.R = np.array(rec.R[:], np.float64).reshape(3, 3)
        self.t = np.array(rec.t[:], np.float64)
        self.E = np.array(rec.E[:], np.float64).reshape(3, 3)
        self.n_ransac_inliers, self.n_inliers, self.rounds_run = rec.n_ransac_inliers, rec.n_inliers, rec.rounds_run
        self.rounds = [dict(n_members=q.n_members, iterations=q.iterations, status=q.status, cost_initial=q.cost_initial,
                            cost_final=q.cost_final, n_ransac_inliers=q.n_ransac_inliers, n_inliers=q.n_inliers, accepted=bool(q.accepted))
                       for q in rec.round[:rec.rounds_run]]


class AlignResult:
    """what LocalMap.align_pose returns: R (3 x 3), t = b1_T_b2 of the answer (X_1 = R X_2 + t; the identity without one); status
    (ALIGN_OK, ALIGN_NO_OBS, ALIGN_NO_MODEL); used (ALIGN_USED_SAC: the winning hypothesis, ALIGN_USED_FIT: a least-squares fit);
    n_inliers and inliers, one bool per pair, at inlier_dist with the answer; mean_error, the mean distance over all pairs;
    n_matches.  The hypotheses' own (mode "sac"): sac_R, sac_t, sac_n_inliers (at threshold), best_hypothesis (-1: none), sample
    (the winner's three pairs in draw order), n_models"""

    def __init__(self, res, flags):
        self.R = np.array(res.R[:], np.float64).reshape(3, 3)
        self.t = np.array(res.t[:], np.float64)
        self.sac_R = np.array(res.sac_R[:], np.float64).reshape(3, 3)
        self.sac_t = np.array(res.sac_t[:], np.float64)
        self.mean_error = res.mean_error
        self.status, self.used, self.n_inliers, self.n_matches = res.status, res.used, res.n_inliers, res.n_matches
        self.sac_n_inliers, self.best_hypothesis, self.sample = res.sac_n_inliers, res.best_hypothesis, tuple(res.sample[:])
        self.n_models = res.n_models
        self.inliers = flags.astype(bool)


ALIGN_OK, ALIGN_NO_OBS, ALIGN_NO_MODEL = 0, 1, 2
ALIGN_MODE_ALL, ALIGN_MODE_SAC = 0, 1
ALIGN_MODES = {"all": ALIGN_MODE_ALL, "sac": ALIGN_MODE_SAC}
ALIGN_USED_SAC, ALIGN_USED_FIT = 0, 1
ALIGN_MAX_ITERATIONS, ALIGN_SAMPLE = 16384, 3


def align_solve(p1, p2, member=None, with_gap=False):
    """test hook (host): the closed-form least-squares rigid fit over the pairs (p1[i], p2[i]) with member[i] (None: all) -> (R 3 x
    3, t) = b1_T_b2, or None when the fit is not valid; with_gap: -> (that, (l1 - l2) / (l1 - l4) of Horn's matrix)"""
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 3)
    n = len(p1)
    p2 = np.ascontiguousarray(p2, np.float64).reshape(n, 3)
    mem = None if member is None else np.ascontiguousarray(member, np.uint8).reshape(n)
    R, t, gap = np.zeros(9), np.zeros(3), C.c_double(0.0)
    k = _lib.load().mcorb_align_solve(n, p1.ctypes.data if n else None, p2.ctypes.data if n else None,
                                      None if mem is None else mem.ctypes.data, R.ctypes.data, t.ctypes.data, C.addressof(gap))
    _lib.check(min(k, 0))
    pose = (R.reshape(3, 3), t) if k else None
    return (pose, gap.value) if with_gap else pose


def align_eval(R, t, p1, p2):
    """test hook (host): the distances |p1 - (R p2 + t)| (n) of the pairs at the pose (R, t)"""
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 3)
    n = len(p1)
    p2 = np.ascontiguousarray(p2, np.float64).reshape(n, 3)
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    dist = np.zeros(max(n, 1))
    _lib.check(_lib.load().mcorb_align_eval(n, p1.ctypes.data if n else None, p2.ctypes.data if n else None, R.ctypes.data, t.ctypes.data,
                                            dist.ctypes.data))
    return dist[:n]


def rel_threshold(K00_02):
    """the reference's threshold of the relative problem: 2 * sac_threshold(K[0](0, 2))"""
    return _lib.load().mcorb_rel_threshold(float(K00_02))


def _rel_arrays(cam1, uv1, cam2, uv2):
    """the hooks' inputs: the keypoints go down as doubles (a float's value gives the bits relative_pose computes from it)"""
    cam1 = np.ascontiguousarray(cam1, np.int32).reshape(-1)
    n = len(cam1)
    return (n, cam1, np.ascontiguousarray(uv1, np.float64).reshape(n, 2), np.ascontiguousarray(cam2, np.int32).reshape(n),
            np.ascontiguousarray(uv2, np.float64).reshape(n, 2))


def rel_solve(cams, cam1, uv1, cam2, uv2):
    """test hook (host): the 17-point solver on 17 matches -> (R 3 x 3, t) = b1_T_b2, or None without a model"""
    n, cam1, uv1, cam2, uv2 = _rel_arrays(cam1, uv1, cam2, uv2)
    assert n == REL_SAMPLE
    ncams, ca = _pose_cams(cams)
    R, t = np.zeros(9), np.zeros(3)
    k = _lib.load().mcorb_rel_solve(ncams, ca, cam1.ctypes.data, uv1.ctypes.data, cam2.ctypes.data, uv2.ctypes.data, R.ctypes.data,
                                    t.ctypes.data)
    _lib.check(min(k, 0))
    return (R.reshape(3, 3), t) if k else None


def rel_eval(cams, R, t, cam1, uv1, cam2, uv2):
    """test hook (host): the scores (n) of the matches at the pose (R, t) = b1_T_b2"""
    n, cam1, uv1, cam2, uv2 = _rel_arrays(cam1, uv1, cam2, uv2)
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    score = np.zeros(max(n, 1))
    ncams, ca = _pose_cams(cams)
    _lib.check(_lib.load().mcorb_rel_eval(ncams, ca, n, cam1.ctypes.data, uv1.ctypes.data, cam2.ctypes.data, uv2.ctypes.data, R.ctypes.data,
                                          t.ctypes.data, score.ctypes.data))
    return score[:n]


def rel_polish(cams, R, t, cam1, uv1, cam2, uv2, member, threshold, rounds=2, polish_iterations=10):
    """test hook (host): the polish of the pose (R, t) = b1_T_b2 over the matches with member[i], keypoints as doubles; the
    current count and flags are the pose's own over all matches -> (R 3 x 3, t, inliers, RelPolish) of the accepted pose"""
    n, cam1, uv1, cam2, uv2 = _rel_arrays(cam1, uv1, cam2, uv2)
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    member = np.ascontiguousarray(member, np.uint8).reshape(n)
    ncams, ca = _pose_cams(cams)
    pp, rec = _lib.RelPolishParams(int(rounds), int(polish_iterations)), _lib.RelPolishC()
    Ro, to, flags = np.zeros(9), np.zeros(3), np.zeros(max(n, 1), np.uint8)
    _lib.check(_lib.load().mcorb_rel_polish_run(ncams, ca, n, cam1.ctypes.data, uv1.ctypes.data, cam2.ctypes.data, uv2.ctypes.data,
                                                member.ctypes.data, R.ctypes.data, t.ctypes.data, float(threshold), C.byref(pp),
                                                C.byref(rec), Ro.ctypes.data, to.ctypes.data, flags.ctypes.data))
    return Ro.reshape(3, 3), to, flags[:n].astype(bool), RelPolish(rec)


def ess_solve(cam, uv1, uv2, with_roots=False):
    """test hook (host): the five-point solver on 5 matches (keypoints as doubles) -> [E 3 x 3], at most 10, in ascending order of
    the root z each began from; with_roots: -> (that, [z])"""
    uv1 = np.ascontiguousarray(uv1, np.float64).reshape(5, 2)
    uv2 = np.ascontiguousarray(uv2, np.float64).reshape(5, 2)
    E, z = np.zeros((10, 9)), np.zeros(10)
    k = _lib.load().mcorb_ess_solve(_pose_cams(cam)[1], uv1.ctypes.data, uv2.ctypes.data, E.ctypes.data, z.ctypes.data)
    _lib.check(min(k, 0))
    models = [E[i].reshape(3, 3).copy() for i in range(k)]
    return (models, z[:k].tolist()) if with_roots else models


def ess_eval(cam, E, uv1, uv2):
    """test hook (host): the Sampson values (n) of the matches at E"""
    uv1 = np.ascontiguousarray(uv1, np.float64).reshape(-1, 2)
    n = len(uv1)
    uv2 = np.ascontiguousarray(uv2, np.float64).reshape(n, 2)
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    err = np.zeros(max(n, 1))
    _lib.check(_lib.load().mcorb_ess_eval(_pose_cams(cam)[1], n, uv1.ctypes.data, uv2.ctypes.data, E.ctypes.data, err.ctypes.data))
    return err[:n]


def ess_decompose(E, cam=None, uv1=None, uv2=None):
    """test hook (host): the four candidates of E -> (R+ 3 x 3, R- 3 x 3, t^): (R+, t^), (R-, t^), (R+, -t^), (R-, -t^); with cam and
    matches: -> (that, depths n x 4 x 2: each match's z in camera 1 and camera 2 under each candidate)"""
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    Rp, Rm, t = np.zeros(9), np.zeros(9), np.zeros(3)
    n, depth, a1, a2, ca = 0, np.zeros(8), None, None, None
    if cam is not None:
        uv1 = np.ascontiguousarray(uv1, np.float64).reshape(-1, 2)
        n = len(uv1)
        uv2 = np.ascontiguousarray(uv2, np.float64).reshape(n, 2)
        depth, a1, a2, ca = np.zeros((max(n, 1), 4, 2)), uv1.ctypes.data, uv2.ctypes.data, _pose_cams(cam)[1]
    _lib.check(_lib.load().mcorb_ess_decompose(E.ctypes.data, Rp.ctypes.data, Rm.ctypes.data, t.ctypes.data, ca, n, a1, a2, depth.ctypes.data))
    cands = (Rp.reshape(3, 3), Rm.reshape(3, 3), t)
    return cands if cam is None else (cands, depth[:n])


def ess_polish_run(cam, R, t, uv1, uv2, member, threshold_px=1.0, distance_thresh=50.0, rounds=2, polish_iterations=10):
    """test hook (host): the polish of the pose (R, t) = c1_T_c2, |t| = 1, over the matches with member[i], keypoints as doubles; the
    current counts and flags are the pose's own over all matches -> (R 3 x 3, t, E 3 x 3, inliers, EssentialPolish) of the accepted
    pose"""
    uv1 = np.ascontiguousarray(uv1, np.float64).reshape(-1, 2)
    n = len(uv1)
    uv2 = np.ascontiguousarray(uv2, np.float64).reshape(n, 2)
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    member = np.ascontiguousarray(member, np.uint8).reshape(n)
    pp, rec = _lib.EssPolishParams(int(rounds), int(polish_iterations)), _lib.EssPolishC()
    Ro, to, Eo, flags = np.zeros(9), np.zeros(3), np.zeros(9), np.zeros(max(n, 1), np.uint8)
    _lib.check(_lib.load().mcorb_ess_polish_run(_pose_cams(cam)[1], n, uv1.ctypes.data, uv2.ctypes.data, member.ctypes.data, R.ctypes.data,
                                                t.ctypes.data, float(threshold_px), float(distance_thresh), C.byref(pp), C.byref(rec),
                                                Ro.ctypes.data, to.ctypes.data, Eo.ctypes.data, flags.ctypes.data))
    return Ro.reshape(3, 3), to, Eo.reshape(3, 3), flags[:n].astype(bool), EssentialPolish(rec)


def sac_threshold(K00_02):
    """the reference's RANSAC threshold: 1 - cos(atan(sqrt(2) * 0.5 / K[0](0, 2)))"""
    return _lib.load().mcorb_sac_threshold(float(K00_02))


def sac_solve(cams, cam, uv, pts):
    """test hook (host): the rig poses (at most 4) of the minimal solver on three observations of camera cam -- keypoints uv
    (3 x 2), points pts (3 x 3) -> [(R 3 x 3, t)]"""
    uv = np.ascontiguousarray(uv, np.float32).reshape(3, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(3, 3)
    ncams, ca = _pose_cams(cams)
    assert 0 <= cam < ncams
    R, t = np.zeros((4, 9)), np.zeros((4, 3))
    k = _lib.load().mcorb_sac_solve(ca + int(cam) * C.sizeof(_lib.TrackCam), uv.ctypes.data, pts.ctypes.data, R.ctypes.data, t.ctypes.data)
    _lib.check(min(k, 0))
    return [(R[i].reshape(3, 3).copy(), t[i].copy()) for i in range(k)]


def sac_solve_rig(cams, cam, uv, pts):
    """test hook (host): the rig poses (at most 4) of the rig solver on three observations of cameras cam (3) -- keypoints uv
    (3 x 2), points pts (3 x 3) -> [(R 3 x 3, t)]"""
    cam = np.ascontiguousarray(cam, np.int32).reshape(3)
    uv = np.ascontiguousarray(uv, np.float32).reshape(3, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(3, 3)
    ncams, ca = _pose_cams(cams)
    R, t = np.zeros((4, 9)), np.zeros((4, 3))
    k = _lib.load().mcorb_sac_solve_rig(ncams, ca, cam.ctypes.data, uv.ctypes.data, pts.ctypes.data, R.ctypes.data, t.ctypes.data)
    _lib.check(min(k, 0))
    return [(R[i].reshape(3, 3).copy(), t[i].copy()) for i in range(k)]


def sac_rig_roots(cams, cam, uv, pts):
    """test hook (host): the rig solver on four observations of cameras cam (4) -- the three of sac_solve_rig and the fourth,
    disambiguating one -> ([(R 3 x 3, t)] as sac_solve_rig gives them, mask: bit k set iff root k has a pose, best: the root the
    estimator takes (-1: none), (R 3 x 3, t) of that root, zero without)"""
    cam = np.ascontiguousarray(cam, np.int32).reshape(4)
    uv = np.ascontiguousarray(uv, np.float32).reshape(4, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(4, 3)
    ncams, ca = _pose_cams(cams)
    R, t, Rb, tb = np.zeros((4, 9)), np.zeros((4, 3)), np.zeros(9), np.zeros(3)
    mask, best = np.zeros(1, np.int32), np.zeros(1, np.int32)
    k = _lib.load().mcorb_host_sac_rig_roots(ncams, ca, cam.ctypes.data, uv.ctypes.data, pts.ctypes.data, R.ctypes.data, t.ctypes.data,
                                             mask.ctypes.data, best.ctypes.data, Rb.ctypes.data, tb.ctypes.data)
    _lib.check(min(k, 0))
    return [(R[i].reshape(3, 3).copy(), t[i].copy()) for i in range(k)], int(mask[0]), int(best[0]), (Rb.reshape(3, 3), tb)


_CAM_DOUBLES = C.sizeof(_lib.TrackCam) // 8


def _cam_rows(view):
    """the cameras of a track_view as doubles, ncams x 17"""
    return np.frombuffer(view.cams, np.float64).reshape(_lib.MAX_CAMS, _CAM_DOUBLES)[:view.ncams]


def _rig_table(rigs):
    """the rigs of n problems -> (ncams: the largest rig's, n x ncams x 17 doubles, smaller rigs padded with zeros)"""
    ncams = max([r.ncams for r in rigs], default=1)
    table = np.zeros((len(rigs), ncams, _CAM_DOUBLES))
    for i, r in enumerate(rigs):
        table[i, :r.ncams] = _cam_rows(r)
    return ncams, table


def _own_rig(rigs, *cams):
    """the entries check a camera index against the table's one ncams, the largest rig's: an index outside a problem's own,
    smaller rig would read a camera of zeros there, so it is refused here as the host hooks refuse it"""
    own = np.array([r.ncams for r in rigs], np.int64).reshape(len(rigs), 1)
    if len(rigs) and any((np.asarray(c).reshape(len(rigs), -1) >= own).any() for c in cams):
        raise McorbError(E_ARG, "a camera index outside the rig")


def _p(a):
    return a.ctypes.data if a.size else None


def dev_sac_solve(rigs, cam, uv, pts, device=0):
    """test hook (device): sac_solve on n problems in one launch -- problem i: camera cam[i] of rigs[i], uv (n x 3 x 2), pts (n x 3 x
    3) -> (count n, R n x 4 x 9, t n x 4 x 3), zero behind a problem's count"""
    n = len(rigs)
    cam = np.ascontiguousarray(cam, np.int64).reshape(n)
    uv = np.ascontiguousarray(uv, np.float32).reshape(n, 3, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(n, 3, 3)
    cams = np.zeros((n, _CAM_DOUBLES))
    for i, r in enumerate(rigs):
        assert 0 <= cam[i] < r.ncams
        cams[i] = _cam_rows(r)[cam[i]]
    count, R, t = np.zeros(n, np.int32), np.zeros((n, 4, 9)), np.zeros((n, 4, 3))
    _lib.check(_lib.load().mcorb_dev_sac_solve_selftest(int(device), n, _p(cams), _p(uv), _p(pts), _p(count), _p(R), _p(t)))
    return count, R, t


def dev_sac_solve_rig(rigs, cam, uv, pts, device=0):
    """test hook (device): sac_rig_roots on n problems in one launch of the rig hypotheses kernel's shape and body -- problem i:
    cameras cam[i] (4) of rigs[i], uv (n x 4 x 2), pts (n x 4 x 3) -> (count n, R n x 4 x 9, t n x 4 x 3, mask n, best n, best_R n x
    9, best_t n x 3)"""
    n = len(rigs)
    cam = np.ascontiguousarray(cam, np.int32).reshape(n, 4)
    uv = np.ascontiguousarray(uv, np.float32).reshape(n, 4, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(n, 4, 3)
    _own_rig(rigs, cam)
    ncams, cams = _rig_table(rigs)
    count, mask, best = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    R, t, Rb, tb = np.zeros((n, 4, 9)), np.zeros((n, 4, 3)), np.zeros((n, 9)), np.zeros((n, 3))
    _lib.check(_lib.load().mcorb_dev_sac_solve_rig_selftest(int(device), n, ncams, _p(cams), _p(cam), _p(uv), _p(pts), _p(count), _p(R),
                                                            _p(t), _p(mask), _p(best), _p(Rb), _p(tb)))
    return count, R, t, mask, best, Rb, tb


def dev_rel_solve(rigs, cam1, uv1, cam2, uv2, device=0):
    """test hook (device): rel_solve on n problems in one launch -- problem i: 17 matches of rigs[i], cam1 and cam2 (n x 17), uv1
    and uv2 (n x 17 x 2, doubles) -> (count n, R n x 9, t n x 3), zero without a model"""
    n = len(rigs)
    cam1 = np.ascontiguousarray(cam1, np.int32).reshape(n, REL_SAMPLE)
    cam2 = np.ascontiguousarray(cam2, np.int32).reshape(n, REL_SAMPLE)
    uv1 = np.ascontiguousarray(uv1, np.float64).reshape(n, REL_SAMPLE, 2)
    uv2 = np.ascontiguousarray(uv2, np.float64).reshape(n, REL_SAMPLE, 2)
    _own_rig(rigs, cam1, cam2)
    ncams, cams = _rig_table(rigs)
    count, R, t = np.zeros(n, np.int32), np.zeros((n, 9)), np.zeros((n, 3))
    _lib.check(_lib.load().mcorb_dev_rel_solve_selftest(int(device), n, ncams, _p(cams), _p(cam1), _p(uv1), _p(cam2), _p(uv2), _p(count),
                                                        _p(R), _p(t)))
    return count, R, t


def dev_ess_solve(rigs, uv1, uv2, device=0):
    """test hook (device): ess_solve on n problems in one launch of the essential hypotheses kernel's shape and body -- problem i:
    camera 0 of rigs[i], uv1 and uv2 (n x 5 x 2, doubles) -> (count n, E n x 10 x 9, z n x 10), zero behind a problem's count"""
    n = len(rigs)
    uv1 = np.ascontiguousarray(uv1, np.float64).reshape(n, 5, 2)
    uv2 = np.ascontiguousarray(uv2, np.float64).reshape(n, 5, 2)
    cams = np.zeros((n, _CAM_DOUBLES))
    for i, r in enumerate(rigs):
        cams[i] = _cam_rows(r)[0]
    count, E, z = np.zeros(n, np.int32), np.zeros((n, 10, 9)), np.zeros((n, 10))
    _lib.check(_lib.load().mcorb_dev_ess_solve_selftest(int(device), n, _p(cams), _p(uv1), _p(uv2), _p(count), _p(E), _p(z)))
    return count, E, z


def dev_align_solve(problems, device=0):
    """test hook (device): align_solve on n problems in one launch, a workgroup each -- problems: [(p1 k x 3, p2 k x 3, member k or
    None: all)] -> (valid n, R n x 9, t n x 3, gap n), R and t zero without a valid fit"""
    n = len(problems)
    npairs = np.array([len(np.asarray(p[0]).reshape(-1, 3)) for p in problems], np.int32).reshape(n)
    p1 = np.concatenate([np.asarray(p[0], np.float64).reshape(-1, 3) for p in problems] + [np.zeros((0, 3))])
    p2 = np.concatenate([np.asarray(p[1], np.float64).reshape(-1, 3) for p in problems] + [np.zeros((0, 3))])
    member = np.concatenate([np.ones(k, np.uint8) if p[2] is None else (np.asarray(p[2]).reshape(k) != 0).astype(np.uint8)
                             for p, k in zip(problems, npairs)] + [np.zeros(0, np.uint8)])
    p1, p2, member = np.ascontiguousarray(p1), np.ascontiguousarray(p2), np.ascontiguousarray(member)
    valid, R, t, gap = np.zeros(n, np.int32), np.zeros((n, 9)), np.zeros((n, 3)), np.zeros(n)
    _lib.check(_lib.load().mcorb_dev_align_solve_selftest(int(device), n, _p(npairs), _p(p1), _p(p2), _p(member), _p(valid), _p(R), _p(t),
                                                          _p(gap)))
    return valid, R, t, gap


def sac_eval(cams, R, t, cam, uv, pts):
    """test hook (host): the scores (n) of the observations at the pose (R, t)"""
    cam = np.ascontiguousarray(cam, np.int32).reshape(-1)
    n = len(cam)
    uv = np.ascontiguousarray(uv, np.float32).reshape(n, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(n, 3)
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    score = np.zeros(max(n, 1))
    ncams, ca = _pose_cams(cams)
    _lib.check(_lib.load().mcorb_sac_eval(ncams, ca, n, cam.ctypes.data, uv.ctypes.data, pts.ctypes.data, R.ctypes.data, t.ctypes.data,
                                          score.ctypes.data))
    return score[:n]


def pose_params(inv_sigma2, max_iterations=25):
    """mcorb_pose_params: inv_sigma2 = GetInverseScaleSigmaSquares(), one per pyramid level"""
    s2 = np.asarray(inv_sigma2, np.float64).reshape(-1)
    p = _lib.PoseParams()
    p.nlevels, p.max_iterations = len(s2), int(max_iterations)
    for k in range(min(len(s2), _lib.MAX_LEVELS)):
        p.inv_sigma2[k] = float(s2[k])
    return p


def pose_cams(cam_R, cam_t, K_mats):
    """the rig of LocalMap.refine_pose: per camera body_P_sensor = (cam_R, cam_t) and the 3x3 calibration (Cal3_S2: fx, s, u0,
    fy, v0), as track_view takes them"""
    return track_view(np.eye(3), np.zeros(3), cam_R, cam_t, K_mats, 0, 0)


def _pose_cams(cams):
    """-> (ncams, the address of the mcorb_track_cam array) of a track_view"""
    return cams.ncams, C.addressof(cams.cams)


def pose_of_view(view):
    """(R, t) = w_T_b of a track_view read as a rig whose body is camera 0's frame: R0^T, -(R0^T t0)"""
    R, t = np.zeros(9), np.zeros(3)
    _lib.load().mcorb_pose_of_view(C.byref(view), R.ctypes.data, t.ctypes.data)
    return R.reshape(3, 3), t


def pose_eval(cams, R, t, cam, uv, pts):
    """test hook (host): residual r (n x 2), Jacobian J (n x 2 x 6, w.r.t. the right perturbation (omega, upsilon)) and Huber
    weight w (n) of the observations at the pose (R, t)"""
    cam = np.ascontiguousarray(cam, np.int32).reshape(-1)
    n = len(cam)
    uv = np.ascontiguousarray(uv, np.float32).reshape(n, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(n, 3)
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    r, J, w = np.zeros((max(n, 1), 2)), np.zeros((max(n, 1), 2, 6)), np.zeros(max(n, 1))
    ncams, ca = _pose_cams(cams)
    _lib.check(_lib.load().mcorb_pose_eval(ncams, ca, n, cam.ctypes.data, uv.ctypes.data, pts.ctypes.data, R.ctypes.data, t.ctypes.data,
                                           r.ctypes.data, J.ctypes.data, w.ctypes.data))
    return r[:n], J[:n], w[:n]


def ba_params(sigma, max_iterations=25):
    """mcorb_ba_params: sigma per pyramid level, as the back end hands it to Isotropic::Sigma"""
    s = np.asarray(sigma, np.float64).reshape(-1)
    p = _lib.BAParams()
    p.nlevels, p.max_iterations = len(s), int(max_iterations)
    for k in range(min(len(s), _lib.MAX_LEVELS)):
        p.sigma[k] = float(s[k])
    return p


def ba_eval(cams, R, t, cam, uv, pts, sigma):
    """test hook (host): whitened residual r (n x 2), Jacobians J (n x 2 x 6, by the pose's right perturbation) and JX (n x 2 x 3,
    by the point) and Huber weight w (n) of the observations at the pose (R, t); sigma: one per observation"""
    cam = np.ascontiguousarray(cam, np.int32).reshape(-1)
    n = len(cam)
    uv = np.ascontiguousarray(uv, np.float32).reshape(n, 2)
    pts = np.ascontiguousarray(pts, np.float64).reshape(n, 3)
    sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, np.float64), (n,)))
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    r, J, JX, w = np.zeros((max(n, 1), 2)), np.zeros((max(n, 1), 2, 6)), np.zeros((max(n, 1), 2, 3)), np.zeros(max(n, 1))
    ncams, ca = _pose_cams(cams)
    _lib.check(_lib.load().mcorb_ba_eval(ncams, ca, n, cam.ctypes.data, uv.ctypes.data, pts.ctypes.data, sigma.ctypes.data, R.ctypes.data,
                                         t.ctypes.data, r.ctypes.data, J.ctypes.data, JX.ctypes.data, w.ctypes.data))
    return r[:n], J[:n], JX[:n], w[:n]


class TrackResult:
    """what LocalMap.track and LocalMap.track_wait return, every member a list with one array per camera.  The projected landmarks in candidate order:
    proj_lid, proj_xy (the projected keypoint's pt, float32) and, per projected query before the serial part, best_kp (-1: none)
    and best_dist (10000 with -1).  After the de-duplication, in the reference's order: match_kp (bestMatches as keypoint
    indices), match_lid (bestMatchLandmarkIds), match_dist and match_pt (bestMatchLandmarks: the store's points; None for a call
    submitted with want_pts=False).  n_candidates:
    the distinct landmarks of the call"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def track_view(R0, t0, cam_R, cam_t, K_mats, cols, rows):
    """the view of LocalMap.track: (R0, t0) = cameraRig.c0_T_w, the predicted pose; cam_R / cam_t: per camera the pose of its
    PinholePose (R_T_mats[i].inverse(), which the caller computes); K_mats: per camera the 3x3 calibration, of which fx, s, u0, fy
    and v0 are read (Cal3_S2); cols / rows: imgCols / imgRows"""
    v = _lib.TrackView()
    v.R0[:] = np.asarray(R0, np.float64).reshape(9).tolist()
    v.t0[:] = np.asarray(t0, np.float64).reshape(3).tolist()
    v.ncams, v.cols, v.rows = len(cam_R), int(cols), int(rows)
    if not 1 <= v.ncams <= _lib.MAX_CAMS or not len(cam_t) == len(K_mats) == v.ncams:
        raise ValueError("track_view: 1 .. %d cameras, one R, t and K each" % _lib.MAX_CAMS)
    for c in range(v.ncams):
        K = np.asarray(K_mats[c], np.float64).reshape(3, 3)
        cam = v.cams[c]
        cam.R[:] = np.asarray(cam_R[c], np.float64).reshape(9).tolist()
        cam.t[:] = np.asarray(cam_t[c], np.float64).reshape(3).tolist()
        cam.fx, cam.s, cam.u0, cam.fy, cam.v0 = float(K[0, 0]), float(K[0, 1]), float(K[0, 2]), float(K[1, 1]), float(K[1, 2])
    return v


class ObsFrameArrays:
    """the observing keyframe of LocalMap.observe (mcorb_obs_frame); keeps the array the struct points to"""

    def __init__(self, kf_id, match_index, centres_w):
        self.match_index = np.ascontiguousarray(match_index, np.int32)
        if self.match_index.ndim != 2:
            raise ValueError("obs_frame: match_index is nfeat x ncams")
        nfeat, ncams = self.match_index.shape
        if not 1 <= ncams <= _lib.MAX_CAMS or len(centres_w) != ncams:
            raise ValueError("obs_frame: 1 .. %d cameras, one centre each" % _lib.MAX_CAMS)
        f = self.struct = _lib.ObsFrame()
        f.kf_id, f.nfeat, f.ncams, f.match_index = int(kf_id), nfeat, ncams, self.match_index.ctypes.data
        for c in range(ncams):
            f.centre_w[c][:] = np.asarray(centres_w[c], np.float64).reshape(3).tolist()


def obs_frame(kf_id, lf, centres_w):
    """the keyframe of LocalMap.observe from its id, mcorb_lf_feature records (Rig.lf_features; or an nfeat x ncams matchIndex array)
    and W_T_cur's translation per camera (the translation column of pose * cur_T_ref.inv(), GlobalMap.cpp:45-49)"""
    lf = np.asarray(lf)
    mi = lf["match_index"][:, :len(centres_w)] if lf.dtype.names else lf
    return ObsFrameArrays(kf_id, mi, centres_w)


def _hook_cases(who, X, nv1, nv, P, K, centre, kps, octave, inv_sigma2, per_case):
    """the cases of a test hook (map_gates, init_cases, map_refine), contiguous and checked: the views back to back and the
    hook's own `per_case` arrays, a row per case -> (n, the leading arguments of the C entry: n and the pointers of X .. octave,
    what they point to (the caller holds it across the call), inv_sigma2 as float32)"""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    n = len(X)
    nv1, nv = np.ascontiguousarray(nv1, np.int32).reshape(-1), np.ascontiguousarray(nv, np.int32).reshape(-1)
    views = [np.ascontiguousarray(P, np.float64).reshape(-1, 12), np.ascontiguousarray(K, np.float64).reshape(-1, 9),
             np.ascontiguousarray(centre, np.float64).reshape(-1, 3), np.ascontiguousarray(kps, np.float32).reshape(-1, 2),
             np.ascontiguousarray(octave, np.int32).reshape(-1)]
    V = int(nv.sum()) if len(nv) == n else -1
    if not (all(len(a) == n for a in [nv1, *per_case]) and all(len(a) == V for a in views)):
        raise ValueError(who + ": array lengths do not fit the view counts")
    keep = [X, nv1, nv] + views
    return n, (n,) + tuple(a.ctypes.data for a in keep), keep, np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1)


def map_gates(X, nv1, nv, P, K, centre, kps, octave, F, inv_sigma2, device=None):
    """the test hooks mcorb_host_map_gates (device None) / mcorb_dev_map_gates_selftest: everything of a match but the
    triangulation for n cases with caller-given X -> (verdict, n_rays, dist2, cos, normal).  Views back to back: P (V x 12),
    K (V x 9), centre (V x 3), kps (V x 2 float32), octave (V); per case X (3), nv1, nv, F (9)"""
    F = np.ascontiguousarray(F, np.float64).reshape(-1, 9)
    n, cases, _keep, sig = _hook_cases("map_gates", X, nv1, nv, P, K, centre, kps, octave, inv_sigma2, [F])
    verdict, rays, vals = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 5))
    args = cases + (F.ctypes.data, sig.ctypes.data, len(sig), verdict.ctypes.data, rays.ctypes.data, vals.ctypes.data)
    L = _lib.load()
    _lib.check(L.mcorb_host_map_gates(*args) if device is None else L.mcorb_dev_map_gates_selftest(device, *args))
    return verdict[:n], rays[:n], vals[:n, 0].copy(), vals[:n, 1].copy(), vals[:n, 2:].copy()


def init_cases(X, nv1, nv, P, K, centre, kps, octave, inv_sigma2, ncams, R, t, min_baseline, inliers, device=None):
    """the test hooks mcorb_host_init_cases (device None) / mcorb_dev_init_cases_selftest: everything of LocalMap.initialize but
    the triangulation and the store, the n cases standing for the n matches of one call -> InitResult (new_lid counts from 0).
    Views back to back as for map_gates, but centre is centre_w for a view of prev and cam_centre_body for a view of cur"""
    Rr, tt = np.ascontiguousarray(R, np.float64).reshape(9), np.ascontiguousarray(t, np.float64).reshape(3)
    fl = np.ascontiguousarray(np.asarray(inliers).reshape(-1) != 0, np.uint8)
    n, cases, _keep, sig = _hook_cases("init_cases", X, nv1, nv, P, K, centre, kps, octave, inv_sigma2, [fl])
    m = max(n, 1)
    verdict, rays, off, vals = np.zeros(m, np.int32), np.zeros(m, np.int32), np.full(m, -1, np.int32), np.zeros((m, 8))
    o = _lib.InitResultC()
    args = cases + (sig.ctypes.data, len(sig), int(ncams), Rr.ctypes.data, tt.ctypes.data, float(min_baseline), fl.ctypes.data,
                    verdict.ctypes.data, rays.ctypes.data, off.ctypes.data, vals.ctypes.data, C.byref(o))
    L = _lib.load()
    _lib.check(L.mcorb_host_init_cases(*args) if device is None else L.mcorb_dev_init_cases_selftest(device, *args))
    return InitResult(inliers=fl[:n].astype(bool), verdict=verdict[:n].astype(np.uint8), new_lid=off[:n], n_rays=rays[:n],
                      pt3d=vals[:n, 0:3].copy(), normal=vals[:n, 3:6].copy(), dist2=vals[:n, 6].copy(), cos_parallax=vals[:n, 7].copy(),
                      **_init_scalars(o))


def map_refine(X0, nv1, nv, P, K, centre, kps, octave, twc_cur, twc_prev, inv_sigma2, device=None):
    """the test hooks mcorb_host_map_refine (device None) / mcorb_dev_map_refine_selftest: everything of a match of
    LocalMap.triangulate_new after the DLT for n cases with caller-given X0 -> (verdict, n_rays, solves, cos (float32), X, normal,
    dist, cost_initial, cost_final).  Views back to back as for map_gates; per case X0 (3), nv1, nv, twc_cur (3), twc_prev (3)"""
    tc, tp = np.ascontiguousarray(twc_cur, np.float64).reshape(-1, 3), np.ascontiguousarray(twc_prev, np.float64).reshape(-1, 3)
    n, cases, _keep, sig = _hook_cases("map_refine", X0, nv1, nv, P, K, centre, kps, octave, inv_sigma2, [tc, tp])
    m = max(n, 1)
    verdict, rays, solves, cosp, vals = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.float32), np.zeros((m, 9))
    args = cases + (tc.ctypes.data, tp.ctypes.data, sig.ctypes.data, len(sig), verdict.ctypes.data, rays.ctypes.data,
                    solves.ctypes.data, cosp.ctypes.data, vals.ctypes.data)
    L = _lib.load()
    _lib.check(L.mcorb_host_map_refine(*args) if device is None else L.mcorb_dev_map_refine_selftest(device, *args))
    return (verdict[:n], rays[:n], solves[:n], cosp[:n], vals[:n, 0:3].copy(), vals[:n, 3:6].copy(), vals[:n, 6].copy(),
            vals[:n, 7].copy(), vals[:n, 8].copy())


class DescriptorBlock:
    """nsets descriptor sets resident in HBM (mcorb_descblock): upload a keyframe's LF descriptors once, match any two sets with
    Rig.match_sets (findInterMatches' knnMatch, FrontEnd.cpp:3344-3500)."""

    def __init__(self, nsets, kcap, device=0):
        self.L = _lib.load()
        self.h = C.c_void_p()
        _lib.check(self.L.mcorb_descblock_create(device, nsets, kcap, C.byref(self.h)))
        self.nsets, self.kcap = nsets, kcap

    def upload(self, set_index, desc):
        d = _u8(desc).reshape(-1, 32)
        _lib.check(self.L.mcorb_descblock_upload(self.h, set_index, d.ctypes.data, len(d)))

    def close(self):
        if getattr(self, "h", None):
            self.L.mcorb_descblock_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_tracks(ncams, counts, pair_lists):
    """computeIntraMatches' serial track merge (MultiCameraFrame.cpp:1167-1268) on host arrays, no device: counts[c] keypoints
    per camera, pair_lists[p] = (idx1, idx2) of camera pair p in (0,1), (0,2), .., (1,2), .. order -> (tracks [n][ncams], mergeable)."""
    L = _lib.load()
    counts = np.ascontiguousarray(counts, np.int32)
    npairs = ncams * (ncams - 1) // 2
    assert len(pair_lists) == npairs and len(counts) == ncams
    keep = [(np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)) for a, b in pair_lists]
    p1, p2 = (C.c_void_p * npairs)(), (C.c_void_p * npairs)()
    for p, (a, b) in enumerate(keep):
        assert len(a) == len(b)
        p1[p], p2[p] = a.ctypes.data, b.ctypes.data
    npair = np.array([len(a) for a, _ in keep], np.int32)
    cap = int(npair.sum()) + 1
    tr = np.full((cap, ncams), -1, np.int32)
    n, mg = C.c_int(), C.c_int()
    _lib.check(L.mcorb_host_merge_tracks(ncams, counts.ctypes.data, p1, p2, npair.ctypes.data, tr.ctypes.data, cap, C.byref(n), C.byref(mg)))
    return tr[:n.value].copy(), mg.value


def fundamental_from_extrinsics(K_i, R_i, t_i, K_j, R_j, t_j):
    """F with x_j^T F x_i = 0 from the two cameras' extrinsics, the construction of MultiCameraFrame.cpp:1126-1142."""
    def T(R, t):
        M = np.eye(4)
        M[:3, :3] = np.asarray(R, np.float64)
        M[:3, 3] = np.asarray(t, np.float64).reshape(3)
        return M
    Tji = T(R_j, t_j) @ np.linalg.inv(T(R_i, t_i))
    tx, ty, tz = Tji[0, 3], Tji[1, 3], Tji[2, 3]
    skew = np.array([[0, -tz, ty], [tz, 0, -tx], [-ty, tx, 0]], np.float64)
    return np.linalg.inv(np.asarray(K_j, np.float64).T) @ skew @ Tji[:3, :3] @ np.linalg.inv(np.asarray(K_i, np.float64))


class IntraMatch:
    """MultiCameraFrame.h:42-57 (matchIndex widened from 5 to ncams entries)."""

    def __init__(self, matchIndex):
        self.matchIndex = list(matchIndex)
        self.mono = True
        self.n_rays = 0

    @classmethod
    def from_lf(cls, row):
        """one entry of currentFrame->intraMatches after obtainLfFeatures (a row of Rig.lf_features' array)"""
        m = cls(row["match_index"])
        m.mono = bool(row["mono"])
        m.n_rays = int(row["n_rays"])
        m.uv_ref = (float(row["uv_ref"][0]), float(row["uv_ref"][1]))
        m.point3D = np.array(row["point3d"], np.float64)
        m.matchDesc = np.array(row["desc"], np.uint8)
        return m


class MultiCameraFrame:
    """Mirror of the extract + intra-rig-match members of MultiCameraFrame
    (MultiCameraFrame.h:70-90) for one rig frame."""

    def __init__(self, ncams, width, height, params=None, rig=None, **kw):
        self.num_cams_ = ncams
        self.rig = rig if rig is not None else Rig(ncams, width, height, 1, 1, params=params, **kw)
        self.imgs = []
        self.image_kps, self.image_kps_undist, self.image_descriptors = [], [], []
        self._matched = False
        self._distorted = False   # setDistortion gave some camera coefficients: extraction fills image_kps_undist from the rig
        self.BoW_vecs, self.BoW_feats = [], []   # per camera, filled by extractFeaturesParallel once setVocabulary was called
        self._voc, self._voc_levelsup = None, 4
        self._rows_replaced = False   # setUndistorted() gave rows other than the rig's: the job's tracks do not apply
        self._lf = False   # setLfConfig: extractFeaturesParallel() also fills intraMatches / lfBoW / lfFeatVec from the job
        self.intraMatches, self.intramatch_size, self.mono_size, self.lfBoW, self.lfFeatVec = [], 0, 0, None, None

    def setData(self, img_set, segmap_set=None):
        """setData (MultiCameraFrame.cpp:95-152): accepts the reference's CV_32F [0,1] frames or u8."""
        if len(img_set) != self.num_cams_:
            print("ERROR:: number of images is wrong")   # the reference prints and returns (:98-101)
            return
        self.imgs = list(img_set)
        self.rig.upload(self.imgs)
        self._matched = False

    def extractFeaturesParallel(self):
        """extractFeaturesParallel (MultiCameraFrame.cpp:203-228)."""
        assert self.num_cams_ == len(self.imgs)
        self.rig.extract(self.num_cams_)
        self.image_kps, self.image_descriptors = [], []
        for c in range(self.num_cams_):
            _, k, d = self.rig.features(c)
            self.image_kps.append(k)
            self.image_descriptors.append(d)
        if self._distorted:   # UndistortKeyPoints (:236-245, :300-347), run on the device inside the extraction job
            self.image_kps_undist = [self.rig.features_undist(c) for c in range(self.num_cams_)]
        else:
            self.image_kps_undist = self.image_kps   # RECTIFY, or zero distortion: UndistortKeyPoints copies (:241-242, :302-305)
        self._rows_replaced = False
        if self._voc is not None:   # orb_vocabulary->transform(vec_desc, bowVec, featVec, 4) per camera (:252-261), made by the job
            tf = self.rig.bow_transforms(0, self.num_cams_)
            self.BoW_vecs = [bow for bow, _ in tf]
            self.BoW_feats = [fv for _, fv in tf]
            if self._lf:   # obtainLfFeatures + orb_vocabulary->transform of the LF set (FrontEnd.cpp:1009-1024, :525)
                feats, self.intramatch_size, self.mono_size, _ = self.rig.lf_features(0)
                self.intraMatches = [IntraMatch.from_lf(row) for row in feats]
                self.lfBoW, self.lfFeatVec = self.rig.lf_bow(0)
        self._matched = False

    extractFeatures = extractFeaturesParallel

    def setDistortion(self, K_mats, dist_coeffs):
        """camconfig_.K_mats_ / dist_coeffs_ (CV_64F, 4, 5, 8 or 12 coefficients per camera; None or empty = no distortion):
        call once at init.  From then on extractFeaturesParallel() fills image_kps_undist as UndistortKeyPoints does, zero test
        included (a camera whose k1 passes it is copied)."""
        if len(K_mats) != self.num_cams_ or len(dist_coeffs) != self.num_cams_:
            raise ValueError("one K and one coefficient set per camera")
        for c in range(self.num_cams_):
            self.rig.set_undistortion(c, K_mats[c], dist_coeffs[c])
        self._distorted = any(d is not None and len(np.ravel(d)) > 0 for d in dist_coeffs)

    def setRectify(self, K_mats, dist_coeffs):
        """camconfig_.RECTIFY (MultiCameraFrame.cpp:123-136): K_mats_ / dist_coeffs_ as setDistortion takes them.  From then on
        setData() leaves cv::undistort(img, K, dist) of every camera image in the rig, and extractFeaturesParallel() copies the
        keypoints into image_kps_undist (:241-242).  A camera given None or no coefficients is cleared.  Excludes setDistortion."""
        if len(K_mats) != self.num_cams_ or len(dist_coeffs) != self.num_cams_:
            raise ValueError("one K and one coefficient set per camera")
        for c in range(self.num_cams_):
            self.rig.set_image_undistortion(c, K_mats[c], dist_coeffs[c])

    def setVocabulary(self, voc, levelsup=4):
        """orb_vocabulary (MultiCameraFrame.cpp:252-261): from now on extractFeaturesParallel() fills BoW_vecs[cam] as
        (word ids, values) and BoW_feats[cam] as {node: feature indices}, and computeIntraMatchesBoW(voc, levelsup=levelsup)
        reads the tracks the extraction job already made.  None unbinds."""
        self.rig.set_vocabulary(voc, levelsup=levelsup, match=True)
        self._voc, self._voc_levelsup = voc, levelsup
        if voc is None:
            self.BoW_vecs, self.BoW_feats = [], []

    def setLfConfig(self, K_mats, R_mats, t_mats, total_feats=3000):
        """camconfig_ K / R / t for obtainLfFeatures (FrontEnd.cpp:213-593): after setVocabulary, extractFeaturesParallel() also
        fills intraMatches (IntraMatch with matchDesc, point3D, uv_ref, mono, n_rays), intramatch_size, mono_size, lfBoW and
        lfFeatVec as FrontEnd::processFrame leaves them (:1009-1024), made by the extraction job.  K_mats = None unbinds."""
        self.rig.set_lf(K_mats, R_mats, t_mats, total_feats)
        self._lf = K_mats is not None
        if not self._lf:
            self.intraMatches, self.intramatch_size, self.mono_size, self.lfBoW, self.lfFeatVec = [], 0, 0, None, None

    def setUndistorted(self, image_kps_undist):
        """image_kps_undist as UndistortKeyPoints (MultiCameraFrame.cpp:300-347) fills it for a distorted, unrectified rig
        (cv::undistortPoints is the caller's).  Read by BruteForceMatch's returned keypoints, the epipolar check of
        computeIntraMatches(old=True) and the BoW-guided matcher's |dy| < 50 gate.  Call after extractFeaturesParallel()."""
        if len(image_kps_undist) != self.num_cams_ or any(len(u) != len(k) for u, k in zip(image_kps_undist, self.image_kps)):
            raise ValueError("image_kps_undist must hold one entry per extracted keypoint")
        self.image_kps_undist = list(image_kps_undist)
        self._rows_replaced = True

    def _ensure_match(self, dist_thresh, ratio):
        key = (float(dist_thresh), float(ratio))
        if self._matched != key:
            self.rig.match(1, dist_thresh=dist_thresh, ratio=ratio)
            self._matched = key

    def BruteForceMatch(self, img1_ind, img2_ind, dist_thresh, neigh_ratio):
        """BruteForceMatch (MultiCameraFrame.cpp:1024-1086): returns indices_1, indices_2, kps1, kps2."""
        if not img1_ind < img2_ind:
            raise ValueError("the reference calls BruteForceMatch with cam1 < cam2 only")
        self._ensure_match(dist_thresh, neigh_ratio)
        i1, i2 = self.rig.pair_matches(0, img1_ind, img2_ind)
        return i1, i2, self.image_kps_undist[img1_ind][i1], self.image_kps_undist[img2_ind][i2]

    def computeIntraMatchesBoW(self, vocabulary, words_=None, levelsup=4):
        """computeIntraMatches(matches, words_) (MultiCameraFrame.cpp:586-943), the call FrontEnd.cpp:1009 makes.  The
        |dy| < 50 gate reads image_kps_undist (:708-716): set it with setUndistorted() when the rig is not rectified."""
        if vocabulary is self._voc and levelsup == self._voc_levelsup and not self._rows_replaced:
            tr, nr, words = self.rig.bow_tracks(0, 1)[0]   # made by the extraction job (setVocabulary)
        else:
            yu = [np.ascontiguousarray(k["y"], np.float32) for k in self.image_kps_undist]
            tr, nr, words = vocabulary.match_rig_frames(self.rig, 0, 1, levelsup=levelsup, y_undist=yu)[0]
        if words_ is not None:
            words_.extend(int(w) for w in words)
        out = [IntraMatch(row) for row in tr]
        for m, n in zip(out, nr):
            m.n_rays = int(n)
        return out

    def setCalibration(self, K_mats, R_mats, t_mats):
        """camconfig_.K_mats_/R_mats_/t_mats_: builds the per-pair fundamental matrices of
        MultiCameraFrame.cpp:1126-1142 (F = K_j^-T [t_ji]x R_ji K_i^-1 with T_ji = T_j0 T_i0^-1) in float64."""
        self.F_mats = np.stack([fundamental_from_extrinsics(K_mats[i], R_mats[i], t_mats[i], K_mats[j], R_mats[j], t_mats[j])
                                for i in range(self.num_cams_ - 1) for j in range(i + 1, self.num_cams_)])

    def computeIntraMatches(self, old=False, dist_thresh=75.0, ratio=0.85, kps_undist=None):
        """computeIntraMatches(matches, old) (MultiCameraFrame.cpp:1100-1288); old=True applies the epipolar
        check (:1178-1207) and needs setCalibration() or F_mats."""
        self._ensure_match(dist_thresh, ratio)
        if old:
            if getattr(self, "F_mats", None) is None:
                raise ValueError("computeIntraMatches(old=True) needs setCalibration(K, R, t) or F_mats")
            tr, mergeable = self.rig.tracks_epipolar(0, self.F_mats, kps_undist if kps_undist is not None else
                                                     (self.image_kps_undist if self.image_kps_undist is not self.image_kps else None))
        else:
            tr, mergeable = self.rig.tracks(0)
        self.cnt_mergable_matches = mergeable
        return [IntraMatch(row) for row in tr]
