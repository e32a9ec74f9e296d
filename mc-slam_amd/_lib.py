"""ctypes declarations for libmcorb.so (include/mcorb.h).

The library is the product: HIP kernels + host engine behind a C ABI.  There is
no Python or CPU fallback -- if the shared object is missing this module raises,
and if no gfx950 device is usable the C calls return MCORB_E_NODEVICE.
"""
import ctypes as C
import os
import sys

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libmcorb.so")

OK, E_EMPTY, E_SIZE, E_CAP, E_ARG, E_HIP, E_NODEVICE, E_STATE, E_OVERFLOW = 0, -1, -2, -3, -4, -5, -6, -7, -8
ORIENT_NONE, ORIENT_IC_ANGLE = 0, 1
BOW_TRANSFORM, BOW_MATCH = 1, 2
OBS_UPDATE, OBS_RECORD = 0, 1
MAX_LEVELS, MAX_CAMS = 16, 16
TRACK_KNN, TRACK_TILE = 10, 1024   # MCORB_TRACK_KNN, MCORB_TRACK_TILE
TRACK_MAX_FRAMES = 32               # MCORB_TRACK_MAX_FRAMES
POSE_LANES = 256                    # MCORB_POSE_LANES
INIT_MAX_MATCHES = 16384           # MCORB_INIT_MAX_MATCHES
INIT_DONE, INIT_BASELINE, INIT_PARALLAX, INIT_FEW = 0, 1, 2, 3   # MCORB_INIT_*
POSE_NO_OBS, POSE_NO_STEP, POSE_CONVERGED, POSE_MAX_ITER = 0, 1, 2, 3   # MCORB_POSE_*

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class Params(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int), ("orientation", C.c_int),
                ("device_id", C.c_int), ("host_threads", C.c_int), ("cand_cap", C.c_int), ("selection", C.c_int),
                ("gpu_jobs", C.c_int), ("reserved", C.c_int * 5)]


class Camera(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("Rt", C.c_double * 12)]


LF_DTYPE = np.dtype([("match_index", "<i4", (MAX_CAMS,)), ("uv_ref", "<f4", (2,)), ("mono", "<i4"), ("n_rays", "<i4"),
                     ("point3d", "<f8", (3,)), ("desc", "u1", (32,))])


class LmapCam(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("K", C.c_double * 9), ("centre_w", C.c_double * 3)]


class LmapView(C.Structure):
    _fields_ = [("Rcw", C.c_double * 9), ("tcw", C.c_double * 3), ("ncams", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("reserved", C.c_int32), ("cams", LmapCam * MAX_CAMS)]


class MapFrame(C.Structure):
    _fields_ = [("nfeat", C.c_int32), ("ncams", C.c_int32), ("match_index", C.c_void_p), ("kps_undist", C.POINTER(C.c_void_p)),
                ("nkps", C.c_void_p), ("centre_w", C.c_double * 3 * MAX_CAMS), ("proj", C.c_double * 12 * MAX_CAMS),
                ("twc", C.c_double * 3)]


class MapOut(C.Structure):
    _fields_ = [("cap_matches", C.c_int32), ("cap_depth", C.c_int32), ("inliers", C.c_void_p), ("verdict", C.c_void_p),
                ("new_lid", C.c_void_p), ("pt3d", C.c_void_p), ("normal", C.c_void_p), ("dist2", C.c_void_p),
                ("cos_parallax", C.c_void_p), ("neigh_skipped", C.c_void_p), ("depth_vec", C.c_void_p), ("n_matches", C.c_int32),
                ("n_depth", C.c_int32), ("n_triangulated", C.c_int32), ("next_lid", C.c_int32)]


class MapNewOut(C.Structure):
    _fields_ = [("cap_matches", C.c_int32), ("cap_depth", C.c_int32), ("inliers", C.c_void_p), ("verdict", C.c_void_p),
                ("new_lid", C.c_void_p), ("pt3d", C.c_void_p), ("normal", C.c_void_p), ("dist", C.c_void_p),
                ("cos_parallax", C.c_void_p), ("iterations", C.c_void_p), ("cost_initial", C.c_void_p), ("cost_final", C.c_void_p),
                ("depth_vec", C.c_void_p), ("avg_depth", C.c_double), ("n_rays_hist", C.c_int32 * MAX_CAMS),
                ("n_by_verdict", C.c_int32 * 9), ("n_matches", C.c_int32), ("n_depth", C.c_int32), ("n_triangulated", C.c_int32),
                ("next_lid", C.c_int32)]


class InitResultC(C.Structure):
    _fields_ = [("cap_matches", C.c_int32), ("status", C.c_int32), ("inliers", C.c_void_p), ("verdict", C.c_void_p),
                ("new_lid", C.c_void_p), ("pt3d", C.c_void_p), ("normal", C.c_void_p), ("dist2", C.c_void_p),
                ("cos_parallax", C.c_void_p), ("parallax", C.c_double), ("median_scene_depth", C.c_double), ("t_out", C.c_double * 3),
                ("n_matches", C.c_int32), ("n_initial_inliers", C.c_int32), ("n_parallax", C.c_int32), ("n_triangulated", C.c_int32),
                ("scaled", C.c_int32), ("next_lid", C.c_int32)]


class ObsFrame(C.Structure):
    _fields_ = [("kf_id", C.c_int32), ("nfeat", C.c_int32), ("ncams", C.c_int32), ("reserved", C.c_int32), ("match_index", C.c_void_p),
                ("centre_w", C.c_double * 3 * MAX_CAMS)]


class TrackCam(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("fx", C.c_double), ("fy", C.c_double), ("s", C.c_double),
                ("u0", C.c_double), ("v0", C.c_double)]


class TrackView(C.Structure):
    _fields_ = [("R0", C.c_double * 9), ("t0", C.c_double * 3), ("ncams", C.c_int32), ("cols", C.c_int32), ("rows", C.c_int32),
                ("reserved", C.c_int32), ("cams", TrackCam * MAX_CAMS)]


class TrackFrame(C.Structure):
    _fields_ = [("ncams", C.c_int32), ("reserved", C.c_int32), ("n_kp", C.c_int32 * MAX_CAMS), ("kp_xy", C.c_void_p * MAX_CAMS),
                ("desc", C.c_void_p * MAX_CAMS)]


class TrackOut(C.Structure):
    _fields_ = [("cap_proj", C.c_int32), ("cap_match", C.c_int32), ("proj_lid", C.c_void_p), ("proj_xy", C.c_void_p),
                ("best_kp", C.c_void_p), ("best_dist", C.c_void_p), ("match_kp", C.c_void_p), ("match_lid", C.c_void_p),
                ("match_dist", C.c_void_p), ("match_pt", C.c_void_p), ("n_proj", C.c_int32 * MAX_CAMS),
                ("n_match", C.c_int32 * MAX_CAMS), ("n_candidates", C.c_int32), ("reserved", C.c_int32)]


class PoseParams(C.Structure):
    _fields_ = [("inv_sigma2", C.c_double * MAX_LEVELS), ("nlevels", C.c_int32), ("max_iterations", C.c_int32)]


class PoseResultC(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("cost_initial", C.c_double), ("cost_final", C.c_double),
                ("status", C.c_int32), ("iterations", C.c_int32 * 2), ("n_inliers", C.c_int32), ("n_obs", C.c_int32),
                ("reserved", C.c_int32)]


class BAParams(C.Structure):
    _fields_ = [("sigma", C.c_double * MAX_LEVELS), ("nlevels", C.c_int32), ("max_iterations", C.c_int32)]


class BAResultC(C.Structure):
    _fields_ = [("cost_initial", C.c_double), ("cost_final", C.c_double), ("status", C.c_int32), ("iterations", C.c_int32),
                ("n_inliers", C.c_int32), ("n_obs", C.c_int32)]


BA_SPANS = 7


class RetriParams(C.Structure):
    _fields_ = [("rank_tol", C.c_double), ("landmark_distance_threshold", C.c_double), ("dynamic_outlier_threshold", C.c_double),
                ("max_diff", C.c_double), ("mode", C.c_int32), ("reserved", C.c_int32)]


RETRI_VERDICTS, RETRI_SPANS = 8, 2


class RetriResultC(C.Structure):
    _fields_ = [("counts", C.c_int32 * RETRI_VERDICTS), ("n_pairs", C.c_int32), ("launched", C.c_int32)]


class SacParams(C.Structure):
    _fields_ = [("threshold", C.c_double), ("seed", C.c_uint64), ("max_iterations", C.c_int32), ("solver", C.c_int32)]


class RelParams(C.Structure):
    _fields_ = [("threshold", C.c_double), ("seed", C.c_uint64), ("max_iterations", C.c_int32), ("reserved", C.c_int32)]


class RelResultC(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("status", C.c_int32), ("n_inliers", C.c_int32), ("n_matches", C.c_int32),
                ("best_hypothesis", C.c_int32), ("sample", C.c_int32 * 17), ("n_models", C.c_int32)]


class RelPolishParams(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("max_iterations", C.c_int32)]


class RelPolishRoundC(C.Structure):
    _fields_ = [("cost_initial", C.c_double), ("cost_final", C.c_double), ("n_members", C.c_int32), ("iterations", C.c_int32),
                ("status", C.c_int32), ("n_inliers", C.c_int32), ("accepted", C.c_int32), ("reserved", C.c_int32)]


class RelPolishC(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("round", RelPolishRoundC * 2), ("n_inliers", C.c_int32),
                ("rounds_run", C.c_int32)]


class EssParams(C.Structure):
    _fields_ = [("threshold_px", C.c_double), ("distance_thresh", C.c_double), ("seed", C.c_uint64), ("max_iterations", C.c_int32),
                ("reserved", C.c_int32)]


class EssResultC(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("E", C.c_double * 9), ("status", C.c_int32), ("n_matches", C.c_int32),
                ("n_ransac_inliers", C.c_int32), ("n_inliers", C.c_int32), ("best_hypothesis", C.c_int32), ("best_root", C.c_int32),
                ("sample", C.c_int32 * 5), ("n_models", C.c_int32), ("cheirality", C.c_int32 * 4), ("reserved", C.c_int32)]


class EssPolishParams(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("max_iterations", C.c_int32)]


class EssPolishRoundC(C.Structure):
    _fields_ = [("cost_initial", C.c_double), ("cost_final", C.c_double), ("n_members", C.c_int32), ("iterations", C.c_int32),
                ("status", C.c_int32), ("n_ransac_inliers", C.c_int32), ("n_inliers", C.c_int32), ("accepted", C.c_int32)]


class EssPolishC(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("E", C.c_double * 9), ("round", EssPolishRoundC * 2),
                ("n_ransac_inliers", C.c_int32), ("n_inliers", C.c_int32), ("rounds_run", C.c_int32), ("reserved", C.c_int32)]


class AlignParams(C.Structure):
    _fields_ = [("threshold", C.c_double), ("inlier_dist", C.c_double), ("seed", C.c_uint64), ("max_iterations", C.c_int32),
                ("mode", C.c_int32), ("refit", C.c_int32), ("reserved", C.c_int32)]


class AlignResultC(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("sac_R", C.c_double * 9), ("sac_t", C.c_double * 3),
                ("mean_error", C.c_double), ("status", C.c_int32), ("used", C.c_int32), ("n_inliers", C.c_int32),
                ("n_matches", C.c_int32), ("sac_n_inliers", C.c_int32), ("best_hypothesis", C.c_int32), ("sample", C.c_int32 * 3),
                ("n_models", C.c_int32)]


class SacResultC(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("sac_R", C.c_double * 9), ("sac_t", C.c_double * 3),
                ("status", C.c_int32), ("used", C.c_int32), ("n_inliers", C.c_int32), ("n_matches", C.c_int32),
                ("sac_n_inliers", C.c_int32), ("best_hypothesis", C.c_int32), ("sample", C.c_int32 * 4), ("n_models", C.c_int32),
                ("n_consensus", C.c_int32), ("refine", PoseResultC)]


class McorbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mcorb error %d: %s" % (code, msg))
        self.code = code


_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
_ip = C.POINTER(C.c_int)

# name -> (restype, argtypes); every symbol include/mcorb.h declares
SIGNATURES = {
    "mcorb_default_params": (None, [C.POINTER(Params)]),
    "mcorb_last_error": (C.c_char_p, []),
    "mcorb_version": (C.c_char_p, []),
    "mcorb_device_count": (_i, []),
    "mcorb_rig_create": (_i, [C.POINTER(Params), _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "mcorb_rig_destroy": (None, [_vp]),
    "mcorb_rig_upload_u8": (_i, [_vp, _i, C.POINTER(_vp), _i, _i]),
    "mcorb_rig_upload_f32": (_i, [_vp, _i, C.POINTER(_vp), _i, _i, _i]),
    "mcorb_rig_extract_submit": (_i, [_vp, _i, _i, _i, _i]),
    "mcorb_rig_extract_wait": (_i, [_vp, _i]),
    "mcorb_rig_extract": (_i, [_vp, _i, _i, _i, _i]),
    "mcorb_rig_staging": (_i, [_vp, _i, _i, _vp, _ip]),
    "mcorb_rig_upload_staged": (_i, [_vp, _i, _i]),
    "mcorb_rig_process_submit": (_i, [_vp, _i, _i, _i, _i, _f, _f]),
    "mcorb_rig_process": (_i, [_vp, _i, _i, _i, _i, _f, _f]),
    "mcorb_rig_process_wait": (_i, [_vp, _i]),
    "mcorb_rig_num_keypoints": (_i, [_vp, _i, _i]),
    "mcorb_rig_get_features": (_i, [_vp, _i, _i, _vp, _vp, _i, _ip, _ip]),
    "mcorb_rig_set_undistortion": (_i, [_vp, _i, _vp, _vp, _i]),
    "mcorb_rig_undistortion_active": (_i, [_vp, _i]),
    "mcorb_rig_get_features_undist": (_i, [_vp, _i, _i, _vp, _i, _ip]),
    "mcorb_rig_set_image_undistortion": (_i, [_vp, _i, _vp, _vp, _i]),
    "mcorb_rig_image_undistortion_active": (_i, [_vp, _i]),
    "mcorb_rig_get_undistort_map": (_i, [_vp, _i, _vp, _vp, _i]),
    "mcorb_rig_get_raw_image": (_i, [_vp, _i, _i, _vp, _i]),
    "mcorb_host_undistort_map": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "mcorb_host_remap_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i]),
    "mcorb_rig_match": (_i, [_vp, _i, _i, _f, _f]),
    "mcorb_rig_match_submit": (_i, [_vp, _i, _i, _f, _f]),
    "mcorb_rig_match_wait": (_i, [_vp, _i]),
    "mcorb_rig_get_pair_matches": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _ip]),
    "mcorb_rig_get_pair_knn2": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _ip]),
    "mcorb_rig_get_tracks": (_i, [_vp, _i, _i, _vp, _i, _ip, _ip]),
    "mcorb_rig_level_size": (_i, [_vp, _i, _ip, _ip]),
    "mcorb_rig_get_level": (_i, [_vp, _i, _i, _i, _vp, _i]),
    "mcorb_rig_get_blurred": (_i, [_vp, _i, _i, _i, _vp, _i]),
    "mcorb_rig_get_candidates": (_i, [_vp, _i, _i, _i, _vp, _i, _ip]),
    "mcorb_rig_last_timing": (_i, [_vp, _i, C.POINTER(_f)]),
    "mcorb_rig_select_mode": (_i, [_vp]),
    "mcorb_rig_select_fallbacks": (_i, [_vp, _i]),
    "mcorb_rig_early_reads_rejected": (_i, [_vp, _i]),
    "mcorb_rig_set_graph": (_i, [_vp, _i]),
    "mcorb_dev_sort_selftest": (_i, [_i, _vp, _i, _vp, _vp]),
    "mcorb_rig_match_pairs_external": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _f, _f]),
    "mcorb_rig_match_pairs_external_dev_submit": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _f, _f, _vp]),
    "mcorb_rig_get_pairlist": (_i, [_vp, _i, _i, _vp, _vp, _i, _ip]),
    "mcorb_host_merge_tracks": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _ip, _ip]),
    "mcorb_descblock_create": (_i, [_i, _i, _i, _vp]),
    "mcorb_descblock_destroy": (None, [_vp]),
    "mcorb_descblock_upload": (_i, [_vp, _i, _vp, _i]),
    "mcorb_descblock_desc_ptr": (_vp, [_vp]),
    "mcorb_descblock_counts_dev": (_vp, [_vp]),
    "mcorb_rig_match_sets": (_i, [_vp, _i, _vp, _vp, _i, _f, _f]),
    "mcorb_rig_get_pairknn2": (_i, [_vp, _i, _i, _vp, _vp, _i, _ip]),
    "mcorb_rig_kcap": (_i, [_vp]),
    "mcorb_rig_host_threads": (_i, [_vp]),
    "mcorb_rig_info": (_i, [_vp, _vp]),
    "mcorb_rig_desc_device_ptr": (_vp, [_vp, _i]),
    "mcorb_rig_stream": (_vp, [_vp, _i]),
    "mcorb_rig_export_descriptors": (_i, [_vp, _i, _vp, _vp, _i]),
    "mcorb_rig_match_external": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _f, _f]),
    "mcorb_rig_match_external_submit": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _f, _f]),
    "mcorb_rig_export_descriptors_dev": (_i, [_vp, _i, _vp, _vp, _i, _vp]),
    "mcorb_rig_match_external_dev_submit": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _f, _f, _vp]),
    "mcorb_create": (_i, [C.POINTER(Params), _i, _i, C.POINTER(_vp)]),
    "mcorb_destroy": (None, [_vp]),
    "mcorb_extract": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _ip, _ip]),
    "mcorb_extract_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _ip, _ip]),
    "mcorb_get_tables": (_i, [C.POINTER(Params), _vp, _vp, _vp, _vp, _vp]),
    "mcorb_get_pyramid_level": (_i, [_vp, _i, _vp, _i, _ip, _ip]),
    "mcorb_hamming256": (_i, [_vp, _vp]),
    "mcorb_representative_desc": (_i, [_vp, _i]),
    "mcorb_knn2": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "mcorb_match_ratio": (_i, [_vp, _vp, _i, _vp, _i, _f, _f, _vp, _vp, _i, _ip]),
    "mcorb_vocab_create": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_vp)]),
    "mcorb_vocab_load_text": (_i, [C.c_char_p, _i, C.POINTER(_vp)]),
    "mcorb_vocab_destroy": (None, [_vp]),
    "mcorb_vocab_info": (_i, [_vp, _ip, _ip, _ip, _ip]),
    "mcorb_vocab_transform": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _ip, _vp, _vp, _i, _ip, _vp, _i]),
    "mcorb_rig_transform_image": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _i, _ip, _vp, _vp, _i, _ip, _vp, _i]),
    "mcorb_rig_get_tracks_epipolar": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _ip, _ip]),
    "mcorb_rig_match_bow": (_i, [_vp, _i, _i, _vp, _i, C.c_double, _vp, _vp, _i, _ip, _vp, _i, _ip]),
    "mcorb_rig_transform_images": (_i, [_vp, _i, _i, _i, _vp, _i]),
    "mcorb_rig_get_transform": (_i, [_vp, _i, _i, _vp, _vp, _i, _ip, _vp, _vp, _i, _ip, _vp, _i]),
    "mcorb_rig_match_bow_frames": (_i, [_vp, _i, _i, _i, _vp, _i, C.c_double, _vp]),
    "mcorb_rig_set_vocabulary": (_i, [_vp, _vp, _i, C.c_double, _i]),
    "mcorb_rig_get_bow_tracks": (_i, [_vp, _i, _i, _vp, _vp, _i, _ip, _vp, _i, _ip]),
    "mcorb_rig_obtain_lf_features": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _ip, _ip, _ip, _vp, _i, _ip]),
    "mcorb_rig_obtain_lf_features_frames": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "mcorb_host_select": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i]),
    "mcorb_host_resize_axis": (_i, [_i, _i, _i, _vp]),
    "mcorb_host_triangulate": (_i, [_vp, _vp, _i, _vp]),
    "mcorb_host_triangulate_branch": (_i, [_vp, _vp, _i, _vp, _vp]),
    "mcorb_rig_set_lf": (_i, [_vp, _vp, _i]),
    "mcorb_rig_get_lf_features": (_i, [_vp, _i, _i, _vp, _i, _ip, _ip, _ip, _vp, _i, _ip]),
    "mcorb_rig_get_lf_bow": (_i, [_vp, _i, _i, _vp, _vp, _i, _ip, _vp, _vp, _i, _ip, _vp, _i]),
    "mcorb_dev_triangulate_selftest": (_i, [_i, _vp, _vp, _vp, _i, _vp, _vp]),
    "mcorb_kfdb_create": (_i, [_vp, _i, _i, _i, _i, C.POINTER(_vp)]),
    "mcorb_kfdb_destroy": (None, [_vp]),
    "mcorb_kfdb_add": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _ip]),
    "mcorb_kfdb_add_rig_frame": (_i, [_vp, _vp, _i, _i, _ip]),
    "mcorb_kfdb_size": (_i, [_vp]),
    "mcorb_kfdb_get_entry": (_i, [_vp, _i, _vp, _vp, _i, _ip, _vp, _vp, _i, _ip, _vp, _i, _vp, _i, _ip]),
    "mcorb_kfdb_query": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _ip]),
    "mcorb_kfdb_query_entries": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "mcorb_kfdb_score": (_i, [_vp, _i, _i, C.POINTER(C.c_double)]),
    "mcorb_kfdb_feature_matches": (_i, [_vp, _i, _i, C.c_double, _vp, _vp, _i, _ip]),
    "mcorb_kfdb_last_timing": (_i, [_vp, C.POINTER(_f)]),
    "mcorb_kfdb_reserve_probes": (_i, [_vp, _i]),
    "mcorb_kfdb_set_probe": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i]),
    "mcorb_kfdb_set_probe_rig_frame": (_i, [_vp, _i, _vp, _i, _i]),
    "mcorb_kfdb_get_probe": (_i, [_vp, _i, _vp, _vp, _i, _ip, _vp, _vp, _i, _ip, _vp, _i, _vp, _i, _ip]),
    "mcorb_kfdb_query_probes": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "mcorb_kfdb_score_probe": (_i, [_vp, _i, _i, C.POINTER(C.c_double)]),
    "mcorb_kfdb_probe_feature_matches": (_i, [_vp, _i, _vp, _i, C.c_double, _vp, _vp, _i, _vp]),
    "mcorb_kfdb_probe_inter_matches_bf": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _ip]),
    "mcorb_kfdb_last_probe_timing": (_i, [_vp, C.POINTER(_f)]),
    "mcorb_lmap_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "mcorb_lmap_destroy": (None, [_vp]),
    "mcorb_lmap_set": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mcorb_lmap_set_desc_from_entry": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp]),
    "mcorb_lmap_get": (_i, [_vp, _i, _vp, _vp, _vp, _ip, _ip]),
    "mcorb_lmap_search": (_i, [_vp, C.POINTER(LmapView), _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, C.c_double, _vp, _vp, _i, _ip,
                               _vp, _vp, _i, _ip, _vp, _vp, _i, _ip]),
    "mcorb_lmap_last_timing": (_i, [_vp, C.POINTER(_f), _ip]),
    "mcorb_lmap_triangulate_neighbours": (_i, [_vp, C.POINTER(MapFrame), _vp, C.POINTER(MapFrame), C.POINTER(_vp), _i, C.POINTER(_vp),
                                               C.POINTER(_vp), C.POINTER(_vp), _vp, _vp, _vp, _i, _vp, _vp, C.c_int32,
                                               C.POINTER(MapOut)]),
    "mcorb_lmap_depths": (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
    "mcorb_lmap_last_triangulate_timing": (_i, [_vp, C.POINTER(_f), _ip, _ip]),
    "mcorb_lmap_triangulate_new": (_i, [_vp, C.POINTER(MapFrame), _vp, C.POINTER(MapFrame), _vp, _vp, _vp, _i, _vp, _vp, _i, _i,
                                        C.POINTER(MapNewOut)]),
    "mcorb_lmap_last_triangulate_new_timing": (_i, [_vp, C.POINTER(_f), _ip]),
    "mcorb_host_map_refine": (_i, [_i] + [_vp] * 11 + [_i] + [_vp] * 5),
    "mcorb_dev_map_refine_selftest": (_i, [_i, _i] + [_vp] * 11 + [_i] + [_vp] * 5),
    "mcorb_lmap_initialize": (_i, [_vp, C.POINTER(MapFrame), _vp, C.POINTER(MapFrame), _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i,
                                   C.c_int32, C.c_double, C.POINTER(InitResultC)]),
    "mcorb_lmap_last_initialize_timing": (_i, [_vp, C.POINTER(_f), _ip]),
    "mcorb_host_init_cases": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp,
                                   C.POINTER(InitResultC)]),
    "mcorb_dev_init_cases_selftest": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, C.c_double, _vp, _vp, _vp,
                                           _vp, _vp, C.POINTER(InitResultC)]),
    "mcorb_host_map_gates": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "mcorb_dev_map_gates_selftest": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "mcorb_lmap_set_rays": (_i, [_vp, _vp, _i, _vp]),
    "mcorb_lmap_get_observations": (_i, [_vp, _i, C.POINTER(C.c_int32), _vp, _vp, _i, _ip]),
    "mcorb_lmap_observe": (_i, [_vp, C.POINTER(ObsFrame), _vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "mcorb_lmap_update_points": (_i, [_vp, _vp, _i, _vp, C.c_double, _vp, _vp]),
    "mcorb_lmap_delete": (_i, [_vp, _vp, _i, _vp, _vp, _i, _ip]),
    "mcorb_lmap_observers": (_i, [_vp, _vp, _i, _vp, _i, _ip]),
    "mcorb_lmap_last_landmark_timing": (_i, [_vp, C.POINTER(_f)]),
    "mcorb_lmap_track": (_i, [_vp, C.POINTER(TrackView), C.POINTER(TrackFrame), _vp, _i, C.c_double, _i, C.POINTER(TrackOut)]),
    "mcorb_lmap_track_rig_frame": (_i, [_vp, C.POINTER(TrackView), _vp, _i, _i, _vp, _i, C.c_double, _i, C.POINTER(TrackOut)]),
    "mcorb_lmap_last_track_timing": (_i, [_vp, C.POINTER(_f)]),
    "mcorb_lmap_last_track_timing4": (_i, [_vp, C.POINTER(_f)]),
    "mcorb_lmap_last_track_timing5": (_i, [_vp, C.POINTER(_f)]),
    "mcorb_lmap_track_submit": (_i, [_vp, C.POINTER(TrackView), C.POINTER(TrackFrame), _vp, _i, C.c_double, _i, _i]),
    "mcorb_lmap_track_rig_frame_submit": (_i, [_vp, C.POINTER(TrackView), _vp, _i, _i, _vp, _i, C.c_double, _i, _i]),
    "mcorb_lmap_track_wait": (_i, [_vp, C.POINTER(TrackOut)]),
    "mcorb_lmap_track_rig_frames_submit": (_i, [_vp, C.POINTER(TrackView), _vp, _i, _vp, _i, _vp, _vp, C.c_double, _i, _i]),
    "mcorb_lmap_track_frames_wait": (_i, [_vp, C.POINTER(TrackOut), _i]),
    "mcorb_lmap_track_rig_frames": (_i, [_vp, C.POINTER(TrackView), _vp, _i, _vp, _i, _vp, _vp, C.c_double, _i, _i, C.POINTER(TrackOut)]),
    "mcorb_host_track_pixel": (C.c_int32, [_f]),
    "mcorb_lmap_refine_pose": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(PoseParams), C.POINTER(PoseResultC), _vp]),
    "mcorb_lmap_last_pose_timing": (_i, [_vp, C.POINTER(_f)]),
    "mcorb_lmap_set_track_refine": (_i, [_vp, C.POINTER(PoseParams)]),
    "mcorb_lmap_last_track_pose": (_i, [_vp, _i, C.POINTER(PoseResultC), _vp, _i]),
    "mcorb_pose_of_view": (None, [C.POINTER(TrackView), _vp, _vp]),
    "mcorb_pose_eval": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcorb_lmap_bundle_adjust": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(BAParams),
                                      _vp, _vp, _vp, C.POINTER(BAResultC), _vp]),
    "mcorb_lmap_last_ba_timing": (_i, [_vp, C.POINTER(_f), C.POINTER(C.c_int32)]),
    "mcorb_ba_eval": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcorb_lmap_retriangulate": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, C.POINTER(RetriParams), _vp, _vp, _vp,
                                      _vp, C.POINTER(RetriResultC), _vp, _vp, _i]),
    "mcorb_lmap_last_retri_timing": (_i, [_vp, C.POINTER(_f)]),
    "mcorb_lmap_ransac_pose": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, C.POINTER(SacParams), C.POINTER(PoseParams),
                                    C.POINTER(SacResultC), _vp]),
    "mcorb_lmap_last_ransac_timing": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "mcorb_lmap_last_ransac_counts": (_i, [_vp, _vp, _vp, _i, C.POINTER(_i)]),
    "mcorb_sac_threshold": (C.c_double, [C.c_double]),
    "mcorb_sac_solve": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mcorb_sac_solve_rig": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcorb_sac_eval": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcorb_host_sac_rig_roots": (_i, [_i] + [_vp] * 10),
    "mcorb_dev_sac_solve_selftest": (_i, [_i, _i] + [_vp] * 6),
    "mcorb_dev_sac_solve_rig_selftest": (_i, [_i, _i, _i] + [_vp] * 11),
    "mcorb_dev_rel_solve_selftest": (_i, [_i, _i, _i] + [_vp] * 8),
    "mcorb_dev_ess_solve_selftest": (_i, [_i, _i] + [_vp] * 6),
    "mcorb_dev_align_solve_selftest": (_i, [_i, _i] + [_vp] * 8),
    "mcorb_lmap_relative_pose": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, C.POINTER(RelParams), C.POINTER(RelResultC), _vp]),
    "mcorb_lmap_last_relative_timing": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "mcorb_lmap_last_relative_counts": (_i, [_vp, _vp, _vp, _i, C.POINTER(_i)]),
    "mcorb_rel_threshold": (C.c_double, [C.c_double]),
    "mcorb_rel_solve": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcorb_rel_eval": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcorb_lmap_relative_pose_polished": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, C.POINTER(RelParams), C.POINTER(RelPolishParams),
                                               C.POINTER(RelResultC), _vp, C.POINTER(RelPolishC)]),
    "mcorb_lmap_last_relative_timing4": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "mcorb_rel_polish_run": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.POINTER(RelPolishParams),
                                  C.POINTER(RelPolishC), _vp, _vp, _vp]),
    "mcorb_lmap_essential_pose": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(EssParams), C.POINTER(EssResultC), _vp]),
    "mcorb_lmap_last_essential_timing": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "mcorb_lmap_last_essential_counts": (_i, [_vp, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    "mcorb_lmap_essential_pose_polished": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(EssParams), C.POINTER(EssPolishParams),
                                                C.POINTER(EssResultC), _vp, C.POINTER(EssPolishC)]),
    "mcorb_lmap_last_essential_timing5": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "mcorb_ess_polish_run": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.POINTER(EssPolishParams),
                                  C.POINTER(EssPolishC), _vp, _vp, _vp, _vp]),
    "mcorb_ess_solve": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mcorb_ess_eval": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "mcorb_ess_decompose": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "mcorb_lmap_align_pose": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(AlignParams), C.POINTER(AlignResultC), _vp]),
    "mcorb_lmap_last_align_timing": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "mcorb_lmap_last_align_counts": (_i, [_vp, _vp, _vp, _i, C.POINTER(_i)]),
    "mcorb_align_solve": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcorb_align_eval": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "mcorb_host_geometry": (_i, [C.POINTER(Params), _i, _i, _vp]),
    "mcorb_synth_rig_frame": (_i, [C.c_uint32, _i, _i, _i, _i, _vp, _i]),
}

_lib = None
LOADED_BEFORE_TORCH = False   # libmcorb.so (and with it /opt/rocm's HIP runtime) entered the process before torch did


def require_torch_first(what):
    """The stream-ordered multi-GPU calls exchange device pointers and HIP stream handles with torch (tensors of the collective,
    torch.cuda.Stream().cuda_stream).  That only works when both sides use ONE HIP runtime, which is the case when torch -- which
    ships its own libamdhip64 -- is imported BEFORE libmcorb.so is loaded: libmcorb then binds to the runtime
    already in the process.  The other order gives two runtimes whose handles mean nothing to each other; instead of letting
    that surface as a hang or an 'invalid resource handle' three calls later, refuse here."""
    if LOADED_BEFORE_TORCH and "torch" in sys.modules:
        raise RuntimeError("mc-slam_amd: %s was called with a torch-owned stream / tensor, but libmcorb.so was loaded before torch was "
                           "imported in this process: `import torch` first, then `import mcorb` (INTEGRATION.md section 5)" % what)


def load():
    """Load libmcorb.so; raises if it has not been built (no fallback path exists)."""
    global _lib, LOADED_BEFORE_TORCH
    if _lib is not None:
        return _lib
    LOADED_BEFORE_TORCH = "torch" not in sys.modules
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmcorb.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                          "g.build()'` or `make -C mc-slam_amd/csrc` (hipcc, gfx950). There is no CPU fallback."
                          % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)   # AttributeError here means the .so is stale
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(code):
    if code != OK:
        raise McorbError(code, load().mcorb_last_error().decode("utf-8", "replace"))
    return code


def default_params(**kw):
    p = Params()
    load().mcorb_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p
