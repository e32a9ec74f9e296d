/*
 * mcorb.h -- C ABI of libmcorb, the MI355X (gfx950) multi-camera ORB front-end.
 *
 * Drop-in boundary for MC-SLAM's hot path.  Every entry point
 * names the reference interface it replaces (paths relative to the MC-SLAM
 * checkout).  Plain pointers and sizes only; no C++ types, no exceptions; every
 * call returns a status code (0 ok, <0 error) unless stated otherwise.
 *
 * All compute runs in hand-written HIP kernels on the selected device; the
 * library has no CPU fallback and fails with MCORB_E_NODEVICE / MCORB_E_HIP
 * when no gfx950 device can be used.  The one host-side stage is the quad-tree
 * keypoint selection (DistributeOctTree), which the reference's own design
 * makes serial and order-defining; it runs on a host worker pool between two
 * GPU phases (DESIGN.md "Selection").
 */
#ifndef MCORB_H
#define MCORB_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCORB_OK 0
#define MCORB_E_EMPTY (-1)     /* empty image: the reference's `return -1` (ORBextractor.cpp:1090-1091) */
#define MCORB_E_SIZE (-2)      /* image too small / too tall: the reference's cell or root-node
                                  arithmetic would divide by zero (ORBextractor.cpp:558,799-802) */
#define MCORB_E_CAP (-3)       /* caller buffer too small */
#define MCORB_E_ARG (-4)       /* bad argument */
#define MCORB_E_HIP (-5)       /* HIP runtime error, see mcorb_last_error() */
#define MCORB_E_NODEVICE (-6)  /* no usable gfx950 device */
#define MCORB_E_STATE (-7)     /* call out of order (e.g. match before extract) */
#define MCORB_E_OVERFLOW (-8)  /* a sparse level's candidate list does not fit the host buffer (raise cand_cap) */

#define MCORB_MAX_LEVELS 16
#define MCORB_MAX_CAMS 16      /* IntraMatch::matchIndex is array<int,5> in the reference
                                  (MultiCameraFrame.h:44); widened here for the 8-camera rig */
/* DistributeOctTree (ORBextractor.cpp:554-778) after the GPU bucketing: HOST = worker threads between two GPU phases (needs ~10 cores
 * per GPU at full rate); GPU = one wave per (image, level), the whole job is one submission and the host only reads results
 * (levels whose tree goes below the bucketing depth -- clustered corners -- fall back to the host stage for that batch).
 * AUTO = GPU, unless the environment says MCORB_SELECT=host|gpu. */
#define MCORB_SELECT_AUTO 0
#define MCORB_SELECT_HOST 1
#define MCORB_SELECT_GPU 2
#define MCORB_ORIENT_NONE 0    /* reference behaviour: angle = 0 (ORBextractor.cpp:475) */
#define MCORB_ORIENT_IC_ANGLE 1 /* the reference's dormant IC_Angle (ORBextractor.cpp:75-102) */

/* Field order is bit-compatible with cv::KeyPoint (pt.x, pt.y, size, angle,
 * response, octave, class_id), the element type of the reference's outputs. */
typedef struct mcorb_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} mcorb_keypoint;

/* Constructor arguments of ORBextractor (ORBextractor.h:49-50) plus placement. */
typedef struct mcorb_params {
    int nfeatures;        /* ORBextractor.nFeatures */
    float scale_factor;   /* ORBextractor.scaleFactor */
    int nlevels;          /* ORBextractor.nLevels, 1..MCORB_MAX_LEVELS */
    int ini_th_fast;      /* ORBextractor.iniThFAST */
    int min_th_fast;      /* ORBextractor.minThFAST */
    int orientation;      /* MCORB_ORIENT_* */
    int device_id;        /* HIP device ordinal */
    int host_threads;     /* selection workers; 0 = one per camera image, capped at hw concurrency */
    int cand_cap;         /* host-side candidate slots per image (the device list is sized for the worst case);
                             only sparse levels are copied to the host; 0 = default (max(65536, w*h/4)) */
    int selection;        /* MCORB_SELECT_*: where DistributeOctTree's list discipline runs (0 = default) */
    int gpu_jobs;         /* at most this many slots' jobs on the GPU at once; further slots wait for a turn while the finished
                             ones are post-processed on the host (0 = no limit: every slot's job goes straight to the GPU) */
    int reserved[5];
} mcorb_params;

void mcorb_default_params(mcorb_params *p);   /* 2000, 1.2, 8, 20, 7, none, dev 0 */
const char *mcorb_last_error(void);           /* thread-local message of the last failure */
const char *mcorb_version(void);
/* number of visible HIP devices whose arch is gfx950 (does not create a context) */
int mcorb_device_count(void);

/* ------------------------------------------------------------------------- */
/* Rig engine: one object per GPU, handles a batch of equally sized images    */
/* (cameras x frames).  Replaces MultiCameraFrame's extract + intra-rig match */
/* members (MultiCameraFrame.h:73-90) and the frame hand-off of               */
/* MultiCameraFrame::setData (MultiCameraFrame.cpp:95-152).                   */
/* ------------------------------------------------------------------------- */
typedef struct mcorb_rig mcorb_rig;

/* ncams cameras of width x height; up to max_frames rig frames per batch
 * (images are indexed m = frame*ncams + cam); nslots >= 1 independent buffer
 * sets so that batches can be in flight concurrently (submit/wait below). */
int mcorb_rig_create(const mcorb_params *p, int ncams, int width, int height, int max_frames,
                     int nslots, mcorb_rig **out);
void mcorb_rig_destroy(mcorb_rig *r);

/* Stage `nimg` 8-bit gray images (host, stride bytes per row) into slot's
 * level-0 planes through pinned buffers + hipMemcpyAsync.  Replaces the u8 end
 * of the hand-off (MultiCameraFrame.cpp:108-140). */
int mcorb_rig_upload_u8(mcorb_rig *r, int slot, const uint8_t *const *images, int nimg, int stride);
/* Zero-copy variant of the hand-off: the reader decodes straight into the slot's pinned staging buffer
 * (image m: *ptr, W bytes per row, H rows) and mcorb_rig_upload_staged starts the DMA of images 0..nimg-1.
 * This is the "pinned hipMemcpyAsync" staging of DatasetReader::loadNext's cv::imread target
 * (MCDataUtils/src/DatasetReader.cpp:688-719) without the intermediate clone. */
int mcorb_rig_staging(mcorb_rig *r, int slot, int m, uint8_t **ptr, int *stride);
int mcorb_rig_upload_staged(mcorb_rig *r, int slot, int nimg);
/* Same for the reference's staging format: CV_32F in [0,1], 1 or 3 (BGR)
 * channels (DatasetReader.cpp:699-712); x255, round-half-even, saturate and
 * BGR2GRAY run on the device. */
int mcorb_rig_upload_f32(mcorb_rig *r, int slot, const float *const *images, int nimg,
                         int stride_bytes, int channels);

/* extractFeaturesParallel (MultiCameraFrame.cpp:203-262) for the `nimg` images
 * already resident in `slot`: pyramid, FAST, selection, blur, descriptors.
 * lap_x0/lap_x1 = vLappingArea (ORBextractor.cpp:1153), {0,0} in the reference.
 * submit returns once the first GPU phase is enqueued; wait blocks until
 * keypoints and descriptors of the slot are complete on host and device. */
int mcorb_rig_extract_submit(mcorb_rig *r, int slot, int nimg, int lap_x0, int lap_x1);
int mcorb_rig_extract_wait(mcorb_rig *r, int slot);
/* submit + wait */
int mcorb_rig_extract(mcorb_rig *r, int slot, int nimg, int lap_x0, int lap_x1);

/* One pass of the whole hot path for `nframes` rig frames (nframes*ncams images
 * resident in the slot): extraction as above, then the intra-rig match below,
 * with a single device synchronisation at the end. */
int mcorb_rig_process_submit(mcorb_rig *r, int slot, int nframes, int lap_x0, int lap_x1,
                             float dist_thresh, float ratio);
int mcorb_rig_process_wait(mcorb_rig *r, int slot);
/* the same, synchronously on the calling thread (lowest latency for one frame at a time) */
int mcorb_rig_process(mcorb_rig *r, int slot, int nframes, int lap_x0, int lap_x1, float dist_thresh, float ratio);

/* results of image m of a slot: ORBextractor::operator() outputs
 * (ORBextractor.cpp:1085-1171): keypoints, N x 32 descriptors, monoIndex */
int mcorb_rig_num_keypoints(mcorb_rig *r, int slot, int m);
int mcorb_rig_get_features(mcorb_rig *r, int slot, int m, mcorb_keypoint *kps, uint8_t *desc, int cap,
                           int *n_out, int *mono_index_out);

/* MultiCameraFrame::UndistortKeyPoints (MultiCameraFrame.cpp:300-347) on the device, inside every extraction job: for a camera
 * with undistortion set, k_undistort runs cv::undistortPoints(pts, pts, K, dist, noArray(), K) (OpenCV 4.x, 5 fixed iterations,
 * fp64, no contraction) on every keypoint the job selects, and the result comes back with the job.  K (3x3 row-major) and dist are
 * camconfig's CV_64F values; both go through float as in the reference (:324-325).  ncoeffs: 4, 5, 8 or 12; dist == NULL or
 * ncoeffs == 0 clears the camera.  MCORB_E_ARG: bad camera, count (14, the tilt model, included) or a non-finite / zero fx, fy;
 * MCORB_E_STATE while any slot has a job submitted and not yet waited for.  With no camera set a job is exactly what it is
 * without this call.
 * The reference's zero test, quirk included: it passes a camera through unchanged when dist_coeffs_[cam].at<float>(0) == 0.0 on
 * the CV_64F Mat (:302), i.e. when the LOW 32 BITS of the double k1 are a float zero -- true for k1 == 0, and also for short binary
 * values such as k1 = -0.25 whatever the other coefficients say.  mcorb_rig_undistortion_active reports that decision: 1 if the
 * reference would call undistortPoints for the camera, 0 if it copies (camera not set, or passed through). */
int mcorb_rig_set_undistortion(mcorb_rig *r, int cam, const double *K, const double *dist, int ncoeffs);
int mcorb_rig_undistortion_active(mcorb_rig *r, int cam);
/* image_kps_undist of image m (m = frame*ncams + cam): the records of mcorb_rig_get_features with x, y replaced (:336-344); for a
 * camera that is not set or passed through, the raw records.  MCORB_E_STATE for an image not extracted since the last
 * mcorb_rig_set_undistortion.  With undistortion set for any camera, the consumers below that take an undistorted set
 * (mcorb_rig_get_tracks_epipolar's kps_undist, mcorb_rig_match_bow_frames' y_undist, mcorb_rig_obtain_lf_features(_frames)'
 * kps_undist) read this set where the caller passes NULL (as a whole or per entry), and so does mcorb_rig_match_bow; an explicit
 * pointer still wins.  With nothing set they read the raw keypoints, as without this feature. */
int mcorb_rig_get_features_undist(mcorb_rig *r, int slot, int m, mcorb_keypoint *kps, int cap, int *n_out);

/* The RECTIFY branch of MultiCameraFrame::setData (MultiCameraFrame.cpp:123-136) on the device, at the hand-off: for a camera with
 * image undistortion set, every upload form (u8, staged, f32) lands the plane in a raw buffer and k_remap_u8 writes
 * cv::undistort(img, undistImg, K, dist) into level 0 of the pyramid behind the copies, so a job -- and a job re-run on the
 * resident images -- reads the undistorted image and mcorb_rig_get_level(.., 0, ..) returns it.  The fixed-point map of
 * cv::undistort (OpenCV 4.x: stripes of min(max(1, 4096 / w), h) rows, initUndistortRectifyMap to CV_16SC2 per stripe, all in
 * fp64 without contraction) is built once per camera on the host by this call; the per-frame work is the resampling,
 * remap(INTER_LINEAR, BORDER_CONSTANT 0).  K (3x3 row-major) and dist are camconfig's CV_64F values, used as they are.
 * ncoeffs: 4, 5, 8 or 12; dist == NULL or ncoeffs == 0 clears the camera (cameras not set are copied through).  There is no zero
 * test: the reference calls cv::undistort for all-zero coefficients too.  MCORB_E_ARG: bad camera, count (14, the tilt model,
 * included), non-finite values or a zero fx, fy.  MCORB_E_STATE while any slot has a job submitted and not yet waited for.
 * RECTIFY is rig-wide in the reference and excludes UndistortKeyPoints (image_kps_undist is then the raw keypoint set, :241-242):
 * this call returns MCORB_E_STATE while any camera has keypoint undistortion set, and mcorb_rig_set_undistortion returns it while
 * any camera has image undistortion set.  A rig that never sets it allocates nothing and uploads exactly as before.
 * mcorb_rig_image_undistortion_active: 1 if the camera is set, else 0. */
int mcorb_rig_set_image_undistortion(mcorb_rig *r, int cam, const double *K, const double *dist, int ncoeffs);
int mcorb_rig_image_undistortion_active(mcorb_rig *r, int cam);
/* test hooks: the camera's maps as built on the host (map1_xy: width * height (x, y) pairs, map2: width * height; cap_pixels >=
 * width * height; MCORB_E_STATE for a camera not set), and the raw plane of image m as uploaded (MCORB_E_STATE on a rig that never
 * set image undistortion; meaningful for images uploaded while it was set) */
int mcorb_rig_get_undistort_map(mcorb_rig *r, int cam, int16_t *map1_xy, uint16_t *map2, int cap_pixels);
int mcorb_rig_get_raw_image(mcorb_rig *r, int slot, int m, uint8_t *dst, int dst_stride);
/* the two halves alone, on the host, no device: the map of a w x h image, and remap(INTER_LINEAR, BORDER_CONSTANT 0) under a map */
int mcorb_host_undistort_map(const double *K, const double *dist, int ncoeffs, int w, int h, int16_t *map1_xy, uint16_t *map2);
int mcorb_host_remap_u8(const uint8_t *src, int src_stride, int w, int h, const int16_t *map1_xy, const uint16_t *map2,
                        uint8_t *dst, int dst_stride);

/* computeIntraMatches(matches, false) (MultiCameraFrame.cpp:1100-1288) for the
 * first `nframes` rig frames of a slot: BruteForceMatch(i, j, dist_thresh,
 * ratio) for all i<j on the GPU (all-pairs Hamming k-NN, k = 2), then the
 * reference's track merge on the host. */
int mcorb_rig_match(mcorb_rig *r, int slot, int nframes, float dist_thresh, float ratio);
int mcorb_rig_match_submit(mcorb_rig *r, int slot, int nframes, float dist_thresh, float ratio);
int mcorb_rig_match_wait(mcorb_rig *r, int slot);
/* BruteForceMatch outputs of pair (cam_i < cam_j) of a frame: indices_1/2
 * (MultiCameraFrame.cpp:1070-1071); kps1/kps2 are kps[idx] of the two images */
int mcorb_rig_get_pair_matches(mcorb_rig *r, int slot, int frame, int cam_i, int cam_j,
                               uint32_t *idx1, uint32_t *idx2, int cap, int *n_out);
/* raw knnMatch(k=2) table of the pair, nq x 2 (trainIdx, distance); -1 = absent */
int mcorb_rig_get_pair_knn2(mcorb_rig *r, int slot, int frame, int cam_i, int cam_j,
                            int32_t *idx, int32_t *dist, int cap_rows, int *nq_out);
/* IntraMatch tracks of a frame: ntracks x ncams matchIndex rows, -1 = absent;
 * mergeable = cnt_mergable_matches (MultiCameraFrame.cpp:1256) */
int mcorb_rig_get_tracks(mcorb_rig *r, int slot, int frame, int32_t *tracks, int cap_tracks,
                         int *ntracks_out, int *mergeable_out);

/* computeIntraMatches(matches, old=true) (MultiCameraFrame.cpp:1123-1143,1178-1207): the same merge as
 * mcorb_rig_get_tracks with the epipolar check applied to every BruteForceMatch pair first.
 * F: one row-major 3x3 per camera pair (i<j in the order (0,1),(0,2)..), x_j^T F x_i = 0 -- the matrix
 * the reference builds from K_mats_/R_mats_/t_mats_ (:1126-1142); that cv::Mat algebra stays with the
 * caller (include/mcorb_adapter.hpp does it with cv:: when OpenCV is there).  kps_undist[c]: the camera's
 * image_kps_undist (pt and octave are read), NULL = the extracted keypoints (no distortion). */
int mcorb_rig_get_tracks_epipolar(mcorb_rig *r, int slot, int frame, const double *F, const mcorb_keypoint *const *kps_undist,
                                  int32_t *tracks, int cap_tracks, int *ntracks_out, int *mergeable_out);

/* intermediates for stage-by-stage parity tests (device -> host copies) */
int mcorb_rig_level_size(mcorb_rig *r, int level, int *w, int *h);
int mcorb_rig_get_level(mcorb_rig *r, int slot, int m, int level, uint8_t *dst, int dst_stride);
int mcorb_rig_get_blurred(mcorb_rig *r, int slot, int m, int level, uint8_t *dst, int dst_stride);
/* vToDistributeKeys of a level (ORBextractor.cpp:793-871): packed (y<<20 | x<<8 | response) */
int mcorb_rig_get_candidates(mcorb_rig *r, int slot, int m, int level, uint32_t *packed, int cap, int *n_out);

/* timing of the last completed job of a slot, microseconds between HIP events
 * recorded on the slot's stream around the launches:
 * [0] pyramid+FAST+compaction, [1] selection: host wall time (MCORB_SELECT_HOST) or k_select + k_assemble (MCORB_SELECT_GPU), [2] blur + describe(+D2H),
 * [3] k-NN + finalize, [4] pyramid launches, [5] FAST kernel alone, [6] compaction kernel (side stream),
 * [7] k-NN kernel alone, [8] blur kernel, [9] describe kernel */
int mcorb_rig_last_timing(mcorb_rig *r, int slot, float us[10]);
/* MCORB_SELECT_HOST or MCORB_SELECT_GPU: what this rig runs; jobs of a slot that fell back to the host stage so far */
int mcorb_rig_select_mode(mcorb_rig *r);
int mcorb_rig_select_fallbacks(mcorb_rig *r, int slot);
/* small batches (results through host-mapped memory): images whose early read the signal word's checksum rejected so far -- their
 * keypoint records were built after the job's end event instead (0 in every run so far) */
int mcorb_rig_early_reads_rejected(mcorb_rig *r, int slot);
/* MCORB_SELECT_GPU only: a job is the same ~20 launches and copies every time, so a slot captures it once into a HIP graph and
 * replays it with one call.  every = 0: never (launch by launch, per-kernel HIP events: mcorb_rig_last_timing is complete),
 * 1: every job (last_timing reports [0] = the whole job, the rest 0), K > 1: all but every K-th job of a slot, which runs
 * launch by launch -- a timed sample of the same pipeline.  Default: the environment's MCORB_GRAPH, else 1 for a rig with one slot
 * (one job at a time: the replay saves ~60 us of a 0.4 ms rig frame) and 0 otherwise (with several jobs in flight it measured slower). */
int mcorb_rig_set_graph(mcorb_rig *r, int every);
/* test hook for the GPU selection's sort: the permutation std::sort (libstdc++) leaves n keys in, computed by one GPU wave
 * (perm_dev) and by std::sort itself on the host (perm_std); entries compare by key only (mcorb_sortmodel.h) */
int mcorb_dev_sort_selftest(int device, const uint32_t *keys, int n, uint32_t *perm_dev, uint32_t *perm_std);

/* multi-GPU plumbing (one process per GPU; the collective itself is the
 * caller's: bench.py's throughput path uses one RCCL all-to-all with uneven splits per round, its
 * --exchange allgather path the all-gather SURVEY 8(e) describes; both over torch.distributed).
 * Descriptor block layout on the device: [sets][kcap][32] bytes. */
int mcorb_rig_kcap(mcorb_rig *r);
/* worker threads of the rig's host stage (selection, track merges): what mcorb_params.host_threads / the core budget resolved to */
int mcorb_rig_host_threads(mcorb_rig *r);
/* sizes of one image's device structures (what the byte counts of the measurements are made of):
 * out = {kcap, FAST cells, blur tiles, candidate slots per cell, candidate list capacity, quad-tree bucket entries,
 *        bytes of one pyramid block, levels} */
int mcorb_rig_info(mcorb_rig *r, int32_t out[8]);
void *mcorb_rig_desc_device_ptr(mcorb_rig *r, int slot);
void *mcorb_rig_stream(mcorb_rig *r, int slot);
/* copy the first nimg descriptor sets of a slot into caller device memory
 * (e.g. a tensor that is then all-gathered); counts_host receives the counts */
int mcorb_rig_export_descriptors(mcorb_rig *r, int slot, void *dst_dev, int32_t *counts_host, int nimg);
/* computeIntraMatches(matches,false) over an external (all-gathered) descriptor
 * block: `ntotal` sets with counts[set] descriptors each; sets[f*ncams + c] names
 * the set that holds camera c of frame f.  Results are read back with
 * mcorb_rig_get_pair_matches / _get_pair_knn2 / _get_tracks as for mcorb_rig_match. */
int mcorb_rig_match_external(mcorb_rig *r, int slot, const void *desc_dev, const int32_t *counts, int ntotal,
                             const int32_t *sets, int nframes, float dist_thresh, float ratio);
/* asynchronous form: counts/sets must stay valid until mcorb_rig_match_wait(r, slot) returns */
int mcorb_rig_match_external_submit(mcorb_rig *r, int slot, const void *desc_dev, const int32_t *counts, int ntotal,
                                    const int32_t *sets, int nframes, float dist_thresh, float ratio);

/* Stream-ordered forms of the two calls above, for a pipelined exchange without host synchronisation:
 * _export_descriptors_dev enqueues the copies (descriptor sets + their int32 counts, both into caller DEVICE memory)
 * on the slot's stream and makes `then_stream` (a HIP stream of this process, e.g. the stream the collective is issued
 * on; NULL = block until the copies are done) wait for them;
 * _match_external_dev_submit takes the counts from device memory and lets the slot's stream wait for everything
 * enqueued so far on `after_stream` (the collective; NULL = the caller has synchronised already).
 * The legacy NULL stream cannot be named here (its handle IS NULL): issue the collective on a stream created with
 * hipStreamCreate / torch.cuda.Stream().
 * An external block holds at most max(4096, 64 x images per slot) sets (MCORB_E_ARG beyond). */
int mcorb_rig_export_descriptors_dev(mcorb_rig *r, int slot, void *dst_dev, int32_t *counts_dev, int nimg, void *then_stream);
int mcorb_rig_match_external_dev_submit(mcorb_rig *r, int slot, const void *desc_dev, const int32_t *counts_dev, int ntotal,
                                        const int32_t *sets, int nframes, float dist_thresh, float ratio, void *after_stream);

/* Pair-partitioned matching, the multi-GPU split SURVEY.md 8(e) describes for ONE rig frame across GPUs: every camera's
 * descriptors are all-gathered, BruteForceMatch of camera pair (i, j) (MultiCameraFrame.cpp:1118 loop, :1024-1086) runs on one
 * rank, and the accepted (query, train) lists return to the rank that runs computeIntraMatches' serial merge (:1167-1268).
 * _match_pairs_external*: pair_sets[2p], pair_sets[2p + 1] = query / train set of pair p inside the external block; at most
 * (images per slot) distinct sets and ncams (ncams - 1) / 2 x (frames per slot) pairs per job; no tracks are built
 * (mcorb_rig_get_tracks fails), the lists are read with mcorb_rig_get_pairlist (pair = index into pair_sets).  The _dev_submit
 * form orders the job behind `after_stream` like mcorb_rig_match_external_dev_submit; wait with mcorb_rig_match_wait.
 * LIFETIME: the submit forms return before the slot's driver thread has read `sets` / `pair_sets` (and the host `counts` of the
 * non-_dev forms): those arrays must stay valid and unchanged until mcorb_rig_match_wait has returned for that slot.
 * mcorb_host_merge_tracks: the merge itself on caller-supplied lists (pairs in (0,1), (0,2), .., (1,2), .. order, npair[p]
 * entries each, counts[c] keypoints per camera) -> tracks [n][ncams], -1 = absent; no device involved. */
int mcorb_rig_match_pairs_external(mcorb_rig *r, int slot, const void *desc_dev, const int32_t *counts, int ntotal,
                                   const int32_t *pair_sets, int npairs, float dist_thresh, float ratio);
int mcorb_rig_match_pairs_external_dev_submit(mcorb_rig *r, int slot, const void *desc_dev, const int32_t *counts_dev, int ntotal,
                                              const int32_t *pair_sets, int npairs, float dist_thresh, float ratio, void *after_stream);
int mcorb_rig_get_pairlist(mcorb_rig *r, int slot, int pair, uint32_t *idx1, uint32_t *idx2, int cap, int *n_out);
int mcorb_host_merge_tracks(int ncams, const int32_t *counts, const uint32_t *const *idx1, const uint32_t *const *idx2,
                            const int32_t *npair, int32_t *tracks, int cap_tracks, int *ntracks_out, int *mergeable_out);

/* Device-resident descriptor sets + matching between any two of them (findInterMatches / findMatchesMono call
 * knnMatch(k = 2) on the LF descriptors of consecutive keyframes, <= 3000 x 3000, ratio 0.7, threshold 50, FrontEnd.cpp:3114-3500).
 * A block holds nsets sets of up to kcap descriptors in HBM (kcap = mcorb_rig_kcap of the rig that will match them: create that
 * rig with nfeatures >= the largest set).  Upload a keyframe's descriptors ONCE; the previous keyframe's set stays resident, so an
 * inter-frame match moves one set over PCIe, not two (mcorb_knn2 re-uploads both).  mcorb_rig_match_sets = BFMatcher knnMatch(k=2)
 * + the (dist_thresh, ratio) filter of BruteForceMatch on explicit (query set, train set) pairs; read the accepted pairs with
 * mcorb_rig_get_pairlist and the raw k-NN table (DMatch order: lowest train index first on ties) with mcorb_rig_get_pairknn2. */
typedef struct mcorb_descblock mcorb_descblock;
int mcorb_descblock_create(int device, int nsets, int kcap, mcorb_descblock **out);
void mcorb_descblock_destroy(mcorb_descblock *b);
int mcorb_descblock_upload(mcorb_descblock *b, int set, const uint8_t *desc, int n);
void *mcorb_descblock_desc_ptr(mcorb_descblock *b);
int32_t *mcorb_descblock_counts_dev(mcorb_descblock *b);
int mcorb_rig_match_sets(mcorb_rig *r, int slot, mcorb_descblock *b, const int32_t *pair_sets, int npairs, float dist_thresh, float ratio);
int mcorb_rig_get_pairknn2(mcorb_rig *r, int slot, int pair, int32_t *idx, int32_t *dist, int cap_rows, int *nq_out);

/* ------------------------------------------------------------------------- */
/* Single-camera extractor: ORBextractor (ORBextractor.h:43-116)              */
/* ------------------------------------------------------------------------- */
typedef struct mcorb_extractor mcorb_t;

/* ORBextractor::ORBextractor (ORBextractor.cpp:408-468); buffers are sized for
 * images up to max_width x max_height (geometry is rebuilt when the size changes) */
int mcorb_create(const mcorb_params *p, int max_width, int max_height, mcorb_t **out);
void mcorb_destroy(mcorb_t *e);
/* ORBextractor::operator() (ORBextractor.cpp:1085-1171); the mask argument of
 * the reference is ignored there and absent here.  Returns MCORB_OK and
 * *mono_index_out = the reference's return value, or MCORB_E_EMPTY for the
 * reference's -1. */
int mcorb_extract(mcorb_t *e, const uint8_t *gray, int w, int h, int stride_bytes,
                  int lap_x0, int lap_x1, mcorb_keypoint *kps, uint8_t *desc, int cap,
                  int *n_out, int *mono_index_out);
/* same, fed with the reference's CV_32F [0,1] frame (setData, MultiCameraFrame.cpp:108-116) */
int mcorb_extract_f32(mcorb_t *e, const float *img01, int w, int h, int stride_bytes, int channels,
                      int lap_x0, int lap_x1, mcorb_keypoint *kps, uint8_t *desc, int cap,
                      int *n_out, int *mono_index_out);
/* GetLevels / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (ORBextractor.h:61-81) + mnFeaturesPerLevel */
int mcorb_get_tables(const mcorb_params *p, float *scale, float *inv_scale, float *sigma2,
                     float *inv_sigma2, int *features_per_level);
/* mvImagePyramid[level] interior of the last call (ORBextractor.h:89) */
int mcorb_get_pyramid_level(mcorb_t *e, int level, uint8_t *dst, int dst_stride, int *w, int *h);

/* ------------------------------------------------------------------------- */
/* Descriptor distance / matchers                                             */
/* ------------------------------------------------------------------------- */
/* ORBextractor::DescriptorDistance (ORBextractor.cpp:1202-1218); host, 0..256 */
int mcorb_hamming256(const uint8_t a[32], const uint8_t b[32]);
/* MultiCameraFrame::computeRepresentativeDesc (MultiCameraFrame.cpp:530-567): index of the descriptor
 * (n x 32 bytes, n <= 64: one per camera of a track) with the least median distance to the rest. Host. */
int mcorb_representative_desc(const uint8_t *descs, int n);
/* DescriptorMatcher("BruteForce-Hamming")->knnMatch(q, t, out, 2)
 * (MultiCameraFrame.cpp:1053-1055; FrontEnd.cpp findInterMatches): host
 * descriptor arrays in, nq x 2 (trainIdx, distance) out, -1 = absent. */
int mcorb_knn2(mcorb_t *e, const uint8_t *q, int nq, const uint8_t *t, int nt, int32_t *idx, int32_t *dist);
/* BruteForceMatch (MultiCameraFrame.cpp:1024-1086): knn2 + ratio/threshold filter */
int mcorb_match_ratio(mcorb_t *e, const uint8_t *q, int nq, const uint8_t *t, int nt,
                      float dist_thresh, float ratio, uint32_t *idx1, uint32_t *idx2, int cap, int *n_out);

/* ------------------------------------------------------------------------- */
/* DBoW2 vocabulary: transform(features, BowVector, FeatureVector, levelsup)  */
/* (MultiCameraFrame.cpp:257, FrontEnd.cpp:525,929).  The    */
/* tree descent runs on the GPU; the std::map-ordered weight accumulation and */
/* normalisation on the host, in feature order.                               */
/* ------------------------------------------------------------------------- */
typedef struct mcorb_vocab mcorb_vocab;
/* nodes 1..nnodes in file order (node 0 is the root): parent id, leaf flag, 32-byte descriptor, weight.
 * scoring: 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA, 5 DOT_PRODUCT;
 * weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY (DBoW2's enums; ORBvoc.txt is "10 6 0 0").
 * device == -1: a host-only vocabulary (no device tables; the transforms return MCORB_E_NODEVICE), enough for a host-only
 * keyframe database (mcorb_kfdb_create). */
int mcorb_vocab_create(int k, int L, int scoring, int weighting, const int32_t *parent, const uint8_t *is_leaf,
                       const uint8_t *desc, const double *weight, int nnodes, int device, mcorb_vocab **out);
/* TemplatedVocabulary::loadFromTextFile (FrontEnd.h:137-138) */
int mcorb_vocab_load_text(const char *path, int device, mcorb_vocab **out);
void mcorb_vocab_destroy(mcorb_vocab *v);
int mcorb_vocab_info(const mcorb_vocab *v, int *k, int *L, int *nnodes, int *nwords);
/* transform n descriptors (host, n x 32).  BowVector: (word id, value) ascending by id;
 * FeatureVector: node ids ascending, fv_offsets[i]..fv_offsets[i+1] index fv_feats (feature indices). */
int mcorb_vocab_transform(mcorb_vocab *v, const uint8_t *desc, int n, int levelsup, uint32_t *bow_ids, double *bow_vals,
                          int bow_cap, int *nbow, uint32_t *fv_nodes, int32_t *fv_offsets, int fv_cap, int *nfv,
                          int32_t *fv_feats, int feat_cap);
/* same for image m of a rig slot, reading the descriptors where extraction left them in HBM */
int mcorb_rig_transform_image(mcorb_rig *r, int slot, int m, mcorb_vocab *v, int levelsup, uint32_t *bow_ids,
                              double *bow_vals, int bow_cap, int *nbow, uint32_t *fv_nodes, int32_t *fv_offsets,
                              int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap);

/* computeIntraMatches(matches, words_), the BoW-guided live variant (MultiCameraFrame.cpp:586-943,
 * FrontEnd.cpp:1009) for one extracted rig frame of a slot: vocabulary descent and the per-node
 * best / second-best distance table on the GPU, the reference's serial track bookkeeping on the host.
 * tracks: ntracks x ncams matchIndex rows (-1 absent); n_rays per track; words: node id pushed to
 * words_ for every accepted feature.  max_neighbor_ratio = ORBextractor::max_neighbor_ratio (0.85). */
/* transform() of images [img0, img0 + nimg) of a slot at once (one descent launch; the order-defined folds of the
 * images run on the worker pool); read each image's vectors with mcorb_rig_get_transform (layout as
 * mcorb_vocab_transform's outputs) */
int mcorb_rig_transform_images(mcorb_rig *r, int slot, int img0, int nimg, mcorb_vocab *v, int levelsup);
int mcorb_rig_get_transform(mcorb_rig *r, int slot, int m, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow,
                            uint32_t *fv_nodes, int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap);
int mcorb_rig_match_bow(mcorb_rig *r, int slot, int frame, mcorb_vocab *v, int levelsup, double max_neighbor_ratio,
                        int32_t *tracks, int32_t *n_rays, int cap_tracks, int *ntracks_out, uint32_t *words,
                        int cap_words, int *nwords_out);
/* The same for frames [frame0, frame0 + nframes) of a slot at once (one descent launch, one table launch, the serial
 * bookkeeping of the frames on the worker pool); results are kept per frame and read with mcorb_rig_get_bow_tracks.
 * y_undist (may be NULL): y_undist[m], m = frame * ncams + cam, points at the undistorted rows of image m's keypoints --
 * image_kps_undist[cam][k].pt.y, which the reference's |dy| < 50 gate reads (MultiCameraFrame.cpp:708-716); NULL = the raw
 * rows (RECTIFY, or zero distortion: image_kps_undist == image_kps, MultiCameraFrame.cpp:302-307). */
int mcorb_rig_match_bow_frames(mcorb_rig *r, int slot, int frame0, int nframes, mcorb_vocab *v, int levelsup,
                               double max_neighbor_ratio, const float *const *y_undist);
int mcorb_rig_get_bow_tracks(mcorb_rig *r, int slot, int frame, int32_t *tracks, int32_t *n_rays, int cap_tracks,
                             int *ntracks_out, uint32_t *words, int cap_words, int *nwords_out);

/* Bind a vocabulary to the rig: every later extraction job (extract, extract_submit, process, process_submit; all slots) also runs
 * the requested BoW stages on the GPU inside the same submission, with no host round trip between the descent and the match table:
 *   MCORB_BOW_TRANSFORM  transform(desc, BowVector, FeatureVector, levelsup) of every image (MultiCameraFrame.cpp:257); read with
 *                        mcorb_rig_get_transform for every image of the job.
 *   MCORB_BOW_MATCH      also computeIntraMatches(matches, words_) of every frame (:586-943; implies the transform); read with
 *                        mcorb_rig_get_bow_tracks for every frame of the job.  The |dy| < 50 gate reads the rig's own undistorted
 *                        rows when undistortion is set (mcorb_rig_set_undistortion), else the raw keypoint rows; a job whose image
 *                        count is not a whole number of frames is refused (MCORB_E_ARG) at submit.
 * The results equal the explicit calls' (mcorb_rig_transform_images, mcorb_rig_match_bow_frames with y_undist = NULL) bit for bit;
 * a later explicit call still overwrites them.  v = NULL or flags = 0 unbinds: a job is then exactly what it is without this call.
 * The vocabulary must live on the rig's device and outlive the binding.  MCORB_E_ARG: another device, levelsup < 0, unknown flags,
 * or a rig whose kcap (mcorb_rig_kcap) exceeds MCORB_BOW_MAX_KCAP -- the per-image fold sorts an image's keys in LDS; kcap is
 * nfeatures + 4 x nlevels + 48 rounded up to 64, so nfeatures = 4000 at 8 levels fits.  MCORB_E_STATE while a submitted job has
 * not been waited for. */
#define MCORB_BOW_TRANSFORM 1
#define MCORB_BOW_MATCH 2
#define MCORB_BOW_MAX_KCAP 4096
int mcorb_rig_set_vocabulary(mcorb_rig *r, mcorb_vocab *v, int levelsup, double max_neighbor_ratio, int flags);

/* ------------------------------------------------------------------------- */
/* FrontEnd::obtainLfFeatures (MCSlam/src/FrontEnd.cpp:213-593): the consumer  */
/* of the IntraMatch tracks.  Host code.                     */
/* ------------------------------------------------------------------------- */
/* one camera of camconfig_: K_mats_[i] (row-major 3x3) and build_Rt(R_mats_[i], t_mats_[i]) (row-major 3x4) */
typedef struct mcorb_camera {
    double K[9];
    double Rt[12];
} mcorb_camera;
/* one entry of currentFrame->intraMatches as obtainLfFeatures leaves it: IntraMatch{matchIndex, uv_ref, mono, n_rays,
 * matchDesc, point3D} (MultiCameraFrame.h:42-57); point3d is meaningful when mono == 0 */
typedef struct mcorb_lf_feature {
    int32_t match_index[MCORB_MAX_CAMS];
    float uv_ref[2];
    int32_t mono, n_rays;
    double point3d[3];
    uint8_t desc[32];
} mcorb_lf_feature;
/* tracks: ntracks x ncams ints (matches_map, -1 = absent) of `frame` of the slot, words (may be NULL): words_ per track;
 * cams: ncams entries; seg_masks (may be NULL, or NULL per camera = all zero): per camera a float image with `seg_stride`
 * floats per row, a view is dropped where the mask at the RAW keypoint is >= 0.7 (:262-270); kps_undist (may be NULL):
 * image_kps_undist per camera (uv_ref and the response of mono features are read from it, :397-408, :497-505);
 * total_feats: 3000 in the reference (:430).  out receives the accepted multi-view tracks in track order (triangulated with
 * cv::sfm::triangulatePoints' DLT, kept when 0.5 < z < 40, :309) followed by the mono features in argsorte(responses, false)
 * order (:514-521); *intramatch_size_out / *mono_size_out = lf_frame->intramatch_size / mono_size; words_fil (may be NULL)
 * = the std::set filled at :344.  lIds is all -1 (one per output entry) and lfBoW is mcorb_vocab_transform of the output
 * descriptors (:525).  Parity: every integer / ordering result exact; point3d and uv_ref of triangulated tracks to 1e-9
 * relative (the SVD behind the reference's triangulation is un-vendored: unpinned). */
int mcorb_rig_obtain_lf_features(mcorb_rig *r, int slot, int frame, const int32_t *tracks, int ntracks, const uint32_t *words,
                                 const mcorb_camera *cams, const float *const *seg_masks, int seg_stride,
                                 const mcorb_keypoint *const *kps_undist, int total_feats, mcorb_lf_feature *out, int cap,
                                 int *n_out, int *intramatch_size_out, int *mono_size_out, uint32_t *words_fil, int cap_words,
                                 int *nwords_fil_out);
/* The same for all frames [frame0, frame0 + nframes) of a slot in one call, one worker-pool task per frame (FrontEnd.cpp:1024
 * calls obtainLfFeatures once per frame; a batch holds many).  tracks / words: the frames' arrays back to back -- ntracks[f]
 * tracks (ncams ints each) and, if words != NULL, as many words per frame; seg_masks / kps_undist: nframes * ncams pointers
 * (index f * ncams + cam) or NULL; out: nframes blocks of `cap` entries; words_fil (may be NULL): nframes blocks of cap_words;
 * n_out / intramatch_size_out / mono_size_out / nwords_fil_out: nframes entries each.  Returns the first failing frame's status. */
int mcorb_rig_obtain_lf_features_frames(mcorb_rig *r, int slot, int frame0, int nframes, const int32_t *tracks, const int32_t *ntracks,
                                        const uint32_t *words, const mcorb_camera *cams, const float *const *seg_masks, int seg_stride,
                                        const mcorb_keypoint *const *kps_undist, int total_feats, mcorb_lf_feature *out, int cap,
                                        int *n_out, int *intramatch_size_out, int *mono_size_out, uint32_t *words_fil, int cap_words,
                                        int *nwords_fil_out);

/* Bind obtainLfFeatures to the rig's jobs (FrontEnd.cpp:1009-1024): every later extraction job whose vocabulary is bound with
 * MCORB_BOW_MATCH (mcorb_rig_set_vocabulary) also runs, for every frame, obtainLfFeatures on the job's own BoW-guided tracks
 * (mcorb_rig_get_bow_tracks) with words_ all 1 (:1010), all-zero segmentation masks (mc_slam_app.cpp:224) and the rig's
 * image_kps_undist (its own undistorted set when mcorb_rig_set_undistortion is active, else the raw keypoints), and the LF
 * set's transform() with the bound levelsup (:525).  The triangulations run on the GPU (k_lf_tracks), the order-dependent
 * bookkeeping on the host.  Results equal mcorb_rig_obtain_lf_features(those tracks, ones, NULL, 0, NULL, total_feats) and
 * mcorb_vocab_transform(its descriptors, levelsup) bit for bit; extract / process and their waits return once they are ready.
 * cams: ncams entries (K, build_Rt); total_feats: 3000 in the reference (FrontEnd.cpp:515), >= 0; cams = NULL unbinds (a job is
 * then exactly what it is without this call).  MCORB_E_STATE while a submitted job has not been waited for. */
int mcorb_rig_set_lf(mcorb_rig *r, const mcorb_camera *cams, int total_feats);
/* the job's obtainLfFeatures output of one frame, laid out as mcorb_rig_obtain_lf_features'.  MCORB_E_STATE for a frame the
 * slot's last extraction did not run the stage on; MCORB_E_CAP (with the needed counts set) when out / words_fil are short */
int mcorb_rig_get_lf_features(mcorb_rig *r, int slot, int frame, mcorb_lf_feature *out, int cap, int *n_out,
                              int *intramatch_size_out, int *mono_size_out, uint32_t *words_fil, int cap_words, int *nwords_fil_out);
/* the job's lfBoW / lfFeatVec of one frame, laid out as mcorb_rig_get_transform's; same states */
int mcorb_rig_get_lf_bow(mcorb_rig *r, int slot, int frame, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow,
                         uint32_t *fv_nodes, int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap);
/* test hook: k_lf_tracks' triangulation of n arbitrary problems on the device (x: 2 * nv[i] normalised coordinates, P: nv[i]
 * row-major 3x4 matrices, problems back to back; 2 <= nv[i] <= MCORB_MAX_CAMS); branch[i] = the exit of the null-vector solver
 * taken: 0 zero trace, 1 unshifted steps only, 2 Rayleigh-quotient steps, 3 Sylvester check failed and re-run */
int mcorb_dev_triangulate_selftest(int device, const double *x, const double *P, const int32_t *nv, int n, double *X, int32_t *branch);

/* ------------------------------------------------------------------------- */
/* Keyframe database: place recognition's consumer of lfBoW, lfFeatVec and    */
/* the LF descriptors -- LoopCloser::callerDetectLoop (MCSlam/src/            */
/* LoopCloser.cpp:59-193: orb_database->add :78, ->query :112, vocabulary     */
/* score :119) and LoopCloser::featureMatchesBow (:195-241); Relocalization   */
/* runs the same sequence (relocalization.cpp:64-99,205-237,327-360).         */
/* DBoW2's TemplatedDatabase is un-vendored: its published semantics are      */
/* restated (use_di = true, L1_NORM only).                                    */
/* ------------------------------------------------------------------------- */
typedef struct mcorb_kfdb mcorb_kfdb;
#define MCORB_KFDB_MAX_WORDS 4096   /* a device database stages a query's BowVector in LDS: max_words <= this */
/* A database of up to max_entries keyframes, each with a BowVector of up to max_words words and up to max_feats LF features
 * (descriptors, FeatureVector nodes and feature indices): fixed strides per entry.  device >= 0: the store lives in HBM on that
 * device, which must be the vocabulary's; queries, scores and featureMatchesBow's search run in HIP kernels.  device == -1: a
 * host-only database that needs no GPU (DBoW2's own structure: a word-major inverted file); every call below works on it, and a
 * host-only vocabulary (mcorb_vocab_create with device -1) is enough to create it.  Only L1_NORM vocabularies (scoring 0, what
 * ORBvoc.txt is) are accepted: anything else is MCORB_E_ARG. */
int mcorb_kfdb_create(const mcorb_vocab *v, int device, int max_entries, int max_words, int max_feats, mcorb_kfdb **out);
void mcorb_kfdb_destroy(mcorb_kfdb *db);
/* TemplatedDatabase::add(BowVector, FeatureVector) plus the keyframe's LF descriptors (ndesc x 32; m_image_intraMatches'
 * matchDesc, LoopCloser.cpp:209-215), host vectors in the layout mcorb_vocab_transform writes; every (word, value) is stored as
 * given.  *entry_out = the new entry id, counted from 0 (EntryId entryId = orb_database->size()).  MCORB_E_CAP, with nothing
 * added, for a full database or vectors longer than the caps; MCORB_E_ARG for ids that do not ascend or feature indices outside
 * the descriptor set. */
int mcorb_kfdb_add(mcorb_kfdb *db, const uint32_t *bow_ids, const double *bow_vals, int nbow, const uint32_t *fv_nodes,
                   const int32_t *fv_offsets, int nfv, const int32_t *fv_feats, const uint8_t *desc, int ndesc, int *entry_out);
/* The same for lfBoW, lfFeatVec and the LF descriptors of a frame the slot's last job ran the LF stage on (mcorb_rig_set_lf;
 * MCORB_E_STATE otherwise, like mcorb_rig_get_lf_bow).  The descriptors are gathered from the slot's descriptor block device to
 * device on the slot's stream; the two vectors, which the job assembles on the host, are uploaded. */
int mcorb_kfdb_add_rig_frame(mcorb_kfdb *db, mcorb_rig *r, int slot, int frame, int *entry_out);
int mcorb_kfdb_size(const mcorb_kfdb *db);
/* an entry as it is stored (a device database reads it back from HBM); MCORB_E_CAP with the counts set when an output is short */
int mcorb_kfdb_get_entry(mcorb_kfdb *db, int entry, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow, uint32_t *fv_nodes,
                         int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap, uint8_t *desc, int desc_cap,
                         int *ndesc);
/* TemplatedDatabase::query(vec, ret, max_results, max_id), queryL1: every entry e with max_id == -1 || (int)e < max_id that
 * shares a word with the query, scored with the sum over the shared words in ascending word id of (|q - d| - |q|) - |d| (fp64,
 * one accumulator); the list in ascending entry id is sorted with std::sort by that raw value, cut to max_results when
 * max_results > 0, and each score becomes -s / 2.0.  ids / scores: cap entries; *n_out = the count (MCORB_E_CAP when cap is short). */
int mcorb_kfdb_query(mcorb_kfdb *db, const uint32_t *bow_ids, const double *bow_vals, int nbow, int max_results, int max_id,
                     uint32_t *ids, double *scores, int cap, int *n_out);
/* The same for nq queries that are entries of the database, in one launch (callerDetectLoop: add, then query yourself with
 * maxId = entryId - dislocal).  Only entries below a query's max_id count, so a batch of keyframes can all be added first and
 * then queried together, each with its own max_id: the results equal interleaved add / query (for max_id != -1, which is "no
 * limit"; callerDetectLoop queries only when entryId > dislocal, :102-109, so its maxId is >= 1).  ids / scores: nq blocks of
 * cap entries; n_out: nq counts. */
int mcorb_kfdb_query_entries(mcorb_kfdb *db, const int32_t *entries, const int32_t *max_ids, int nq, int max_results, uint32_t *ids,
                             double *scores, int cap, int *n_out);
/* TemplatedVocabulary::score of two stored BowVectors (LoopCloser.cpp:119): 0 when they share no word */
int mcorb_kfdb_score(mcorb_kfdb *db, int entry_a, int entry_b, double *score);
/* LoopCloser::featureMatchesBow (:195-241): for every FeatureVector node the two entries share, in ascending node id,
 * getMatches_distRatio (ORBextractor.cpp:1228-1290) of best_entry's descriptors (A) against curr_entry's (B), outputs appended in
 * node order.  indices_1 index best_entry's LF set, indices_2 curr_entry's.  max_neighbor_ratio: 0.85 in the reference. */
int mcorb_kfdb_feature_matches(mcorb_kfdb *db, int best_entry, int curr_entry, double max_neighbor_ratio, uint32_t *indices_1,
                               uint32_t *indices_2, int cap, int *n_out);
/* a device database's last k_kfdb_score (us[0]) and k_kfdb_best2 (us[1]) launch, microseconds between HIP events */
int mcorb_kfdb_last_timing(mcorb_kfdb *db, float us[2]);

/* Probe slots: a frame's lfBoW, lfFeatVec and LF descriptors held in the database's layout (the strides and caps of an entry)
 * WITHOUT being an entry -- the current frame of FrontEnd::trackFrame (FrontEnd.cpp:6015-6023), which is matched against the last
 * keyframe and deleted when it is not one, and of Relocalization (relocalization.cpp:327-371), which queries the database with
 * a frame that is never added.  No probe call changes the size, an entry, or the result of any call above.
 * reserve_probes allocates nprobes slots (1 .. 128), once per database (MCORB_E_STATE the second time).  set_probe takes
 * mcorb_kfdb_add's arguments and validates them the same way (MCORB_E_CAP / MCORB_E_ARG leave the slot as it was); setting a slot
 * again overwrites it.  set_probe_rig_frame is mcorb_kfdb_add_rig_frame's path into a slot (same MCORB_E_STATE conditions).
 * get_probe reads a slot back as mcorb_kfdb_get_entry reads an entry.  Every call that names a slot that was never set is
 * MCORB_E_STATE; a slot index outside [0, nprobes) is MCORB_E_ARG. */
int mcorb_kfdb_reserve_probes(mcorb_kfdb *db, int nprobes);
int mcorb_kfdb_set_probe(mcorb_kfdb *db, int probe, const uint32_t *bow_ids, const double *bow_vals, int nbow, const uint32_t *fv_nodes,
                         const int32_t *fv_offsets, int nfv, const int32_t *fv_feats, const uint8_t *desc, int ndesc);
int mcorb_kfdb_set_probe_rig_frame(mcorb_kfdb *db, int probe, mcorb_rig *r, int slot, int frame);
int mcorb_kfdb_get_probe(mcorb_kfdb *db, int probe, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow, uint32_t *fv_nodes,
                         int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap, uint8_t *desc, int desc_cap,
                         int *ndesc);
/* mcorb_kfdb_query_entries / mcorb_kfdb_score with probes as the queries: one launch for all nq probes; a probe's result equals
 * mcorb_kfdb_query of the same vectors.  score_probe: TemplatedVocabulary::score(entry's BowVector, probe's). */
int mcorb_kfdb_query_probes(mcorb_kfdb *db, const int32_t *probes, const int32_t *max_ids, int nq, int max_results, uint32_t *ids,
                            double *scores, int cap, int *n_out);
int mcorb_kfdb_score_probe(mcorb_kfdb *db, int entry, int probe, double *score);
/* FrontEnd::InterMatchingBow (FrontEnd.cpp:3676-3788, as findInterMatchesBow calls it, :3905-3971) / Relocalization::
 * featureMatchesBow (relocalization.cpp:327-371) of one entry (A: the last keyframe, the best candidate) against np probes: per
 * probe, mcorb_kfdb_feature_matches' walk -- getMatches_distRatio(A, B) for every FeatureVector node entry and probe share, in
 * ascending node id, outputs appended (itr_cng_match is unused in the reference).  A device database searches all probes in one
 * launch of k_kfdb_best2 (the many-probe launch) and one copy back.  indices_1 (into the entry's LF set) and indices_2 (into the
 * probe's): np blocks of cap; n_out: np counts (MCORB_E_CAP when a block is short, with the counts set).  The reference's
 * `words` are the entry's FeatureVector nodes of indices_1. */
int mcorb_kfdb_probe_feature_matches(mcorb_kfdb *db, int entry, const int32_t *probes, int np, double max_neighbor_ratio,
                                     uint32_t *indices_1, uint32_t *indices_2, int cap, int *n_out);
/* FrontEnd::findInterMatches (FrontEnd.cpp:3344-3499) of an entry (lf_prev) and a probe (lf_cur): knnMatch(descs_prev, descs_cur,
 * 2) -- BFMatcher's order, the lowest train index first among equal distances; a device database runs it through the k-NN kernel
 * of mcorb_knn2 -- and then, in query order: a row whose lids_prev is -1 is dropped when (double)d0 > 0.7 * (double)d1 (rows of
 * landmarks skip that); when neither feature is mono, the row is dropped unless (float)sqrt(dx*dx + dy*dy + dz*dz) <= 2.0 (fp64,
 * summed in that order: cv::norm of the 3x1 CV_64F difference); the first row to claim a train index holds its output position
 * and a later one replaces it only when strictly closer.  lids_prev / mono_prev / p3d_prev (n x 3): per LF feature of the entry;
 * mono_cur / p3d_cur: of the probe.  query_idx / train_idx / dist: matches_z_filtered, cap rows.  The one divergence: with a
 * probe of fewer than two features the reference reads m[1] out of bounds; here a row without a second neighbour is dropped
 * unless it is a landmark's.  An empty set on either side gives no match.  (Device: max_feats <= 65535, MCORB_E_SIZE otherwise.) */
int mcorb_kfdb_probe_inter_matches_bf(mcorb_kfdb *db, int entry, int probe, const int32_t *lids_prev, const uint8_t *mono_prev,
                                      const double *p3d_prev, const uint8_t *mono_cur, const double *p3d_cur, int32_t *query_idx,
                                      int32_t *train_idx, int32_t *dist, int cap, int *n_out);
/* a device database's last k_kfdb_best2, many-probe launch, microseconds between HIP events */
int mcorb_kfdb_last_probe_timing(mcorb_kfdb *db, float *us);

/* ------------------------------------------------------------------------- */
/* Local map: FrontEnd::searchLocalMap2 (MCSlam/src/FrontEnd.cpp:4901-5223)   */
/* from the landmarks of the neighbouring keyframes to the camera-filtered    */
/* matches (:4953-5171, without the fbow block :5062-5095): the frustum test  */
/* per landmark and camera, transform() of the accepted descriptors,          */
/* InterMatchingBow against the current frame, the filter by viewing camera.  */
/* OptimizePose and the 4x4 inverses stay with the caller.                    */
/* ------------------------------------------------------------------------- */
typedef struct mcorb_lmap mcorb_lmap;
/* one camera of the current frame: camconfig_.R_mats_ / t_mats_ / K_mats_ (row-major) and the translation column of
 * W_T_cur_vec[cam] = pose * cur_T_ref.inv() (:4964-4970), which the caller computes */
typedef struct mcorb_lmap_cam {
    double R[9], t[3], K[9], centre_w[3];
} mcorb_lmap_cam;
/* Rcw / tcw: the rotation rows and the translation column of currentFrame->pose.inv() (:4953-4955); width / height: im_size_ */
typedef struct mcorb_lmap_view {
    double Rcw[9], tcw[3];
    int32_t ncams, width, height, reserved;
    mcorb_lmap_cam cams[MCORB_MAX_CAMS];
} mcorb_lmap_view;
/* A store of up to max_landmarks landmarks, slot = lId: pt3D, normal, the descriptor of the landmark's latest observation
 * (KFs.back()->intraMatches[featInds.back()].matchDesc, :5031-5033) and that observation's mono flag; a search takes up to
 * max_candidates candidates.  device >= 0: points, normals and descriptors live in HBM on that device, which must be the
 * vocabulary's, and the frustum test, the descent and the best / second-best search run in HIP kernels (k_lmap_cull,
 * k_bow_descend, k_kfdb_best2).  device == -1: a host-only store on a host-only vocabulary (mcorb_vocab_create with device -1)
 * that needs no GPU, written as the reference's loops are; it searches host-only databases.  MCORB_E_ARG for a vocabulary on
 * another device. */
int mcorb_lmap_create(mcorb_vocab *v, int device, int max_landmarks, int max_candidates, mcorb_lmap **out);
void mcorb_lmap_destroy(mcorb_lmap *m);
/* Sets n landmarks: slot lids[i] takes pt3d[3 * i ..], normal[3 * i ..], desc[32 * i ..] and mono[i] (0 / 1).  Any of the four
 * arrays may be NULL, which keeps what the slots hold; a slot counts as set once it has a point and a normal, so pt3d or normal
 * may be NULL only for slots that are set (MCORB_E_STATE otherwise).  Of an id that occurs twice the last occurrence holds.
 * MCORB_E_ARG for an id outside [0, max_landmarks); nothing is stored on an error. */
int mcorb_lmap_set(mcorb_lmap *m, const int32_t *lids, int n, const double *pt3d, const double *normal, const uint8_t *desc,
                   const uint8_t *mono);
/* The descriptors of LF features feats[i] of a database entry into slots lids[i], and mono[i] with them (mono may be NULL: kept).
 * A device store copies the rows device to device in one launch: a keyframe's descriptors are in HBM since it was added.
 * MCORB_E_ARG for an id outside the store, a feature index outside the entry, a missing entry or a database on another device;
 * the slots need not be set yet. */
int mcorb_lmap_set_desc_from_entry(mcorb_lmap *m, mcorb_kfdb *db, int entry, const int32_t *lids, const int32_t *feats, int n,
                                   const uint8_t *mono);
/* a slot as stored (a device store reads it back from HBM); outputs may be NULL.  *has_desc = 0: no descriptor yet (desc is
 * then left alone).  MCORB_E_STATE for a slot that was never set. */
int mcorb_lmap_get(mcorb_lmap *m, int lid, double pt3d[3], double normal[3], uint8_t desc[32], int *mono, int *has_desc);
/* searchLocalMap2, :4953-5171.
 * neighbour_lids: the lIds arrays of the keyframes of kfMap back to back in kfMap's order (ascending kfID); matched_lids: the
 * members of matchedlmset.  db / probe: the current frame in a probe slot of a keyframe database on the store's device -- its
 * FeatureVector and descriptors are currentFrame->lfFeatVec and img_desc2.  matched_cur / mono_cur / cam_cur: one entry per LF
 * feature of the probe -- matchedFeatsCurFrame, im2.mono, and the first camera whose matchIndex is not -1 (ii2).
 * 1. candidates (:4990-4998): neighbour_lids in order, skipping -1, ids seen before in this call and members of matched_lids.
 * 2. the frustum test (:5000-5027), all in fp64 with separate multiplies and adds, a matrix product as cv::Mat evaluates it
 *    (per element the sum over k ascending from 0.0, then the addend): pt_body = Rcw * pt + tcw; per camera pt_c = R * pt_body
 *    + t, dropped if z < 0; curDir = pt - centre_w, dropped if normal . curDir < 0.5 * sqrt(curDir . curDir); tmp = K * pt_c
 *    and then tmp * (1.0 / tmp_z) (cv::MatExpr's division by a scalar), dropped if x < 30 || x > width - 30 || y < 30 ||
 *    y > height - 30.  A NaN fails none of these.  A landmark is accepted when at least one camera keeps it.
 *    new_lids / cam_masks (bit c: camera c, lm_projected_cam_ids): the accepted landmarks in candidate order.
 * 3. transform(newlm_vecDescs, levelsup)'s FeatureVector of the accepted descriptors (:5106).
 * 4. InterMatchingBow (:5111, :3791-3845) of that FeatureVector (A) against the probe's (B): ind1 (into new_lids) / ind2 (into
 *    the probe's LF set) as mcorb_kfdb_probe_feature_matches walks.
 * 5. the filter (:5122-5171), in ind order: a pair is a match when !matched_cur[ind2], the landmark's mono flag and
 *    mono_cur[ind2] are both set and cam_cur[ind2] is one of the landmark's cameras; match_query = ind1, match_train = ind2.
 * Each *n_ receives its count; MCORB_E_CAP (with the counts set) when an output is short.  MCORB_E_ARG for an id other than -1
 * outside the store, ncams outside 1 .. MCORB_MAX_CAMS or a database on another device; MCORB_E_STATE for a candidate that was
 * never set, an accepted landmark without a descriptor or a probe slot that was never set; MCORB_E_CAP, before anything runs,
 * for more candidates than max_candidates. */
int mcorb_lmap_search(mcorb_lmap *m, const mcorb_lmap_view *view, const int32_t *neighbour_lids, int n_lids,
                      const int32_t *matched_lids, int n_matched, mcorb_kfdb *db, int probe, const uint8_t *matched_cur,
                      const uint8_t *mono_cur, const int32_t *cam_cur, int levelsup, double max_neighbor_ratio, int32_t *new_lids,
                      uint32_t *cam_masks, int cap_new, int *n_new, uint32_t *ind1, uint32_t *ind2, int cap_ind, int *n_ind,
                      int32_t *match_query, int32_t *match_train, int cap_matches, int *n_matches);
/* a device store's last k_lmap_cull (us[0]) and k_kfdb_best2 (us[1]) launch, microseconds between HIP events, and the number of
 * candidates of the last search (may be NULL) */
int mcorb_lmap_last_timing(mcorb_lmap *m, float us[2], int *n_candidates);

/* ------------------------------------------------------------------------- */
/* Mapping: FrontEnd::triangulateNeighbors (MCSlam/src/FrontEnd.cpp:4856-4899) */
/* with triangulateMatches (:5758-5953) and getSceneDepthStats (:4838-4853):  */
/* the still-unassigned inter-frame matches of the current frame against its  */
/* neighbouring keyframes become new landmarks of the local map; and the      */
/* other half of FrontEnd::mapping (:6421-6463), TriangulateNewLandmarks       */
/* (:6465-6700), as mcorb_lmap_triangulate_new below.  insertKeyFrame, uv_ref  */
/* and the cv::Mat inverses stay with the caller.                             */
/* ------------------------------------------------------------------------- */
/* one keyframe's observations */
typedef struct mcorb_map_frame {
    int32_t nfeat, ncams;
    const int32_t *match_index;              /* nfeat x ncams: intraMatches[i].matchIndex, -1 = no view */
    const mcorb_keypoint *const *kps_undist; /* per camera: image_kps_undist (pt and octave are read) */
    const int32_t *nkps;                     /* per camera */
    double centre_w[MCORB_MAX_CAMS][3];      /* per camera: the translation column of W_T_cur = pose * cur_T_ref.inv()
                                              * (Landmark::updateNormal, GlobalMap.cpp:45-49) */
    double proj[MCORB_MAX_CAMS][12];         /* per camera: rows 0..2 of cur_T_ref * pose.inv() (:5761-5776), row-major 3x4 */
    double twc[3];                           /* the pose's translation column (:4860, :4869) */
} mcorb_map_frame;
/* the outputs of mcorb_lmap_triangulate_neighbours.  The per-match arrays hold the neighbours' matches back to back, cap_matches
 * entries each (3 x cap_matches for pt3d and normal); neigh_skipped has one entry per neighbour; depth_vec has cap_depth. */
typedef struct mcorb_map_out {
    int32_t cap_matches, cap_depth;  /* in */
    uint8_t *inliers;                /* triangulateMatches' inliers[i] */
    uint8_t *verdict;                /* how the match ended: 0 a new landmark, 1 epipolar line with den == 0, 2 epipolar distance,
                                      * 3 behind a camera, 4 reprojection error (chi-square), 5 outside the parallax window,
                                      * 6 one of the two features had a landmark already, 7 the neighbour was skipped */
    int32_t *new_lid;                /* the new landmark's id, or -1 */
    double *pt3d, *normal;           /* of the new landmark (zero where new_lid is -1) */
    double *dist2, *cos_parallax;    /* for verdicts 0 and 5, else zero */
    uint8_t *neigh_skipped;          /* 0 used, 1 baseline / medianDepth < 0.01, 2 no landmark in its lIds */
    double *depth_vec;               /* dist2 of the new landmarks in the order they were made (what :5933 appends) */
    int32_t n_matches, n_depth, n_triangulated, next_lid;   /* out; next_lid: the first id not given out */
} mcorb_map_out;
/* triangulateNeighbors.  cur / lids_cur: the current frame and its lIds (nfeat entries; the reference reads currentFrame->lIds at
 * :5819 although the parameter is curFrame -- in the live call they are one object); neigh / lids_neigh: n_neigh keyframes in
 * kfMap.rbegin() order (descending id) and their lIds; every frame has cur->ncams cameras.  F21[s]: ncams x ncams row-major 3x3
 * matrices for neighbour s, index [c_cur][c_neigh] = the cameras of the first current view and of the first neighbour view
 * (:5841-5845; the inverses in it are the caller's).  match_query / match_train / n_matches: interMatches per neighbour (queryIdx
 * into the neighbour's features, trainIdx into the current frame's).  K: ncams row-major 3x3 K_mats_; inv_sigma2: nlevels values of
 * GetInverseScaleSigmaSquares(); Rcw / tcw: rows and column of currentFrame->pose.inv() (:4857-4859); next_lid: the id the first new
 * landmark takes (GlobalMap::insertLandmark counts up).
 * Per neighbour in order: medianDepth = element (n - 1) / 2 of the sorted z of Rcw * pt3D + tcw over its landmarks (read from the
 * store), baseline = norm(cur->twc - neigh->twc); the neighbour is skipped when baseline / medianDepth < 0.01 (:4868-4873).  A
 * neighbour with no landmark in its lIds is undefined behaviour in the reference (it indexes an empty vector); here it is skipped
 * and flagged 2.  Then its matches in order: skipped (verdict 6, inliers false) when lids_neigh[q] != -1 || lids_cur[t] != -1;
 * otherwise the views of both features (cameras ascending, the neighbour's first), the epipolar gate in the reference's mixed
 * float / double arithmetic, cv::sfm::triangulatePoints (the DLT of mcorb_rig_obtain_lf_features: 1e-9 relative against an SVD,
 * unpinned), per view p.z < 0 and the chi-square gate err * invSigma2[octave] > 5.991, and the parallax window cos < 0.99998 &&
 * cos > 0.5; a match that passes every reject gate but fails the window keeps inliers true and makes no landmark, as in the
 * reference.  A new landmark takes the next id, which is written to both lIds arrays (and so skips every later match of either
 * feature, across neighbours for the current frame's), its dist2 is appended to depth_vec, and its point and its normal --
 * Landmark::updateNormal for the neighbour (KFs.size() == 1) and then for the current frame, every division by a scalar a
 * multiplication by the reciprocal as cv::MatExpr does it -- and its n_rays are stored in slot id of the map (flags: point and
 * normal set, no descriptor yet).  All arithmetic is fp64 (float where the reference has float) with separate multiplies and adds in cv::Mat's
 * order.  A device store computes the per-match part in k_map_triangulate and the depths in k_map_depth, one submission for all
 * neighbours, and moves the accepted points and normals into their slots device to device; a host-only store runs the same
 * code serially; the results are equal bit for bit.
 * MCORB_E_ARG, before anything runs: a frame with another camera count, an index outside a frame or its keypoints, an octave
 * outside [0, nlevels), a matched feature without a view, a match of more than MCORB_MAX_CAMS views in total (the solver's design
 * limit), an id outside [-1, max_landmarks).  MCORB_E_STATE: a neighbour's landmark that was never set.  MCORB_E_CAP, with
 * n_matches / n_depth / n_triangulated set and nothing stored or written: cap_matches or cap_depth short, or new ids at or beyond
 * max_landmarks. */
int mcorb_lmap_triangulate_neighbours(mcorb_lmap *m, const mcorb_map_frame *cur, int32_t *lids_cur, const mcorb_map_frame *neigh,
                                      int32_t *const *lids_neigh, int n_neigh, const double *const *F21,
                                      const int32_t *const *match_query, const int32_t *const *match_train, const int32_t *n_matches,
                                      const double *K, const float *inv_sigma2, int nlevels, const double Rcw[9], const double tcw[3],
                                      int32_t next_lid, mcorb_map_out *out);
/* getSceneDepthStats' depthVec (:4843-4848) before its sort: z[i] = row 2 of Rcw * pt3D(lids[i]) + tcw, k_map_depth on a device store.
 * MCORB_E_ARG for an id outside the store, MCORB_E_STATE for a slot that was never set. */
int mcorb_lmap_depths(mcorb_lmap *m, const double Rcw[9], const double tcw[3], const int32_t *lids, int n, double *z);
/* a device store's last k_map_triangulate launches (us[0], both instances) and k_map_depth launch (us[1]), microseconds between HIP
 * events, the matches that were launched and the landmarks whose depth was taken (both may be NULL) */
int mcorb_lmap_last_triangulate_timing(mcorb_lmap *m, float us[2], int *n_launched, int *n_depth);
/* test hooks: everything of a match but the triangulation -- the epipolar gate, then for the caller's X the per-view gates, the
 * parallax window and the normal -- for n cases on the host and in one launch on the device.  Case i has nv[i] views, the first
 * nv1[i] the neighbour's (1 <= nv1 < nv <= MCORB_MAX_CAMS), views back to back: P 12, K 9, centre 3 doubles, kps 2 floats and one
 * octave per view; X 3 and F 9 doubles per case.  verdict / n_rays: n entries; vals: 5 per case (dist2, cos, normal). */
int mcorb_host_map_gates(int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P, const double *K,
                         const double *centre, const float *kps, const int32_t *octave, const double *F, const float *inv_sigma2,
                         int nlevels, int32_t *verdict, int32_t *n_rays, double *vals);
int mcorb_dev_map_gates_selftest(int device, int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P,
                                 const double *K, const double *centre, const float *kps, const int32_t *octave, const double *F,
                                 const float *inv_sigma2, int nlevels, int32_t *verdict, int32_t *n_rays, double *vals);

/* the outputs of mcorb_lmap_triangulate_new.  The per-match arrays have cap_matches entries (3 x cap_matches for pt3d and normal);
 * depth_vec has cap_depth. */
typedef struct mcorb_map_new_out {
    int32_t cap_matches, cap_depth;  /* in */
    uint8_t *inliers;                /* triangulation_inliers[i] as the function leaves it: true exactly for a new landmark */
    uint8_t *verdict;                /* 0 a new landmark, 3 behind a camera at the initial point, 4 chi-square after the refinement,
                                      * 5 parallax (cos >= 0.99998: NOT an inlier here, unlike triangulate_neighbours' window), 6 the
                                      * current feature had a landmark already, 8 degenerate (an initial point that is not finite) */
    int32_t *new_lid;                /* the new landmark's id, or -1 */
    double *pt3d, *normal;           /* of the new landmark (zero where new_lid is -1) */
    double *dist;                    /* norm(X - cur->twc), for verdicts 0 and 5, else zero */
    float *cos_parallax;             /* the reference's float, for verdicts 0 and 5, else zero */
    int32_t *iterations;             /* solves of the refinement, for verdicts 0, 4 and 5, else zero */
    double *cost_initial, *cost_final; /* 0.5 * sum |r|^2 at the initial point and at the result, for verdicts 0, 4 and 5 */
    double *depth_vec;               /* dist of the new landmarks in the order they were made (:6616) */
    double avg_depth;                /* out: their sum, added in that order (:6617; the reference never divides it) */
    int32_t n_rays_hist[MCORB_MAX_CAMS]; /* out: [views of the current feature - 1] per new landmark (:6687) */
    int32_t n_by_verdict[9];         /* out: matches per verdict */
    int32_t n_matches, n_depth, n_triangulated, next_lid;   /* out; next_lid: the first id not given out */
} mcorb_map_new_out;
/* FrontEnd::TriangulateNewLandmarks (:6465-6700): the current frame's new_inter_matches against the previous keyframe become new
 * landmarks.  cur / lids_cur, prev / lids_prev: the two frames (mcorb_map_frame, as above) and their lIds; match_query /
 * match_train: queryIdx into prev's features, trainIdx into cur's; K, inv_sigma2, nlevels, next_lid as above.
 * Matches in order: verdict 6 when lids_cur[t] != -1 -- only the current frame's id is tested (:6486), so lids_prev[q] is
 * overwritten by a later landmark, as in the reference.  Otherwise the views of both features (getDataForGTSAMTriangulation,
 * :4802-4827: prev's first, cameras ascending; the camera is proj and K with skew 0), then
 *   the initial point: the DLT of triangulate_neighbours on normalised coordinates.  Stated deviation: gtsam's triangulateSafe
 *     runs its DLT on pixel coordinates through an SVD with a rank test at 0.001; degenerate is here "a component is not finite"
 *     (verdict 8).  p.z <= 0 in any view at the initial point is verdict 3; the distance and reprojection thresholds are off (-1, 0);
 *   the refinement: TriangulationFactor<PinholeCamera<Cal3_S2>> with unit noise, recalled as the tracking and pose sections recall
 *     gtsam: r = (fx u + u0 - kx, fy v + v0 - ky), and r = (2 fx, 2 fx) with a zero Jacobian when p.z <= 0 (throwCheirality is
 *     false by default, so the reference's catch at :6577 is dead and a point that ends behind a camera fails the chi-square gate).
 *     Stated deviations: p = P[:, :3] X + P[:, 3] instead of gtsam's transformTo (rounding level), and a stated Levenberg-Marquardt
 *     schedule with the reference's parameters (:6529-6538) in place of gtsam's: lambda 1, factor 10, (H + lambda I) delta = -g by a
 *     3 x 3 LDL^T, a trial accepted iff the cost falls, the end on an accepted decrease <= 1.0 or <= 1e-5 * cost, after 50 solves,
 *     or when lambda > 1e5; the result is the last accepted point or the initial one;
 *   the cull: the first view with |r|^2 * inv_sigma2[octave] > 5.991 at the result is verdict 4 (a NaN passes);
 *   the parallax: dist = norm(X - cur->twc), dist1 = (float)norm(X - prev->twc), cos = (float)(dot / (dist1 * dist)); cos >= 0.99998
 *     is verdict 5 and inliers false; there is no lower bound and a NaN makes a landmark.
 * A new landmark takes the next id, written to both lIds; dist is appended to depth_vec and added to avg_depth; its point, its
 * normal (updateNormal for prev, then for cur, as above) and n_rays go into slot id of the map.  All arithmetic is fp64 (float where
 * stated) with separate multiplies and adds.  A device store computes the per-match part in k_map_refine_new, one lane per match
 * whose current feature is free on entry, and moves the accepted records into their slots device to device; a host-only store
 * runs the same code serially; the results are equal bit for bit (a NaN that is returned is the default quiet NaN).
 * MCORB_E_ARG, MCORB_E_CAP and MCORB_E_STATE (a pending tracking call) as for mcorb_lmap_triangulate_neighbours, before anything
 * runs and with the store and both lIds untouched. */
int mcorb_lmap_triangulate_new(mcorb_lmap *m, const mcorb_map_frame *cur, int32_t *lids_cur, const mcorb_map_frame *prev, int32_t *lids_prev,
                               const int32_t *match_query, const int32_t *match_train, int n_matches, const double *K,
                               const float *inv_sigma2, int nlevels, int32_t next_lid, mcorb_map_new_out *out);
/* a device store's last k_map_refine_new launches (both instances), microseconds between HIP events, and the matches that were
 * launched (may be NULL); a call with nothing to launch launches nothing and leaves both */
int mcorb_lmap_last_triangulate_new_timing(mcorb_lmap *m, float us[1], int *n_launched);
/* test hooks: everything of a match after the DLT -- the degenerate and behind tests at X0, the refinement, the cull, the parallax
 * and the normal -- for n cases on the host and in one launch on the device.  Views as for mcorb_host_map_gates; X0, twc_cur and
 * twc_prev 3 doubles per case.  verdict / n_rays / solves / cosp: n entries; vals: 9 per case (X, normal, dist, cost_initial,
 * cost_final). */
int mcorb_host_map_refine(int n, const double *X0, const int32_t *nv1, const int32_t *nv, const double *P, const double *K,
                          const double *centre, const float *kps, const int32_t *octave, const double *twc_cur, const double *twc_prev,
                          const float *inv_sigma2, int nlevels, int32_t *verdict, int32_t *n_rays, int32_t *solves, float *cosp,
                          double *vals);
int mcorb_dev_map_refine_selftest(int device, int n, const double *X0, const int32_t *nv1, const int32_t *nv, const double *P,
                                  const double *K, const double *centre, const float *kps, const int32_t *octave, const double *twc_cur,
                                  const double *twc_prev, const float *inv_sigma2, int nlevels, int32_t *verdict, int32_t *n_rays,
                                  int32_t *solves, float *cosp, double *vals);

/* ------------------------------------------------------------------------- */
/* Map initialization: FrontEnd::initialization (MCSlam/src/FrontEnd.cpp       */
/* :2481-2860) from the pose between the first two rig frames to the first     */
/* landmarks, lines :2633-2839.  The MIN_FEATS and first-frame arms, the        */
/* choice of lf_prev, the matchers and estimators (mcorb_lmap_ransac_pose,      */
/* _relative_pose, _align_pose), the one-camera findEssentialMat / recoverPose  */
/* arm (mcorb_lmap_essential_pose gives its T and flags), insertKeyFrame,       */
/* numTrackedLMs, uv_ref, the trial counter and the 4x4                         */
/* inverses stay with the caller.                                              */
/* ------------------------------------------------------------------------- */
#define MCORB_INIT_MAX_MATCHES 16384
#define MCORB_INIT_DONE 0       /* initialised: the landmarks are stored */
#define MCORB_INIT_BASELINE 1   /* norm(t) <= min_baseline: nothing ran */
#define MCORB_INIT_PARALLAX 2   /* parllaxVec empty or its median >= 0.99998 (a NaN included) */
#define MCORB_INIT_FEW 3        /* num_triangulated <= 50 */
/* the outputs of mcorb_lmap_initialize.  The per-match arrays have cap_matches entries (3 x cap_matches for pt3d and normal). */
typedef struct mcorb_init_result {
    int32_t cap_matches;             /* in */
    int32_t status;                  /* out: MCORB_INIT_* */
    uint8_t *inliers;                /* in: the estimator's flags, inter_matches' then mono_matches' (:2637); out: as the loop
                                      * leaves them -- true exactly for verdict 0 */
    uint8_t *verdict;                /* 0 a landmark candidate, 3 behind a camera, 4 reprojection error (chi-square), 5 cos >=
                                      * 0.99998 or NaN (NOT an inlier here: :2752), 9 the flag was clear on entry */
    int32_t *new_lid;                /* the new landmark's id, or -1 (always -1 unless status is MCORB_INIT_DONE) */
    double *pt3d;                    /* verdict 0: the point -- the stored (scaled) one when status is DONE; else zero */
    double *normal;                  /* of the stored landmark (zero where new_lid is -1) */
    double *dist2, *cos_parallax;    /* for verdicts 0 and 5, else zero; a NaN is the default quiet NaN */
    double parallax, median_scene_depth;   /* out: :2761-2772, both 0.0 unless parllaxVec and depthVec are both non-empty */
    double t_out[3];                 /* out: t, or t * (1.0 / median_scene_depth) when scaled */
    int32_t n_matches, n_initial_inliers, n_parallax, n_triangulated;   /* out: n, the flags set on entry, parllaxVec.size(),
                                                                         * num_triangulated = depthVec.size() */
    int32_t scaled, next_lid;        /* out: 1 when pose and points were scaled; the first id not given out */
} mcorb_init_result;
/* prev / lids_prev: lf_prev with proj = rows of prev_T_ref * lf_prev->pose.inv() (:2640-2648) and its centre_w; cur / lids_cur:
 * currentFrame with proj = rows of cur_T_ref * T.inv() (:2649-2656); cur->centre_w and both twc are not read.  R, t: T's rotation
 * (row-major) and translation.  cam_centre_body: ncams x 3, per camera the translation column of cur_T_ref.inv().  match_query /
 * match_train / n: inter_matches followed by mono_matches (:2636; queryIdx into prev's features, trainIdx into cur's), n <=
 * MCORB_INIT_MAX_MATCHES.  K, inv_sigma2, nlevels, next_lid as for mcorb_lmap_triangulate_neighbours.  min_baseline: the caller's
 * kf_translation_threshold * 0.5.
 *   1. (:2633) sqrt(t0 * t0 + t1 * t1 + t2 * t2) > min_baseline, or status BASELINE: nothing runs, every output but status,
 *      n_matches, t_out (= t) and next_lid is left alone.
 *   2. (:2665-2757) Per match with its flag set: the views of both features (get3D_2DCorrs: prev's first, cameras ascending), the
 *      DLT of triangulate_neighbours on them -- there is no epipolar gate here --, per view in order p.z < 0 (verdict 3) and err *
 *      inv_sigma2[octave] > 5.991 (verdict 4), which clear the flag at the first such view (a NaN z is not behind, a NaN err
 *      passes); otherwise cos = dot / (dist1 * dist2) joins parllaxVec, and cos < 0.99998 alone -- no lower bound -- makes the
 *      match a landmark candidate (verdict 0) whose dist2 joins depthVec; otherwise, a NaN included, verdict 5 and the flag is
 *      cleared.  A match whose flag is clear on entry is verdict 9 and untouched.
 *   3. (:2761-2772) With both vectors non-empty, parallax and median_scene_depth are element size / 2 of the sorted vectors.
 *      std::sort over a NaN is undefined in the reference; stated: the order is that of the usual monotone 64-bit key of a
 *      double's bits after the default-NaN rule, so a NaN sorts after +inf.
 *   4. (:2776, :2783) Initialised iff parllaxVec is non-empty, parallax < 0.99998 and num_triangulated > 50; otherwise status
 *      PARALLAX or FEW: nothing is stored, both lIds arrays stay as they were, the outputs are as the loop left them.
 *   5. (:2785-2790, :2816-2818) When ncams == 1 || n < 50 -- the second arm cannot hold together with num_triangulated > 50 and
 *      is restated as written --: s = 1.0 / median_scene_depth, t_out = t * s and every accepted point is X * s (cv::MatExpr's
 *      division by a scalar).
 *   6. (:2807-2832) The accepted matches in match order take ids next_lid, next_lid + 1, ..; lids_prev[q] and lids_cur[t] are
 *      set in that order with no "already assigned" test, so a later match overwrites.  Slot id takes the (scaled) point, the
 *      normal of Landmark(pt, lf_prev, ..) then addLfFrame(currentFrame, ..) on that point -- prev's views with prev->centre_w,
 *      cur's views with centres computed here as the translation column of [R | t_out] * cur_T_ref.inv(), per row ((R_i0 c0 +
 *      R_i1 c1) + R_i2 c2) + t_out_i -- and n_rays; flags: point and normal set, no descriptor yet.  The observation lists stay
 *      the caller's (mcorb_lmap_observe with MCORB_OBS_RECORD for both frames), as after mcorb_lmap_triangulate_neighbours.
 * All arithmetic is fp64 (float where the reference has float) with separate multiplies and adds.  A device store runs
 * k_init_triangulate, k_init_select and k_init_put in one submission with one wait; a host-only store runs the same header
 * serially; the results are equal bit for bit.
 * Refused before anything runs, the store and both lIds arrays untouched: MCORB_E_ARG for what mcorb_lmap_triangulate_neighbours
 * refuses (a NULL, a frame with another camera count, an index outside a frame or its keypoints, an octave outside [0, nlevels),
 * a matched feature without a view, a match of more than MCORB_MAX_CAMS views, an id outside [-1, max_landmarks)) and for n >
 * MCORB_INIT_MAX_MATCHES; MCORB_E_CAP (n_matches set) for cap_matches < n or when next_lid + the number of flags set on entry --
 * the most ids the call can give out -- exceeds max_landmarks; MCORB_E_STATE while a tracking call is pending. */
int mcorb_lmap_initialize(mcorb_lmap *m, const mcorb_map_frame *prev, int32_t *lids_prev, const mcorb_map_frame *cur, int32_t *lids_cur,
                          const double R[9], const double t[3], const double *cam_centre_body, const int32_t *match_query,
                          const int32_t *match_train, int n, const double *K, const float *inv_sigma2, int nlevels, int32_t next_lid,
                          double min_baseline, mcorb_init_result *out);
/* a device store's last k_init_triangulate launches (us[0], both instances), k_init_select (us[1]) and k_init_put (us[2]),
 * microseconds between HIP events, and the matches that were launched (may be NULL); a call that ends with BASELINE launches
 * nothing and leaves them */
int mcorb_lmap_last_initialize_timing(mcorb_lmap *m, float us[3], int *n_launched);
/* test hooks: everything of mcorb_lmap_initialize but the triangulation and the store, for n caller-given cases that stand for
 * the n matches of one call, on the host and in one submission of k_init_select and k_init_put on the device.  Views as for
 * mcorb_host_map_gates, but centre is centre_w for a view of prev and the camera's cam_centre_body for a view of cur; X 3 doubles
 * per case.  inliers: in and out.  verdict / n_rays / lid_offset: n entries (lid_offset: the id an accepted case takes, counted
 * from 0, or -1); vals: 8 per case (pt3d, normal, dist2, cos).  res: every scalar of mcorb_init_result (its arrays are not
 * touched; next_lid counts from 0). */
int mcorb_host_init_cases(int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P, const double *K,
                          const double *centre, const float *kps, const int32_t *octave, const float *inv_sigma2, int nlevels,
                          int ncams, const double R[9], const double t[3], double min_baseline, uint8_t *inliers, int32_t *verdict,
                          int32_t *n_rays, int32_t *lid_offset, double *vals, mcorb_init_result *res);
int mcorb_dev_init_cases_selftest(int device, int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P,
                                  const double *K, const double *centre, const float *kps, const int32_t *octave,
                                  const float *inv_sigma2, int nlevels, int ncams, const double R[9], const double t[3],
                                  double min_baseline, uint8_t *inliers, int32_t *verdict, int32_t *n_rays, int32_t *lid_offset,
                                  double *vals, mcorb_init_result *res);

/* ------------------------------------------------------------------------- */
/* Landmarks: the local map kept up to date as keyframes are inserted --      */
/* Landmark::addLfFrame with updateNormal(frame, featInd)                     */
/* (MCSlam/src/GlobalMap.cpp:24-74, constructor :6-14; FrontEnd.cpp:6326-6335, */
/* :6680-6682, :2819-2821), GlobalMap::updateLandmark (GlobalMap.cpp:162-185;  */
/* Backend.cpp:3835-3864, :3594-3663), GlobalMap::deleteLandmark               */
/* (GlobalMap.cpp:151-160; Backend.cpp:3442-3449) and kfMap's keys             */
/* (FrontEnd.cpp:4925-4933).  insertKeyFrame, the pose estimation, the         */
/* optimisations and the 4x4 inverses stay with the caller.                    */
/* ------------------------------------------------------------------------- */
/* Beside its point, normal, descriptor and mono flag a slot holds n_rays (Landmark::n_rays; in HBM on a device store) and, as host
 * state, its observations (kf_id, feat) in the order they were added: the reference's KFs / featInds.  mcorb_lmap_set leaves both
 * alone; mcorb_lmap_triangulate_neighbours stores a new landmark's n_rays but, as its frames carry no keyframe id, records no
 * observation: the caller registers the two with MCORB_OBS_RECORD. */
/* the observing keyframe of mcorb_lmap_observe */
typedef struct mcorb_obs_frame {
    int32_t kf_id, nfeat, ncams, reserved;   /* kf_id >= 0 */
    const int32_t *match_index;              /* nfeat x ncams: intraMatches[i].matchIndex, -1 = no view */
    double centre_w[MCORB_MAX_CAMS][3];      /* per camera: the translation column of W_T_cur = pose * cur_T_ref.inv()
                                              * (GlobalMap.cpp:45-49), which the caller computes */
} mcorb_obs_frame;
#define MCORB_OBS_UPDATE 0   /* addLfFrame (the constructor for a slot without an observation): the normal and n_rays change */
#define MCORB_OBS_RECORD 1   /* the observation is appended, normal and n_rays stay: for a landmark fresh from
                              * mcorb_lmap_triangulate_neighbours, whose normal already holds both frames */
/* n_rays of slots that are set, for a caller that loads an existing map.  Of an id that occurs twice the last occurrence holds.
 * MCORB_E_ARG for an id outside the store or a negative count, MCORB_E_STATE for a slot that was never set. */
int mcorb_lmap_set_rays(mcorb_lmap *m, const int32_t *lids, int n, const int32_t *n_rays);
/* a slot's n_rays and its observations in the order they were added (outputs may be NULL with cap 0); *n = their count,
 * MCORB_E_CAP when cap is short, MCORB_E_STATE for a slot that was never set */
int mcorb_lmap_get_observations(mcorb_lmap *m, int lid, int32_t *n_rays, int32_t *kfs, int32_t *feats, int cap, int *n);
/* A batch of addLfFrame for one keyframe: item i is landmark lids[i] seen as LF feature feats[i] of `frame`.  Per item, in batch
 * order, with the reference's serial meaning (a landmark may occur more than once: two features of one frame may match it):
 *   acc = the sum over the cameras ascending with matchIndex != -1, from 0.0, of normal_cur * (1.0 / cv::norm(normal_cur)) with
 *   normal_cur = pt3D - centre_w[cam] (the norm adds three squares in order, then sqrt; cv::MatExpr's division by a scalar is a
 *   multiplication by the reciprocal), n the number of those cameras;
 *   MCORB_OBS_UPDATE, a slot without an observation (GlobalMap.cpp:58-61): normal = acc * (1.0 / n), n_rays = n;
 *   MCORB_OBS_UPDATE otherwise (:62-67): normal = normal * (double)n_rays + acc, n_rays += n, normal = normal * (1.0 / n_rays);
 *   MCORB_OBS_RECORD: normal and n_rays untouched;
 *   in both modes (kf_id, feats[i]) is appended to the slot's observations, with entry >= 0 row feats[i] of that entry of db
 *   becomes the slot's descriptor (KFs.back()'s, FrontEnd.cpp:5031-5033; device to device on a device store) and mono[i] (mono may
 *   be NULL: kept) its mono flag.  db may be NULL with entry = -1, which keeps the descriptors.
 * All arithmetic is fp64 with separate multiplies and adds.  A device store runs it in k_lmap_observe, one lane per item, a batch
 * that names a landmark more than once in rounds (round r: every landmark's r-th occurrence); a host-only store runs the same
 * code serially; the results are equal bit for bit.  n_rays_out (may be NULL): n entries, the slot's n_rays after item i.
 * MCORB_E_ARG, before anything runs: an id outside the store, kf_id < 0, feats[i] outside the frame, a feature without a view,
 * ncams outside 1 .. MCORB_MAX_CAMS, an unknown mode, a database on another device, a missing entry or a row outside it;
 * MCORB_E_STATE: a slot without a point. */
int mcorb_lmap_observe(mcorb_lmap *m, const mcorb_obs_frame *frame, const int32_t *lids, const int32_t *feats, int n, int mode,
                       mcorb_kfdb *db, int entry, const uint8_t *mono, int32_t *n_rays_out);
/* A batch of GlobalMap::updateLandmark, in batch order: d = pt3D - pt_new[3 * i ..] per element, diff_norm[i] = sqrt(d0 * d0 +
 * d1 * d1 + d2 * d2) added in order; the point is replaced and updated[i] = 1 iff diff_norm < max_diff (the reference's 5.0), in
 * that form: a NaN stores nothing (and is returned as the default quiet NaN, 0x7ff8000000000000: IEEE 754 leaves a NaN's sign and
 * payload to the implementation, and host and device differ in it).  Normal, n_rays and observations are untouched (Landmark::updateNormal() without arguments
 * assigns nothing, GlobalMap.cpp:76-104).  A later item of the same landmark compares against the point the earlier one left.
 * k_lmap_update on a device store, with mcorb_lmap_observe's rounds.  updated / diff_norm may be NULL.  The call sums nothing:
 * updateVariables' mean_correction is the caller's serial sum over diff_norm.  MCORB_E_ARG for an id outside the store,
 * MCORB_E_STATE for a slot without a point; nothing is stored on an error. */
int mcorb_lmap_update_points(mcorb_lmap *m, const int32_t *lids, int n, const double *pt_new, double max_diff, uint8_t *updated,
                             double *diff_norm);
/* A batch of GlobalMap::deleteLandmark: the slots' flags, n_rays and observations are cleared, and the dropped (kf_id, feat)
 * pairs come back in lids order, then observation order -- the lIds entries the caller sets to -1 (GlobalMap.cpp:154-157).
 * *n_out = their count; MCORB_E_CAP when cap is short, MCORB_E_STATE for a slot that was never set, MCORB_E_ARG for an id outside
 * the store or twice in the batch; nothing is deleted on an error.  A deleted slot may be set again; a search that names it as a
 * candidate gets MCORB_E_STATE. */
int mcorb_lmap_delete(mcorb_lmap *m, const int32_t *lids, int n, int32_t *kfs, int32_t *feats, int cap, int *n_out);
/* kfMap's keys (FrontEnd.cpp:4925-4933): the ascending, duplicate-free kf_ids of the observations of lids[0 .. n).  Host only.
 * *n_out = their count; MCORB_E_CAP when cap is short, MCORB_E_STATE for a slot that was never set. */
int mcorb_lmap_observers(mcorb_lmap *m, const int32_t *lids, int n, int32_t *kf_ids, int cap, int *n_out);
/* a device store's last k_lmap_observe rounds (us[0]) and last k_lmap_update rounds (us[1]), microseconds between HIP events; a
 * call without items leaves them */
int mcorb_lmap_last_landmark_timing(mcorb_lmap *m, float us[2]);

/* ------------------------------------------------------------------------- */
/* Fast tracking: FrontEnd::startTrackingModule (MCSlam/src/FrontEnd.cpp:1570- */
/* 1689) between the map-entry query and refinePose -- Tracking::project_      */
/* (MCSlam/src/Tracking.cpp:208-260) of the gathered landmarks into every      */
/* camera from the predicted pose, and Tracking::queryCurrentFrame /           */
/* querryEachFrame (:319-449): the 10 nearest keypoints by image position, the */
/* 100 px gate, the best Hamming distance below 20 and the serial              */
/* de-duplication per keypoint.  Tracking::queryPoints and the JSON map stay   */
/* with the caller; refinePose's RANSAC is mcorb_lmap_ransac_pose and the pose */
/* refinement behind it mcorb_lmap_refine_pose, both below.                    */
/* ------------------------------------------------------------------------- */
#define MCORB_TRACK_KNN 10      /* the neighbours a projection is compared with (Tracking.cpp:335-345) */
#define MCORB_TRACK_TILE 1024   /* keypoints per LDS tile of k_track_match; a camera may have any number */
/* one camera of the rig: the pose (R, t) of its gtsam::PinholePose -- R_T_mats[i].inverse(), which the caller computes; R is
 * row-major -- and the Cal3_S2 calibration */
typedef struct mcorb_track_cam {
    double R[9], t[3], fx, fy, s, u0, v0;
} mcorb_track_cam;
/* (R0, t0): cameraRig.c0_T_w, the predicted pose; cols / rows: imgCols / imgRows */
typedef struct mcorb_track_view {
    double R0[9], t0[3];
    int32_t ncams, cols, rows, reserved;
    mcorb_track_cam cams[MCORB_MAX_CAMS];
} mcorb_track_view;
/* the current frame, host arrays: per camera n_kp keypoints, kp_xy = image_kps[c][k].pt as 2 floats each (not the undistorted
 * set) and desc = image_descriptors[c][k], 32 bytes each */
typedef struct mcorb_track_frame {
    int32_t ncams, reserved;
    int32_t n_kp[MCORB_MAX_CAMS];
    const float *kp_xy[MCORB_MAX_CAMS];
    const uint8_t *desc[MCORB_MAX_CAMS];
} mcorb_track_frame;
/* the outputs of mcorb_lmap_track.  Every array is camera-major: camera c's entries start at c * cap_proj (c * cap_match).  An
 * array may be NULL with its capacity 0; match_pt may be NULL at any capacity. */
typedef struct mcorb_track_out {
    int32_t cap_proj, cap_match;
    int32_t *proj_lid;     /* [ncams][cap_proj]     projectedLandmarkIds[c], in candidate order */
    float *proj_xy;        /* [ncams][cap_proj][2]  the projected keypoint's pt */
    int32_t *best_kp;      /* [ncams][cap_proj]     bestMatchIndex of that query before the serial part, -1: none */
    int32_t *best_dist;    /* [ncams][cap_proj]     its Hamming distance, 10000 with best_kp -1 */
    int32_t *match_kp;     /* [ncams][cap_match]    bestMatches[c] as keypoint indices, in the reference's order */
    int32_t *match_lid;    /* [ncams][cap_match]    bestMatchLandmarkIds[c] */
    int32_t *match_dist;   /* [ncams][cap_match]    the distance recorded with the entry */
    double *match_pt;      /* [ncams][cap_match][3] bestMatchLandmarks[c]: the store's point of match_lid */
    int32_t n_proj[MCORB_MAX_CAMS], n_match[MCORB_MAX_CAMS];
    int32_t n_candidates, reserved;
} mcorb_track_out;
/* One frame of fast tracking.  All arithmetic is fp64, one IEEE operation per operator in the order written.
 * 1. candidates: lids in the caller's order (the reference iterates an unordered_map: unspecified there), skipping -1 and ids
 *    seen before in this call.
 * 2. projection (project_, with gtsam's Pose3::transformFrom / transformTo and PinholePose::project2 as recalled -- gtsam is not
 *    vendored): p0 = R0 * X + t0, an element being (a0 * b0 + a1 * b1 + a2 * b2) + t; per camera q = R^T * (p0 - t), an element
 *    a0 * b0 + a1 * b1 + a2 * b2.  A landmark with q.z <= 0 in any camera is dropped from all (the try encloses project2; a NaN z
 *    does not drop).  Otherwise d = 1.0 / q.z, u = q.x * d, v = q.y * d, px = (fx * u + s * v) + u0, py = fy * v + v0, x =
 *    (float)px, y = (float)py, and the camera is dropped iff x < 0 || x > cols || y < 0 || y > rows in float (both edges and a NaN
 *    are kept; a NaN x or y is returned as the default quiet NaN 0x7fc00000, whose sign host and device would not agree on).
 * 3. neighbours: d2 = dx * dx + dy * dy with dx = (double)x - (double)kx (cvflann::L2<double>); the candidates are the keypoints
 *    with !(d2 > max_d2), the reference's form, less those with a NaN d2, which has no place in an order; of these the
 *    MCORB_TRACK_KNN smallest under the total order (d2, k) are taken: the exact neighbours, where the reference's kd-tree
 *    search is approximate, and only existing keypoints, where the reference's zero-initialised row names keypoint 0.
 * 4. the descriptor gate, over the neighbours in (d2, k) order: best = 10000; a neighbour is taken iff dist < best && dist <
 *    max_hamming (the reference's 20), so of equal distances the nearer keypoint holds.
 * 5. the de-duplication (querryEachFrame:380-415), serial per camera in query order over a list of (kp, lid, dist): for a query
 *    with a match k, the first entry whose keypoint has the same ((int)pt.x, (int)pt.y) is looked up; none: the triple is
 *    appended; one whose recorded dist is greater: it is erased and the triple appended; otherwise nothing.  (The reference
 *    compares with bestDists[k], an element of a vector that was only reserved and never written when the entry found is another
 *    keypoint of the same pixel; here the found entry's own distance is compared.)  (int) of a coordinate is truncation toward
 *    zero for |v| < 2^31 and INT32_MIN otherwise, a NaN included, so every float has a pixel.  The list never holds two entries
 *    of one pixel and an entry is replaced only by a strictly smaller distance, the replacement being appended: what is left is,
 *    per pixel, the query with the least (dist, place in candidate order), and the list holds these in candidate order.
 * A device store runs 2 in k_track_project, 3 + 4 in k_track_match, the compaction of every camera's kept candidates, in
 * candidate order, in k_track_compact, and 5 in that closed form in k_track_dedup_min / _win / _emit, in one submission whose
 * rows and matches land in host-mapped memory; 1 runs on the host.  A host-only store runs the same header serially and keeps
 * the list of 5 as the reference has it; the results are equal bit for bit.  No landmark is changed (the candidate walk uses the
 * store's per-slot stamps, scratch that no call reads as state).
 * Before anything runs: MCORB_E_ARG for view->ncams outside 1 .. MCORB_MAX_CAMS, a frame of another camera count, a negative
 * n_kp, max_hamming or capacity, a NULL array with a non-zero count, an id other than -1 outside the store; MCORB_E_STATE for a
 * candidate without a point or without a descriptor; MCORB_E_CAP for more candidates than max_candidates.  Afterwards:
 * MCORB_E_CAP, with every count set and no array written, when n_proj[c] > cap_proj or n_match[c] > cap_match for a camera. */
int mcorb_lmap_track(mcorb_lmap *m, const mcorb_track_view *view, const mcorb_track_frame *frame, const int32_t *lids, int n_lids,
                     double max_d2, int max_hamming, mcorb_track_out *out);
/* mcorb_lmap_track on a frame of a rig slot's last extraction job, read where the job left it: the mcorb_track_frame has ncams =
 * the rig's cameras, camera c being image frame * ncams + c of the slot, kp_xy that image's image_kps[c][k].pt exactly as
 * mcorb_rig_get_features returns it (not the undistorted set) and desc its descriptors in the same order.  Every output is bit
 * for bit what mcorb_lmap_track gives on those host arrays; steps, deviations, error rules and MCORB_E_CAP are those above.
 * On a device store nothing of the frame crosses PCIe: k_track_points rebuilds the keypoints from the slot's packed selection
 * words into a buffer of the store, k_track_match reads the slot's descriptors in HBM, and only the candidates go up and the
 * kept rows come down.  A host-only store (device -1) reads the slot's host records and runs the serial path; no kernel is
 * launched.  Before anything runs, besides the refusals above: MCORB_E_ARG for a NULL rig, a slot out of range, a view whose
 * ncams is not the rig's, a rig on another device than a device store; MCORB_E_STATE for a busy slot, frame < 0 or (frame + 1) *
 * ncams beyond the images of the slot's last finished extraction.  After any refusal n_candidates, n_proj and n_match are zero
 * and the store is unchanged.  Nothing of the slot is cached: every call reads the slot as it is.  The caller must not submit a
 * job on the slot during the call (the call reads the slot's buffers on the store's stream). */
int mcorb_lmap_track_rig_frame(mcorb_lmap *m, const mcorb_track_view *view, mcorb_rig *r, int slot, int frame, const int32_t *lids,
                               int n_lids, double max_d2, int max_hamming, mcorb_track_out *out);
/* a device store's last k_track_project (us[0]) and k_track_match (us[1]) launch, microseconds between HIP events; a call that
 * launches nothing leaves them */
int mcorb_lmap_last_track_timing(mcorb_lmap *m, float us[2]);
/* the same for all four kernels of the last call: k_track_points (0 after mcorb_lmap_track, which does not run it),
 * k_track_project, k_track_match, k_track_compact; a call that launches nothing leaves them */
int mcorb_lmap_last_track_timing4(mcorb_lmap *m, float us[4]);
/* the four above and, us[4], the de-duplication: the clear of its table and its three kernels */
int mcorb_lmap_last_track_timing5(mcorb_lmap *m, float us[5]);
/* The asynchronous pair.  mcorb_lmap_track_submit / mcorb_lmap_track_rig_frame_submit do everything mcorb_lmap_track /
 * mcorb_lmap_track_rig_frame do up to and excluding the synchronisation -- every refusal above with the same code, the candidate
 * walk, the copy up, every launch -- and return; want_pts: whether the wait may be given a match_pt.  The caller's arrays (lids,
 * kp_xy, desc, the view) may be changed or freed as soon as the call returns.  A host-only store runs the serial path to its end
 * and keeps the result.  A call without candidates is pending too.  A refused submission leaves nothing pending.
 * mcorb_lmap_track_wait synchronises, reads the event times and writes out (the capacities and arrays of mcorb_lmap_track; a
 * match_pt after want_pts = 0 is MCORB_E_ARG), with the same MCORB_E_CAP rule: every count set, no array written.  Whatever it
 * returns, nothing is pending afterwards.  Without a pending call: MCORB_E_STATE.
 * While a call is pending every other entry on the store -- a second submission included -- returns MCORB_E_STATE and changes
 * nothing; the mcorb_lmap_last_*timing* calls answer, and mcorb_lmap_destroy waits for the stream first.  Between the submission and
 * the wait of a slot entry the caller must not submit a job on the slot, as during mcorb_lmap_track_rig_frame; the slot must be
 * idle at the submission (MCORB_E_STATE).  A store is used by one thread at a time across a pair.
 * The synchronous entries are a submission and its wait over the same code. */
int mcorb_lmap_track_submit(mcorb_lmap *m, const mcorb_track_view *view, const mcorb_track_frame *frame, const int32_t *lids, int n_lids,
                            double max_d2, int max_hamming, int want_pts);
int mcorb_lmap_track_rig_frame_submit(mcorb_lmap *m, const mcorb_track_view *view, mcorb_rig *r, int slot, int frame, const int32_t *lids,
                                      int n_lids, double max_d2, int max_hamming, int want_pts);
int mcorb_lmap_track_wait(mcorb_lmap *m, mcorb_track_out *out);
/* The batch: nf frames of a rig slot's last extraction job against the store in one submission with one wait, and nothing on the
 * host between them.  Frame f of the call is frames[f] of the slot (any order, repeats allowed), seen from views[f], with the ids
 * lids[lid_first[f] .. lid_first[f + 1]); outs[f] receives, bit for bit, what mcorb_lmap_track_rig_frame returns for (views[f],
 * frames[f], those ids) on the same store and slot: steps 1 - 5 above hold per frame and frames do not interact -- an id named in
 * two frames' lists is a candidate of both, and the de-duplication is per frame and camera.  On a device store the candidate
 * lists, a table with one item per frame and the views go up in one pinned block in one copy; the seven kernels of the single
 * call run once each over all frames (the frame is the grid's z, a frame's block of every array has the single call's layout: a
 * single call is this with nf = 1), and the rows, matches and counts of all frames land in host-mapped memory.  A host-only store runs the serial
 * path frame by frame.
 * Refused before anything runs -- nothing is pending then, the store is unchanged and every count of every outs[f] is zero:
 * everything mcorb_lmap_track_rig_frame_submit refuses, for any frame, with that call's code; MCORB_E_ARG for nf < 1, nf >
 * MCORB_TRACK_MAX_FRAMES, a NULL views, frames or lid_first, a negative or decreasing lid_first, a view whose ncams is not the
 * rig's; MCORB_E_CAP when one frame has more than max_candidates candidates (the frames together may have more).
 * There is one pending call per store: a batch is a pending call with a frame count, a single submission one of one frame, and
 * every rule of the pair above holds.  mcorb_lmap_track_frames_wait serves any pending call: n_outs other than its frame count is
 * MCORB_E_ARG; mcorb_lmap_track_wait on a pending batch of more than one frame synchronises and returns MCORB_E_STATE.  Whatever
 * either wait returns, nothing is pending afterwards.  MCORB_E_CAP after the run: when any frame's output is short in any camera,
 * every count of every frame is set and no array of any frame is written.
 * After a batch the mcorb_lmap_last_track_timing* calls hold the batch's intervals, each over all its frames; a batch without any
 * candidate launches nothing and leaves them. */
#define MCORB_TRACK_MAX_FRAMES 32
int mcorb_lmap_track_rig_frames_submit(mcorb_lmap *m, const mcorb_track_view *views, mcorb_rig *r, int slot, const int32_t *frames, int nf,
                                       const int32_t *lids, const int32_t *lid_first /* nf + 1 */, double max_d2, int max_hamming,
                                       int want_pts);
int mcorb_lmap_track_frames_wait(mcorb_lmap *m, mcorb_track_out *outs, int n_outs);
/* the submission and its wait; outs: nf of them */
int mcorb_lmap_track_rig_frames(mcorb_lmap *m, const mcorb_track_view *views, mcorb_rig *r, int slot, const int32_t *frames, int nf,
                                const int32_t *lids, const int32_t *lid_first, double max_d2, int max_hamming, int want_pts,
                                mcorb_track_out *outs);

/* ------------------------------------------------------------------------- */
/* The rig pose from a frame's 2D-3D matches: the cost function and the       */
/* outlier rule of FrontEnd::OptimizePose (MCSlam/src/FrontEnd.cpp:4272-4409)  */
/* with the RigResectioningFactor (MCSlam/include/MCSlam/                      */
/* GtsamFactorHelpers.h:48-100), around a stated Levenberg-Marquardt: gtsam's  */
/* optimizer is not vendored.  This serves a frame that has a predicted pose;  */
/* the RANSAC in front of it is mcorb_lmap_ransac_pose, further below.         */
/* ------------------------------------------------------------------------- */
#define MCORB_POSE_LANES 256      /* the lanes whose partial sums fix the order of every addition (below) */
#define MCORB_POSE_NO_OBS 0       /* no observation: the initial pose */
#define MCORB_POSE_NO_STEP 1      /* no trial was ever accepted in the second round: the initial pose */
#define MCORB_POSE_CONVERGED 2    /* the second round ended on an accepted step with a small decrease */
#define MCORB_POSE_MAX_ITER 3     /* the second round ended at max_iterations solves, or when lambda left its bounds */
/* inv_sigma2: ORBextractor::GetInverseScaleSigmaSquares(); max_iterations: solves per round, 1 .. 100 (the reference sets 25) */
typedef struct mcorb_pose_params {
    double inv_sigma2[MCORB_MAX_LEVELS];
    int32_t nlevels, max_iterations;
} mcorb_pose_params;
/* (R, t) = w_T_b, the body's pose in the world after the second round, R row-major; status: MCORB_POSE_*, the second round's;
 * iterations: the solves of each round; cost_initial: the first round's cost at the initial pose; cost_final: the second round's
 * at the returned pose, over the observations that round had; n_obs: the observations of the problem */
typedef struct mcorb_pose_result {
    double R[9], t[3];
    double cost_initial, cost_final;
    int32_t status, iterations[2], n_inliers, n_obs, reserved;
} mcorb_pose_result;
/* The pose of a rig from n observations: observation i is the keypoint uv[2 i], uv[2 i + 1] (a KeyPoint::pt) of pyramid level
 * octave[i] in camera cam[i], of the point pts[3 i ..] or, with lids, the store's point of landmark lids[i] (a device store's
 * kernel gathers it from HBM); exactly one of lids / pts is non-NULL.  cams: the rig, a mcorb_track_cam read as body_P_sensor and
 * Cal3_S2; (R, t): the initial w_T_b.  All arithmetic is fp64, one IEEE operation per operator in the order written
 * (csrc/mcorb_pose.h), with one square root:
 * - the residual: p_b = R^T (X - t), q = Rc^T (p_b - tc); q.z <= 0 (the reference's form): r = (2 fx, 2 fx) with a zero Jacobian;
 *   otherwise d = 1.0 / q.z, u = q.x d, v = q.y d, r = ((fx u + s v) + u0 - kx, (fy v + v0) - ky).  The Jacobian is taken w.r.t. the
 *   right perturbation (omega, upsilon), gtsam's order: Dpi(q) Rc^T [ [p_b]x | -I ].
 * - Huber at k = the double nearest sqrt(5.991) on a one-pixel sigma: e = sqrt(r.r), w = e <= k ? 1 : k / e, rho = e <= k ?
 *   0.5 r.r : k (e - 0.5 k).
 * - the normal equations: the 21 upper entries of H = sum w J^T J, g = sum w J^T r and the cost sum rho over the observations
 *   that are still in.  Lane l of MCORB_POSE_LANES adds observations l, l + 256, .. in ascending order into +0.0; each block of
 *   64 lanes folds with strides 32 .. 1, s[l] = s[l] + s[l + stride], and the four block sums combine as (b0 + b1) + (b2 + b3).
 * - the step: (H + lambda diag(H)) delta = -g by an LDL^T without square roots; a pivot that is not > 0 means no step.  The
 *   retraction: a = omega / 2, C = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a) (Cayley), R' = R C, t' = t + R upsilon.
 * - the loop: lambda = 1e-4, halved after an accepted trial, doubled otherwise; a trial is accepted iff its cost is less; a round
 *   ends on an accepted step whose decrease is < 1e-6 or < 1e-6 * cost, after max_iterations solves, or when lambda leaves
 *   [1e-16, 1e32].  (gtsam's own schedule, LevenbergMarquardtParams::SetCeresDefaults, is not restated.)
 * - two rounds, each from the initial pose; after each, an observation with r.r * inv_sigma2[octave] > 5.991 at the round's
 *   result leaves for good and its inlier flag is 0.
 * A device store runs all of it in one launch of k_pose_refine, one workgroup of MCORB_POSE_LANES lanes, whose result lands in
 * host-mapped memory; a host-only store runs the same header serially: the results are equal bit for bit.  inlier (may be NULL):
 * n flags.  Before anything runs: MCORB_E_ARG for n < 0, ncams outside 1 .. MCORB_MAX_CAMS, nlevels outside 1 ..
 * MCORB_MAX_LEVELS, max_iterations outside 1 .. 100, a NULL array, a camera index or octave out of range, an id outside the
 * store, both or neither of lids / pts; MCORB_E_STATE for a landmark without a point and while a tracking call is pending.
 * The store is unchanged in every case. */
int mcorb_lmap_refine_pose(mcorb_lmap *m, int n, const int32_t *cam, const float *uv, const int32_t *octave, const int32_t *lids,
                           const double *pts, int ncams, const mcorb_track_cam *cams, const double *R, const double *t,
                           const mcorb_pose_params *params, mcorb_pose_result *res, uint8_t *inlier);
/* a device store's last k_pose_refine launch of mcorb_lmap_refine_pose, microseconds between HIP events; a call without
 * observations launches nothing and leaves it */
int mcorb_lmap_last_pose_timing(mcorb_lmap *m, float us[1]);
/* The refinement behind fast tracking.  params != NULL: from now on every tracking submission on the store -- mcorb_lmap_track,
 * mcorb_lmap_track_rig_frame, the pair, mcorb_lmap_track_rig_frames -- appends, per frame, the refinement of the view's rig from
 * the frame's de-duplicated matches, in the same submission: the rig is the view's cameras, the initial pose (R0^T, -(R0^T t0))
 * (mcorb_pose_of_view), the observations the matches camera by camera in match order, uv the matched keypoint's pt, the point
 * the store's point of the matched landmark, the octave 0 (querryEachFrame's bestMatches carry none).  The kernel builds that
 * list on the device and reads nothing from the host.  NULL: off, the default; with it off every tracking entry is exactly what
 * it is without this call.  MCORB_E_ARG for parameters mcorb_lmap_refine_pose refuses, MCORB_E_STATE while a call is pending. */
int mcorb_lmap_set_track_refine(mcorb_lmap *m, const mcorb_pose_params *params);
/* frame f's pose of the last tracking call, after its wait and until the next submission: bit for bit what
 * mcorb_lmap_refine_pose returns on that frame's match_kp -> pt, match_lid and camera arrays.  flags (may be NULL): cap inlier
 * flags, MCORB_E_CAP (with out set) when cap < out->n_obs.  MCORB_E_STATE when the last call ran without the option, is pending
 * or never happened; MCORB_E_ARG for a frame outside the call. */
int mcorb_lmap_last_track_pose(mcorb_lmap *m, int f, mcorb_pose_result *out, uint8_t *flags, int cap);
/* w_T_b of a view read as a rig whose body is camera 0's frame: R = R0^T, t = -(R0^T t0), an element -((a0 b0 + a1 b1) + a2 b2) */
void mcorb_pose_of_view(const mcorb_track_view *view, double R[9], double t[3]);
/* test hook, host: residual r (n x 2), Jacobian J (n x 2 x 6) and Huber weight w (n) of n observations at the pose (R, t) */
int mcorb_pose_eval(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam, const float *uv, const double *pts, const double *R,
                    const double *t, double *r, double *J, double *w);

/* ------------------------------------------------------------------------- */
/* Local bundle adjustment: rig keyframes and landmarks together, with the     */
/* projection factor of the reference's back end (MCSlam/src/Backend.cpp:      */
/* 1380-1393, 1426-1440) around the Levenberg-Marquardt stated above, the      */
/* landmarks eliminated by the Schur complement.        */
/* ------------------------------------------------------------------------- */
#define MCORB_BA_MAX_KF 16           /* keyframes of a window */
#define MCORB_BA_MAX_LANDMARKS 65536
#define MCORB_BA_MAX_OBS (1 << 20)
#define MCORB_BA_NO_OBS 0            /* no observation: the initial state */
#define MCORB_BA_NO_STEP 1           /* no trial was ever accepted: the initial state, on the bits */
#define MCORB_BA_CONVERGED 2         /* the loop ended on an accepted step with a small decrease */
#define MCORB_BA_MAX_ITER 3          /* the loop ended at max_iterations solves, or when lambda left its bounds */
/* sigma: per pyramid level what the reference hands noiseModel::Isotropic::Sigma(2, .) -- GetInverseScaleSigmaSquares()[octave]
 * as it stands there, or MeasurementNoiseSigma on every level; the call whitens by 1.0 / sigma[octave] and does not judge the
 * value.  max_iterations: solves, 1 .. 100 */
typedef struct mcorb_ba_params {
    double sigma[MCORB_MAX_LEVELS];
    int32_t nlevels, max_iterations;
} mcorb_ba_params;
/* status: MCORB_BA_*; iterations: the solves taken; cost_initial / cost_final: the cost at the initial and at the returned state
 * (a NaN is the default quiet NaN); n_inliers: the observations whose whitened r.r is not > 5.991 at the returned state */
typedef struct mcorb_ba_result {
    double cost_initial, cost_final;
    int32_t status, iterations, n_inliers, n_obs;
} mcorb_ba_result;
/* A window of nkf keyframes (1 .. MCORB_BA_MAX_KF) of one rig and nlm landmarks (0 .. MCORB_BA_MAX_LANDMARKS), adjusted together
 * over nobs observations (0 .. MCORB_BA_MAX_OBS).  Keyframe k has the pose w_T_b = (kf_R[9 k ..] row-major, kf_t[3 k ..]) and is
 * held when fixed[k] != 0: the fixed keyframes hold the gauge (the reference's pose prior is not restated).  The rig is
 * mcorb_lmap_refine_pose's.  Landmark j's point is pts[3 j ..] or, with lids, the store's point of lids[j] (exactly one of the two
 * is non-NULL).  Observation i is the keypoint uv[2 i], uv[2 i + 1] of level octave[i] in camera obs_cam[i] of keyframe obs_kf[i],
 * of landmark obs_lm[i], an index into the call's landmark list.  All arithmetic is fp64, one IEEE operation per operator in the
 * order written (csrc/mcorb_ba.h):
 * - the observations are sorted stably by (landmark, keyframe); "in order" means that order.
 * - an observation: r and the pose Jacobian J are mcorb_lmap_refine_pose's; the point Jacobian is JX = Dpi(q) M, M = Rc^T R^T, an
 *   entry of M (a0 b0 + a1 b1) + a2 b2, a row of JX (D0 M0 + D1 M1) + D2 M2 (the second row has no D0 term), zero behind the
 *   camera.  r, J and JX are multiplied by 1.0 / sigma[octave]; Huber at the double nearest sqrt(5.991) on the whitened r.
 * - per landmark, in order into +0.0: V = sum w JX^T JX (6 entries), gp = sum w JX^T r, cost = sum rho and, per free keyframe
 *   that sees it (a view), U = sum w J^T J (21), g = sum w J^T r (6), W = sum w J^T JX (6 x 3); a term is w (x0 y0 + x1 y1).  An
 *   observation in a fixed keyframe adds to V, gp and the cost only.
 * - V' = V with d + lambda d on the diagonal, by a 3 x 3 LDL^T written out; a pivot that is not > 0 makes the landmark inactive
 *   for this solve: it adds nothing to the reduced system and does not move.
 * - the reduced system over the free keyframes that have an observation, ascending: U_a = fold U_aj, E_ab = fold W_aj V'^-1
 *   W_bj^T (a <= b), rhs_a = fold (g_aj - W_aj V'^-1 gp_j), a product entry (x0 y0 + x1 y1) + x2 y2; fold is
 *   mcorb_lmap_refine_pose's tree over the landmarks (lane l of 256 adds landmarks l, l + 256, ..).  S_aa = (U_a + lambda
 *   diag(U_a)) - E_aa, S_ab = -E_ab; S delta = -rhs by mcorb_lmap_refine_pose's LDL^T on 6 x (free keyframes) unknowns, every dot
 *   product subtracted in ascending order; a pivot that is not > 0 means no step.  Without a free keyframe only the points move.
 * - per active landmark: tt = gp + sum over its free keyframes, ascending, of W^T delta_a; X' = X + V'^-1 (-tt).  The poses
 *   retract as mcorb_lmap_refine_pose's.
 * - the loop, its constants and the status are mcorb_lmap_refine_pose's round on the whole state; cost = fold cost_j.
 * R_out (9 nkf), t_out (3 nkf), pts_out (3 nlm): the returned state (fixed keyframes and landmarks nobody observes as they
 * came).  inlier (may be NULL): nobs flags in the caller's order.  A device store runs a chain of kernels in one submission
 * with one wait (the loop's record lives in device memory; the kernels queued behind its end return at once); a host-only store
 * runs the same header serially: the results are equal bit for bit.  A call without observations launches nothing.  Before
 * anything runs: MCORB_E_ARG for a count outside its range, a NULL array, kf / cam / lm / octave out of range, an id outside the
 * store, both or neither of lids / pts, a sigma that is not > 0, nlevels outside 1 .. MCORB_MAX_LEVELS, max_iterations outside
 * 1 .. 100; MCORB_E_STATE for a landmark without a point and while a tracking call is pending.  The store is unchanged in every
 * case: the caller applies mcorb_lmap_update_points. */
int mcorb_lmap_bundle_adjust(mcorb_lmap *m, int nkf, const double *kf_R, const double *kf_t, const uint8_t *fixed, int ncams,
                             const mcorb_track_cam *cams, int nlm, const int32_t *lids, const double *pts, int nobs,
                             const int32_t *obs_kf, const int32_t *obs_cam, const int32_t *obs_lm, const float *uv,
                             const int32_t *octave, const mcorb_ba_params *params, double *R_out, double *t_out, double *pts_out,
                             mcorb_ba_result *res, uint8_t *inlier);
/* a device store's last chain, microseconds between HIP events: [0] the copy-in, the first linearization and its cost, [1] ..
 * [4] k_ba_schur, k_ba_solve, k_ba_update and k_ba_accept of the first iteration, [5] every later iteration together (those
 * queued behind the end included), [6] the final pass.  launches_idle (may be NULL): the launches that were queued behind the
 * end.  A call without observations launches nothing and leaves both */
#define MCORB_BA_SPANS 7
int mcorb_lmap_last_ba_timing(mcorb_lmap *m, float us[MCORB_BA_SPANS], int32_t *launches_idle);
/* test hook, host: per observation the whitened residual r (n x 2), Jacobians J (n x 2 x 6) and JX (n x 2 x 3) and the Huber
 * weight w (n) at the pose (R, t) and the point pts[3 i ..], with inv_s = 1.0 / sigma[i] */
int mcorb_ba_eval(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam, const float *uv, const double *pts,
                  const double *sigma, const double *R, const double *t, double *r, double *J, double *JX, double *w);

/* ------------------------------------------------------------------------- */
/* Re-triangulation after the back end moved keyframes: the loop at the end of */
/* Backend::UpdateVariables_SmartFactors (MCSlam/src/Backend.cpp:3577-3663) --  */
/* every landmark seen in a moved keyframe is triangulated again from all of   */
/* its observations (triangulateSafe / triangulatePoint3), then updated        */
/* (GlobalMap::updateLandmark) or deleted.              */
/* ------------------------------------------------------------------------- */
#define MCORB_RETRI_MAX_KF 1024      /* keyframes of a call: a landmark's smart factor spans more than a BA window */
#define MCORB_RETRI_REPORT 0         /* mode: the store stays as it is */
#define MCORB_RETRI_APPLY 1          /* mode: valid points are written through updateLandmark's gate, failed landmarks deleted */
#define MCORB_RETRI_NOT_SELECTED 0   /* no observation in a moved keyframe */
#define MCORB_RETRI_FEW_VIEWS 1      /* selected, fewer than two observations (:3605): left alone */
#define MCORB_RETRI_VALID_UPDATED 2  /* valid, and diff_norm < max_diff */
#define MCORB_RETRI_VALID_REJECTED 3 /* valid, and updateLandmark's gate refused the point */
#define MCORB_RETRI_DEGENERATE 4     /* rank < 3, or a component of the point is not finite */
#define MCORB_RETRI_BEHIND 5
#define MCORB_RETRI_FAR 6
#define MCORB_RETRI_OUTLIER 7
#define MCORB_RETRI_VERDICTS 8
/* rank_tol: gtsam's TriangulationParameters::rankTolerance (1.0 by default; on pixel-scale rows, which are not normalised);
 * landmark_distance_threshold, dynamic_outlier_threshold: a value <= 0 (or NaN) disables the check, the reference's setting;
 * max_diff: GlobalMap::updateLandmark's gate (5.0 in the reference); mode: MCORB_RETRI_REPORT or MCORB_RETRI_APPLY */
typedef struct mcorb_retri_params {
    double rank_tol, landmark_distance_threshold, dynamic_outlier_threshold, max_diff;
    int32_t mode, reserved;
} mcorb_retri_params;
/* counts: the landmarks per verdict; n_pairs: the (kf, feat) pairs of the landmarks with a failed verdict (DEGENERATE, BEHIND,
 * FAR, OUTLIER) -- written and deleted in MCORB_RETRI_APPLY mode, counted in both; launched: 1 when the kernels ran */
typedef struct mcorb_retri_result {
    int32_t counts[MCORB_RETRI_VERDICTS];
    int32_t n_pairs, launched;
} mcorb_retri_result;
/* The arrays are mcorb_lmap_bundle_adjust's: nkf keyframes (1 .. MCORB_RETRI_MAX_KF) with the poses w_T_b = (kf_R[9 k ..] row-major,
 * kf_t[3 k ..]) after the optimisation and moved[k] != 0 where the caller found the pose moved (Backend.cpp:3550-3554 stays the
 * caller's), the rig of mcorb_lmap_refine_pose, nlm landmarks (0 .. MCORB_BA_MAX_LANDMARKS) by store id, duplicate-free, and nobs
 * observations (0 .. MCORB_BA_MAX_OBS): the keypoint uv[2 i], uv[2 i + 1] in camera obs_cam[i] of keyframe obs_kf[i], of landmark
 * obs_lm[i], an index into lids.  All arithmetic is fp64, one IEEE operation per operator in the order written
 * (csrc/mcorb_retri.h):
 * - a landmark is selected iff one of its observations lies in a keyframe with moved != 0; the observations are sorted stably by
 *   (landmark, keyframe, camera), "in order" means that order; a selected landmark with fewer than two is MCORB_RETRI_FEW_VIEWS.
 * - a view, once per (keyframe, camera): R_cw = Rc^T R^T with an entry (a0 b0 + a1 b1) + a2 b2, t_cw = Rc^T (R^T (0 - t) - tc)
 *   as mcorb_lmap_refine_pose forms a camera-frame point, the centre (R tc)_r + t_r, and P = K [R_cw | t_cw] with K = (fx s u0;
 *   0 fy v0; 0 0 1), an entry (k0 m0 + k1 m1) + k2 m2.
 * - per observation the rows a = u P[2] - P[0] and b = v P[2] - P[1]; G = sum (a a^T + b b^T), 10 sums of terms a_i a_j + b_i b_j:
 *   lane l of 16 adds the landmark's observations l, l + 16, .. ascending into +0.0, the 16 sums fold with strides 8, 4, 2, 1
 *   (s[l] = s[l] + s[l + stride]).
 * - six cyclic Jacobi sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) of the 4 x 4 G with mcorb_lmap_align_pose's
 *   rotation; v = the eigenvector of the smallest diagonal entry (the first of equals), X = v[0..2] * (1.0 / v[3]); lambda_3 =
 *   the smallest of the other three.  MCORB_RETRI_DEGENERATE iff not sqrt(max(lambda_3, 0)) > rank_tol, or a component of X is
 *   not finite.
 * - over the observations in order: far iff landmark_distance_threshold > 0 and |X - centre| > it, else behind iff z <= 0 with
 *   (x, y, z) = P (X, 1), each ((p0 X0 + p1 X1) + p2 X2) + p3; the first observation that fails names MCORB_RETRI_FAR or _BEHIND.
 *   Otherwise MCORB_RETRI_OUTLIER iff dynamic_outlier_threshold > 0 and not max |(x / z - u, y / z - v)| <= it (a NaN norm
 *   counts as +inf).
 * - a valid point goes through mcorb_lmap_update_points' rule: diff_norm = |pt - X| (a NaN is the default quiet NaN), VALID_UPDATED
 *   iff diff_norm < max_diff.  Normal, ray count and observations are untouched.
 * Per landmark: pts_out[3 j ..] (X; zeros for NOT_SELECTED and FEW_VIEWS; a NaN component is the default quiet NaN), diff_norm[j]
 * (zero unless valid), n_views[j] (its observations in the call) and verdict[j]; any of the four may be NULL.  MCORB_RETRI_APPLY
 * writes the VALID_UPDATED points into the store and deletes the landmarks with a failed verdict as mcorb_lmap_delete does, in
 * lids order: their (kf_id, feat) pairs go to kfs / feats (cap entries) and res->n_pairs counts them; more than cap gives
 * MCORB_E_CAP with the count in res->n_pairs and the store unchanged.  (A cap below the pairs of all named landmarks makes the
 * call run its kernels twice, the first time in report mode to count.)  In that mode every landmark must also have a normal, as
 * mcorb_lmap_delete asks.  A device store runs k_retri_views and k_retri_solve in one submission with one wait; a host-only store
 * runs the same header landmark by landmark: the results are equal bit for bit.  A call with no observation in a moved keyframe
 * launches nothing: every landmark is NOT_SELECTED.  Before anything runs, with the store unchanged: MCORB_E_ARG for a count
 * outside its range, a NULL array, kf / cam / lm out of range, an id outside the store or twice in lids, an unknown mode, a
 * rank_tol or max_diff that is NaN; MCORB_E_STATE for a landmark without a point and while a tracking call is pending. */
int mcorb_lmap_retriangulate(mcorb_lmap *m, int nkf, const double *kf_R, const double *kf_t, const uint8_t *moved, int ncams,
                             const mcorb_track_cam *cams, int nlm, const int32_t *lids, int nobs, const int32_t *obs_kf,
                             const int32_t *obs_cam, const int32_t *obs_lm, const float *uv, const mcorb_retri_params *params,
                             double *pts_out, double *diff_norm, int32_t *n_views, int32_t *verdict, mcorb_retri_result *res,
                             int32_t *kfs, int32_t *feats, int cap);
/* a device store's last chain, microseconds between HIP events: [0] k_retri_views, [1] k_retri_solve.  A call that launches
 * nothing leaves them */
#define MCORB_RETRI_SPANS 2
int mcorb_lmap_last_retri_timing(mcorb_lmap *m, float us[MCORB_RETRI_SPANS]);

/* ------------------------------------------------------------------------- */
/* The absolute rig pose by RANSAC in front of the refinement: the consensus   */
/* step every matcher of the reference ends in -- OpenGV's sac::Ransac<        */
/* AbsolutePoseSacProblem>(GP3P) as FrontEnd::absolutePoseFromGP3P (MCSlam/src/ */
/* FrontEnd.cpp:4660-4798), FrontEnd::refinePose (:1691-1786), LoopCloser::     */
/* checkAbsolutePose and Relocalization::checkAbsolutePose call it.  OpenGV is */
/* not vendored: its reprojection distance is recalled, and three things are   */
/* stated instead of OpenGV's -- the draws, the minimal solver and the absence */
/* of the adaptive stop.                                */
/* ------------------------------------------------------------------------- */
#define MCORB_SAC_MAX_ITERATIONS 1024
#define MCORB_SAC_SOLVER_CENTRAL 0 /* all four samples from one camera, a central P3P there: what a zero-filled struct selects */
#define MCORB_SAC_SOLVER_RIG 1     /* the samples from any cameras, a generalized solver on the rig's rays */
#define MCORB_SAC_OK 0            /* a hypothesis won */
#define MCORB_SAC_NO_OBS 1        /* an empty consensus set: the identity, nothing ran */
#define MCORB_SAC_NO_MODEL 2      /* no hypothesis had a model: the identity, every flag 0 */
/* threshold: on 1 - cos(angle between the bearing and the point's direction); the reference's is mcorb_sac_threshold(K[0](0, 2)).
 * max_iterations: the hypotheses, 1 .. MCORB_SAC_MAX_ITERATIONS (the reference sets 100), all of them examined.  seed: of the
 * draws.  solver: MCORB_SAC_SOLVER_* (the field was `reserved` and zero: the struct's size and layout are what they were) */
typedef struct mcorb_sac_params {
    double threshold;
    uint64_t seed;
    int32_t max_iterations, solver;
} mcorb_sac_params;
/* (R, t): the final w_T_b, R row-major; status: MCORB_SAC_*; used: 0 = the RANSAC's model, 1 = the refinement's result; n_inliers:
 * the inlier matches of the answer; n_matches: the matches.  The RANSAC's own: (sac_R, sac_t), sac_n_inliers, best_hypothesis (-1:
 * none), sample (the winner's four observations, the first three the solver's, the fourth the disambiguating one), n_models (the
 * hypotheses that had a model), n_consensus (the size of the consensus set).  refine: with refine_params the mcorb_pose_result of
 * the refinement from (sac_R, sac_t), zero otherwise */
typedef struct mcorb_sac_result {
    double R[9], t[3];
    double sac_R[9], sac_t[3];
    int32_t status, used, n_inliers, n_matches;
    int32_t sac_n_inliers, best_hypothesis, sample[4], n_models, n_consensus;
    mcorb_pose_result refine;
} mcorb_sac_result;
/* The pose of a rig from n observations without a predicted pose.  The observations, the rig and (R, t) = w_T_b are those of
 * mcorb_lmap_refine_pose.  match (may be NULL: every observation is its own match): non-decreasing match indices, so that a
 * match's observations are contiguous.  The consensus set is the first observation of each match (the reference's break at
 * :4704); the refinement uses all.  All arithmetic is fp64, one IEEE operation per operator in the order written
 * (csrc/mcorb_sac.h), + - * /, comparisons and sqrt:
 * - the bearing: y = (v - v0) / fy, x = ((u - u0) - s y) / fx, f = (x, y, 1) / sqrt((x x + y y) + 1).
 * - the score (OpenGV's reprojection distance, recalled): q the point in the camera's frame as the refinement computes it,
 *   score = 1 - ((f.x q.x + f.y q.y) + f.z q.z) / sqrt((q.x q.x + q.y q.y) + q.z q.z); an inlier iff score < threshold (a NaN
 *   is none).
 * - the draws (stated): draw j of hypothesis h is the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 (1 + 16 h + j).  Draw 0
 *   mod S picks a consensus observation, whose camera c is the hypothesis's; draws 1 .. 15 mod S_c pick three more from camera
 *   c's consensus observations in input order, a draw equal to an earlier member being dropped.  S_c < 4 or no fourth member
 *   after 16 draws: no model.
 * - the solver (stated): a central P3P in camera c on the first three members -- Grunert's quartic solved after Ferrari, the
 *   camera-frame points aligned to the world's by orthonormal triads, w_T_b = w_T_c (b_T_c)^-1 -- the fourth member picking the
 *   solution with the smallest score (a tie: the lowest root index; a NaN never).  Not OpenGV's generalized GP3P, which samples
 *   across cameras.
 * - with solver MCORB_SAC_SOLVER_RIG (stated as well) the sample and the solver are the rig's: all 16 draws mod S pick from the
 *   whole consensus set in input order, a draw equal to an earlier member being dropped, fewer than four members after them: no
 *   model -- so a camera needs no four observations of its own.  Observation i is the body-frame ray c_i + l d_i (c_i the
 *   camera's centre, d_i = R_i f_i); Grunert's quartic on (d_i, P_i) gives at most four starts (l_1, l_2, l_3), each takes 20
 *   Newton steps on |B_i - B_j|^2 = |P_i - P_j|^2, B_i = c_i + l_i d_i (the 3 x 3 solve by cofactors), and the triads of (B_i)
 *   and (P_i) give w_T_b directly; a pose is kept iff its three points score below 1e-12 in their own cameras, and the fourth
 *   member, scored in its own camera, picks as above.  At most 4 of the problem's up to 8 solutions are found, those that
 *   continue the central ones; this is not OpenGV's GP3P either, and it is not pinned against it.
 * - the consensus: a hypothesis's count is the number of inliers of its model over the consensus set; the largest count wins, a
 *   tie goes to the lowest h.  All max_iterations hypotheses are examined (stated: OpenGV's adaptive stop returns the best of a
 *   prefix).
 * With refine_params (absolutePoseFromGP3P when initialized, :4771-4795) mcorb_lmap_refine_pose's refinement runs over all n
 * observations from the RANSAC's pose -- bit for bit that call on the same observations from (sac_R, sac_t) -- a match being an
 * inlier of it iff all its observations are, and the rule of :4786 follows: if the RANSAC's inlier matches outnumber the
 * refinement's, the RANSAC's pose and flags are the answer (used = 0), otherwise the refinement's (used = 1).  With status
 * MCORB_SAC_NO_OBS or MCORB_SAC_NO_MODEL used is 0.
 * A device store runs k_sac_hypotheses, k_sac_score and k_sac_pick (and k_pose_refine behind them) in one submission with one
 * wait; a host-only store runs the same header serially: the results are equal bit for bit.  inlier (may be NULL): one flag per
 * match.  Before anything runs, the store unchanged: everything mcorb_lmap_refine_pose refuses (the octaves are checked against
 * refine_params' levels, or MCORB_MAX_LEVELS without), MCORB_E_ARG for a threshold that is not finite and positive,
 * max_iterations outside 1 .. MCORB_SAC_MAX_ITERATIONS, a solver that is not one of MCORB_SAC_SOLVER_*, a match array that
 * decreases or is negative; MCORB_E_STATE while a tracking call is pending.  With MCORB_SAC_SOLVER_RIG a device store runs
 * k_sac_hypotheses_rig in k_sac_hypotheses' place. */
int mcorb_lmap_ransac_pose(mcorb_lmap *m, int n, const int32_t *cam, const float *uv, const int32_t *octave, const int32_t *match,
                           const int32_t *lids, const double *pts, int ncams, const mcorb_track_cam *cams,
                           const mcorb_sac_params *params, const mcorb_pose_params *refine_params, mcorb_sac_result *res,
                           uint8_t *inlier);
/* a device store's last k_sac_hypotheses or k_sac_hypotheses_rig (us[0]), k_sac_score (us[1]) and k_sac_pick (us[2]) launch, microseconds between HIP
 * events, and its hypotheses; a call with an empty consensus set launches nothing and leaves them */
int mcorb_lmap_last_ransac_timing(mcorb_lmap *m, float us[3], int *n_hyp);
/* test hook: the counts of all hypotheses of the last call that ran any, and whether each had a model (a hypothesis without one
 * has count 0); a device store copies them down from where k_sac_score left them.  MCORB_E_CAP (with n_hyp set) when cap < n_hyp */
int mcorb_lmap_last_ransac_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, int cap, int *n_hyp);
/* the reference's threshold: 1 - cos(atan(sqrt(2) * 0.5 / K00_02)) */
double mcorb_sac_threshold(double K00_02);
/* test hook, host: the rig poses (at most 4; R as 9, t as 3 doubles each) of the minimal solver on three observations of camera
 * cam -- keypoints uv (3 x 2), points pts (3 x 3) -> the count */
int mcorb_sac_solve(const mcorb_track_cam *cam, const float *uv, const double *pts, double *R, double *t);
/* test hook, host: the same of the rig solver on three observations of cameras cam[3] of the rig cams[ncams] */
int mcorb_sac_solve_rig(int ncams, const mcorb_track_cam *cams, const int32_t *cam, const float *uv, const double *pts, double *R, double *t);
/* test hook, host: the rig solver on four observations of cameras cam[4] -- the three of mcorb_sac_solve_rig and the fourth,
 * disambiguating one -- -> the count and the poses as mcorb_sac_solve_rig gives them, mask: bit k set iff root k of the quartic
 * has a pose, best: the root whose pose the estimator takes by the fourth point's score (-1: none) and that pose (zero without) */
int mcorb_host_sac_rig_roots(int ncams, const mcorb_track_cam *cams, const int32_t *cam, const float *uv, const double *pts, double *R, double *t,
                             int32_t *mask, int32_t *best, double *best_R, double *best_t);
/* test hook, device: mcorb_sac_solve on n problems in one launch, a lane each -- cam[n], uv (n x 3 x 2), pts (n x 3 x 3) -> count[n]
 * and R (n x 4 x 9), t (n x 4 x 3), zero behind a problem's count.  n == 0 launches nothing */
int mcorb_dev_sac_solve_selftest(int device, int n, const mcorb_track_cam *cam, const float *uv, const double *pts, int32_t *count, double *R,
                                 double *t);
/* test hook, device: mcorb_host_sac_rig_roots on n problems in one launch of k_sac_hypotheses_rig's shape and body, a quad each --
 * problem i has the rig cams[ncams i ..], cam (n x 4), uv (n x 4 x 2), pts (n x 4 x 3) -> count[n], R (n x 4 x 9), t (n x 4 x 3),
 * zero behind a problem's count, mask[n], best[n], best_R (n x 9), best_t (n x 3).  Refuses what mcorb_sac_solve_rig refuses */
int mcorb_dev_sac_solve_rig_selftest(int device, int n, int ncams, const mcorb_track_cam *cams, const int32_t *cam, const float *uv,
                                     const double *pts, int32_t *count, double *R, double *t, int32_t *mask, int32_t *best, double *best_R,
                                     double *best_t);
/* test hook, host: the scores of n observations at the pose (R, t); a NaN is the default quiet NaN */
int mcorb_sac_eval(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam, const float *uv, const double *pts, const double *R,
                   const double *t, double *score);

/* ------------------------------------------------------------------------- */
/* The relative rig pose between two frames by RANSAC on 2D-2D matches: the    */
/* estimator the reference's front end selects by default (FrontEnd.h:623,     */
/* SEVENTEEN_PT) -- OpenGV's sac::Ransac<NoncentralRelativePoseSacProblem>     */
/* (SEVENTEENPT) as FrontEnd::poseFromSeventeenPt (MCSlam/src/FrontEnd.cpp:    */
/* 4532-4657, 10000 iterations) and LoopCloser::checkEssentialMatrix           */
/* (LoopCloser.cpp:353-446, 2000 iterations).  It needs no landmarks.  OpenGV  */
/* is not in the tree: its distance is recalled; the draws, the linear solver  */
/* and the absence of the adaptive stop are stated.     */
/* ------------------------------------------------------------------------- */
#define MCORB_REL_MAX_ITERATIONS 16384
#define MCORB_REL_SAMPLE 17
#define MCORB_REL_OK 0            /* a hypothesis won */
#define MCORB_REL_NO_OBS 1        /* no matches: the identity, nothing ran */
#define MCORB_REL_NO_MODEL 2      /* no hypothesis had a model (fewer than 17 matches, a central rig): the identity, every flag 0 */
/* threshold: on the sum over both views of 1 - cos(angle between the bearing and the triangulated point's direction); the
 * reference's is mcorb_rel_threshold(K[0](0, 2)).  max_iterations: the hypotheses, 1 .. MCORB_REL_MAX_ITERATIONS (the reference
 * sets 10000, its loop closer 2000), all of them examined.  seed: of the draws */
typedef struct mcorb_rel_params {
    double threshold;
    uint64_t seed;
    int32_t max_iterations, reserved;
} mcorb_rel_params;
/* (R, t) = b1_T_b2, R row-major: X_b1 = R X_b2 + t, the reference's T before `WTp * T` (:4646); status: MCORB_REL_*; n_inliers: the
 * winner's inlier matches; n_matches: n; best_hypothesis (-1: none); sample: the winner's 17 matches in draw order; n_models: the
 * hypotheses that had a model */
typedef struct mcorb_rel_result {
    double R[9], t[3];
    int32_t status, n_inliers, n_matches, best_hypothesis, sample[MCORB_REL_SAMPLE], n_models;
} mcorb_rel_result;
/* The pose of a rig's second frame in its first from n 2D-2D matches.  Match i is the keypoint uv1[i] (KeyPoint::pt) in camera
 * cam1[i] of frame 1 and uv2[i] in camera cam2[i] of frame 2: the first camera of each frame's IntraMatch (the breaks at :4559,
 * :4576), which the caller passes.  The rig is mcorb_lmap_refine_pose's.  All arithmetic is fp64, one IEEE operation per operator
 * in the order written (csrc/mcorb_rel.h), + - * /, comparisons and sqrt:
 * - the rays: f the bearing of mcorb_lmap_ransac_pose (with s = 0 the reference's :4551-4557), d = cams[cam].R f, c = cams[cam].t,
 *   m = c x d.
 * - the sample: 17 distinct matches by a partial Fisher-Yates walk without rejection.  Draw j = 0 .. 16 of hypothesis h is the
 *   splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 (1 + 32 h + j); idx = draw mod (n - j); the earlier picks are walked in
 *   ascending order and idx steps over each that is <= it; member j is idx.  n < 17: no model.
 * - the solver (stated: Li, Hartley and Kim's linear method on the generalized epipolar constraint d1^T E d2 + d1^T R m2 + m1^T R
 *   d2 = 0, E = [t]x R): the R part's nine columns are projected out of the E part's, E is the null vector of what remains, the two
 *   rotations of E are read off in closed form and polished, t follows by least squares with its scale, the candidate with the
 *   smaller residual wins, and a model whose translation scale is not observable (a central rig) is no model (csrc/mcorb_rel.h,
 *   rel_solve17).
 * - the score (OpenGV's distance of the non-central relative problem, recalled): with a = d1, b = R d2, w = (R c2 + t) - c1 the
 *   midpoint P1 of the rays' closest points, P2 = P1 - w, and (1 - a.P1 / |P1|) + (1 - b.P2 / (|P2| |b|)); a match is an inlier
 *   iff score < threshold, strictly; a NaN is no inlier.
 * - the consensus: the largest inlier count over all n matches wins, a tie goes to the lowest hypothesis, a hypothesis without a
 *   model never wins; all max_iterations hypotheses are examined (no adaptive stop).
 * A device store runs k_rel_hypotheses, k_rel_score and k_rel_pick in one submission on its stream with one wait; a host-only
 * store runs the same header serially: the results are equal bit for bit.  The store's landmarks are neither read nor written.
 * inlier (may be NULL): one flag per match.  Refused before anything runs: MCORB_E_ARG for a NULL, n < 0, ncams outside 1 ..
 * MCORB_MAX_CAMS, a camera outside the rig, a threshold that is not finite and positive, max_iterations outside 1 ..
 * MCORB_REL_MAX_ITERATIONS; MCORB_E_STATE while a tracking call is pending. */
int mcorb_lmap_relative_pose(mcorb_lmap *m, int n, const int32_t *cam1, const float *uv1, const int32_t *cam2, const float *uv2, int ncams,
                             const mcorb_track_cam *cams, const mcorb_rel_params *params, mcorb_rel_result *res, uint8_t *inlier);
/* a device store's last k_rel_hypotheses (us[0]), k_rel_score (us[1]) and k_rel_pick (us[2]) launch, microseconds between HIP
 * events, and its hypotheses; a call without matches launches nothing and leaves them */
int mcorb_lmap_last_relative_timing(mcorb_lmap *m, float us[3], int *n_hyp);
/* test hook: the counts of all hypotheses of the last call that ran any, and whether each had a model (a hypothesis without one
 * has count 0); a device store copies them down from where k_rel_score left them.  MCORB_E_CAP (with n_hyp set) when cap < n_hyp */
int mcorb_lmap_last_relative_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, int cap, int *n_hyp);
/* the reference's threshold (:4604): 2 * mcorb_sac_threshold(K00_02) */
double mcorb_rel_threshold(double K00_02);
/* test hook, host: the solver on 17 matches (cam1[17], uv1 17 x 2, cam2[17], uv2 17 x 2) of the rig cams[ncams] -> 1 with (R as 9,
 * t as 3 doubles) = b1_T_b2, 0 without a model, or a negative error.  The hooks take the keypoints in double: a float's value
 * gives the bits mcorb_lmap_relative_pose computes from that float, and a test can state a problem without rounding in either
 * frame */
int mcorb_rel_solve(int ncams, const mcorb_track_cam *cams, const int32_t *cam1, const double *uv1, const int32_t *cam2, const double *uv2,
                    double *R, double *t);
/* test hook, device: mcorb_rel_solve on n problems in one launch, a lane each -- problem i has the rig cams[ncams i ..], cam1 and
 * cam2 (n x 17), uv1 and uv2 (n x 17 x 2) -> count[n] (1 or 0), R (n x 9), t (n x 3), zero without a model.  Refuses what
 * mcorb_rel_solve refuses; n == 0 launches nothing */
int mcorb_dev_rel_solve_selftest(int device, int n, int ncams, const mcorb_track_cam *cams, const int32_t *cam1, const double *uv1,
                                 const int32_t *cam2, const double *uv2, int32_t *count, double *R, double *t);
/* test hook, host: the scores of n matches at the pose (R, t); a NaN is the default quiet NaN */
int mcorb_rel_eval(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam1, const double *uv1, const int32_t *cam2,
                   const double *uv2, const double *R, const double *t, double *score);

/* The polish of the winner over its inliers: opt-in, mcorb_lmap_relative_pose itself is as it was.  Stated, not recalled: OpenGV's
 * optimizeModelCoefficients for this problem is not in the tree and the reference does not call it.
 * rounds: 1 .. MCORB_REL_POLISH_ROUNDS; max_iterations: the solves of a round, 1 .. MCORB_REL_POLISH_MAX_ITERATIONS */
#define MCORB_REL_POLISH_ROUNDS 2
#define MCORB_REL_POLISH_MAX_ITERATIONS 100
typedef struct mcorb_rel_polish_params {
    int32_t rounds, max_iterations;
} mcorb_rel_polish_params;
/* a round: its members, the solves it took and its MCORB_POSE_* status, the cost (the sum over the members of 2 score / threshold;
 * a NaN is the default quiet NaN) at its start and its end, the inliers of all matches at its result, and whether that result
 * replaced the current pose (n_inliers >= the current count) */
typedef struct mcorb_rel_polish_round {
    double cost_initial, cost_final;
    int32_t n_members, iterations, status, n_inliers, accepted, reserved;
} mcorb_rel_polish_round;
/* (R, t) and n_inliers: the RANSAC winner's, what mcorb_lmap_relative_pose returns; round[k]: zero for a round that did not run;
 * rounds_run: the rounds that ran, a refused one included */
typedef struct mcorb_rel_polish {
    double R[9], t[3];
    mcorb_rel_polish_round round[MCORB_REL_POLISH_ROUNDS];
    int32_t n_inliers, rounds_run;
} mcorb_rel_polish;
/* mcorb_lmap_relative_pose followed by the polish (csrc/mcorb_rel.h), fp64, one IEEE operation per operator in the order written:
 * - the residual of a match at a pose: with the score's a, b, w, P1 and P2 the 6-vector (a - P1 / |P1|, b / |b| - P2 / |P2|) / sqrt(
 *   threshold); its squared length is 2 score / threshold.
 * - the Jacobian: forward differences through the Cayley retraction of mcorb_lmap_refine_pose, h = 2^-20 per unknown.
 * - a round: mcorb_lmap_refine_pose's Levenberg-Marquardt (its damping, schedule and stops) from the current pose over the round's
 *   members, the 28 sums added in the tree of 256 lanes; then all n matches are scored at the result, and it replaces the current
 *   pose, flags and count iff its count is at least the current count -- otherwise polishing ends.  Round 1's members are the
 *   winner's inliers, round 2's are round 1's.
 * res->R, t, n_inliers and the flags are the accepted pose's; best_hypothesis, sample and n_models stay the winner's.  Without a
 * winner (MCORB_REL_NO_OBS, MCORB_REL_NO_MODEL) no round runs.  A device store runs k_rel_hypotheses, k_rel_score, k_rel_pick and
 * k_rel_fit (one workgroup) in one submission with one wait; a host-only store gives the same bits.  Refused before anything runs:
 * what mcorb_lmap_relative_pose refuses, a NULL pp or polish, rounds or max_iterations outside their ranges */
int mcorb_lmap_relative_pose_polished(mcorb_lmap *m, int n, const int32_t *cam1, const float *uv1, const int32_t *cam2, const float *uv2,
                                      int ncams, const mcorb_track_cam *cams, const mcorb_rel_params *params,
                                      const mcorb_rel_polish_params *pp, mcorb_rel_result *res, uint8_t *inlier, mcorb_rel_polish *polish);
/* mcorb_lmap_last_relative_timing with us[3]: k_rel_fit of the last polished call (0 before one) */
int mcorb_lmap_last_relative_timing4(mcorb_lmap *m, float us[4], int *n_hyp);
/* test hook, host: the polish of the given pose (R, t) over the given members (member[n], nonzero: in) of n matches, keypoints in
 * double as in the other mcorb_rel_* hooks.  The current count and flags are those of (R, t) at the threshold over all n matches.
 * -> the polish record (its R, t, n_inliers: the pose handed in and its count), the accepted pose and its flags (inlier[n]) */
int mcorb_rel_polish_run(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam1, const double *uv1, const int32_t *cam2,
                         const double *uv2, const uint8_t *member, const double *R, const double *t, double threshold,
                         const mcorb_rel_polish_params *pp, mcorb_rel_polish *polish, double *R_out, double *t_out, uint8_t *inlier);

/* ------------------------------------------------------------------------- */
/* The rig pose between two frames from 3D-3D correspondences: the third       */
/* estimator of FrontEnd::estimatePoseLF, PC_ALIGN (MCSlam/src/FrontEnd.cpp:   */
/* 4421-4440), FrontEnd::poseFromPCAlignment (:4441-4530).  Its live code is   */
/* OpenGV's point_cloud::optimize_nonlinear over all correspondences (mode 0); */
/* what its SAC argument is for is commented out there: sac::Ransac<           */
/* PointCloudSacProblem> (mode 1).  OpenGV is not in the tree: its distance    */
/* and sample size are recalled; the draws, the solver (Horn's closed form)    */
/* and the absence of the adaptive stop are stated.     */
/* ------------------------------------------------------------------------- */
#define MCORB_ALIGN_MAX_ITERATIONS 16384
#define MCORB_ALIGN_SAMPLE 3
#define MCORB_ALIGN_OK 0            /* there is an answer */
#define MCORB_ALIGN_NO_OBS 1        /* no pairs: the identity, nothing ran */
#define MCORB_ALIGN_NO_MODEL 2      /* mode 0: the fit is not valid; mode 1: no hypothesis had a model (fewer than 3 pairs, collinear
                                       points): the identity, every flag 0, mean_error 0 */
#define MCORB_ALIGN_MODE_ALL 0      /* the least-squares fit over all pairs: the reference's live code */
#define MCORB_ALIGN_MODE_SAC 1      /* RANSAC on samples of three pairs: the reference's commented code */
#define MCORB_ALIGN_USED_SAC 0      /* the answer is the winning hypothesis (also: there is no answer) */
#define MCORB_ALIGN_USED_FIT 1      /* the answer is a least-squares fit: mode 0's, or mode 1's refit over the winner's inliers */
/* threshold: mode 1's, on |p1 - (R p2 + t)| in the points' unit (the reference's is 0.2); inlier_dist: the reference's verdict on
 * the same distance with the answer (0.1 there), both modes; seed: of the draws; max_iterations: mode 1's hypotheses, 1 ..
 * MCORB_ALIGN_MAX_ITERATIONS (the reference's 100), all examined; mode: MCORB_ALIGN_MODE_*; refit: mode 1 -- non-zero: the answer is
 * the least-squares fit over the winner's inliers at `threshold` where that fit is valid */
typedef struct mcorb_align_params {
    double threshold, inlier_dist;
    uint64_t seed;
    int32_t max_iterations, mode, refit, reserved;
} mcorb_align_params;
/* (R, t) = b1_T_b2 of the answer, R row-major: X_1 = R X_2 + t, the reference's T (:4509-4514); (sac_R, sac_t): mode 1's winning
 * hypothesis (the identity in mode 0 and without one); mean_error: the mean of |p1 - (R p2 + t)| over all n pairs with the answer
 * (a NaN is the default quiet NaN); status: MCORB_ALIGN_*; used: MCORB_ALIGN_USED_*; n_inliers: the pairs with distance <
 * inlier_dist, what the reference returns; n_matches: n; sac_n_inliers: the winner's count at `threshold`; best_hypothesis (-1:
 * none); sample: the winner's three pairs in draw order; n_models: the hypotheses that had a model */
typedef struct mcorb_align_result {
    double R[9], t[3], sac_R[9], sac_t[3], mean_error;
    int32_t status, used, n_inliers, n_matches, sac_n_inliers, best_hypothesis, sample[MCORB_ALIGN_SAMPLE], n_models;
} mcorb_align_result;
/* The pose of a rig's second frame in its first from n pairs of triangulated points.  Pair i is pts2[i] (lf_cur->points_3D[m.
 * trainIdx]) and either pts1[i] (lf_prev->points_3D[m.queryIdx]) or the point of the store's landmark lids1[i] (map->getLandmark(
 * l_id)->pt3D, :4447-4455): exactly one of lids1 and pts1 is given; points are 3 doubles each.  All arithmetic is fp64, one IEEE
 * operation per operator in the order written (csrc/mcorb_align.h), + - * /, comparisons and sqrt:
 * - the distance of a pair at a pose: |p1 - (R p2 + t)|; an inlier iff distance < the limit, strictly; a NaN is no inlier.
 * - align_fit over a set of pairs (stated; Horn's unit-quaternion absolute orientation): the centroids, then M = sum (p2 - c2)
 *   (p1 - c1)^T, each sum in a fixed order -- member i in lane i mod 256, each lane in ascending i, the lanes folded per block of 64
 *   with strides 32 .. 1 and the four blocks as (b0 + b1) + (b2 + b3); the eigenvector of the largest eigenvalue of Horn's
 *   symmetric 4 x 4 matrix by six sweeps of cyclic Jacobi; R from that quaternion, t = c1 - R c2.  Not valid: fewer than 3
 *   members, a number that is not finite, or l1 - l2 <= 1e-12 (l1 - l4) of the eigenvalues (collinear members).
 * - mode 0: align_fit over all pairs.
 * - mode 1: hypothesis h draws 3 distinct pairs by mcorb_lmap_relative_pose's walk on the draws j = 0 .. 2 (the splitmix64
 *   finaliser of seed + 0x9E3779B97F4A7C15 (1 + 32 h + j)); its model is align_fit on them; the largest count over all n pairs at
 *   `threshold` wins, a tie goes to the lowest hypothesis, a hypothesis without a model never wins; no adaptive stop.  With
 *   refit the answer is align_fit over the winner's inliers, or the winner where that fit is not valid.
 * - then the reference's verdict at inlier_dist with the answer: the flags, their count, the mean distance.
 * A device store runs k_align_hypotheses, k_align_score, k_align_pick and k_align_fit (mode 0: k_align_fit alone) in one
 * submission on its stream with one wait and reads lids1's points from its own landmark array on the device; a host-only store
 * runs the same header serially: the results are equal bit for bit.  The store's landmarks are never written.  inlier (may be
 * NULL): one flag per pair.  Refused before anything runs, the store unchanged: MCORB_E_ARG for a NULL, both or neither of lids1
 * and pts1, n < 0, a lid that is not a slot with a point, a threshold or inlier_dist that is not finite and positive,
 * max_iterations outside 1 .. MCORB_ALIGN_MAX_ITERATIONS in mode 1, an unknown mode; MCORB_E_STATE while a tracking call is
 * pending. */
int mcorb_lmap_align_pose(mcorb_lmap *m, int n, const int32_t *lids1, const double *pts1, const double *pts2,
                          const mcorb_align_params *params, mcorb_align_result *res, uint8_t *inlier);
/* a device store's last k_align_hypotheses (us[0]), k_align_score (us[1]), k_align_pick (us[2]) and k_align_fit (us[3]) launch,
 * microseconds between HIP events, and the hypotheses of the last mode-1 launch; a call without pairs launches nothing and leaves
 * them; mode 0 leaves us[0 .. 2] and the hypotheses and sets us[3] */
int mcorb_lmap_last_align_timing(mcorb_lmap *m, float us[4], int *n_hyp);
/* test hook: the counts of all hypotheses of the last mode-1 call that ran any, and whether each had a model; a device store
 * copies them down from where k_align_score left them.  MCORB_E_CAP (with n_hyp set) when cap < n_hyp */
int mcorb_lmap_last_align_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, int cap, int *n_hyp);
/* test hook, host: align_fit over the pairs i of (p1, p2: n x 3 doubles) with member[i] != 0 (member NULL: all) -> 1 with (R as
 * 9, t as 3 doubles) = b1_T_b2, 0 when the fit is not valid (R, t are then what it computed), or a negative error.  gap (may be
 * NULL): (l1 - l2) / (l1 - l4) of Horn's matrix, a NaN as the default quiet NaN */
int mcorb_align_solve(int n, const double *p1, const double *p2, const uint8_t *member, double *R, double *t, double *gap);
/* test hook, device: mcorb_align_solve on n problems in one launch, a workgroup of k_align_fit's shape and fit passes each --
 * problem i has npairs[i] pairs, the problems' pairs back to back in p1, p2 and member (one byte a pair; none may be NULL unless
 * no problem has a pair) -> valid[n], R (n x 9), t (n x 3), zero without a valid fit, gap[n].  n == 0 launches nothing */
int mcorb_dev_align_solve_selftest(int device, int n, const int32_t *npairs, const double *p1, const double *p2, const uint8_t *member,
                                   int32_t *valid, double *R, double *t, double *gap);
/* test hook, host: the distances of n pairs at the pose (R, t); a NaN is the default quiet NaN */
int mcorb_align_eval(int n, const double *p1, const double *p2, const double *R, const double *t, double *dist);

/* ------------------------------------------------------------------------- */
/* The pose of one camera between two frames from 2D-2D matches: what the      */
/* reference gets from cv::findEssentialMat(..., RANSAC, prob, thr, mask) and  */
/* cv::recoverPose(...) in the one-camera arm of its bootstrap (MCSlam/src/    */
/* FrontEnd.cpp:2591-2628) and at six more places (:2105, :3023, :6842, :6959, */
/* :7142, :7172).  OpenCV is not in the tree: the Sampson distance and         */
/* recoverPose's cheirality vote are recalled; the draws, the minimal solver,  */
/* the absence of the adaptive stop, the triangulation inside the vote and the */
/* rotations from E are stated.                         */
/* ------------------------------------------------------------------------- */
#define MCORB_ESS_MAX_ITERATIONS 16384
#define MCORB_ESS_SAMPLE 5
#define MCORB_ESS_MAX_ROOTS 10     /* the models of a hypothesis: slot 10 h + c is root c of hypothesis h */
#define MCORB_ESS_OK 0            /* a model won */
#define MCORB_ESS_NO_OBS 1        /* no matches: the identity, nothing ran */
#define MCORB_ESS_NO_MODEL 2      /* no hypothesis had a model (fewer than 5 matches among the causes): the identity, every flag 0 */
/* threshold_px: findEssentialMat's, in pixels (the reference passes 1.0 or 0.5); distance_thresh: recoverPose's, in units of the
 * baseline (OpenCV's default is 50); seed: of the draws; max_iterations: the hypotheses, 1 .. MCORB_ESS_MAX_ITERATIONS, all of
 * them examined (the reference's `prob` has no counterpart; OpenCV's cap is 1000) */
typedef struct mcorb_ess_params {
    double threshold_px, distance_thresh;
    uint64_t seed;
    int32_t max_iterations, reserved;
} mcorb_ess_params;
/* (R, t) = c1_T_c2, R row-major: X_c1 = R X_c2 + t with |t| = 1, what :2620-2625 put into T (the identity without a winner); E:
 * the winning model, x1^T E x2 = 0 on normalised points, |E|_F^2 = 2; status: MCORB_ESS_*; n_matches: n; n_ransac_inliers: the
 * winner's count at the threshold; n_inliers: those of them that pass the winning candidate's depth test, the flags set;
 * best_hypothesis, best_root (-1: none); sample: the winner's five matches in draw order; n_models: the (hypothesis, root) slots
 * that had a model; cheirality: the four candidates' counts in the order (R+, t^), (R-, t^), (R+, -t^), (R-, -t^) */
typedef struct mcorb_ess_result {
    double R[9], t[3], E[9];
    int32_t status, n_matches, n_ransac_inliers, n_inliers, best_hypothesis, best_root, sample[MCORB_ESS_SAMPLE], n_models, cheirality[4],
        reserved;
} mcorb_ess_result;
/* The pose of a camera's second frame in its first from n matches: uv1[i] (KeyPoint::pt) in frame 1, uv2[i] in frame 2.  Of cam
 * only fx, fy, s, u0, v0 are read.  All arithmetic is fp64, one IEEE operation per operator in the order written
 * (csrc/mcorb_ess.h), + - * /, comparisons and sqrt:
 * - the points: y = (v - v0) / fy, x = ((u - u0) - s y) / fx; the bearing is (x, y, 1) / sqrt((x x + y y) + 1).
 * - the sample: 5 distinct matches by mcorb_lmap_relative_pose's walk on the draws j = 0 .. 4.  n < 5: no model.
 * - the solver (stated): an orthonormal basis X, Y, Z, W of the null space of the five rows vec(d1 d2^T); the ten cubics of E = x X
 *   + y Y + z Z + W (2 E E^T E - tr(E E^T) E and det E) as a 10 x 10 matrix C(z) over x^3, x^2 y, x y^2, y^3, x^2, x y, y^2, x, y, 1;
 *   det C(z) at 11 fixed nodes by LU with partial pivoting and a constant 11 x 11 table for its 11 coefficients; the real roots
 *   by the chain of derivatives with 48 bisections per bracket; per root, in ascending z, (x, y) from C(z) and three Gauss-Newton
 *   steps on the ten cubics; the model is kept iff it is finite and its residuals on the sample's five rows and on the ten
 *   cubics are below 1e-9.  At most 10 models per hypothesis.
 * - the score (OpenCV's Sampson distance, recalled): r = x1^T E x2, a = E x2, b = E^T x1, err = r r / (a0 a0 + a1 a1 + b0 b0 + b1
 *   b1); a match is an inlier iff err < (threshold_px / ((fx + fy) / 2))^2, strictly; a NaN is no inlier.
 * - the consensus: the largest count over all n matches wins, a tie goes to the lowest hypothesis, then to the lowest root.
 * - the pose (recoverPose's vote, recalled; the rotations and the triangulation stated): t^ the longest cross product of E's
 *   columns, R+- = cof(E) -+ [t^]x E with three polar steps; over the winner's inliers each of the four candidates counts the
 *   matches whose midpoint of mcorb_lmap_relative_pose's score has z strictly inside (0, distance_thresh) in both cameras; the
 *   largest count wins, a tie goes to the lowest candidate; the flags are the inliers that pass the winner's test.
 * A device store runs k_ess_hypotheses, k_ess_score, k_ess_pick and k_ess_finish in one submission on its stream with one wait;
 * a host-only store runs the same header serially: the results are equal bit for bit.  The store's landmarks are neither read
 * nor written.  inlier (may be NULL): one flag per match.  Refused before anything runs: MCORB_E_ARG for a NULL, n < 0, a
 * threshold, distance or focal length that is not finite and positive, max_iterations outside 1 .. MCORB_ESS_MAX_ITERATIONS;
 * MCORB_E_STATE while a tracking call is pending. */
int mcorb_lmap_essential_pose(mcorb_lmap *m, int n, const float *uv1, const float *uv2, const mcorb_track_cam *cam,
                              const mcorb_ess_params *params, mcorb_ess_result *res, uint8_t *inlier);
/* a device store's last k_ess_hypotheses (us[0]), k_ess_score (us[1]), k_ess_pick (us[2]) and k_ess_finish (us[3]) launch,
 * microseconds between HIP events, and its hypotheses; a call without matches launches nothing and leaves them */
int mcorb_lmap_last_essential_timing(mcorb_lmap *m, float us[4], int *n_hyp);
/* test hook: the counts of all 10 n_hyp slots of the last call that ran any, whether each had a model (a slot without one has
 * count 0) and (models may be NULL) their E, 9 doubles per slot; a device store copies them down from where its kernels left
 * them.  MCORB_E_CAP (with n_slots set) when cap < n_slots */
int mcorb_lmap_last_essential_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, double *models, int cap, int *n_slots);
/* test hook, host: the solver on 5 matches (uv1, uv2: 5 x 2) -> the number of models, their E (9 doubles each, at most 10) in E
 * and (z may be NULL) the root each came from before its Gauss-Newton steps, ascending; or a negative error.  The hooks take the
 * keypoints in double: a float's value gives the bits mcorb_lmap_essential_pose computes from that float */
int mcorb_ess_solve(const mcorb_track_cam *cam, const double *uv1, const double *uv2, double *E, double *z);
/* test hook, device: mcorb_ess_solve on n problems in one launch of k_ess_hypotheses' shape and body, sixteen lanes a problem and
 * four problems a workgroup -- cam[n], uv1 and uv2 (n x 5 x 2) -> count[n], E (n x 10 x 9) and z (n x 10), zero behind a
 * problem's count.  n == 0 launches nothing */
int mcorb_dev_ess_solve_selftest(int device, int n, const mcorb_track_cam *cam, const double *uv1, const double *uv2, int32_t *count, double *E,
                                 double *z);
/* test hook, host: the Sampson values of n matches at E; a NaN is the default quiet NaN */
int mcorb_ess_eval(const mcorb_track_cam *cam, int n, const double *uv1, const double *uv2, const double *E, double *err);
/* test hook, host: the four candidates of E -- Rp, Rm (9 doubles each) and t^ -- and, where n > 0, the depths of the n matches in
 * both cameras under each: depth[(4 i + c) * 2 + {0, 1}] */
int mcorb_ess_decompose(const double *E, double *Rp, double *Rm, double *t, const mcorb_track_cam *cam, int n, const double *uv1,
                        const double *uv2, double *depth);

/* The polish of the winner over its inliers: opt-in, mcorb_lmap_essential_pose itself is as it was.  Stated, not recalled: OpenCV
 * has no such step behind recoverPose and the reference calls none (deviation 6).
 * rounds: 1 .. MCORB_ESS_POLISH_ROUNDS; max_iterations: the solves of a round, 1 .. MCORB_ESS_POLISH_MAX_ITERATIONS */
#define MCORB_ESS_POLISH_ROUNDS 2
#define MCORB_ESS_POLISH_MAX_ITERATIONS 100
typedef struct mcorb_ess_polish_params {
    int32_t rounds, max_iterations;
} mcorb_ess_polish_params;
/* a round: its members, the solves it took and its MCORB_POSE_* status, the cost (the sum over the members of err / thr^2; a NaN is
 * the default quiet NaN) at its start and its end, the matches within the threshold (n_ransac_inliers) and those of them that
 * pass the depth test (n_inliers) of all matches at its result, and whether that result replaced the current pose (n_inliers >=
 * the current n_inliers) */
typedef struct mcorb_ess_polish_round {
    double cost_initial, cost_final;
    int32_t n_members, iterations, status, n_ransac_inliers, n_inliers, accepted;
} mcorb_ess_polish_round;
/* R, t, E and both counts: the RANSAC winner's, what mcorb_lmap_essential_pose returns; round[k]: zero for a round that did not
 * run; rounds_run: the rounds that ran, a refused one included */
typedef struct mcorb_ess_polish {
    double R[9], t[3], E[9];
    mcorb_ess_polish_round round[MCORB_ESS_POLISH_ROUNDS];
    int32_t n_ransac_inliers, n_inliers, rounds_run, reserved;
} mcorb_ess_polish;
/* mcorb_lmap_essential_pose followed by the polish (csrc/mcorb_ess_polish.h), fp64, one IEEE operation per operator in the order
 * written:
 * - the unknowns: five, delta[0 .. 2] a rotation and delta[3 .. 4] a move of t in its tangent plane (the Sampson value does not
 *   depend on |t|).  The retraction: R' = R C(delta[0 .. 2]) with mcorb_lmap_refine_pose's Cayley matrix, t' = u / |u| with u = (t +
 *   delta[3] b1) + delta[4] b2, b1 = (t x e_k) / |t x e_k| for the smallest |t_k| (the first of equals), b2 = t x b1.
 * - the residual of a match: with E = [t]x R and the score's r, a, b: (r / sqrt(((a0 a0 + a1 a1) + b0 b0) + b1 b1)) * (1 / thr), thr =
 *   threshold_px / ((fx + fy) / 2); its square is err / thr^2.
 * - the Jacobian: forward differences through the retraction, h = 2^-20 per unknown.
 * - the solve: mcorb_lmap_refine_pose's on five unknowns; with fewer than five members (fewer residuals than unknowns) it is
 *   refused whatever the damping, and the round ends in MCORB_POSE_NO_STEP.
 * - a round: mcorb_lmap_refine_pose's Levenberg-Marquardt (its damping, schedule and stops) on the five unknowns from the current
 *   pose over the round's members, the 21 sums added in the tree of 256 lanes; then all n matches are tested at the result (err <
 *   thr^2, strictly, and the depths strictly inside (0, distance_thresh) in both cameras), and it replaces the current pose, E,
 *   flags and both counts iff its n_inliers is at least the current one -- otherwise polishing ends.  Round 1's members are the
 *   winner's flags, round 2's are round 1's.  The four-candidate vote is not run again.
 * res->R, t, E, n_ransac_inliers, n_inliers and the flags are the accepted pose's (E = [t]x R after an accepted round);
 * cheirality, best_hypothesis, best_root, sample and n_models stay the winner's.  Without a winner (MCORB_ESS_NO_OBS,
 * MCORB_ESS_NO_MODEL) no round runs.  A device store runs k_ess_hypotheses, k_ess_score, k_ess_pick, k_ess_finish and k_ess_fit (one
 * workgroup) in one submission with one wait; a host-only store gives the same bits.  Refused before anything runs: what
 * mcorb_lmap_essential_pose refuses, a NULL pp or polish, rounds or max_iterations outside their ranges */
int mcorb_lmap_essential_pose_polished(mcorb_lmap *m, int n, const float *uv1, const float *uv2, const mcorb_track_cam *cam,
                                       const mcorb_ess_params *params, const mcorb_ess_polish_params *pp, mcorb_ess_result *res,
                                       uint8_t *inlier, mcorb_ess_polish *polish);
/* mcorb_lmap_last_essential_timing with us[4]: k_ess_fit of the last polished call (0 before one) */
int mcorb_lmap_last_essential_timing5(mcorb_lmap *m, float us[5], int *n_hyp);
/* test hook, host: the polish of the given pose (R, t), |t| = 1, over the given members (member[n], nonzero: in) of n matches,
 * keypoints in double as in the other mcorb_ess_* hooks.  The current counts and flags are those of (R, t) itself over all n matches
 * (E = [t]x R).  -> the polish record (its R, t, E and counts: the pose handed in and its own), the accepted pose, its E and its
 * flags (inlier[n]) */
int mcorb_ess_polish_run(const mcorb_track_cam *cam, int n, const double *uv1, const double *uv2, const uint8_t *member, const double *R,
                         const double *t, double threshold_px, double distance_thresh, const mcorb_ess_polish_params *pp,
                         mcorb_ess_polish *polish, double *R_out, double *t_out, double *E_out, uint8_t *inlier);

/* ------------------------------------------------------------------------- */
/* Host stages exposed for the CPU test-suite (no device needed)              */
/* ------------------------------------------------------------------------- */
/* The engine's quad-tree selection, DistributeOctTree's equivalent (ORBextractor.cpp:554-778), run
 * end to end on the host: the candidate bucketing that k_compact performs on the device is
 * restated on the CPU, then the host tree logic runs on it.  packed = (y<<20 | x<<8 | response),
 * x/y relative to minBorder, in vToDistributeKeys order (the "first maximum wins" tie of the final
 * pick follows the input order); wCell/hCell = cell grid of the detection loop, from which the same
 * order (cell row, cell col, y, x) is recovered for nodes deeper than the bucketing (pass 0,0 when
 * the candidates are in plain raster order).  out_idx receives indices into `packed` in result
 * order.  Returns the count, MCORB_E_SIZE, or MCORB_E_CAP. */
int mcorb_host_select(const uint32_t *packed, int n, int minX, int maxX, int minY, int maxY,
                      int nfeatures_level, int wCell, int hCell, int32_t *out_idx, int cap);
/* The engine's cv::resize coefficient table for one axis: per destination index
 * (s0, s1, c0, c1) as int32 quadruples (x axis: clamped per HResizeLinear; y axis:
 * row indices clipped, fraction kept). */
int mcorb_host_resize_axis(int ssize, int dsize, int is_x, int32_t *quads);
/* level geometry the engine derives for a w x h image: per level
 * {w, h, nCols, nRows, wCell, hCell}; returns MCORB_OK or MCORB_E_SIZE */
int mcorb_host_geometry(const mcorb_params *p, int w, int h, int32_t *six_per_level);
/* the N-view DLT triangulation of mcorb_rig_obtain_lf_features alone (cv::sfm::triangulatePoints for one point):
 * x = nv normalised image points (x0, y0, x1, y1, ..), P = nv row-major 3x4 [R|t], 2 <= nv <= MCORB_MAX_CAMS */
int mcorb_host_triangulate(const double *x, const double *P, int nv, double X[3]);
/* the same, also giving the null-vector solver's exit (the codes of mcorb_dev_triangulate_selftest) */
int mcorb_host_triangulate_branch(const double *x, const double *P, int nv, double X[3], int32_t *branch);
/* the pixel coordinate of a keypoint coordinate as the de-duplication of mcorb_lmap_track takes it (step 5): truncation toward zero
 * for |v| < 2^31, INT32_MIN otherwise, a NaN included.  The function the host tail and k_track_dedup_min share */
int32_t mcorb_host_track_pixel(float v);

/* ------------------------------------------------------------------------- */
/* Synthetic input; host utility, see csrc/mcorb_synth.c       */
/* ------------------------------------------------------------------------- */
int mcorb_synth_rig_frame(uint32_t frame, int ncams, int cam, int w, int h, uint8_t *out, int stride);

#ifdef __cplusplus
}
#endif
#endif
