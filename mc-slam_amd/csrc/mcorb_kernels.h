// mcorb_kernels.h -- launch wrappers of the gfx950 kernels (mcorb_kernels.hip, mcorb_select_gpu.hip, mcorb_handoff_gpu.hip,
// mcorb_bow_gpu.hip, mcorb_lf_gpu.hip, mcorb_kfdb_gpu.hip, mcorb_lmap_gpu.hip, mcorb_mapping_gpu.hip, mcorb_landmark_gpu.hip,
// mcorb_track_gpu.hip, mcorb_pose_gpu.hip, mcorb_sac_gpu.hip, mcorb_rel_gpu.hip, mcorb_ess_gpu.hip, mcorb_align_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/mcorb.h"
#include "mcorb_align.h"
#include "mcorb_ba.h"
#include "mcorb_retri.h"
#include "mcorb_common.h"
#include "mcorb_init.h"
#include "mcorb_mapping_new.h"
#include "mcorb_pose.h"
#include "mcorb_ess.h"
#include "mcorb_ess_polish.h"
#include "mcorb_rel.h"
#include "mcorb_sac.h"
#include "mcorb_signal.h"
#include "mcorb_track.h"
#include "mcorb_undistort.h"
#include "mcorb_undistort_image.h"

namespace mcorb {

constexpr int kKnnChunk = 4096;  // train descriptors per k-NN partial (one workgroup column); the in-chunk index must stay below 8192
// Chunk length a launch of `npairs` camera pairs uses.  A workgroup walks one chunk of the train set for 256 queries: with the
// 192 pairs of a 32-frame batch that is 1 536 workgroups of 63 tiles, plenty; the 6 pairs of ONE rig frame (how MC-SLAM calls
// the front-end) are 48 workgroups on 256 CUs, each walking all 63 tiles: 44 us of a 0.6 ms frame.  Few pairs -> short chunks
// -> more, shorter workgroups (the partials are merged by k_knn2_finalize either way).  Multiples of 64 (one LDS stage).
__host__ __device__ inline int knn_chunk_len(int npairs) { return npairs <= 12 ? 256 : npairs <= 24 ? 512 : npairs <= 48 ? 1024 : kKnnChunk; }
// The accepted (query << 16 | train) pairs of a camera pair come back in blocks of 256 queries: mlist[pair][block * 256 + k],
// k < mcount[pair * knn_qblocks(kcap) + block]; blocks are in query order (concatenate them).
constexpr int kKnnQueriesPerBlock = 256;   // = the k-NN workgroup's queries (64 per wave x 4 waves; static_assert in mcorb_kernels.hip)
inline int knn_qblocks(int kcap) { return (kcap + kKnnQueriesPerBlock - 1) / kKnnQueriesPerBlock; }
inline size_t knn_mlist_stride(int kcap) { return (size_t)knn_qblocks(kcap) * kKnnQueriesPerBlock; }
// partials (uint2) a slot needs for jobs of up to max_pairs pairs at capacity kcap
inline size_t knn_part_entries(int max_pairs, int kcap)
{
    size_t need = 0;
    for (int np : {12, 24, 48, max_pairs}) {
        const int n = np < max_pairs ? np : max_pairs, cl = knn_chunk_len(n);
        const size_t e = (size_t)n * ((kcap + cl - 1) / cl) * kcap;
        need = need > e ? need : e;
    }
    return need;
}
constexpr int kKnnExpandBytes = 128;   // bytes of one descriptor expanded to 256 e2m1 nibbles of +-1 (k_expand)

// one row of the knnMatch(k=2) table, 8 bytes so the PCIe write-back stays small:
// idx = trainIdx0 | trainIdx1 << 16 (0xffff = absent), d = dist0 | dist1 << 9 | accept << 18
// (accept = BruteForceMatch's ratio + threshold test)
struct KnnRow { uint32_t idx, d; };
__host__ __device__ inline int knn_idx0(const KnnRow &r) { return (r.idx & 0xffffu) == 0xffffu ? -1 : (int)(r.idx & 0xffffu); }
__host__ __device__ inline int knn_idx1(const KnnRow &r) { return (r.idx >> 16) == 0xffffu ? -1 : (int)(r.idx >> 16); }
__host__ __device__ inline int knn_d0(const KnnRow &r) { return knn_idx0(r) < 0 ? -1 : (int)(r.d & 0x1ffu); }
__host__ __device__ inline int knn_d1(const KnnRow &r) { return knn_idx1(r) < 0 ? -1 : (int)((r.d >> 9) & 0x1ffu); }
__host__ __device__ inline bool knn_accept(const KnnRow &r) { return (r.d >> 18) & 1u; }

hipError_t upload_umax(const int umax[16]);
void launch_stage_f32(hipStream_t st, const float *src, int w, int h, int pitch_f, int channels, size_t img_stride_f,
                      uint8_t *pyr, const Geom &g, int nimg);
// cv::undistort at the hand-off (mcorb_rig_set_image_undistortion).  A camera's maps on the device: rows padded with zero entries
// to remap_map_pitch(w) (k_remap_u8 loads four entries at a time), map1 as (x, y) pairs of shorts; mode 0: not set, copied through
struct RemapCam { const int16_t *map1; const uint16_t *map2; int32_t mode, pad; };
__host__ __device__ inline int remap_map_pitch(int w) { return (w + 3) & ~3; }
// upload_f32's conversion into the raw planes (image m at m * w * h, row stride w) instead of level 0
void launch_stage_f32_raw(hipStream_t st, const float *src, int w, int h, int pitch_f, int channels, size_t img_stride_f,
                          uint8_t *raw, int nimg);
// level 0 of images [0, nimg) from their raw planes: image m is camera m % ncams
void launch_remap_u8(hipStream_t st, const uint8_t *raw, uint8_t *pyr, const Geom &g, const RemapCam *cams, int ncams, int nimg);
// win[2*l], win[2*l+1]: LDS source-window pitch (bytes, multiple of 4) and rows of level l's resize workgroups
void launch_pyramid(hipStream_t st, uint8_t *pyr, const Geom &g, const ResizeTap *tabs, const int *win, int nimg);
// k_fast_cells' per-cell records for this geometry (built once per rig, uploaded by the caller): ROI origin, size,
// pass-1 lane layout; appended to `tab`, returns their dword offset
int fast_cell_table(const Geom &g, std::vector<uint32_t> &tab);
void launch_fast(hipStream_t st, const uint8_t *pyr, const Geom &g, int iniTh, int minTh, const uint32_t *cellRec,
                 uint32_t *cell_kp, int *cell_cnt, int nimg);
// tbl: device table blocks (tbl_ints(g.bucketTotal) ints per image, layout in mcorb_common.h); cand / overflow: host-mapped
// lut: path-code tables (LevelGeom::lutx / luty); one_copy: one table copy in LDS even where four fit (a rig's MCORB_COMPACT_ONE_COPY)
void launch_compact(hipStream_t st, const uint32_t *cell_kp, const int *cell_cnt, const Geom &g, const uint16_t *lut,
                    uint32_t *sorted_dev, uint32_t *cand, int *tbl, int *overflow, int nimg, bool one_copy = false);
void launch_blur(hipStream_t st, const uint8_t *pyr, uint8_t *blur, const Geom &g, int nimg);
void launch_describe(hipStream_t st, const uint8_t *pyr, const uint8_t *blur, const Geom &g, const uint32_t *sel,
                     const int *nsel, int orientation, uint8_t *desc, float *angles, int nimg,
                     uint8_t *desc_host = nullptr);   // desc_host (k_describe_fused only): host-mapped second destination
// desc / counts: `kcap`-strided bit descriptors and their counts; setmap[i] (null = identity) = the set that becomes local
// set i, i < nsets; pairs: (query, train) LOCAL set indices; expanded: nsets * kcap * kKnnExpandBytes bytes of scratch;
// lcounts: nsets ints (receives the clamped counts); part: knn_part_entries(max pairs per launch, kcap) partials
void launch_knn2(hipStream_t st, const uint8_t *desc, const int *counts, const int *setmap, int nsets, const int2 *pairs, int npairs,
                 int kcap, void *expanded, int *lcounts, uint2 *part, float dist_thresh, float ratio, KnnRow *out, uint32_t *mlist,
                 int *mcount, hipEvent_t ev_exp, hipEvent_t ev_mid);   // events (optional): after k_expand, after k_knn2

// DistributeOctTree's list discipline + operator()'s assembly on the GPU (mcorb_select_gpu.hip).  tbl: k_compact's device table
// blocks, sorted: its bucket-sorted candidate lists (read only where a tree goes below the bucketing depth); sel_val / sel_cnt: select_cap(g) retained candidates and their count per (image, level), -1 = the level needs the host
// stage (fallback |= 1); sel / nsel: what the descriptor kernel and the matcher read; resp / mono: FAST responses and monoIndex
// for the host's keypoint records; fallback bit 1 = more than kcap keypoints.
int select_cap(const Geom &g);
bool select_fits(const Geom &g);   // false: the level trees of this geometry do not fit a wave's LDS (very large feature budgets)
hipError_t configure_select(const Geom &g);   // a rig that selects on the GPU calls this once, with its device current, before its first job
// deep_cap: a bucket with more candidates than this is not scanned node by node when a tree goes below the bucketing depth
// prof: shader-clock stamps of k_select's phases on stderr (a rig's MCORB_SELECT_PROF)
hipError_t launch_select(hipStream_t st, const int *tbl, const uint32_t *sorted, const Geom &g, uint32_t *sel_val, int *sel_cnt, int *fallback, int nimg,
                         int deep_cap = 4096, bool prof = false);
void launch_assemble(hipStream_t st, const uint32_t *sel_val, const int *sel_cnt, const Geom &g, const float *scale, int lap0, int lap1,
                     uint32_t *sel, uint8_t *resp, int *nsel, int *mono, int *fallback, int nimg,
                     // optional (all or none): host-mapped copies of sel / resp and a per-image signal word set behind them
                     uint32_t *sel_h = nullptr, uint8_t *resp_h = nullptr, unsigned long long *sig_h = nullptr);
// (the signal word of an image, k_assemble -> host: mcorb_signal.h)
// test hook: std::sort's permutation of n 64-bit entries (upper halves compared) by one wave (wave_std_sort)
hipError_t sort_selftest(const uint64_t *in_dev, int n, uint64_t *out_dev);

// UndistortKeyPoints of the selected keypoints of nimg images (k_undistort, mcorb_undistort.h): sel / nsel as the descriptor
// kernel reads them, cams: ncams per-camera tables in device memory (image m is camera m % ncams), scale: the level scale factors;
// out[m * kcap + k] = the undistorted pt of keypoint k of image m (device or host-mapped memory)
void launch_undistort(hipStream_t st, const uint32_t *sel, const int *nsel, int kcap, int nimg, int ncams, const UndistCam *cams,
                      const float *scale, int nlevels, float2 *out);

// device -> host-mapped pinned memory with a small grid (instead of the runtime's blit kernel); sizes rounded up to 16 bytes
void launch_copy_to_host(hipStream_t st, const void *src_dev, void *dst_host_mapped, size_t bytes);

// all frames [0, nframes) of a batch whose first image is img0 of `desc` (kcap-strided sets); tables indexed by the
// batch-local image index f * ncams + c (see k_bow_best2)
void launch_bow_best2(hipStream_t st, const uint8_t *desc, int img0, int kcap, int ncams, int nframes, const float *yv,
                      const int *slot_of, const int2 *node_range, const int *rg_base, const int *node_feats, const int *nfeat, int4 *out);
// k_bow_fold: transform()'s FeatureVector + BowVector of nimg images from their descent results (res, kcap-strided), into
// bow_rec records (mcorb_common.h) in device memory, and also in host-mapped memory when out_host is given (kcap <= kBowFoldMaxKcap)
void launch_bow_fold(hipStream_t st, const BowRes *res, const int *nsel, int kcap, int nimg, int weighting, int scoring, int *out_dev,
                     int *out_host);
// k_bow_tables: k_bow_best2's slot_of / nfeat / rg_base / yv / node_range of nframes frames from k_bow_fold's device records
// (node_feats: the records' feature lists, kcap-strided); undist = NULL: the rows are the keypoint records' y, rebuilt from sel
void launch_bow_tables(hipStream_t st, const int *fold, int kcap, int ncams, int nframes, const int *nsel, const uint32_t *sel,
                       const float *scale, int nlevels, const float2 *undist, int *slot_of, int *node_feats, int *nfeat, int *rg_base,
                       float *yv, int2 *node_range);
void launch_bow_descend(hipStream_t st, const uint8_t *desc, int n, const int *child_start, const int *child_count,
                        const void *child_desc, const int *child_id, const int *word_id, const double *weight, int nid_level,
                        BowRes *out);

// k_lf_tracks (mcorb_lf_gpu.hip): the per-track half of obtainLfFeatures for ntr tracks (trk: {first view, view count, frame,
// output record}, views: LfView) of the slot's descriptors (kcap-strided, image = frame * ncams + cam), records to out[record]
void launch_lf_tracks(hipStream_t st, const int4 *trk, const LfView *views, int ntr, const LfCam *cams, const uint8_t *desc, int kcap,
                      int ncams, LfTrackOut *out);
// the same triangulation on n arbitrary problems (mcorb_dev_triangulate_selftest)
void launch_tri_selftest(hipStream_t st, const double *x, const double *P, const int *nv, const int *voff, int n, double *X, int *branch);

// the keyframe database's kernels (mcorb_kfdb_gpu.hip).  k_kfdb_score: nq queries (q_sel[q] indexes q_ids / q_vals / q_n, strided
// like the store) against entries [0, q_limit[q]) -- or, with e_list, against entry e_list[q * out_stride + x] for x below the
// limit -- raw sum and shared-word count to raw / shared[q * out_stride + x]; max_limit = the largest q_limit
void launch_kfdb_score(hipStream_t st, const uint32_t *ids, const double *vals, const int *nbow, int stride, const uint32_t *q_ids,
                       const double *q_vals, const int *q_n, const int *q_sel, const int *q_limit, const int *e_list, int nq,
                       int max_limit, int out_stride, double *raw, int *shared);
// k_kfdb_best2: one frame A against one or many frames B (the many-probe launch): items {position in feats_a, shared-node record},
// recs {B's set, first position, count, -} in that B's feature list (feats_b + set * feats_stride; its descriptors at desc_b + set *
// desc_stride bytes; a single pair: B's own base, set 0) -> {best B feature or -1, best, second, A feature}
void launch_kfdb_best2(hipStream_t st, const uint8_t *desc_a, const int *feats_a, const uint8_t *desc_b, size_t desc_stride,
                       const int *feats_b, size_t feats_stride, const int2 *items, int nitems, const int4 *recs, int4 *out);
// k_kfdb_gather: dst[i] = descriptor src[i] of desc, 32 bytes each
void launch_kfdb_gather(hipStream_t st, const uint8_t *desc, const int *src, int n, uint8_t *dst);

// the local map's kernels (mcorb_lmap_gpu.hip).  k_lmap_cull: searchLocalMap2's frustum test of candidates cand[0 .. n) (slots of
// geom: 6 doubles per landmark, pt3D then normal) against the cameras of *view (device memory) -> one camera bit mask each
constexpr int kLmapCullT = 256;   // k_lmap_cull's workgroup: one lane per candidate
void launch_lmap_cull(hipStream_t st, const mcorb_lmap_view *view, const double *geom, const int *cand, int n, uint32_t *masks);
// k_lmap_put: entry i of a batch into slot lids[i] (-1: skipped) -- pt[3 * i ..] and normal[3 * i ..] into geom, row rows[i] (rows
// == NULL: row i) of src_desc into desc; a NULL source leaves that part of the slots alone
void launch_lmap_put(hipStream_t st, const int *lids, int n, const double *pt, const double *normal, const uint8_t *src_desc,
                     const int *rows, double *geom, uint8_t *desc);

// the mapping step's kernels (mcorb_mapping_gpu.hip).  k_map_triangulate: one lane per inter-frame match, one wave per block
// record of a.blocks -- first nblocks_small records of matches with at most 4 views (the instance without the run-time-shaped
// solver), then nblocks_any of the rest -- one MapOut to a.out[item.rec]
void launch_map_triangulate(hipStream_t st, const MapArgs &a, int nblocks_small, int nblocks_any);
// k_map_depth: z[i] = row 2 of Rcw * pt3D(lids[i]) + tcw (getSceneDepthStats)
void launch_map_depth(hipStream_t st, const double Rcw[9], const double tcw[3], const double *geom, const int *lids, int n, double *z);
// k_map_put: point, normal and n_rays of record put[i].x into slot put[i].y of geom / nrays
void launch_map_put(hipStream_t st, const MapOut *rec, const int2 *put, int n, double *geom, int32_t *nrays);
// the gates of n caller-given cases (mcorb_dev_map_gates_selftest); every pointer of c is device memory
void launch_map_gates(hipStream_t st, const MapGateCases &c, int n, MapOut *out);
// k_map_refine_new: one lane per match of TriangulateNewLandmarks, k_map_triangulate's blocks and two instances; a.blocks[0 ..
// nblocks_small) hold matches of at most 4 views
void launch_map_refine_new(hipStream_t st, const MapNewArgs &n, int nblocks_small, int nblocks_any);
// everything after the DLT for n caller-given cases (mcorb_dev_map_refine_selftest); every pointer of c is device memory
void launch_map_refine_cases(hipStream_t st, const MapRefineCases &c, int n, MapOut *out, MapNewExtra *extra);


// the landmarks' life (mcorb_landmark_gpu.hip).  k_lmap_observe: one lane per item of one round of mcorb_lmap_observe -- no two
// items of a launch name one slot -- Landmark::updateNormal(frame, featInd) on the slot's point, normal and ray count
void launch_lmap_observe(hipStream_t st, const LmCentres &cen, int ncams, const LmObsItem *items, int n, double *geom, int32_t *nrays);
// k_lmap_update: one lane per item of one round of mcorb_lmap_update_points: GlobalMap::updateLandmark, result to out[item.idx]
void launch_lmap_update(hipStream_t st, const LmUpdItem *items, int n, double max_diff, double *geom, LmUpdOut *out);
// k_lmap_put_rays: nrays[lids[i]] = vals[i], or 0 with vals == NULL; every slot at most once
void launch_lmap_put_rays(hipStream_t st, const int32_t *lids, const int32_t *vals, int n, int32_t *nrays);

// fast tracking (mcorb_track_gpu.hip): seven kernels, five launches, each once per call for its nf frames, frame blockIdx.z.
// items[f] (device memory; TrItem, mcorb_track.h) says where frame f's view, candidates, block of every per-pair array,
// de-duplication tables, keypoints and descriptors are; max_n: the most candidates of a frame, which sizes the grid's x; cand, xy,
// valid, pts, best, rows, slot, win, matches: the frames' blocks back to back, [c * n + i] inside a frame's.
// k_track_project: Tracking::project_ of a frame's candidates (slots of geom) into the cameras of its view (views: device
// memory) -> camera-major xy and valid (0: dropped), and the gathered points into pts (may be NULL)
constexpr int kTrackProjectT = 256;   // k_track_project's workgroup: one lane per candidate
void launch_track_project(hipStream_t st, const TrItem *items, int nf, int max_n, const mcorb_track_view *views, const double *geom,
                          const int *cand, float2 *xy, uint8_t *valid, double *pts);
// k_track_match: per camera c < ncams and candidate i with valid[c * n + i], the best keypoint of the frame by position and
// descriptor -> best[c * n + i]; kp_xy / kp_desc: the keypoints and descriptors the items' kp0 / desc0 and frame.first[c] count
// in (the store's keypoint buffer and the slot's descriptors, or the uploaded host arrays); lm_desc: the store's descriptors,
// 32 bytes per slot
constexpr int kTrackMatchWaves = 4;   // waves of a workgroup, which shares one LDS tile of keypoints
constexpr int kTrackMatchQ = 4;       // consecutive candidates a wave serves
constexpr int kTrackMatchT = 64 * kTrackMatchWaves;
void launch_track_match(hipStream_t st, const TrItem *items, int nf, int max_n, int ncams, const float2 *kp_xy, const uint8_t *kp_desc,
                        const uint8_t *lm_desc, const int *cand, const float2 *xy, const uint8_t *valid, double max_d2, int max_hamming,
                        TrBest *best);
// k_track_points (a rig slot's frames): pt of the selected keypoints of images img0 .. img0 + ncams of the slot (sel / nsel as
// k_undistort reads them, rows of kcap) -> out[kp0 + c * kcap + k] for k < min(nsel[img0 + c], kcap): k_track_match's kp_xy with
// first[c] = c * kcap; a frame without candidates is skipped
void launch_track_points(hipStream_t st, const TrItem *items, int nf, int max_n, const uint32_t *sel, const int *nsel, int kcap, int ncams,
                         const float *scale, int nlevels, float2 *out);
// k_track_compact: per camera the candidates with valid[c * n + i], in candidate order -> rows[c * n + 0 .. n_proj[c]) and
// n_proj[c]; n_proj: MCORB_MAX_CAMS counts per frame, written for the frames with a candidate; rows / n_proj may be host-mapped
// pinned memory
void launch_track_compact(hipStream_t st, const TrItem *items, int nf, int max_n, int ncams, const uint8_t *valid, const float2 *xy,
                          const TrBest *best, TrRow *rows, int32_t *n_proj);
// k_track_dedup_min, k_track_dedup_win, k_track_dedup_emit: per camera, of the candidates with valid[c * n + i] and a match, the one
// with the least (dist, i) per pixel of the matched keypoint, in candidate order -> matches[c * n + 0 .. n_match[c]) and
// n_match[c] (as n_proj; may be host-mapped).  owner / val: every frame's tables, ncams << tr_dedup_log2(n) slots from the item's
// tab on, every byte 0xff; slot (int32) and win (bytes): scratch, laid out as valid
constexpr int kTrackDedupT = 256;     // one lane per (camera, candidate)
void launch_track_dedup(hipStream_t st, const TrItem *items, int nf, int max_n, int ncams, const float2 *kp_xy, const uint8_t *valid,
                        const TrBest *best, uint32_t *owner, unsigned long long *val, int32_t *slot, uint8_t *win, TrMatch *matches,
                        int32_t *n_match);

// the pose refinement (mcorb_pose_gpu.hip).  k_pose_refine: problem blockIdx.x of jobs (device memory), one workgroup of
// MCORB_POSE_LANES lanes for both rounds.  obs / lids / pts / alive / flags: every problem's block begins at its obs0; pts or lids
// is NULL (a point is pts[i] or geom's of lids[i]).  A problem with from_track builds its obs and lids itself, from win / best /
// cand / kp_xy of the tracking submission in front of it (these may be NULL otherwise).  out (one per problem) and flags may be
// host-mapped
void launch_pose_refine(hipStream_t st, const PoseJob *jobs, int njobs, PoseObs *obs, int32_t *lids, const double *pts, const double *geom,
                        uint8_t *alive, const uint8_t *win, const TrBest *best, const int *cand, const float2 *kp_xy,
                        mcorb_pose_result *out, uint8_t *flags);

// the local bundle adjustment (mcorb_ba_gpu.hip): the kernels of one chain, in stream order -- k_ba_begin (the state and the
// record), then per iteration k_ba_linearize (one lane per landmark; returns at once unless the state moved), k_ba_schur (one
// workgroup per keyframe pair and per keyframe of the system), k_ba_solve (one workgroup), k_ba_update (one lane per landmark:
// the back-substitution and the trial's cost), k_ba_accept (one workgroup; first: the fold of the initial cost in front of
// iteration 0), and at the end k_ba_flags with k_ba_result.  Every kernel but the first and the last two returns at once when
// the record says the loop is over
void launch_ba_begin(hipStream_t st, const BaArgs &a);
void launch_ba_linearize(hipStream_t st, const BaArgs &a);
void launch_ba_schur(hipStream_t st, const BaArgs &a);
void launch_ba_solve(hipStream_t st, const BaArgs &a);
void launch_ba_update(hipStream_t st, const BaArgs &a);
void launch_ba_accept(hipStream_t st, const BaArgs &a, bool first);
void launch_ba_final(hipStream_t st, const BaArgs &a);

// the re-triangulation of landmarks after the back end moved keyframes (mcorb_retri_gpu.hip): k_retri_views (one lane per
// (keyframe, camera) of the keyframes that have an observation: 15 doubles), then k_retri_solve (16 lanes per landmark: the
// selection, G and its fold, the Jacobi, the checks, the gated store into the HBM point, the record into host-mapped memory)
void launch_retri_views(hipStream_t st, const RetriArgs &a);
void launch_retri_solve(hipStream_t st, const RetriArgs &a);

// the RANSAC in front of it (mcorb_sac_gpu.hip), three launches.  job, obs, lids | pts, cons / cam_first / cam_cons (the
// consensus observations in input order, and camera by camera) and is_first (per observation: the first of its match) are device
// memory.  k_sac_hypotheses: one lane per hypothesis, models[H]; with MCORB_SAC_SOLVER_RIG k_sac_hypotheses_rig in its place, four
// lanes per hypothesis (cam_first and cam_cons are not read).  k_sac_score: a workgroup per (tile of kSacTile consensus
// observations, block of kSacHypBlock hypotheses), integer adds into count[H], which the caller has zeroed on the stream.
// k_sac_pick: the winner, the flags of all n observations (host-mapped), the record out (host-mapped) and, with pose_job, the
// winner's pose into pose_job->init for the launch_pose_refine behind it
#ifndef MCORB_SAC_HYP_BLOCK
#define MCORB_SAC_HYP_BLOCK 8   // measured against 32 and 128 (make EXTRA=-DMCORB_SAC_HYP_BLOCK=..)
#endif
constexpr int kSacTile = 256, kSacHypBlock = MCORB_SAC_HYP_BLOCK;
struct SacArgs {
    const SacJob *job;
    const PoseObs *obs;
    const int32_t *lids;
    const double *pts, *geom;
    const int32_t *cons, *cam_first, *cam_cons;
    const uint8_t *is_first;
    SacModel *models;
    int32_t *count;
    SacOut *out;
    uint8_t *flags;
    PoseJob *pose_job;
};
void launch_sac_hypotheses(hipStream_t st, const SacArgs &a, int H);
void launch_sac_hypotheses_rig(hipStream_t st, const SacArgs &a, int H);
void launch_sac_score(hipStream_t st, const SacArgs &a, int S, int H);
void launch_sac_pick(hipStream_t st, const SacArgs &a, int n);

// the relative pose between two frames by RANSAC (mcorb_rel_gpu.hip), three launches.  job and obs (the S matches) are device
// memory.  k_rel_hypotheses: one lane per hypothesis, models[H].  k_rel_score: a workgroup per (tile of kRelTile matches, block of
// kRelHypBlock hypotheses), integer adds into count[H], which the caller has zeroed on the stream.  k_rel_pick: the winner, the
// flags of all S matches (host-mapped) and the record out (host-mapped)
#ifndef MCORB_REL_HYP_BLOCK
#define MCORB_REL_HYP_BLOCK 32   // measured against 8 and 128 (make EXTRA=-DMCORB_REL_HYP_BLOCK=..)
#endif
constexpr int kRelTile = 256, kRelHypBlock = MCORB_REL_HYP_BLOCK;
struct RelArgs {
    const RelJob *job;
    const RelObs *obs;
    RelModel *models;
    int32_t *count;
    RelOut *out;
    uint8_t *flags;
};
void launch_rel_hypotheses(hipStream_t st, const RelArgs &a, int H);
void launch_rel_score(hipStream_t st, const RelArgs &a, int S, int H);
void launch_rel_pick(hipStream_t st, const RelArgs &a, int S);
// the polish behind a pick whose out and flags are device memory (pick; member[0 .. S)): k_rel_fit, one workgroup -- the rounds of
// mcorb_rel.h over the members, member[S .. 2 S) the other set of flags, then the accepted record, its flags and the polish
// record to host-mapped memory
struct RelFitArgs {
    const RelJob *job;
    const RelObs *obs;
    const RelOut *pick;
    uint8_t *member;
    int32_t rounds, max_iterations;
    RelOut *out;
    uint8_t *flags;
    RelPolish *polish;
};
void launch_rel_fit(hipStream_t st, const RelFitArgs &a);

// the pose of one camera between two frames by five-point RANSAC (mcorb_ess_gpu.hip), four launches.  job and obs (the S
// matches) are device memory.  k_ess_hypotheses: kEssLanes lanes per hypothesis, four hypotheses per wave; models[10 H] (slot 10 h
// + c is root c of hypothesis h), valid[10 H] (the models' flags once more, densely, for k_ess_pick's walk) and samples[5 H].  k_ess_score: a workgroup per (tile of kEssTile matches, block of kEssSlotBlock
// slots), integer adds into count[10 H], which the caller has zeroed on the stream together with cheir[4].  k_ess_pick: the winner
// and its four candidates into pick, the candidates' votes over the winner's inliers into cheir.  k_ess_finish: the flags of
// all S matches and the record out (both host-mapped)
constexpr int kEssTile = 256, kEssSlotBlock = 40, kEssLanes = 16;
struct EssArgs {
    const EssJob *job;
    const EssObs *obs;
    EssModel *models;
    int32_t *samples, *valid, *count, *cheir;
    EssPick *pick;
    EssOut *out;
    uint8_t *flags;
};
void launch_ess_hypotheses(hipStream_t st, const EssArgs &a, int H);
void launch_ess_score(hipStream_t st, const EssArgs &a, int S, int H);
void launch_ess_pick(hipStream_t st, const EssArgs &a, int S);
void launch_ess_finish(hipStream_t st, const EssArgs &a, int S);
// the polish behind a k_ess_finish whose out and flags are device memory (pick; member[0 .. S)): k_ess_fit, one workgroup -- the
// rounds of mcorb_ess_polish.h over the members, member[S .. 2 S) the other set of flags, then the accepted record, its flags and
// the polish record to host-mapped memory.  inv_thr: ess_fit_scale of the call
struct EssFitArgs {
    const EssJob *job;
    const EssObs *obs;
    const EssOut *pick;
    uint8_t *member;
    int32_t rounds, max_iterations;
    double inv_thr;
    EssOut *out;
    uint8_t *flags;
    EssPolish *polish;
};
void launch_ess_fit(hipStream_t st, const EssFitArgs &a);

// the pose between two frames from 3D-3D pairs (mcorb_align_gpu.hip).  job, p2 and p1 or lids1 (the n pairs; lids1: frame 1's
// points are geom's, 6 doubles per slot) are device memory.  Mode 1: k_align_hypotheses -- one lane per hypothesis, models[H];
// k_align_score -- a workgroup per (tile of kAlignTile pairs, block of kAlignHypBlock hypotheses), integer adds into count[H],
// which the caller has zeroed on the stream; k_align_pick -- the winner into pick and its flags at the threshold into member[n],
// both device memory; then k_align_fit, which mode 0 launches alone: one workgroup -- the refit over member (mode 0: the fit over
// all pairs), the verdict's flags (host-mapped) and the record out (host-mapped)
constexpr int kAlignTile = 256, kAlignHypBlock = 32;
struct AlignArgs {
    const AlignJob *job;
    const double *p1, *p2;
    const int32_t *lids1;
    const double *geom;
    AlignModel *models;
    int32_t *count;
    AlignPick *pick;
    uint8_t *member;
    AlignOut *out;
    uint8_t *flags;
};
void launch_align_hypotheses(hipStream_t st, const AlignArgs &a, int H);
void launch_align_score(hipStream_t st, const AlignArgs &a, int n, int H);
void launch_align_pick(hipStream_t st, const AlignArgs &a, int n);
void launch_align_fit(hipStream_t st, const AlignArgs &a);

// The minimal solvers on n caller-given problems, one launch each (mcorb_dev_*_solve_selftest); every pointer is device memory.
// Each kernel runs the text its estimator's hypotheses kernel runs behind the sample, in that kernel's launch shape: a lane per
// problem (sac, rel), a quad per problem (sac rig: cams[n][ncams], obs and pts four per problem, the fourth the disambiguating
// one), sixteen lanes per problem and four problems per workgroup (ess: jobs[n] carry the cameras), a workgroup of kAlignTile
// per problem (align: problem b is pairs first[b] .. first[b] + cnt[b]).  R and t of sac and sac rig hold four slots a
// problem and are zeroed by the caller; every other output is written whole
void launch_sac_solve_selftest(hipStream_t st, const mcorb_track_cam *cams, const float *uv, const double *pts, int n, double *R, double *t,
                               int32_t *count);
void launch_sac_solve_rig_selftest(hipStream_t st, const mcorb_track_cam *cams, int ncams, const PoseObs *obs, const double *pts, int n, double *R,
                                   double *t, int32_t *count, int32_t *mask, int32_t *best, SacModel *win);
void launch_rel_solve_selftest(hipStream_t st, const mcorb_track_cam *cams, int ncams, const int32_t *cam1, const double *uv1, const int32_t *cam2,
                               const double *uv2, int n, double *R, double *t, int32_t *count);
void launch_ess_solve_selftest(hipStream_t st, const EssJob *jobs, const double *uv1, const double *uv2, int n, EssModel *models, int32_t *valid,
                               double *z);
void launch_align_solve_selftest(hipStream_t st, const double *p1, const double *p2, const uint8_t *member, const int32_t *first,
                                 const int32_t *cnt, int n, double *R, double *t, double *gap, int32_t *valid);

// map initialization (mcorb_init_gpu.hip, mcorb_init.h).  k_init_triangulate: k_map_triangulate's blocks and two instances over
// the matches whose flag is set, one MapOut to a.out[match]; k_init_select: one workgroup -- the sizes and medians of parllaxVec
// and depthVec into *sel, every match's id offset (the accepted matches before it) into offset, keys: 2 * n words of scratch;
// k_init_put: one lane per match -- the verdict and the scale from *sel, the stored point, normal and n_rays of an accepted match
// into slot job.next_lid + offset of geom / nrays, every match's record into h_rec and the call's record into *h_call (both
// host-mapped).  The views of a match come from the packed block (a, query, train) or, for the self-test, from cases
struct InitPutArgs {
    InitJob job;
    MapArgs a;
    const int32_t *query, *train;
    MapCases cases;
    const MapOut *rec;
    const uint8_t *flags;
    const int32_t *offset;
    const InitSel *sel;
    MapOut *h_rec;
    InitCall *h_call;
    double *geom;
    int32_t *nrays;
};
constexpr int kInitSelectT = 1024, kInitPutT = 256;
void launch_init_triangulate(hipStream_t st, const MapArgs &a, int nblocks_small, int nblocks_any);
void launch_init_select(hipStream_t st, const MapOut *rec, const uint8_t *flags, int n, uint64_t *keys, int32_t *offset, InitSel *sel);
void launch_init_put(hipStream_t st, const InitPutArgs &p, bool from_cases);
// init_after of n caller-given cases (mcorb_dev_init_cases_selftest); every pointer of c is device memory
void launch_init_gates(hipStream_t st, const MapCases &c, int n, MapOut *out);

}  // namespace mcorb
