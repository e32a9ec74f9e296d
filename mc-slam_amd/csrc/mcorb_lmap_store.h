// mcorb_lmap_store.h -- the local map object, shared by its search (mcorb_lmap.cpp), by the mapping step that fills it
// (mcorb_mapping.cpp), by the calls that keep its landmarks up to date (mcorb_landmark.cpp) and by fast tracking (mcorb_track.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "mcorb_kfdb_store.h"
#include "mcorb_mapping_new.h"
#include "mcorb_pose.h"
#include "mcorb_sac.h"
#include "mcorb_track.h"

namespace mcorb {
constexpr uint8_t kHasPt = 1, kHasNormal = 2, kHasDesc = 4, kMono = 8, kSet = kHasPt | kHasNormal;
struct LmObs { int32_t kf_id, feat; };   // one observation of a landmark: KFs[i]'s id, featInds[i]
// the buffers of a k_pose_refine launch (mcorb_pose.cpp), grow-only: the packed input (the PoseJobs, then -- the explicit entry --
// the observations and their ids or points; one block, one copy), the observation list a tracking submission's prologue builds,
// the flags of the observations that are still in, and what the host reads: results and inlier flags, host-mapped
struct PoseBufs {
    HostBuf<uint8_t> h_in;
    DevBuf<uint8_t> d_in;
    DevBuf<PoseObs> d_obs;
    DevBuf<int32_t> d_lids;
    DevBuf<uint8_t> d_alive;
    HostBuf<mcorb_pose_result> h_out;
    HostBuf<uint8_t> h_flags;
};
// the buffers of a mcorb_lmap_ransac_pose submission (mcorb_sac.cpp), grow-only: the packed input (the PoseJob of the
// refinement behind it, the SacJob, the observations, their ids or points, the consensus lists and the first-of-match bytes;
// one block, one copy), the models and counts of the hypotheses, and what the host reads: the pick's record and the flags per
// observation, host-mapped.  The refinement's own buffers are `pose`
struct SacBufs {
    HostBuf<uint8_t> h_in;
    DevBuf<uint8_t> d_in;
    DevBuf<SacModel> d_models;
    DevBuf<int32_t> d_count;
    HostBuf<SacOut> h_out;
    HostBuf<uint8_t> h_flags;
    PoseBufs pose;
};
}  // namespace mcorb

struct mcorb_lmap {
    int device = -1, max_landmarks = 0, max_candidates = 0;
    mcorb_vocab *voc = nullptr;
    std::mutex mu;   // one call at a time: the scratch below is the store's
    std::vector<uint8_t> flags;      // per slot
    std::vector<int> stamp;          // per slot: the last search (or batch) that saw it
    int tick = 0;
    // host-only store
    std::vector<double> geom;        // [max_landmarks][6]: pt3D, normal
    std::vector<uint8_t> desc;       // [max_landmarks][32]
    // device store
    mcorb::Stream st;
    mcorb::Event ev0, ev1;
    mcorb::DevBuf<double> d_geom;
    mcorb::DevBuf<uint8_t> d_desc;
    mcorb::DevBuf<mcorb_lmap_view> d_view;
    // scratch of a batch (grow-only) and of a search (max_candidates)
    mcorb::DevBuf<int> d_blids, d_brows;
    mcorb::DevBuf<double> d_bpt, d_bnormal;
    mcorb::DevBuf<uint8_t> d_bdesc;
    mcorb::DevBuf<int> d_cand, d_afeats;
    mcorb::DevBuf<uint32_t> d_masks;
    mcorb::HostBuf<uint32_t> h_masks;
    mcorb::DevBuf<uint8_t> d_adesc;         // the accepted rows, gathered
    mcorb::Best2Search best2;
    float us_cull = 0.f, us_best2 = 0.f;
    int last_candidates = 0;
    // scratch of mcorb_lmap_triangulate_neighbours (mcorb_mapping.cpp), grow-only: the packed input (one block, one copy), the
    // result records, the depth list and the write-back list
    mcorb::HostBuf<uint8_t> h_mapin;
    mcorb::DevBuf<uint8_t> d_mapin;
    mcorb::HostBuf<mcorb::MapOut> h_mapout;
    mcorb::DevBuf<mcorb::MapOut> d_mapout;
    mcorb::HostBuf<double> h_mapz;
    mcorb::DevBuf<double> d_mapz;
    mcorb::HostBuf<int2> h_mapput;
    mcorb::DevBuf<int2> d_mapput;
    mcorb::Event ev2, ev3;
    float us_map_depth = 0.f, us_map_tri = 0.f;
    int last_map_launched = 0, last_map_depth = 0;
    // mcorb_lmap_triangulate_new (mcorb_mapping.cpp) shares the scratch above (ev2 / ev3 around its kernel) and adds the second
    // half of its records
    mcorb::HostBuf<mcorb::MapNewExtra> h_mapextra;
    mcorb::DevBuf<mcorb::MapNewExtra> d_mapextra;
    float us_map_new = 0.f;
    int last_map_new_launched = 0;
    // the landmarks' life (mcorb_landmark.cpp).  n_rays: the host's copy of every slot's ray count (a device store's kernels read
    // and write d_nrays); obs: per slot the observations (kf_id, feat) in the order they were added (KFs / featInds); occ: per
    // slot how often a batch has named it so far, zero between calls
    std::vector<int32_t> n_rays;
    std::vector<std::vector<mcorb::LmObs>> obs;
    std::vector<int32_t> occ;
    mcorb::DevBuf<int32_t> d_nrays;
    mcorb::HostBuf<mcorb::LmObsItem> h_obsitems;
    mcorb::DevBuf<mcorb::LmObsItem> d_obsitems;
    mcorb::HostBuf<mcorb::LmUpdItem> h_upditems;
    mcorb::DevBuf<mcorb::LmUpdItem> d_upditems;
    mcorb::HostBuf<mcorb::LmUpdOut> h_updout;
    mcorb::DevBuf<mcorb::LmUpdOut> d_updout;
    mcorb::HostBuf<int32_t> h_rays;        // a batch of (slot, n_rays) pairs for k_lmap_put_rays: slots, then values
    mcorb::DevBuf<int32_t> d_rays;
    mcorb::Event ev4, ev5, ev6, ev7;
    float us_observe = 0.f, us_update = 0.f;
    // scratch of mcorb_lmap_track / mcorb_lmap_track_rig_frame (mcorb_track.cpp), grow-only: the packed input (candidates, then --
    // host arrays only -- the keypoints and the descriptors of every camera; one block, one copy), a rig slot's keypoints
    // (k_track_points), the projections, validity bytes and gathered points, the queries' results, and what the host tail reads:
    // the compacted rows and the counts per camera, host-mapped pinned memory k_track_compact writes.  mcorb_lmap_track_rig_frames
    // uses the same buffers, sized for all its frames: the pinned block holds the TrBatchItems, the views and every frame's
    // candidates, a frame's block of every per-pair array begins at ncams * (its first candidate), the counts are MCORB_MAX_CAMS
    // per frame and the keypoints nf * ncams rows
    mcorb::HostBuf<uint8_t> h_trackin;
    mcorb::DevBuf<uint8_t> d_trackin;
    mcorb::DevBuf<float2> d_trackkp;
    mcorb::DevBuf<float2> d_trackxy;
    mcorb::DevBuf<uint8_t> d_trackvalid;
    mcorb::DevBuf<double> d_trackpt;
    mcorb::HostBuf<double> h_trackpt;
    mcorb::DevBuf<mcorb::TrBest> d_trackbest;
    mcorb::HostBuf<mcorb::TrRow> h_trackrows;
    mcorb::HostBuf<int32_t> h_tracknproj;
    mcorb::Event ev8, ev9, ev10, ev11, ev12;   // in front of k_track_project | match | compact | behind it | in front of k_track_points
    float us_track_points = 0.f, us_track_project = 0.f, us_track_match = 0.f, us_track_compact = 0.f;
    // the de-duplication on the device: per camera the arg-min table (owner, val: cleared in every submission), per (camera,
    // candidate) the slot and the winner flag, and what the host reads: the matches and their counts, host-mapped as the rows are
    mcorb::DevBuf<uint32_t> d_trackowner;
    mcorb::DevBuf<unsigned long long> d_trackval;
    mcorb::DevBuf<int32_t> d_trackslot;
    mcorb::DevBuf<uint8_t> d_trackwin;
    mcorb::HostBuf<mcorb::TrMatch> h_trackmatch;
    mcorb::HostBuf<int32_t> h_tracknmatch;
    mcorb::Event ev13;                         // behind k_track_dedup_emit (ev11 is in front of the table's clear)
    float us_track_dedup = 0.f;
    // a tracking call that was submitted and not yet waited for (mcorb_lmap_track_submit .. mcorb_lmap_track_wait).  While
    // track_pending is set every other entry refuses (check_lmap) and the scratch above belongs to the call.  launched: a
    // device store has work on its stream; points: k_track_points is part of it.  A host-only store keeps its finished result in
    // rows / matches.  A call has nf frames (one, but for mcorb_lmap_track_rig_frames): frame f's candidates are cand[first[f] ..
    // first[f + 1]), its block of rows / matches begins at ncams * first[f], its counts at f * MCORB_MAX_CAMS
    struct TrackCall {
        int ncams = 0, nf = 1;
        bool launched = false, points = false, want_pts = false;
        bool refine = false;                      // the call ran with mcorb_lmap_set_track_refine on: pose / pose_flags hold
        std::vector<mcorb_pose_result> pose;      // a host-only store's results and those of frames without a launch, per frame
        std::vector<uint8_t> pose_flags;          // a host-only store's inlier flags, frame f's from ncams * first[f] on
        std::vector<int> cand;
        std::vector<size_t> first;
        std::vector<mcorb::TrRow> rows;
        std::vector<mcorb::TrMatch> matches;
        std::vector<int32_t> n_proj, n_match;
    } track_call;
    std::atomic<bool> track_pending{false};
    // the pose refinement (mcorb_pose.cpp): pose_x serves mcorb_lmap_refine_pose, pose_t the refinement behind a tracking
    // submission (track_refine: mcorb_lmap_set_track_refine), whose results stay readable until the next submission.
    // track_pose_nf: the frames of the last tracking call if it ran with the option, 0 otherwise
    mcorb::PoseBufs pose_x, pose_t;
    mcorb::Event ev14, ev15;                   // in front of and behind k_pose_refine of mcorb_lmap_refine_pose
    float us_pose = 0.f;
    bool track_refine = false;
    mcorb_pose_params track_refine_params = {};
    int track_pose_nf = 0;
    // the RANSAC in front of the refinement (mcorb_sac.cpp): ev16 .. ev19 around k_sac_hypotheses, k_sac_score and k_sac_pick
    mcorb::SacBufs sac;
    mcorb::Event ev16, ev17, ev18, ev19;
    float us_sac[3] = {0.f, 0.f, 0.f};
    int sac_last_hyp = 0;                      // the hypotheses of the last call that ran any (either kind of store)
    std::vector<int32_t> sac_host_count, sac_host_valid;   // a host-only store's last counts, for mcorb_lmap_last_ransac_counts
#ifdef MCORB_TRACK_PROF
    float us_track_phase[5] = {};   // the last call's host phases: candidate walk, submission, wait, de-duplication, output
#endif
};

// the pose refinement behind a tracking call (mcorb_pose.cpp); the caller holds the store's lock and has set track_refine_params.
// pose_track_host: a host-only store, or a frame nothing was launched for -- the observations are the frame's matches, the
// cameras back to back in match order (kp_base / kp_stride: the frame's keypoint records, which begin with pt), flags: ncams *
// nc bytes.  pose_track_submit: k_pose_refine for the nf frames of a device submission, behind its de-duplication on the
// store's stream; first: the frames' places in the call's candidate list (nf + 1), frames / kp0: per frame its TrFrame and the
// place of its keypoints in kp_xy
namespace mcorb {
void pose_track_host(mcorb_lmap *m, const mcorb_track_view &view, const int *cand, int nc, const TrMatch *matches, const int32_t *n_match,
                     const uint8_t *const *kp_base, size_t kp_stride, mcorb_pose_result &res, uint8_t *flags);
int pose_track_submit(mcorb_lmap *m, const mcorb_track_view *views, int nf, const size_t *first, const TrFrame *frames, const size_t *kp0,
                      const float2 *kp_xy, const int *d_cand);
// shared with mcorb_sac.cpp: a refinement problem's job, its serial run, and the checks of its parameters
void pose_job_init(PoseJob &job, const mcorb_pose_params &p, int ncams, const mcorb_track_cam *cams, const PoseState &init);
void pose_run_host(const PoseJob &job, const PoseObs *obs, const double *pts, int n, uint8_t *alive, mcorb_pose_result &res);
int pose_check_params(const mcorb_pose_params *p);
}  // namespace mcorb

// a new stamp value; the stamps start over before the counter wraps
inline int next_tick(mcorb_lmap *m)
{
    if (m->tick == 0x7fffffff) { std::fill(m->stamp.begin(), m->stamp.end(), 0); m->tick = 0; }
    return ++m->tick;
}

// the handle alone: the last_*timing* getters and the tracking pair itself
inline int check_lmap_handle(const mcorb_lmap *m, const char *who)
{
    if (!m) { mcorb::set_error(std::string(who) + ": bad argument"); return MCORB_E_ARG; }
    return MCORB_OK;
}

// every other entry: no tracking call may be pending on the store
inline int check_lmap(const mcorb_lmap *m, const char *who)
{
    TRY(check_lmap_handle(m, who));
    if (m->track_pending.load()) {
        mcorb::set_error(std::string(who) + ": a submitted tracking call has not been waited for");
        return MCORB_E_STATE;
    }
    return MCORB_OK;
}

