// mcorb_lmap_store.h -- the local map object, shared by its search (mcorb_lmap.cpp), by the mapping step that fills it
// (mcorb_mapping.cpp), by the map initialization (mcorb_init.cpp), by the calls that keep its landmarks up to date
// (mcorb_landmark.cpp) and by fast tracking (mcorb_track.cpp).
#pragma once
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "mcorb_kfdb_store.h"
#include "mcorb_align.h"
#include "mcorb_ess.h"
#include "mcorb_init.h"
#include "mcorb_map_host.h"
#include "mcorb_mapping_new.h"
#include "mcorb_pose.h"
#include "mcorb_rel.h"
#include "mcorb_retri.h"
#include "mcorb_sac.h"
#include "mcorb_track.h"

namespace mcorb {
constexpr uint8_t kHasPt = 1, kHasNormal = 2, kHasDesc = 4, kMono = 8, kSet = kHasPt | kHasNormal;
struct LmObs { int32_t kf_id, feat; };   // one observation of a landmark: KFs[i]'s id, featInds[i]

// a packed input (mcorb_pack.h) on both sides, grow-only: the pinned block the host fills and its place on the device, one copy
struct Staged {
    HostBuf<uint8_t> h;
    DevBuf<uint8_t> d;
    int reserve(size_t bytes) { TRY(h.grow(bytes, hipHostMallocDefault)); return d.grow(bytes); }
    void upload(Submission &sub, size_t bytes) const { sub.copy(d, h, bytes, hipMemcpyHostToDevice); }
    template <class T> T *host(size_t off) const { return reinterpret_cast<T *>(h.get() + off); }
    template <class T> T *dev(size_t off) const { return reinterpret_cast<T *>(d.get() + off); }
};

// the buffers of a k_pose_refine launch (mcorb_pose.cpp), grow-only: the packed input (the PoseJobs, then -- the explicit entry --
// the observations and their ids or points: ObsLayout), the observation list a tracking submission's prologue builds, the flags
// of the observations that are still in, and what the host reads: results and inlier flags, host-mapped
struct PoseBufs {
    Staged in;
    DevBuf<PoseObs> d_obs;
    DevBuf<int32_t> d_lids;
    DevBuf<uint8_t> d_alive;
    HostBuf<mcorb_pose_result> h_out;
    HostBuf<uint8_t> h_flags;
    // the explicit entries: a problem of n observations whose input is elsewhere
    int reserve(size_t n) { TRY(d_alive.grow(n)); TRY(h_out.grow(1, kHostMapped)); return h_flags.grow(n, kHostMapped); }
    // the refinement behind a tracking submission of nf frames and `rows` = ncams * candidates pairs, whose jobs are the input
    int reserve_track(size_t nf, size_t rows)
    {
        TRY(in.reserve(nf * sizeof(PoseJob)));
        TRY(d_obs.grow(rows));
        TRY(d_lids.grow(rows));
        TRY(d_alive.grow(rows));
        TRY(h_out.grow(nf, kHostMapped));
        return h_flags.grow(rows, kHostMapped);
    }
};

// what the pose estimators' entries share (mcorb_sac.cpp, _rel, _align, _ess).  positive: a threshold, distance or focal length
// an entry accepts.  no_obs: the record of a call without observations -- the identity, no sample; the caller sets its
// "no winner" fields
inline bool positive(double v) { return v > 0 && sac_finite(v); }
template <class Out>
void no_obs(Out &out, int32_t status)
{
    memset(&out, 0, sizeof(out));
    out.R[0] = out.R[4] = out.R[8] = 1.0;
    out.status = status;
    for (int32_t &s : out.sample) s = -1;
}
}  // namespace mcorb

struct mcorb_lmap {
    int device = -1, max_landmarks = 0, max_candidates = 0;
    mcorb_vocab *voc = nullptr;
    std::mutex mu;   // one call at a time: the scratch below is the store's
    std::vector<uint8_t> flags;      // per slot
    std::vector<int> stamp;          // per slot: the last search (or batch) that saw it
    int tick = 0;
    // n_rays: the host's copy of every slot's ray count (a device store's kernels read and write d_nrays); obs: per slot the
    // observations (kf_id, feat) in the order they were added (KFs / featInds)
    std::vector<int32_t> n_rays;
    std::vector<std::vector<mcorb::LmObs>> obs;
    // host-only store
    std::vector<double> geom;        // [max_landmarks][6]: pt3D, normal
    std::vector<uint8_t> desc;       // [max_landmarks][32]
    // device store
    mcorb::Stream st;
    mcorb::DevBuf<double> d_geom;
    mcorb::DevBuf<uint8_t> d_desc;
    mcorb::DevBuf<int32_t> d_nrays;

    // scratch of a search (mcorb_lmap.cpp), max_candidates each
    struct Search {
        mcorb::DevBuf<mcorb_lmap_view> d_view;
        mcorb::DevBuf<int> d_cand, d_afeats;
        mcorb::DevBuf<uint32_t> d_masks;
        mcorb::HostBuf<uint32_t> h_masks;
        mcorb::DevBuf<uint8_t> d_adesc;         // the accepted rows, gathered
        mcorb::Best2Search best2;
        mcorb::Spans<1> cull;                   // around k_lmap_cull
        float us_best2 = 0.f;
        int last_candidates = 0;
        int create(size_t C)
        {
            TRY(cull.create());
            TRY(best2.create());
            TRY(d_view.alloc(1));
            TRY(d_cand.alloc(C));
            TRY(d_afeats.alloc(C));
            TRY(d_masks.alloc(C));
            TRY(h_masks.alloc(C, hipHostMallocDefault));
            return d_adesc.alloc(C * 32);
        }
    } search;

    // a batch of slots on the device (grow-only): what put_device (mcorb_lmap.cpp), mcorb_lmap_observe and mcorb_lmap_depths upload
    struct Batch {
        mcorb::DevBuf<int> d_lids, d_rows;
        mcorb::DevBuf<double> d_pt, d_normal;
        mcorb::DevBuf<uint8_t> d_desc;
        // room for n slots, before the chain: the ids, and the arrays a call sends with them
        int reserve(size_t n, bool pt, bool normal, bool desc, bool rows)
        {
            TRY(d_lids.grow(n));
            if (pt) TRY(d_pt.grow(n * 3));
            if (normal) TRY(d_normal.grow(n * 3));
            if (desc) TRY(d_desc.grow(n * 32));
            return rows ? d_rows.grow(n) : MCORB_OK;
        }
        // src[0 .. n) into d (pageable memory: the submission's wait covers it)
        template <class T>
        static void upload(mcorb::Submission &sub, const mcorb::DevBuf<T> &d, const T *src, size_t n)
        {
            sub.copy(d, src, n * sizeof(T), hipMemcpyHostToDevice);
        }
    } batch;

    // scratch of mcorb_lmap_triangulate_neighbours and mcorb_lmap_triangulate_new (mcorb_mapping.cpp), grow-only: the packed input
    // (MapLayout), the result records -- the second half of triangulate_new's in `extra` --, the depth list and the write-back list
    struct Mapping {
        mcorb::Staged in;
        mcorb::HostBuf<mcorb::MapOut> h_out;
        mcorb::DevBuf<mcorb::MapOut> d_out;
        mcorb::HostBuf<mcorb::MapNewExtra> h_extra;
        mcorb::DevBuf<mcorb::MapNewExtra> d_extra;
        mcorb::HostBuf<double> h_z;
        mcorb::DevBuf<double> d_z;
        mcorb::HostBuf<int2> h_put;
        mcorb::DevBuf<int2> d_put;
        enum { kDepth, kTriangulate };
        mcorb::Spans<2> neigh;                  // triangulate_neighbours: k_map_depth, then k_map_triangulate
        mcorb::Spans<1> refine_new;             // triangulate_new: k_map_refine_new
        int last_launched = 0, last_depth = 0, last_new_launched = 0;
        // a call of nitems records and nz depths; extra: triangulate_new's
        int reserve(size_t bytes, size_t nitems, size_t nz, bool extra)
        {
            TRY(in.reserve(bytes));
            TRY(h_out.grow(nitems, hipHostMallocDefault));
            TRY(d_out.grow(nitems));
            if (extra) {
                TRY(h_extra.grow(nitems, hipHostMallocDefault));
                TRY(d_extra.grow(nitems));
            }
            TRY(h_z.grow(nz, hipHostMallocDefault));
            return d_z.grow(nz);
        }
    } map;

    // the landmarks' life (mcorb_landmark.cpp).  occ: per slot how often a batch has named it so far, zero between calls
    struct Life {
        std::vector<int32_t> occ;
        mcorb::HostBuf<mcorb::LmObsItem> h_obsitems;
        mcorb::DevBuf<mcorb::LmObsItem> d_obsitems;
        mcorb::HostBuf<mcorb::LmUpdItem> h_upditems;
        mcorb::DevBuf<mcorb::LmUpdItem> d_upditems;
        mcorb::HostBuf<mcorb::LmUpdOut> h_updout;
        mcorb::DevBuf<mcorb::LmUpdOut> d_updout;
        mcorb::HostBuf<int32_t> h_rays;        // a batch of (slot, n_rays) pairs for k_lmap_put_rays: slots, then values
        mcorb::DevBuf<int32_t> d_rays;
        mcorb::Spans<1> observe, update;       // around the rounds of k_lmap_observe / k_lmap_update
    } life;

    // a tracking call that was submitted and not yet waited for (mcorb_lmap_track_submit .. mcorb_lmap_track_wait).  While
    // track.pending is set every other entry refuses (check_lmap) and the tracking scratch belongs to the call.  launched: a
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
    };

    // scratch of a tracking call of nf frames (mcorb_track.cpp; nf = 1 but for mcorb_lmap_track_rig_frames), grow-only: the packed
    // input (TrackLayout: a TrItem and a view per frame, the frames' candidates, then -- host arrays only -- the keypoints and the
    // descriptors of every camera), a rig slot's keypoints (k_track_points, nf * ncams rows), the projections, validity bytes and
    // gathered points, the queries' results, and what the host tail reads: the compacted rows and the counts, MCORB_MAX_CAMS per
    // frame, host-mapped pinned memory k_track_compact writes.  A frame's block of every per-pair array begins at ncams * (its
    // first candidate)
    struct Tracking {
        mcorb::Staged in;
        mcorb::DevBuf<float2> d_kp, d_xy;
        mcorb::DevBuf<uint8_t> d_valid;
        mcorb::DevBuf<double> d_pt;
        mcorb::HostBuf<double> h_pt;
        mcorb::DevBuf<mcorb::TrBest> d_best;
        mcorb::HostBuf<mcorb::TrRow> h_rows;
        mcorb::HostBuf<int32_t> h_nproj;
        // the de-duplication on the device: per camera the arg-min table (owner, val: cleared in every submission), per (camera,
        // candidate) the slot and the winner flag, and what the host reads: the matches and their counts, host-mapped as the rows are
        mcorb::DevBuf<uint32_t> d_owner;
        mcorb::DevBuf<unsigned long long> d_val;
        mcorb::DevBuf<int32_t> d_slot;
        mcorb::DevBuf<uint8_t> d_win;
        mcorb::HostBuf<mcorb::TrMatch> h_match;
        mcorb::HostBuf<int32_t> h_nmatch;
        // a submission's pieces in stream order: [k_track_points,] k_track_project, _match, _compact, the table's clear with the
        // three kernels of the de-duplication
        enum { kPoints, kProject, kMatch, kCompact, kDedup };
        mcorb::Spans<5> chain;
        TrackCall call;
        std::atomic<bool> pending{false};
        // mcorb_lmap_set_track_refine: the pose refinement behind every submission (pose.t), whose results stay readable until the
        // next one.  pose_nf: the frames of the last tracking call if it ran with the option, 0 otherwise
        bool refine = false;
        mcorb_pose_params refine_params = {};
        int pose_nf = 0;
#ifdef MCORB_TRACK_PROF
        float us_phase[5] = {};   // the last call's host phases: candidate walk, submission, wait, de-duplication, output
#endif
        // a submission of nf frames: `bytes` of input, rows = ncams * candidates, `slots` table entries, kp keypoint rows of a
        // rig slot, pts gathered points (0: none wanted)
        int reserve(size_t bytes, size_t rows, size_t nf, size_t slots, size_t kp, size_t pts)
        {
            TRY(in.reserve(bytes));
            TRY(d_xy.grow(rows));
            TRY(d_valid.grow(rows));
            TRY(d_best.grow(rows));
            TRY(h_rows.grow(rows, mcorb::kHostMapped));
            TRY(h_nproj.grow(nf * MCORB_MAX_CAMS, mcorb::kHostMapped));
            TRY(d_owner.grow(slots));
            TRY(d_val.grow(slots));
            TRY(d_slot.grow(rows));
            TRY(d_win.grow(rows));
            TRY(h_match.grow(rows, mcorb::kHostMapped));
            TRY(h_nmatch.grow(nf * MCORB_MAX_CAMS, mcorb::kHostMapped));
            TRY(d_kp.grow(kp));
            TRY(d_pt.grow(pts * 3));
            return h_pt.grow(pts * 3, hipHostMallocDefault);
        }
    } track;

    // the pose refinement (mcorb_pose.cpp): x serves mcorb_lmap_refine_pose, t the refinement behind a tracking submission
    struct Pose {
        mcorb::PoseBufs x, t;
        mcorb::Spans<1> refine;                 // around k_pose_refine of mcorb_lmap_refine_pose
    } pose;

    // the local bundle adjustment (mcorb_ba.cpp), grow-only: the packed input (BaLayout); both halves of the state (poses:
    // MCORB_BA_MAX_KF each, points: nlm x 3 each), the landmarks' V, gp and cost, the views, the folded sums of the keyframes and
    // the pairs, the step, the loop's record; and what the host reads, host-mapped: the result with the poses, the points, the flags
    struct Ba {
        mcorb::Staged in;
        mcorb::DevBuf<mcorb::PoseState> d_poses;
        mcorb::DevBuf<double> d_pts, d_V, d_gp, d_cost, d_views, d_diag, d_pairs, d_delta;
        mcorb::DevBuf<mcorb::BaRecord> d_rec;
        mcorb::DevBuf<int32_t> d_count;         // k_ba_flags' inliers per workgroup
        mcorb::HostBuf<mcorb::BaOut> h_out;
        mcorb::HostBuf<double> h_pts;
        mcorb::HostBuf<uint8_t> h_flags;
        enum { kBegin, kSchur, kSolve, kUpdate, kAccept, kRest, kFinal };
        mcorb::Spans<MCORB_BA_SPANS> chain;
        int last_idle = 0;                      // the launches of the last chain that were queued behind the loop's end
        int reserve(size_t bytes, size_t nlm, size_t nobs, size_t nviews)
        {
            TRY(in.reserve(bytes));
            TRY(d_poses.grow(2 * MCORB_BA_MAX_KF));
            TRY(d_pts.grow(2 * 3 * nlm));
            TRY(d_V.grow(6 * nlm));
            TRY(d_gp.grow(3 * nlm));
            TRY(d_cost.grow(nlm));
            TRY(d_views.grow((size_t)mcorb::kBaView * nviews + 1));
            TRY(d_diag.grow((size_t)mcorb::kBaDiag * MCORB_BA_MAX_KF));
            TRY(d_pairs.grow((size_t)mcorb::kBaPair * mcorb::kBaMaxPairs));
            TRY(d_delta.grow(mcorb::kBaMaxN));
            TRY(d_rec.grow(1));
            TRY(d_count.grow(std::max(nobs, 3 * nlm) / 256 + 1));
            TRY(h_out.grow(1, mcorb::kHostMapped));
            TRY(h_pts.grow(3 * nlm + 1, mcorb::kHostMapped));
            return h_flags.grow(nobs, mcorb::kHostMapped);
        }
    } ba;

    // the re-triangulation after the back end moved keyframes (mcorb_retri.cpp), grow-only: the packed input (RetriLayout), the
    // view table, and what the host reads: a record per landmark, host-mapped
    struct Retri {
        mcorb::Staged in;
        mcorb::DevBuf<double> d_views;
        mcorb::HostBuf<mcorb::RetriOut> h_out;
        enum { kViews, kSolve };
        mcorb::Spans<MCORB_RETRI_SPANS> chain;  // k_retri_views, k_retri_solve
        int reserve(size_t bytes, size_t nviews, size_t nlm)
        {
            TRY(in.reserve(bytes));
            TRY(d_views.grow((size_t)mcorb::kRetriView * nviews + 1));
            return h_out.grow(nlm, mcorb::kHostMapped);
        }
    } retri;

    // the RANSAC in front of the refinement (mcorb_sac.cpp), grow-only: the packed input (ObsLayout with its RANSAC part), the
    // models and counts of the hypotheses, and what the host reads: the pick's record and the flags per observation, host-mapped.
    // `pose`: the buffers of the refinement behind it, whose input is part of `in`
    struct Sac {
        mcorb::Staged in;
        mcorb::DevBuf<mcorb::SacModel> d_models;
        mcorb::DevBuf<int32_t> d_count;
        mcorb::HostBuf<mcorb::SacOut> h_out;
        mcorb::HostBuf<uint8_t> h_flags;
        mcorb::PoseBufs pose;
        mcorb::Spans<3> kernels;                // k_sac_hypotheses[_rig], k_sac_score, k_sac_pick
        int last_hyp = 0;                       // the hypotheses of the last call that ran any (either kind of store)
        std::vector<int32_t> host_count, host_valid;   // a host-only store's last counts, for mcorb_lmap_last_ransac_counts
        int reserve(size_t bytes, size_t n, size_t H, bool refine)
        {
            TRY(in.reserve(bytes));
            TRY(d_models.grow(H));
            TRY(d_count.grow(H));
            TRY(h_out.grow(1, mcorb::kHostMapped));
            TRY(h_flags.grow(n, mcorb::kHostMapped));
            return refine ? pose.reserve(n) : MCORB_OK;
        }
    } sac;

    // the relative pose between two frames by RANSAC (mcorb_rel.cpp), grow-only: the packed input (RelLayout), the models and
    // counts of the hypotheses, and what the host reads: the pick's record and the flags per match, host-mapped
    struct Rel {
        mcorb::Staged in;
        mcorb::DevBuf<mcorb::RelModel> d_models;
        mcorb::DevBuf<int32_t> d_count;
        mcorb::HostBuf<mcorb::RelOut> h_out;
        mcorb::HostBuf<uint8_t> h_flags;
        mcorb::Spans<3> kernels;                // k_rel_hypotheses, k_rel_score, k_rel_pick
        int last_hyp = 0;                       // the hypotheses of the last call that ran any (either kind of store)
        std::vector<int32_t> host_count, host_valid;   // a host-only store's last counts, for mcorb_lmap_last_relative_counts
        int reserve(size_t bytes, size_t n, size_t H)
        {
            TRY(in.reserve(bytes));
            TRY(d_models.grow(H));
            TRY(d_count.grow(H));
            TRY(h_out.grow(1, mcorb::kHostMapped));
            return h_flags.grow(n, mcorb::kHostMapped);
        }
        // mcorb_lmap_relative_pose_polished: the pick's record and flags stay in device memory (d_member: the current flags and
        // the other set, 2 n), k_rel_fit writes h_out, h_flags and the polish record
        mcorb::DevBuf<mcorb::RelOut> d_pick;
        mcorb::DevBuf<uint8_t> d_member;
        mcorb::HostBuf<mcorb::RelPolish> h_polish;
        mcorb::Spans<1> fit;                    // k_rel_fit
        int reserve_polish(size_t n)
        {
            TRY(d_pick.grow(1));
            TRY(d_member.grow(2 * n));
            return h_polish.grow(1, mcorb::kHostMapped);
        }
    } rel;

    // the pose between two frames from 3D-3D pairs (mcorb_align.cpp), grow-only: the packed input (AlignLayout), the models and
    // counts of the hypotheses, the winner and its members for the refit, and what the host reads: k_align_fit's record and the
    // flags per pair, host-mapped
    struct Align {
        mcorb::Staged in;
        mcorb::DevBuf<mcorb::AlignModel> d_models;
        mcorb::DevBuf<int32_t> d_count;
        mcorb::DevBuf<mcorb::AlignPick> d_pick;
        mcorb::DevBuf<uint8_t> d_member;
        mcorb::HostBuf<mcorb::AlignOut> h_out;
        mcorb::HostBuf<uint8_t> h_flags;
        mcorb::Spans<3> sac;                    // k_align_hypotheses, k_align_score, k_align_pick (mode 1)
        mcorb::Spans<1> fit;                    // k_align_fit
        int last_hyp = 0;                       // the hypotheses of the last mode-1 call that ran any (either kind of store)
        std::vector<int32_t> host_count, host_valid;   // a host-only store's last counts, for mcorb_lmap_last_align_counts
        int reserve(size_t bytes, size_t n, size_t H)
        {
            TRY(in.reserve(bytes));
            TRY(d_models.grow(H));
            TRY(d_count.grow(H));
            TRY(d_pick.grow(1));
            TRY(d_member.grow(n));
            TRY(h_out.grow(1, mcorb::kHostMapped));
            return h_flags.grow(n, mcorb::kHostMapped);
        }
    } align;

    // the pose of one camera between two frames by five-point RANSAC (mcorb_ess.cpp), grow-only: the packed input (EssLayout), the
    // model of every (hypothesis, root) slot, the hypotheses' samples, the slots' valid flags once more as a dense array, the slots' counts with the four votes behind them, the
    // winner and its candidates, and what the host reads: k_ess_finish's record and the flags per match, host-mapped
    struct Ess {
        mcorb::Staged in;
        mcorb::DevBuf<mcorb::EssModel> d_models;
        mcorb::DevBuf<int32_t> d_samples, d_valid, d_count;
        mcorb::DevBuf<mcorb::EssPick> d_pick;
        mcorb::HostBuf<mcorb::EssOut> h_out;
        mcorb::HostBuf<uint8_t> h_flags;
        mcorb::Spans<4> kernels;                // k_ess_hypotheses, k_ess_score, k_ess_pick, k_ess_finish
        int last_hyp = 0;                       // the hypotheses of the last call that ran any (either kind of store)
        std::vector<int32_t> host_count;        // a host-only store's last counts and models, for mcorb_lmap_last_essential_counts
        std::vector<mcorb::EssModel> host_models;
        int reserve(size_t bytes, size_t n, size_t H)
        {
            TRY(in.reserve(bytes));
            TRY(d_models.grow(H * mcorb::kEssRoots));
            TRY(d_samples.grow(H * mcorb::kEssSample));
            TRY(d_valid.grow(H * mcorb::kEssRoots));
            TRY(d_count.grow(H * mcorb::kEssRoots + 4));
            TRY(d_pick.grow(1));
            TRY(h_out.grow(1, mcorb::kHostMapped));
            return h_flags.grow(n, mcorb::kHostMapped);
        }
        // mcorb_lmap_essential_pose_polished: k_ess_finish's record and flags stay in device memory (d_member: the current flags
        // and the other set, 2 n), k_ess_fit writes h_out, h_flags and the polish record
        mcorb::DevBuf<mcorb::EssOut> d_out;
        mcorb::DevBuf<uint8_t> d_member;
        mcorb::HostBuf<mcorb::EssPolish> h_polish;
        mcorb::Spans<1> fit;                    // k_ess_fit
        int reserve_polish(size_t n)
        {
            TRY(d_out.grow(1));
            TRY(d_member.grow(2 * n));
            return h_polish.grow(1, mcorb::kHostMapped);
        }
    } ess;

    // scratch of mcorb_lmap_initialize (mcorb_init.cpp), grow-only: the packed input (InitLayout), k_init_triangulate's records,
    // k_init_select's keys, id offsets and result, and what the host reads: every match's record and the call's, host-mapped
    struct Init {
        mcorb::Staged in;
        mcorb::DevBuf<mcorb::MapOut> d_rec;
        mcorb::DevBuf<uint64_t> d_keys;
        mcorb::DevBuf<int32_t> d_offset;
        mcorb::DevBuf<mcorb::InitSel> d_sel;
        mcorb::HostBuf<mcorb::MapOut> h_rec;
        mcorb::HostBuf<mcorb::InitCall> h_call;
        enum { kTriangulate, kSelect, kPut };
        mcorb::Spans<3> kernels;                // k_init_triangulate (both instances), k_init_select, k_init_put
        int last_launched = 0;
        int reserve(size_t bytes, size_t n)
        {
            TRY(in.reserve(bytes));
            TRY(d_rec.grow(n));
            TRY(d_keys.grow(2 * n));
            TRY(d_offset.grow(n));
            TRY(d_sel.grow(1));
            TRY(h_rec.grow(n, mcorb::kHostMapped));
            return h_call.grow(1, mcorb::kHostMapped);
        }
    } init;
};

// the pose refinement behind a tracking call (mcorb_pose.cpp); the caller holds the store's lock and has set track_refine_params.
// pose_track_host: a host-only store, or a frame nothing was launched for -- the observations are the frame's matches, the
// cameras back to back in match order (kp_base / kp_stride: the frame's keypoint records, which begin with pt), flags: ncams *
// nc bytes.  pose_track_submit: k_pose_refine for the nf frames of a device submission, a piece of it behind its de-duplication on the
// store's stream; items: the submission's TrItems on the host, which say where a frame's candidates, rows and keypoints in
// kp_xy are
namespace mcorb {
void pose_track_host(mcorb_lmap *m, const mcorb_track_view &view, const int *cand, int nc, const TrMatch *matches, const int32_t *n_match,
                     const uint8_t *const *kp_base, size_t kp_stride, mcorb_pose_result &res, uint8_t *flags);
void pose_track_submit(Submission &sub, mcorb_lmap *m, const mcorb_track_view *views, const TrItem *items, int nf, const float2 *kp_xy,
                       const int *d_cand);
// shared with mcorb_sac.cpp: a refinement problem's job, its serial run, and the checks of its parameters
void pose_job_init(PoseJob &job, const mcorb_pose_params &p, int ncams, const mcorb_track_cam *cams, const PoseState &init);
void pose_run_host(const PoseJob &job, const PoseObs *obs, const double *pts, int n, uint8_t *alive, mcorb_pose_result &res);
int pose_check_params(const mcorb_pose_params *p);
// The observation input of mcorb_lmap_refine_pose and mcorb_lmap_ransac_pose (mcorb_pose.cpp): observation i is the keypoint
// uv[i] of level octave[i] in camera cam[i], of landmark lids[i] or of the point pts[i].  who: the entry's error prefix.
// obs_check: the arguments, before the lock (nlevels: what an octave may reach; match: ransac_pose's indices or NULL);
// obs_check_locked: no tracking call is pending and every landmark has a point.  obs_gather: the observations and their points
// for the serial run.  obs_stage: the observations and their ids or points into a pinned ObsLayout block; obs_enqueue_refine:
// k_pose_refine on the block's PoseJob, observations and ids or points, the rest of the problem in b
struct ObsInput {
    int n;
    const int32_t *cam;
    const float *uv;
    const int32_t *octave, *lids;
    const double *pts;
    int ncams;
    const mcorb_track_cam *cams;
};
int obs_check(const mcorb_lmap *m, const ObsInput &in, int nlevels, const int32_t *match, const char *who);
int obs_check_locked(const mcorb_lmap *m, const ObsInput &in, const char *who);
void obs_gather(const mcorb_lmap *m, const ObsInput &in, std::vector<PoseObs> &obs, std::vector<double> &X);
void obs_stage(const ObsInput &in, const ObsLayout &L, const Staged &s);
void obs_enqueue_refine(const mcorb_lmap *m, const ObsInput &in, const ObsLayout &L, const Staged &s, const PoseBufs &b);

// the body of mcorb_lmap_delete behind its checks (mcorb_landmark.cpp), shared with mcorb_lmap_retriangulate: the caller holds the
// store's lock, the ids are inside the store, duplicate-free and of slots that were set, and kfs / feats hold every pair
int lmap_delete_checked(mcorb_lmap *m, const int32_t *lids, int n, int32_t *kfs, int32_t *feats);

// shared by the test hooks of mcorb_mapping.cpp and mcorb_init.cpp.  to_device: src[0 .. n) into a fresh d
template <class T>
int to_device(DevBuf<T> &d, const T *src, size_t n)
{
    TRY(d.alloc(n));
    HIPCHK(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
    return MCORB_OK;
}

// from_device: d[0 .. n) into dst, behind everything queued on the null stream
template <class T>
int from_device(T *dst, const DevBuf<T> &d, size_t n)
{
    HIPCHK(hipMemcpy(dst, d, n * sizeof(T), hipMemcpyDeviceToHost));
    return MCORB_OK;
}

// zeroed(d, n): a fresh d of n zero elements
template <class T>
int zeroed(DevBuf<T> &d, size_t n)
{
    TRY(d.alloc(n));
    HIPCHK(hipMemset(d, 0, n * sizeof(T)));
    return MCORB_OK;
}

// the device of a self-test entry, made current
inline int selftest_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { set_error("no usable HIP device"); return MCORB_E_NODEVICE; }
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();   // (a stale error of this thread is not this call's)
    return MCORB_OK;
}

// the cases of a self-test on the device: the n checked cases h (check_cases: voff[n] views in all) and the level table
struct CasesDev {
    DevBuf<double> X, P, K, c;
    DevBuf<int32_t> nv1, nv, voff, oct;
    DevBuf<float> kps, sig;
    int upload(int n, const MapCases &h, int nlevels)
    {
        const size_t N = (size_t)n, V = (size_t)h.voff[n];
        TRY(to_device(X, h.X, N * 3));
        TRY(to_device(P, h.P, V * 12));
        TRY(to_device(K, h.K, V * 9));
        TRY(to_device(c, h.centre, V * 3));
        TRY(to_device(nv1, h.nv1, N));
        TRY(to_device(nv, h.nv, N));
        TRY(to_device(voff, h.voff, N + 1));
        TRY(to_device(oct, h.octave, V));
        TRY(to_device(kps, h.kps, V * 2));
        return to_device(sig, h.inv_sigma2, (size_t)nlevels);
    }
    MapCases cases() const { return MapCases{X, nv1, nv, voff, P, K, c, kps, oct, sig}; }
};
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
    if (m->track.pending.load()) {
        mcorb::set_error(std::string(who) + ": a submitted tracking call has not been waited for");
        return MCORB_E_STATE;
    }
    return MCORB_OK;
}

// mcorb_lmap_last_*_counts: the count and the valid flag of every slot (per_hyp of them per hypothesis) of the last call of
// m->*bufs that ran any hypotheses, a device store's from d_count and d_models.  who / fail: the entry's name and its error.
// host_valid(b, s): a host-only store's flag of slot s (host_valid_array: where the store keeps them as host_valid); each(s,
// model): what else the entry hands out per slot of a device store (each_nothing)
inline const auto host_valid_array = [](const auto &b, int s) { return b.host_valid[s]; };
inline const auto each_nothing = [](int, const auto &) {};
template <class Model, class Bufs, class HostValid, class Each>
int last_counts(mcorb_lmap *m, Bufs mcorb_lmap::*bufs, int per_hyp, const char *who, int (*fail)(int, const char *), int32_t *count,
                int32_t *valid, int cap, int *n_slots, HostValid host_valid, Each each)
{
    TRY(check_lmap(m, who));
    if (cap < 0 || !n_slots || (cap && (!count || !valid))) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    const Bufs &b = m->*bufs;
    const int N = b.last_hyp * per_hyp;
    *n_slots = N;
    if (cap < N) return fail(MCORB_E_CAP, "arrays too small");
    if (!N) return MCORB_OK;
    if (m->device < 0) {
        for (int s = 0; s < N; s++) {
            count[s] = b.host_count[s];
            valid[s] = host_valid(b, s);
        }
        return MCORB_OK;
    }
    HIPCHK(hipSetDevice(m->device));
    std::vector<Model> models((size_t)N);
    HIPCHK(hipMemcpy(count, b.d_count, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(models.data(), b.d_models, (size_t)N * sizeof(Model), hipMemcpyDeviceToHost));
    for (int s = 0; s < N; s++) {
        valid[s] = models[s].valid;
        each(s, models[s]);
    }
    return MCORB_OK;
}
