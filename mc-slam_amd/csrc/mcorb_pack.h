// mcorb_pack.h -- the packed inputs of the local map's calls: every call that uploads several arrays puts them into one pinned
// block and copies it once (Staged, mcorb_lmap_store.h).  Pack hands out the items' offsets; the layouts below are the blocks the
// library builds, one per call.  No HIP here: tests/cpp/test_pack_sanitize.cpp includes this file from a plain g++ program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mcorb_align.h"
#include "mcorb_ba.h"
#include "mcorb_ess.h"
#include "mcorb_mapping.h"
#include "mcorb_rel.h"
#include "mcorb_retri.h"
#include "mcorb_sac.h"

namespace mcorb {

// offsets into one block, item by item: every item begins at a multiple of kAlign, an item of no elements takes no space
struct Pack {
    static constexpr size_t kAlign = 32;
    size_t total = 0;
    template <class T>
    size_t add(size_t n)
    {
        const size_t off = total;
        total += (n * sizeof(T) + kAlign - 1) & ~(kAlign - 1);
        return off;
    }
};

// The layouts: a Pack and the offsets of its items, added in the order the members are declared (total: p.total).
// mcorb_lmap_refine_pose and mcorb_lmap_ransac_pose: the PoseJob of the refinement, the observations and their ids (lids) or
// points; sac: the SacJob and the lists the draws index (S consensus observations, ncams + 1 firsts, a byte per observation)
struct ObsLayout {
    Pack p;
    size_t pose_job, sac_job, obs, pt, cons, cam_first, cam_cons, is_first;
    ObsLayout(size_t n, bool lids, bool sac, size_t S, size_t ncams)
        : pose_job(p.add<PoseJob>(1)), sac_job(p.add<SacJob>(sac ? 1 : 0)), obs(p.add<PoseObs>(n)),
          pt(lids ? p.add<int32_t>(n) : p.add<double>(3 * n)), cons(p.add<int32_t>(sac ? S : 0)),
          cam_first(p.add<int32_t>(sac ? ncams + 1 : 0)), cam_cons(p.add<int32_t>(sac ? S : 0)), is_first(p.add<uint8_t>(sac ? n : 0)) {}
};

// mcorb_lmap_relative_pose: the RelJob and the n matches
struct RelLayout {
    Pack p;
    size_t job, obs;
    explicit RelLayout(size_t n) : job(p.add<RelJob>(1)), obs(p.add<RelObs>(n)) {}
};

// mcorb_lmap_essential_pose: the EssJob and the n matches
struct EssLayout {
    Pack p;
    size_t job, obs;
    explicit EssLayout(size_t n) : job(p.add<EssJob>(1)), obs(p.add<EssObs>(n)) {}
};

// mcorb_lmap_align_pose: the AlignJob, frame 1's points or their landmark ids (lids), frame 2's points
struct AlignLayout {
    Pack p;
    size_t job, p1, p2;
    AlignLayout(size_t n, bool lids) : job(p.add<AlignJob>(1)), p1(lids ? p.add<int32_t>(n) : p.add<double>(3 * n)), p2(p.add<double>(3 * n)) {}
};

// mcorb_lmap_bundle_adjust: the BaJob, the keyframes' poses, the landmarks' ids (lids) or points, the sorted observations and the
// per-landmark tables (BaPlan)
struct BaLayout {
    Pack p;
    size_t job, poses, pt, obs, obs_first, view_first, slot;
    BaLayout(size_t nkf, size_t nlm, size_t nobs, bool lids)
        : job(p.add<BaJob>(1)), poses(p.add<PoseState>(nkf)), pt(lids ? p.add<int32_t>(nlm) : p.add<double>(3 * nlm)),
          obs(p.add<BaObs>(nobs)), obs_first(p.add<int32_t>(nlm + 1)), view_first(p.add<int32_t>(nlm + 1)),
          slot(p.add<int8_t>(nlm * MCORB_BA_MAX_KF)) {}
};

// mcorb_lmap_retriangulate: the job, the poses and moved flags of the keyframes that have an observation, the landmarks' ids, the
// sorted observations and the landmarks' spans
struct RetriLayout {
    Pack p;
    size_t job, poses, moved, lids, obs, obs_first;
    RetriLayout(size_t nslots, size_t nlm, size_t nobs)
        : job(p.add<RetriJob>(1)), poses(p.add<PoseState>(nslots)), moved(p.add<uint8_t>(nslots)), lids(p.add<int32_t>(nlm)),
          obs(p.add<RetriObs>(nobs)), obs_first(p.add<int32_t>(nlm + 1)) {}
};

// a tracking submission of nf frames: a TrItem and a view per frame, every frame's candidates, then -- host arrays only -- the
// keypoints (x, y) and descriptors of all cameras
struct TrackLayout {
    Pack p;
    size_t items, views, cand, xy, desc;
    TrackLayout(size_t nf, size_t ncand, size_t total_kp)
        : items(p.add<TrItem>(nf)), views(p.add<mcorb_track_view>(nf)), cand(p.add<int32_t>(ncand)), xy(p.add<float>(2 * total_kp)),
          desc(p.add<uint8_t>(32 * total_kp)) {}
};

// the two mapping entries (mcorb_mapping.h): nframes frames, nF doubles of F tables (none: mcorb_lmap_triangulate_new), K per
// camera, the level table, the frames' match indices and keypoints, the blocks and items, and the nz landmarks whose depth is taken
struct MapLayout {
    Pack p;
    size_t frames, F, K, sig, mi, kp, blocks, items, zlids;
    MapLayout(size_t nframes, size_t nF, size_t ncams, size_t nlevels, size_t nmi, size_t nkp, size_t nblocks, size_t nitems, size_t nz)
        : frames(p.add<MapFrameDev>(nframes)), F(p.add<double>(nF)), K(p.add<double>(ncams * 9)), sig(p.add<float>(nlevels)),
          mi(p.add<int32_t>(nmi)), kp(p.add<MapKp>(nkp)), blocks(p.add<MapBlock>(nblocks)), items(p.add<MapItem>(nitems)),
          zlids(p.add<int32_t>(nz)) {}
    MapArgs args(uint8_t *base, MapOut *out, int ncams) const
    {
        MapArgs a;
        a.frames = (const MapFrameDev *)(base + frames);
        a.mi = (const int32_t *)(base + mi);
        a.kp = (const MapKp *)(base + kp);
        a.F = (const double *)(base + F);
        a.K = (const double *)(base + K);
        a.inv_sigma2 = (const float *)(base + sig);
        a.blocks = (const MapBlock *)(base + blocks);
        a.items = (const MapItem *)(base + items);
        a.out = out;
        a.ncams = ncams;
        return a;
    }
};

// mcorb_lmap_initialize: a MapLayout of two frames (the current one first) without F tables and depths, then the n matches'
// flags on entry and their queryIdx / trainIdx
struct InitLayout {
    MapLayout m;
    size_t flags, query, train;
    InitLayout(size_t ncams, size_t nlevels, size_t nmi, size_t nkp, size_t nblocks, size_t nitems, size_t n)
        : m(2, 0, ncams, nlevels, nmi, nkp, nblocks, nitems, 0), flags(m.p.add<uint8_t>(n)), query(m.p.add<int32_t>(n)),
          train(m.p.add<int32_t>(n)) {}
};

}  // namespace mcorb
