// mcorb_map_host.h -- the argument side of the three triangulation entries, mcorb_lmap_triangulate_neighbours and
// mcorb_lmap_triangulate_new (mcorb_mapping.cpp) and mcorb_lmap_initialize (mcorb_init.cpp): MapCall has the steps every entry
// runs between its own argument checks and its own walk -- check the frames and their ids, count every match's views, order the
// wanted matches into blocks (MapWork), size and pack the block (MapLayout, mcorb_pack.h) -- and check_cases is the checks of the
// test hooks' cases.  No HIP here: the two .cpp files and the plain g++ programs tests/cpp/test_init_sanitize.cpp and
// test_mapping_new_sanitize.cpp include this file, so the programs pack through the code the library packs through.  A program
// defines mcorb::set_error itself.
#pragma once
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mcorb.h"
#include "mcorb_pack.h"

namespace mcorb {
void set_error(const std::string &msg);

// The matches that need a record, as a device store's kernels take them: per segment (a neighbour; the previous keyframe is
// segment 0) by view count, in blocks of one wave, the matches of at most 4 views first.  Segment s's matches are query[s] /
// train[s][0 .. n[s]) and lie at moff[s] in nviews and item_of; wanted(s, j): match j of segment s needs a record
struct MapWork {
    std::vector<int32_t> item_of;
    std::vector<MapItem> items;
    std::vector<MapBlock> blocks;
    int nblocks_small = 0;
    template <class Wanted>
    void order(int nseg, const int32_t *const *query, const int32_t *const *train, const int32_t *n, const size_t *moff,
               const uint8_t *nviews, Wanted wanted)
    {
        std::vector<int> order;
        for (int pass = 0; pass < 2; pass++) {   // 0: at most 4 views, 1: the rest
            for (int s = 0; s < nseg; s++) {
                const uint8_t *nv = nviews + moff[s];
                order.clear();
                for (int j = 0; j < n[s]; j++)
                    if ((nv[j] <= 4) == (pass == 0) && wanted(s, j)) order.push_back(j);
                std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nv[a] < nv[b]; });
                for (size_t k = 0; k < order.size(); k++) {
                    if (k % kMapBlock == 0)
                        blocks.push_back(MapBlock{s, (int32_t)items.size(), (int32_t)std::min<size_t>(kMapBlock, order.size() - k)});
                    const int j = order[k];
                    item_of[moff[s] + j] = (int32_t)items.size();
                    items.push_back(MapItem{query[s][j], train[s][j], (int32_t)items.size()});
                }
            }
            if (pass == 0) nblocks_small = (int)blocks.size();
        }
    }
};

// One call of an entry.  who: the entry's name, the prefix of every error below; max_landmarks: the store's; C: the cameras of
// every frame.  The entry adds its frames in packed order, the current frame first (add), counts the views of its matches
// (count_views), orders the wanted ones (w.order), and once fits() holds takes layout() and packs the block at a base pointer of
// layout().p.total bytes: a device store's pinned input (Staged::h) or a host vector
struct MapCall {
    const char *who;
    int max_landmarks, C, nlevels;
    std::vector<const mcorb_map_frame *> frames;
    MapWork w;
    size_t nmi = 0, nkp = 0;   // what the frames add to the block: match indices and keypoints

    int fail(int code, const char *what) const { set_error(std::string(who) + ": " + what); return code; }
    int bad(const char *what) const { return fail(MCORB_E_ARG, what); }

    // a frame's arrays: camera count, indices inside the keypoint lists
    int check_frame(const mcorb_map_frame &f) const
    {
        if (f.ncams != C || f.nfeat < 0 || !f.nkps || !f.kps_undist || (f.nfeat && !f.match_index)) return bad("bad frame");
        for (int c = 0; c < C; c++)
            if (f.nkps[c] < 0 || (f.nkps[c] && !f.kps_undist[c])) return bad("bad frame");
        for (size_t i = 0; i < (size_t)f.nfeat * C; i++) {
            const int k = f.match_index[i];
            if (k < -1 || k >= f.nkps[i % C]) return bad("match index outside a frame's keypoints");
        }
        return MCORB_OK;
    }
    // a frame's lIds: -1 or a slot of the store
    int check_lids(const mcorb_map_frame &f, const int32_t *lids) const
    {
        for (int i = 0; i < f.nfeat; i++)
            if (lids[i] < -1 || lids[i] >= max_landmarks) return bad("landmark id outside the store");
        return MCORB_OK;
    }
    // a checked frame as the next one of the block
    void add(const mcorb_map_frame &f)
    {
        frames.push_back(&f);
        nmi += (size_t)f.nfeat * f.ncams;
        for (int c = 0; c < f.ncams; c++) nkp += (size_t)f.nkps[c];
    }

    // the views of a feature: their count, or -1 for an octave outside [0, nlevels)
    int views_of(const mcorb_map_frame &f, int feat) const
    {
        int nv = 0;
        for (int c = 0; c < f.ncams; c++) {
            const int k = f.match_index[(size_t)feat * f.ncams + c];
            if (k == -1) continue;
            const int o = f.kps_undist[c][k].octave;
            if (o < 0 || o >= nlevels) return -1;
            nv++;
        }
        return nv;
    }
    // the views of a match of feature q of `other` (a neighbour, the previous keyframe) with feature t of the current frame:
    // nv = their count in both frames, nv_cur = in the current frame alone
    int count_views(const mcorb_map_frame &other, int q, int t, uint8_t &nv, uint8_t &nv_cur) const
    {
        const mcorb_map_frame &cur = *frames[0];
        if (q < 0 || q >= other.nfeat || t < 0 || t >= cur.nfeat) return bad("match index outside a frame");
        const int v1 = views_of(other, q), v2 = views_of(cur, t);
        if (v1 < 0 || v2 < 0) return bad("octave outside nlevels");
        if (v1 < 1 || v2 < 1) return bad("a matched feature without a view");
        if (v1 + v2 > MCORB_MAX_CAMS) return bad("a match of more than MCORB_MAX_CAMS views in total (the solver's design limit)");
        nv = (uint8_t)(v1 + v2);
        nv_cur = (uint8_t)v2;
        return MCORB_OK;
    }

    // the frames' offsets are 32-bit
    int fits() const { return nmi > 0x7fffffff || nkp > 0x7fffffff ? bad("frames too large") : MCORB_OK; }
    // the block: nF doubles of F tables and nz landmarks whose depth is taken (triangulate_neighbours' alone)
    MapLayout layout(size_t nF, size_t nz) const
    {
        return MapLayout(frames.size(), nF, (size_t)C, (size_t)nlevels, nmi, nkp, w.blocks.size(), w.items.size(), nz);
    }
    // the frames, K, the level table, the blocks and the items into the block at base
    void pack(uint8_t *base, const MapLayout &L, const double *K, const float *inv_sigma2) const
    {
        MapFrameDev *fr = (MapFrameDev *)(base + L.frames);
        int32_t *mi = (int32_t *)(base + L.mi);
        MapKp *kp = (MapKp *)(base + L.kp);
        size_t mi_at = 0, kp_at = 0;
        for (const mcorb_map_frame *f : frames) {
            MapFrameDev &d = *fr++;
            memcpy(d.proj, f->proj, sizeof(d.proj));
            memcpy(d.centre, f->centre_w, sizeof(d.centre));
            d.mi_off = (int32_t)mi_at;
            d.pad = 0;
            const size_t n = (size_t)f->nfeat * f->ncams;
            if (n) memcpy(mi + mi_at, f->match_index, n * sizeof(int32_t));
            mi_at += n;
            for (int c = 0; c < MCORB_MAX_CAMS; c++) {
                d.kp_off[c] = (int32_t)kp_at;
                if (c >= f->ncams) continue;
                for (int k = 0; k < f->nkps[c]; k++) {
                    const mcorb_keypoint &s = f->kps_undist[c][k];
                    kp[kp_at + k] = MapKp{s.x, s.y, s.octave};
                }
                kp_at += (size_t)f->nkps[c];
            }
        }
        memcpy(base + L.K, K, (size_t)C * 9 * sizeof(double));
        memcpy(base + L.sig, inv_sigma2, (size_t)nlevels * sizeof(float));
        if (!w.blocks.empty()) memcpy(base + L.blocks, w.blocks.data(), w.blocks.size() * sizeof(MapBlock));
        if (!w.items.empty()) memcpy(base + L.items, w.items.data(), w.items.size() * sizeof(MapItem));
    }
    // mcorb_lmap_initialize's extras behind pack(): the current frame's centres are cam_centre_body, then the n matches' flags
    // on entry and their queryIdx / trainIdx
    void pack_init(uint8_t *base, const InitLayout &L, const double *cam_centre_body, const uint8_t *flags, const int32_t *query,
                   const int32_t *train, size_t n) const
    {
        MapFrameDev &cur = *(MapFrameDev *)(base + L.m.frames);
        memset(cur.centre, 0, sizeof(cur.centre));
        memcpy(cur.centre, cam_centre_body, (size_t)C * 3 * sizeof(double));
        if (!n) return;
        memcpy(base + L.flags, flags, n);
        memcpy(base + L.query, query, n * sizeof(int32_t));
        memcpy(base + L.train, train, n * sizeof(int32_t));
    }
};

// The cases of a test hook on the host: every array is there, the view counts are in range and every octave is a level; fills
// voff, c.voff included.  who: "map gates" (the refine hooks too) or "init cases"
inline int check_cases(const char *who, MapCases &c, int nlevels, int n, std::vector<int32_t> &voff)
{
    const auto bad = [&](const char *what) { set_error(std::string(who) + ": " + what); return MCORB_E_ARG; };
    if (!c.X || !c.nv1 || !c.nv || !c.P || !c.K || !c.centre || !c.kps || !c.octave || !c.inv_sigma2 || nlevels < 1 || n < 1)
        return bad("bad argument");
    voff.resize((size_t)n + 1);
    voff[0] = 0;
    for (int i = 0; i < n; i++) {
        if (c.nv1[i] < 1 || c.nv[i] <= c.nv1[i] || c.nv[i] > MCORB_MAX_CAMS) return bad("view counts out of range");
        voff[i + 1] = voff[i] + c.nv[i];
    }
    for (int w = 0; w < voff[n]; w++)
        if (c.octave[w] < 0 || c.octave[w] >= nlevels) return bad("octave outside nlevels");
    c.voff = voff.data();
    return MCORB_OK;
}

}  // namespace mcorb
