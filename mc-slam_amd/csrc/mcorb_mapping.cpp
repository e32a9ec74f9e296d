// mcorb_mapping.cpp -- FrontEnd::triangulateNeighbors (MCSlam/src/FrontEnd.cpp:4856-4899) with triangulateMatches (:5758-5953) and
// getSceneDepthStats (:4838-4853): the still-unassigned inter-frame matches of the current frame against its neighbouring keyframes
// become new landmarks of the local map (mcorb_lmap_store.h).  Not restated: insertKeyFrame
// and the cv::Mat inverses; the caller passes cur_T_ref * pose.inv() per camera, W_T_cur's translation per camera and F21.
//
// The per-match arithmetic is mcorb_mapping.h.  A device store runs it for every match whose two features have no landmark on
// entry in k_map_triangulate, all neighbours in one submission, with the depths of the neighbours' landmarks (k_map_depth) in front;
// the host-only store runs the same header serially.  What depends on order runs on the host in both: the baseline gate per
// neighbour, and the walk over neighbours and matches in which an accepted match gives both features its new id and thereby skips
// every later match of either feature.  An id is only ever set, never cleared, so a match that is assigned on entry is skipped in
// the walk too and needs no record.  The accepted points, normals and ray counts go from the records into their slots device to
// device (k_map_put); the frames carry no keyframe id, so the caller registers the two observations (mcorb_lmap_observe).
//
// mcorb_lmap_triangulate_new is the other half of FrontEnd::mapping: TriangulateNewLandmarks (:6465-6700) on the current frame's
// new_inter_matches against the previous keyframe.  Its per-match arithmetic is mcorb_mapping_new.h (k_map_refine_new on a device
// store); its walk tests the current frame's id alone, so the previous keyframe's id is overwritten by a later landmark.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

// the packed input of a call (mcorb_mapping.h): offsets into one block
struct Layout {
    size_t frames = 0, F = 0, K = 0, sig = 0, mi = 0, kp = 0, blocks = 0, items = 0, zlids = 0, total = 0;
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

// the entry that is checking its arguments (one call at a time per thread)
thread_local const char *g_who = "lmap triangulate_neighbours";
int bad(const char *what) { set_error(std::string(g_who) + ": " + what); return MCORB_E_ARG; }

// a frame's arrays: camera count, indices inside the keypoint lists
int check_frame(const mcorb_map_frame &f, int ncams)
{
    if (f.ncams != ncams || f.nfeat < 0 || !f.nkps || !f.kps_undist || (f.nfeat && !f.match_index)) return bad("bad frame");
    for (int c = 0; c < ncams; c++)
        if (f.nkps[c] < 0 || (f.nkps[c] && !f.kps_undist[c])) return bad("bad frame");
    for (size_t i = 0; i < (size_t)f.nfeat * ncams; i++) {
        const int k = f.match_index[i];
        if (k < -1 || k >= f.nkps[i % ncams]) return bad("match index outside a frame's keypoints");
    }
    return MCORB_OK;
}

// the views of a feature: their count, or -1 for an octave outside [0, nlevels)
int views_of(const mcorb_map_frame &f, int feat, int nlevels)
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

void pack_frame(const mcorb_map_frame &f, MapFrameDev &d, int32_t *mi, size_t &mi_at, MapKp *kp, size_t &kp_at)
{
    memcpy(d.proj, f.proj, sizeof(d.proj));
    memcpy(d.centre, f.centre_w, sizeof(d.centre));
    d.mi_off = (int32_t)mi_at;
    d.pad = 0;
    const size_t nmi = (size_t)f.nfeat * f.ncams;
    if (nmi) memcpy(mi + mi_at, f.match_index, nmi * sizeof(int32_t));
    mi_at += nmi;
    for (int c = 0; c < MCORB_MAX_CAMS; c++) {
        d.kp_off[c] = (int32_t)kp_at;
        if (c >= f.ncams) continue;
        for (int k = 0; k < f.nkps[c]; k++) {
            const mcorb_keypoint &s = f.kps_undist[c][k];
            kp[kp_at + k] = MapKp{s.x, s.y, s.octave};
        }
        kp_at += (size_t)f.nkps[c];
    }
}

double norm3(const double a[3], const double b[3])   // cv::norm(a - b)
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) { const double d = a[k] - b[k]; s += d * d; }
    return sqrt(s);
}

int check_gate_cases(const double *X, const int32_t *nv1, const int32_t *nv, const double *P, const double *K, const double *centre,
                     const float *kps, const int32_t *octave, const double *F, const float *inv_sigma2, int nlevels, int n,
                     std::vector<int32_t> &voff)
{
    if (!X || !nv1 || !nv || !P || !K || !centre || !kps || !octave || !F || !inv_sigma2 || nlevels < 1 || n < 1) {
        set_error("map gates: bad argument");
        return MCORB_E_ARG;
    }
    voff.resize((size_t)n + 1);
    voff[0] = 0;
    for (int i = 0; i < n; i++) {
        if (nv1[i] < 1 || nv[i] <= nv1[i] || nv[i] > MCORB_MAX_CAMS) { set_error("map gates: view counts out of range"); return MCORB_E_ARG; }
        voff[i + 1] = voff[i] + nv[i];
    }
    for (int w = 0; w < voff[n]; w++)
        if (octave[w] < 0 || octave[w] >= nlevels) { set_error("map gates: octave outside nlevels"); return MCORB_E_ARG; }
    return MCORB_OK;
}

void gates_out(const MapOut *o, int n, int32_t *verdict, int32_t *n_rays, double *vals)
{
    for (int i = 0; i < n; i++) {
        verdict[i] = o[i].verdict;
        n_rays[i] = o[i].n_rays;
        double *v = vals + 5 * (size_t)i;
        v[0] = o[i].dist2; v[1] = o[i].cos;
        for (int k = 0; k < 3; k++) v[2 + k] = o[i].normal[k];
    }
}

// vals: 9 per case (X, normal, dist, cost_initial, cost_final)
void refine_out(const MapOut *o, const MapNewExtra *e, int n, int32_t *verdict, int32_t *n_rays, int32_t *solves, float *cosp, double *vals)
{
    for (int i = 0; i < n; i++) {
        verdict[i] = o[i].verdict;
        n_rays[i] = o[i].n_rays;
        solves[i] = e[i].solves;
        cosp[i] = e[i].cos;
        double *v = vals + 9 * (size_t)i;
        for (int k = 0; k < 3; k++) { v[k] = o[i].X[k]; v[3 + k] = o[i].normal[k]; }
        v[6] = o[i].dist2; v[7] = e[i].cost_initial; v[8] = e[i].cost_final;
    }
}

}  // namespace

extern "C" {

int mcorb_lmap_triangulate_neighbours(mcorb_lmap *m, const mcorb_map_frame *cur, int32_t *lids_cur, const mcorb_map_frame *neigh,
                                      int32_t *const *lids_neigh, int n_neigh, const double *const *F21,
                                      const int32_t *const *match_query, const int32_t *const *match_train, const int32_t *n_matches,
                                      const double *K, const float *inv_sigma2, int nlevels, const double Rcw[9], const double tcw[3],
                                      int32_t next_lid, mcorb_map_out *out)
{
    g_who = "lmap triangulate_neighbours";
    if (out) { out->n_matches = out->n_depth = out->n_triangulated = 0; out->next_lid = next_lid; }
    TRY(check_lmap(m, "lmap triangulate_neighbours"));
    if (!cur || !out || n_neigh < 0 || !K || !inv_sigma2 || nlevels < 1 || !Rcw || !tcw || next_lid < 0 || out->cap_matches < 0 ||
        out->cap_depth < 0 || (cur->nfeat && !lids_cur) || (n_neigh && (!neigh || !lids_neigh || !F21 || !match_query || !match_train ||
        !n_matches || !out->neigh_skipped)))
        return bad("bad argument");
    const int C = cur->ncams;
    if (C < 1 || C > MCORB_MAX_CAMS) return bad("1 .. MCORB_MAX_CAMS cameras");
    std::lock_guard<std::mutex> lk(m->mu);

    // ---- 1. everything that can be refused is refused before anything runs ----
    TRY(check_frame(*cur, C));
    for (int i = 0; i < cur->nfeat; i++)
        if (lids_cur[i] < -1 || lids_cur[i] >= m->max_landmarks) return bad("landmark id outside the store");
    std::vector<size_t> moff((size_t)n_neigh + 1, 0);
    size_t nz = 0;
    for (int s = 0; s < n_neigh; s++) {
        const mcorb_map_frame &f = neigh[s];
        TRY(check_frame(f, C));
        if (n_matches[s] < 0 || (n_matches[s] && (!match_query[s] || !match_train[s])) || !F21[s] || (f.nfeat && !lids_neigh[s]))
            return bad("bad argument");
        moff[s + 1] = moff[s] + (size_t)n_matches[s];
        for (int i = 0; i < f.nfeat; i++) {
            const int l = lids_neigh[s][i];
            if (l < -1 || l >= m->max_landmarks) return bad("landmark id outside the store");
            if (l == -1) continue;
            if (!(m->flags[l] & kHasPt)) { set_error("lmap triangulate_neighbours: a neighbour's landmark was never set"); return MCORB_E_STATE; }
            nz++;
        }
    }
    const size_t total = moff[n_neigh];
    // the views of every match: counted once, here
    std::vector<uint8_t> nviews(total, 0);
    for (int s = 0; s < n_neigh; s++)
        for (int j = 0; j < n_matches[s]; j++) {
            const int q = match_query[s][j], t = match_train[s][j];
            if (q < 0 || q >= neigh[s].nfeat || t < 0 || t >= cur->nfeat) return bad("match index outside a frame");
            const int v1 = views_of(neigh[s], q, nlevels), v2 = views_of(*cur, t, nlevels);
            if (v1 < 0 || v2 < 0) return bad("octave outside nlevels");
            if (v1 < 1 || v2 < 1) return bad("a matched feature without a view");
            if (v1 + v2 > MCORB_MAX_CAMS) return bad("a match of more than MCORB_MAX_CAMS views in total (the solver's design limit)");
            nviews[moff[s] + j] = (uint8_t)(v1 + v2);
        }
    out->n_matches = (int32_t)total;
    if (total > (size_t)out->cap_matches) { set_error("lmap triangulate_neighbours: output too small"); return MCORB_E_CAP; }
    if (total && (!out->inliers || !out->verdict || !out->new_lid || !out->pt3d || !out->normal || !out->dist2 || !out->cos_parallax))
        return bad("bad argument");

    // ---- 2. the matches that need a record, per neighbour by view count: blocks of one wave, <= 4 views first ----
    const bool dev = m->device >= 0;
    std::vector<int32_t> item_of(total, -1);
    std::vector<MapItem> items;
    std::vector<MapBlock> blocks;
    int nblocks_small = 0;
    if (dev) {
        std::vector<int> order;
        for (int pass = 0; pass < 2; pass++) {   // 0: at most 4 views, 1: the rest
            for (int s = 0; s < n_neigh; s++) {
                order.clear();
                for (int j = 0; j < n_matches[s]; j++) {
                    const int nv = nviews[moff[s] + j];
                    if ((nv <= 4) != (pass == 0)) continue;
                    if (lids_neigh[s][match_query[s][j]] != -1 || lids_cur[match_train[s][j]] != -1) continue;
                    order.push_back(j);
                }
                std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nviews[moff[s] + a] < nviews[moff[s] + b]; });
                for (size_t k = 0; k < order.size(); k++) {
                    if (k % kMapBlock == 0)
                        blocks.push_back(MapBlock{s, (int32_t)items.size(), (int32_t)std::min<size_t>(kMapBlock, order.size() - k)});
                    const int j = order[k];
                    item_of[moff[s] + j] = (int32_t)items.size();
                    items.push_back(MapItem{match_query[s][j], match_train[s][j], (int32_t)items.size()});
                }
            }
            if (pass == 0) nblocks_small = (int)blocks.size();
        }
    }

    // ---- 3. the packed input ----
    Layout L;
    size_t nmi = (size_t)cur->nfeat * C, nkp = 0;
    for (int c = 0; c < C; c++) nkp += (size_t)cur->nkps[c];
    for (int s = 0; s < n_neigh; s++) {
        nmi += (size_t)neigh[s].nfeat * C;
        for (int c = 0; c < C; c++) nkp += (size_t)neigh[s].nkps[c];
    }
    if (nmi > 0x7fffffff || nkp > 0x7fffffff) return bad("frames too large");
    L.frames = 0;
    L.F = align8(L.frames + (size_t)(1 + n_neigh) * sizeof(MapFrameDev));
    L.K = L.F + (size_t)n_neigh * C * C * 9 * sizeof(double);
    L.sig = L.K + (size_t)C * 9 * sizeof(double);
    L.mi = align8(L.sig + (size_t)nlevels * sizeof(float));
    L.kp = align8(L.mi + nmi * sizeof(int32_t));
    L.blocks = align8(L.kp + nkp * sizeof(MapKp));
    L.items = align8(L.blocks + blocks.size() * sizeof(MapBlock));
    L.zlids = align8(L.items + items.size() * sizeof(MapItem));
    L.total = align8(L.zlids + nz * sizeof(int32_t));
    std::vector<uint8_t> host_block;
    uint8_t *base;
    if (dev) {
        HIPCHK(hipSetDevice(m->device));
        TRY(m->h_mapin.grow(L.total, hipHostMallocDefault));
        TRY(m->d_mapin.grow(L.total));
        base = m->h_mapin;
    } else {
        host_block.resize(L.total);
        base = host_block.data();
    }
    {
        MapFrameDev *fr = (MapFrameDev *)(base + L.frames);
        int32_t *mi = (int32_t *)(base + L.mi);
        MapKp *kp = (MapKp *)(base + L.kp);
        size_t mi_at = 0, kp_at = 0;
        pack_frame(*cur, fr[0], mi, mi_at, kp, kp_at);
        for (int s = 0; s < n_neigh; s++) {
            pack_frame(neigh[s], fr[1 + s], mi, mi_at, kp, kp_at);
            memcpy(base + L.F + (size_t)s * C * C * 9 * sizeof(double), F21[s], (size_t)C * C * 9 * sizeof(double));
        }
        memcpy(base + L.K, K, (size_t)C * 9 * sizeof(double));
        memcpy(base + L.sig, inv_sigma2, (size_t)nlevels * sizeof(float));
        if (!blocks.empty()) memcpy(base + L.blocks, blocks.data(), blocks.size() * sizeof(MapBlock));
        if (!items.empty()) memcpy(base + L.items, items.data(), items.size() * sizeof(MapItem));
        int32_t *zl = (int32_t *)(base + L.zlids);
        size_t at = 0;
        for (int s = 0; s < n_neigh; s++)
            for (int i = 0; i < neigh[s].nfeat; i++)
                if (lids_neigh[s][i] != -1) zl[at++] = lids_neigh[s][i];
    }

    // ---- 4. the depths of the neighbours' landmarks and the records ----
    std::vector<double> z_host;
    const double *z = nullptr;
    const int nitems = (int)items.size();
    if (dev) {
        hipStream_t st = m->st;
        TRY(m->h_mapz.grow(nz, hipHostMallocDefault));
        TRY(m->d_mapz.grow(nz));
        TRY(m->h_mapout.grow((size_t)nitems, hipHostMallocDefault));
        TRY(m->d_mapout.grow((size_t)nitems));
        HIPCHK(hipMemcpyAsync(m->d_mapin, m->h_mapin, L.total, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(m->ev0, st));
        launch_map_depth(st, Rcw, tcw, m->d_geom, (const int *)(m->d_mapin.get() + L.zlids), (int)nz, m->d_mapz);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(m->ev1, st));
        HIPCHK(hipEventRecord(m->ev2, st));
        launch_map_triangulate(st, L.args(m->d_mapin, m->d_mapout, C), nblocks_small, (int)blocks.size() - nblocks_small);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(m->ev3, st));
        if (nz) HIPCHK(hipMemcpyAsync(m->h_mapz, m->d_mapz, nz * sizeof(double), hipMemcpyDeviceToHost, st));
        if (nitems) HIPCHK(hipMemcpyAsync(m->h_mapout, m->d_mapout, (size_t)nitems * sizeof(MapOut), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0.f;
        ev_elapsed(&ms, m->ev0, m->ev1);
        m->us_map_depth = ms * 1000.f;
        ev_elapsed(&ms, m->ev2, m->ev3);
        m->us_map_tri = ms * 1000.f;
        z = m->h_mapz;
    } else {
        z_host.resize(nz);
        const int32_t *zl = (const int32_t *)(base + L.zlids);
        for (size_t i = 0; i < nz; i++) z_host[i] = map_depth(Rcw, tcw, &m->geom[(size_t)zl[i] * 6]);
        z = z_host.data();
    }
    m->last_map_launched = nitems;
    m->last_map_depth = (int)nz;

    // ---- 5. the baseline gate (:4868-4873) and the walk (:5809-5945), neighbours in order, matches in order ----
    std::vector<int32_t> lc(lids_cur, lids_cur + cur->nfeat);
    std::vector<std::vector<int32_t>> ln((size_t)n_neigh);
    std::vector<MapOut> rec_host;          // host-only store: the records of the new landmarks
    std::vector<int32_t> acc_match;        // the matches that became landmarks, in order
    std::vector<int32_t> acc_rec;          // their records: an item (device) or an entry of rec_host
    std::vector<uint8_t> verdict(total, 0);
    std::vector<uint8_t> skipped((size_t)n_neigh, 0);
    std::vector<double> dist2(total, 0.0), cosp(total, 0.0);
    const MapArgs ha = L.args(base, nullptr, C);
    size_t z_at = 0;
    std::vector<double> zs;
    for (int s = 0; s < n_neigh; s++) {
        ln[s].assign(lids_neigh[s], lids_neigh[s] + neigh[s].nfeat);
        zs.clear();
        for (int i = 0; i < neigh[s].nfeat; i++)
            if (lids_neigh[s][i] != -1) zs.push_back(z[z_at++]);
        if (zs.empty()) skipped[s] = 2;   // (the reference indexes an empty vector here: undefined)
        else {
            std::sort(zs.begin(), zs.end());
            const double medianDepth = zs[(zs.size() - 1) / 2];
            const double baseline = norm3(cur->twc, neigh[s].twc);
            if (baseline / medianDepth < 0.01) skipped[s] = 1;
        }
        for (int j = 0; j < n_matches[s]; j++) {
            const size_t i = moff[s] + j;
            const int q = match_query[s][j], t = match_train[s][j];
            if (skipped[s]) { verdict[i] = kMapNeighbourSkipped; continue; }
            if (ln[s][q] != -1 || lc[t] != -1) { verdict[i] = kMapAssigned; continue; }
            MapOut o_host;
            const MapOut *o;
            if (dev) o = &m->h_mapout[item_of[i]];
            else {
                MapArgs a = ha;
                a.out = &o_host;
                const MapItem it{q, t, 0};
                if (nviews[i] <= 4) map_item<false>(a, s, it); else map_item<true>(a, s, it);
                o = &o_host;
            }
            verdict[i] = (uint8_t)o->verdict;
            dist2[i] = o->dist2;
            cosp[i] = o->cos;
            if (o->verdict != kMapLandmark) continue;
            const int32_t id = next_lid + (int32_t)acc_match.size();
            ln[s][q] = lc[t] = id;
            acc_match.push_back((int32_t)i);
            if (dev) acc_rec.push_back(item_of[i]);
            else { acc_rec.push_back((int32_t)rec_host.size()); rec_host.push_back(o_host); }
        }
    }
    const int ntri = (int)acc_match.size();
    out->n_depth = out->n_triangulated = ntri;
    if (ntri && (size_t)next_lid + (size_t)ntri > (size_t)m->max_landmarks) {
        set_error("lmap triangulate_neighbours: new landmark ids beyond max_landmarks");
        return MCORB_E_CAP;
    }
    if (ntri > out->cap_depth) { set_error("lmap triangulate_neighbours: output too small"); return MCORB_E_CAP; }
    if (ntri && !out->depth_vec) return bad("bad argument");

    // ---- 6. the new landmarks into their slots, then the caller's arrays ----
    const MapOut *recs = dev ? m->h_mapout.get() : rec_host.data();
    if (dev && ntri) {
        hipStream_t st = m->st;
        TRY(m->h_mapput.grow((size_t)ntri, hipHostMallocDefault));
        TRY(m->d_mapput.grow((size_t)ntri));
        for (int k = 0; k < ntri; k++) m->h_mapput[k] = make_int2(acc_rec[k], next_lid + k);
        HIPCHK(hipMemcpyAsync(m->d_mapput, m->h_mapput, (size_t)ntri * sizeof(int2), hipMemcpyHostToDevice, st));
        launch_map_put(st, m->d_mapout, m->d_mapput, ntri, m->d_geom, m->d_nrays);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    } else {
        for (int k = 0; k < ntri; k++) {
            double *g = &m->geom[(size_t)(next_lid + k) * 6];
            memcpy(g, recs[acc_rec[k]].X, 3 * sizeof(double));
            memcpy(g + 3, recs[acc_rec[k]].normal, 3 * sizeof(double));
        }
    }
    for (int k = 0; k < ntri; k++) {
        m->flags[next_lid + k] |= kSet;
        m->n_rays[next_lid + k] = recs[acc_rec[k]].n_rays;
    }
    for (size_t i = 0; i < total; i++) {
        out->verdict[i] = verdict[i];
        out->inliers[i] = verdict[i] == kMapLandmark || verdict[i] == kMapParallax;
        out->new_lid[i] = -1;
        out->dist2[i] = dist2[i];
        out->cos_parallax[i] = cosp[i];
        for (int k = 0; k < 3; k++) out->pt3d[3 * i + k] = out->normal[3 * i + k] = 0.0;
    }
    for (int k = 0; k < ntri; k++) {
        const size_t i = (size_t)acc_match[k];
        const MapOut &o = recs[acc_rec[k]];
        out->new_lid[i] = next_lid + k;
        memcpy(out->pt3d + 3 * i, o.X, 3 * sizeof(double));
        memcpy(out->normal + 3 * i, o.normal, 3 * sizeof(double));
        out->depth_vec[k] = o.dist2;
    }
    if (cur->nfeat) memcpy(lids_cur, lc.data(), lc.size() * sizeof(int32_t));
    for (int s = 0; s < n_neigh; s++) {
        if (neigh[s].nfeat) memcpy(lids_neigh[s], ln[s].data(), ln[s].size() * sizeof(int32_t));
        out->neigh_skipped[s] = skipped[s];
    }
    out->next_lid = next_lid + ntri;
    return MCORB_OK;
}

int mcorb_lmap_depths(mcorb_lmap *m, const double Rcw[9], const double tcw[3], const int32_t *lids, int n, double *z)
{
    TRY(check_lmap(m, "lmap depths"));
    if (!Rcw || !tcw || n < 0 || (n && (!lids || !z))) { set_error("lmap depths: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    for (int i = 0; i < n; i++) {
        if (lids[i] < 0 || lids[i] >= m->max_landmarks) { set_error("lmap depths: landmark id outside the store"); return MCORB_E_ARG; }
        if (!(m->flags[lids[i]] & kHasPt)) { set_error("lmap depths: the slot was never set"); return MCORB_E_STATE; }
    }
    if (n == 0) return MCORB_OK;
    if (m->device < 0) {
        for (int i = 0; i < n; i++) z[i] = map_depth(Rcw, tcw, &m->geom[(size_t)lids[i] * 6]);
        return MCORB_OK;
    }
    HIPCHK(hipSetDevice(m->device));
    hipStream_t st = m->st;
    TRY(m->d_blids.grow((size_t)n));
    TRY(m->d_mapz.grow((size_t)n));
    HIPCHK(hipMemcpyAsync(m->d_blids, lids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    launch_map_depth(st, Rcw, tcw, m->d_geom, m->d_blids, n, m->d_mapz);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(z, m->d_mapz, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // (also covers the pageable arrays)
    return MCORB_OK;
}

int mcorb_lmap_last_triangulate_timing(mcorb_lmap *m, float us[2], int *n_launched, int *n_depth)
{
    TRY(check_lmap_handle(m, "lmap last_triangulate_timing"));
    if (!us) { set_error("lmap last_triangulate_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    us[0] = m->us_map_tri;
    us[1] = m->us_map_depth;
    if (n_launched) *n_launched = m->last_map_launched;
    if (n_depth) *n_depth = m->last_map_depth;
    return MCORB_OK;
}

int mcorb_host_map_gates(int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P, const double *K,
                         const double *centre, const float *kps, const int32_t *octave, const double *F, const float *inv_sigma2,
                         int nlevels, int32_t *verdict, int32_t *n_rays, double *vals)
{
    std::vector<int32_t> voff;
    TRY(check_gate_cases(X, nv1, nv, P, K, centre, kps, octave, F, inv_sigma2, nlevels, n, voff));
    if (!verdict || !n_rays || !vals) { set_error("map gates: bad argument"); return MCORB_E_ARG; }
    const MapGateCases c{X, nv1, nv, voff.data(), P, K, centre, kps, octave, F, inv_sigma2};
    std::vector<MapOut> o((size_t)n);
    for (int i = 0; i < n; i++) map_gate_case(c, i, o[i]);
    gates_out(o.data(), n, verdict, n_rays, vals);
    return MCORB_OK;
}

int mcorb_dev_map_gates_selftest(int device, int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P,
                                 const double *K, const double *centre, const float *kps, const int32_t *octave, const double *F,
                                 const float *inv_sigma2, int nlevels, int32_t *verdict, int32_t *n_rays, double *vals)
{
    std::vector<int32_t> voff;
    TRY(check_gate_cases(X, nv1, nv, P, K, centre, kps, octave, F, inv_sigma2, nlevels, n, voff));
    if (!verdict || !n_rays || !vals) { set_error("map gates: bad argument"); return MCORB_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { set_error("no usable HIP device"); return MCORB_E_NODEVICE; }
    HIPCHK(hipSetDevice(device));
    const size_t N = (size_t)n, V = (size_t)voff[n];
    DevBuf<double> d_X, d_P, d_K, d_c, d_F;
    DevBuf<int32_t> d_nv1, d_nv, d_voff, d_oct;
    DevBuf<float> d_kps, d_sig;
    DevBuf<MapOut> d_out;
    TRY(d_X.alloc(N * 3)); TRY(d_P.alloc(V * 12)); TRY(d_K.alloc(V * 9)); TRY(d_c.alloc(V * 3)); TRY(d_F.alloc(N * 9));
    TRY(d_nv1.alloc(N)); TRY(d_nv.alloc(N)); TRY(d_voff.alloc(N + 1)); TRY(d_oct.alloc(V));
    TRY(d_kps.alloc(V * 2)); TRY(d_sig.alloc((size_t)nlevels)); TRY(d_out.alloc(N));
    HIPCHK(hipMemcpy(d_X, X, N * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_P, P, V * 12 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_K, K, V * 9 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_c, centre, V * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_F, F, N * 9 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nv1, nv1, N * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nv, nv, N * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_voff, voff.data(), (N + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_oct, octave, V * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_kps, kps, V * 2 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_sig, inv_sigma2, (size_t)nlevels * sizeof(float), hipMemcpyHostToDevice));
    const MapGateCases c{d_X, d_nv1, d_nv, d_voff, d_P, d_K, d_c, d_kps, d_oct, d_F, d_sig};
    launch_map_gates(nullptr, c, n, d_out);
    HIPCHK(hipGetLastError());
    std::vector<MapOut> o(N);
    HIPCHK(hipMemcpy(o.data(), d_out, N * sizeof(MapOut), hipMemcpyDeviceToHost));
    gates_out(o.data(), n, verdict, n_rays, vals);
    return MCORB_OK;
}

int mcorb_lmap_triangulate_new(mcorb_lmap *m, const mcorb_map_frame *cur, int32_t *lids_cur, const mcorb_map_frame *prev, int32_t *lids_prev,
                               const int32_t *match_query, const int32_t *match_train, int n_matches, const double *K,
                               const float *inv_sigma2, int nlevels, int32_t next_lid, mcorb_map_new_out *out)
{
    g_who = "lmap triangulate_new";
    if (out) {
        out->n_matches = out->n_depth = out->n_triangulated = 0;
        out->next_lid = next_lid;
        out->avg_depth = 0.0;
        memset(out->n_rays_hist, 0, sizeof(out->n_rays_hist));
        memset(out->n_by_verdict, 0, sizeof(out->n_by_verdict));
    }
    TRY(check_lmap(m, "lmap triangulate_new"));
    if (!cur || !prev || !out || n_matches < 0 || !K || !inv_sigma2 || nlevels < 1 || next_lid < 0 || out->cap_matches < 0 ||
        out->cap_depth < 0 || (cur->nfeat && !lids_cur) || (prev->nfeat && !lids_prev) || (n_matches && (!match_query || !match_train)))
        return bad("bad argument");
    const int C = cur->ncams;
    if (C < 1 || C > MCORB_MAX_CAMS) return bad("1 .. MCORB_MAX_CAMS cameras");
    std::lock_guard<std::mutex> lk(m->mu);

    // ---- 1. everything that can be refused is refused before anything runs ----
    TRY(check_frame(*cur, C));
    TRY(check_frame(*prev, C));
    for (int i = 0; i < cur->nfeat; i++)
        if (lids_cur[i] < -1 || lids_cur[i] >= m->max_landmarks) return bad("landmark id outside the store");
    for (int i = 0; i < prev->nfeat; i++)
        if (lids_prev[i] < -1 || lids_prev[i] >= m->max_landmarks) return bad("landmark id outside the store");
    const size_t total = (size_t)n_matches;
    std::vector<uint8_t> nviews(total, 0), nviews_cur(total, 0);
    for (int j = 0; j < n_matches; j++) {
        const int q = match_query[j], t = match_train[j];
        if (q < 0 || q >= prev->nfeat || t < 0 || t >= cur->nfeat) return bad("match index outside a frame");
        const int v1 = views_of(*prev, q, nlevels), v2 = views_of(*cur, t, nlevels);
        if (v1 < 0 || v2 < 0) return bad("octave outside nlevels");
        if (v1 < 1 || v2 < 1) return bad("a matched feature without a view");
        if (v1 + v2 > MCORB_MAX_CAMS) return bad("a match of more than MCORB_MAX_CAMS views in total (the solver's design limit)");
        nviews[j] = (uint8_t)(v1 + v2);
        nviews_cur[j] = (uint8_t)v2;
    }
    out->n_matches = n_matches;
    if (n_matches > out->cap_matches) { set_error("lmap triangulate_new: output too small"); return MCORB_E_CAP; }
    if (total && (!out->inliers || !out->verdict || !out->new_lid || !out->pt3d || !out->normal || !out->dist || !out->cos_parallax ||
                  !out->iterations || !out->cost_initial || !out->cost_final))
        return bad("bad argument");

    // ---- 2. the matches whose current feature is free on entry, by view count: blocks of one wave, <= 4 views first ----
    const bool dev = m->device >= 0;
    std::vector<int32_t> item_of(total, -1);
    std::vector<MapItem> items;
    std::vector<MapBlock> blocks;
    int nblocks_small = 0;
    if (dev) {
        std::vector<int> order;
        for (int pass = 0; pass < 2; pass++) {   // 0: at most 4 views, 1: the rest
            order.clear();
            for (int j = 0; j < n_matches; j++) {
                if ((nviews[j] <= 4) != (pass == 0) || lids_cur[match_train[j]] != -1) continue;
                order.push_back(j);
            }
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nviews[a] < nviews[b]; });
            for (size_t k = 0; k < order.size(); k++) {
                if (k % kMapBlock == 0)
                    blocks.push_back(MapBlock{0, (int32_t)items.size(), (int32_t)std::min<size_t>(kMapBlock, order.size() - k)});
                const int j = order[k];
                item_of[j] = (int32_t)items.size();
                items.push_back(MapItem{match_query[j], match_train[j], (int32_t)items.size()});
            }
            if (pass == 0) nblocks_small = (int)blocks.size();
        }
    }
    const int nitems = (int)items.size();

    // ---- 3. the packed input: the current frame, then the previous keyframe ----
    Layout L;
    size_t nmi = ((size_t)cur->nfeat + (size_t)prev->nfeat) * C, nkp = 0;
    for (int c = 0; c < C; c++) nkp += (size_t)cur->nkps[c] + (size_t)prev->nkps[c];
    if (nmi > 0x7fffffff || nkp > 0x7fffffff) return bad("frames too large");
    L.frames = 0;
    L.F = align8(L.frames + 2 * sizeof(MapFrameDev));
    L.K = L.F;
    L.sig = L.K + (size_t)C * 9 * sizeof(double);
    L.mi = align8(L.sig + (size_t)nlevels * sizeof(float));
    L.kp = align8(L.mi + nmi * sizeof(int32_t));
    L.blocks = align8(L.kp + nkp * sizeof(MapKp));
    L.items = align8(L.blocks + blocks.size() * sizeof(MapBlock));
    L.zlids = L.total = align8(L.items + items.size() * sizeof(MapItem));
    std::vector<uint8_t> host_block;
    uint8_t *base;
    if (dev && nitems) {
        HIPCHK(hipSetDevice(m->device));
        TRY(m->h_mapin.grow(L.total, hipHostMallocDefault));
        TRY(m->d_mapin.grow(L.total));
        base = m->h_mapin;
    } else {
        host_block.resize(L.total);
        base = host_block.data();
    }
    {
        MapFrameDev *fr = (MapFrameDev *)(base + L.frames);
        size_t mi_at = 0, kp_at = 0;
        pack_frame(*cur, fr[0], (int32_t *)(base + L.mi), mi_at, (MapKp *)(base + L.kp), kp_at);
        pack_frame(*prev, fr[1], (int32_t *)(base + L.mi), mi_at, (MapKp *)(base + L.kp), kp_at);
        memcpy(base + L.K, K, (size_t)C * 9 * sizeof(double));
        memcpy(base + L.sig, inv_sigma2, (size_t)nlevels * sizeof(float));
        if (!blocks.empty()) memcpy(base + L.blocks, blocks.data(), blocks.size() * sizeof(MapBlock));
        if (!items.empty()) memcpy(base + L.items, items.data(), items.size() * sizeof(MapItem));
    }
    MapNewArgs na;
    for (int k = 0; k < 3; k++) { na.twc_cur[k] = cur->twc[k]; na.twc_prev[k] = prev->twc[k]; }

    // ---- 4. the records: one submission ----
    if (dev && nitems) {
        hipStream_t st = m->st;
        TRY(m->h_mapout.grow((size_t)nitems, hipHostMallocDefault));
        TRY(m->d_mapout.grow((size_t)nitems));
        TRY(m->h_mapextra.grow((size_t)nitems, hipHostMallocDefault));
        TRY(m->d_mapextra.grow((size_t)nitems));
        na.a = L.args(m->d_mapin, m->d_mapout, C);
        na.extra = m->d_mapextra;
        HIPCHK(hipMemcpyAsync(m->d_mapin, m->h_mapin, L.total, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(m->ev2, st));
        launch_map_refine_new(st, na, nblocks_small, (int)blocks.size() - nblocks_small);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(m->ev3, st));
        HIPCHK(hipMemcpyAsync(m->h_mapout, m->d_mapout, (size_t)nitems * sizeof(MapOut), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(m->h_mapextra, m->d_mapextra, (size_t)nitems * sizeof(MapNewExtra), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0.f;
        ev_elapsed(&ms, m->ev2, m->ev3);
        m->us_map_new = ms * 1000.f;
        m->last_map_new_launched = nitems;
    }

    // ---- 5. the walk (:6476-6491, :6673-6690): matches in order, only the current frame's id is tested ----
    std::vector<int32_t> lc(lids_cur, lids_cur + cur->nfeat), lp(lids_prev, lids_prev + prev->nfeat);
    std::vector<MapOut> rec(total);
    std::vector<MapNewExtra> ext(total);
    std::vector<int32_t> acc_match;
    int32_t by_verdict[9] = {0}, hist[MCORB_MAX_CAMS] = {0};
    double avg = 0.0;
    na.a = L.args(base, nullptr, C);
    for (int j = 0; j < n_matches; j++) {
        const int q = match_query[j], t = match_train[j];
        new_clear(rec[j], ext[j]);
        if (lc[t] != -1) { rec[j].verdict = kMapAssigned; by_verdict[kMapAssigned]++; continue; }
        if (dev) { rec[j] = m->h_mapout[item_of[j]]; ext[j] = m->h_mapextra[item_of[j]]; }
        else {
            na.a.out = &rec[j];
            na.extra = &ext[j];
            const MapItem it{q, t, 0};
            if (nviews[j] <= 4) map_new_item<false>(na, it); else map_new_item<true>(na, it);
        }
        by_verdict[rec[j].verdict]++;
        if (rec[j].verdict != kMapLandmark) continue;
        lp[q] = lc[t] = next_lid + (int32_t)acc_match.size();
        acc_match.push_back(j);
        avg += rec[j].dist2;
        hist[nviews_cur[j] - 1]++;
    }
    const int ntri = (int)acc_match.size();
    out->n_depth = out->n_triangulated = ntri;
    if (ntri && (size_t)next_lid + (size_t)ntri > (size_t)m->max_landmarks) {
        set_error("lmap triangulate_new: new landmark ids beyond max_landmarks");
        return MCORB_E_CAP;
    }
    if (ntri > out->cap_depth) { set_error("lmap triangulate_new: output too small"); return MCORB_E_CAP; }
    if (ntri && !out->depth_vec) return bad("bad argument");

    // ---- 6. the new landmarks into their slots, then the caller's arrays ----
    if (dev && ntri) {
        hipStream_t st = m->st;
        TRY(m->h_mapput.grow((size_t)ntri, hipHostMallocDefault));
        TRY(m->d_mapput.grow((size_t)ntri));
        for (int k = 0; k < ntri; k++) m->h_mapput[k] = make_int2(item_of[acc_match[k]], next_lid + k);
        HIPCHK(hipMemcpyAsync(m->d_mapput, m->h_mapput, (size_t)ntri * sizeof(int2), hipMemcpyHostToDevice, st));
        launch_map_put(st, m->d_mapout, m->d_mapput, ntri, m->d_geom, m->d_nrays);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    } else {
        for (int k = 0; k < ntri; k++) {
            double *g = &m->geom[(size_t)(next_lid + k) * 6];
            memcpy(g, rec[acc_match[k]].X, 3 * sizeof(double));
            memcpy(g + 3, rec[acc_match[k]].normal, 3 * sizeof(double));
        }
    }
    for (int k = 0; k < ntri; k++) {
        m->flags[next_lid + k] |= kSet;
        m->n_rays[next_lid + k] = rec[acc_match[k]].n_rays;
    }
    for (size_t i = 0; i < total; i++) {
        const MapOut &o = rec[i];
        const bool lm = o.verdict == kMapLandmark;
        out->verdict[i] = (uint8_t)o.verdict;
        out->inliers[i] = lm;
        out->new_lid[i] = -1;
        out->dist[i] = o.dist2;
        out->cos_parallax[i] = ext[i].cos;
        out->iterations[i] = ext[i].solves;
        out->cost_initial[i] = ext[i].cost_initial;
        out->cost_final[i] = ext[i].cost_final;
        for (int k = 0; k < 3; k++) { out->pt3d[3 * i + k] = lm ? o.X[k] : 0.0; out->normal[3 * i + k] = lm ? o.normal[k] : 0.0; }
    }
    for (int k = 0; k < ntri; k++) {
        out->new_lid[acc_match[k]] = next_lid + k;
        out->depth_vec[k] = rec[acc_match[k]].dist2;
    }
    out->avg_depth = avg;
    memcpy(out->n_rays_hist, hist, sizeof(hist));
    memcpy(out->n_by_verdict, by_verdict, sizeof(by_verdict));
    if (cur->nfeat) memcpy(lids_cur, lc.data(), lc.size() * sizeof(int32_t));
    if (prev->nfeat) memcpy(lids_prev, lp.data(), lp.size() * sizeof(int32_t));
    out->next_lid = next_lid + ntri;
    return MCORB_OK;
}

int mcorb_lmap_last_triangulate_new_timing(mcorb_lmap *m, float us[1], int *n_launched)
{
    TRY(check_lmap_handle(m, "lmap last_triangulate_new_timing"));
    if (!us) { set_error("lmap last_triangulate_new_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    us[0] = m->us_map_new;
    if (n_launched) *n_launched = m->last_map_new_launched;
    return MCORB_OK;
}

int mcorb_host_map_refine(int n, const double *X0, const int32_t *nv1, const int32_t *nv, const double *P, const double *K,
                          const double *centre, const float *kps, const int32_t *octave, const double *twc_cur, const double *twc_prev,
                          const float *inv_sigma2, int nlevels, int32_t *verdict, int32_t *n_rays, int32_t *solves, float *cosp,
                          double *vals)
{
    std::vector<int32_t> voff;
    TRY(check_gate_cases(X0, nv1, nv, P, K, centre, kps, octave, twc_cur, inv_sigma2, nlevels, n, voff));
    if (!twc_prev || !verdict || !n_rays || !solves || !cosp || !vals) { set_error("map refine: bad argument"); return MCORB_E_ARG; }
    const MapRefineCases c{X0, nv1, nv, voff.data(), P, K, centre, kps, octave, twc_cur, twc_prev, inv_sigma2};
    std::vector<MapOut> o((size_t)n);
    std::vector<MapNewExtra> e((size_t)n);
    for (int i = 0; i < n; i++) map_refine_case(c, i, o[i], e[i]);
    refine_out(o.data(), e.data(), n, verdict, n_rays, solves, cosp, vals);
    return MCORB_OK;
}

int mcorb_dev_map_refine_selftest(int device, int n, const double *X0, const int32_t *nv1, const int32_t *nv, const double *P,
                                  const double *K, const double *centre, const float *kps, const int32_t *octave, const double *twc_cur,
                                  const double *twc_prev, const float *inv_sigma2, int nlevels, int32_t *verdict, int32_t *n_rays,
                                  int32_t *solves, float *cosp, double *vals)
{
    std::vector<int32_t> voff;
    TRY(check_gate_cases(X0, nv1, nv, P, K, centre, kps, octave, twc_cur, inv_sigma2, nlevels, n, voff));
    if (!twc_prev || !verdict || !n_rays || !solves || !cosp || !vals) { set_error("map refine: bad argument"); return MCORB_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { set_error("no usable HIP device"); return MCORB_E_NODEVICE; }
    HIPCHK(hipSetDevice(device));
    const size_t N = (size_t)n, V = (size_t)voff[n];
    DevBuf<double> d_X, d_P, d_K, d_c, d_tc, d_tp;
    DevBuf<int32_t> d_nv1, d_nv, d_voff, d_oct;
    DevBuf<float> d_kps, d_sig;
    DevBuf<MapOut> d_out;
    DevBuf<MapNewExtra> d_ext;
    TRY(d_X.alloc(N * 3)); TRY(d_P.alloc(V * 12)); TRY(d_K.alloc(V * 9)); TRY(d_c.alloc(V * 3)); TRY(d_tc.alloc(N * 3)); TRY(d_tp.alloc(N * 3));
    TRY(d_nv1.alloc(N)); TRY(d_nv.alloc(N)); TRY(d_voff.alloc(N + 1)); TRY(d_oct.alloc(V));
    TRY(d_kps.alloc(V * 2)); TRY(d_sig.alloc((size_t)nlevels)); TRY(d_out.alloc(N)); TRY(d_ext.alloc(N));
    HIPCHK(hipMemcpy(d_X, X0, N * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_P, P, V * 12 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_K, K, V * 9 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_c, centre, V * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tc, twc_cur, N * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tp, twc_prev, N * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nv1, nv1, N * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nv, nv, N * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_voff, voff.data(), (N + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_oct, octave, V * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_kps, kps, V * 2 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_sig, inv_sigma2, (size_t)nlevels * sizeof(float), hipMemcpyHostToDevice));
    const MapRefineCases c{d_X, d_nv1, d_nv, d_voff, d_P, d_K, d_c, d_kps, d_oct, d_tc, d_tp, d_sig};
    launch_map_refine_cases(nullptr, c, n, d_out, d_ext);
    HIPCHK(hipGetLastError());
    std::vector<MapOut> o(N);
    std::vector<MapNewExtra> e(N);
    HIPCHK(hipMemcpy(o.data(), d_out, N * sizeof(MapOut), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(e.data(), d_ext, N * sizeof(MapNewExtra), hipMemcpyDeviceToHost));
    refine_out(o.data(), e.data(), n, verdict, n_rays, solves, cosp, vals);
    return MCORB_OK;
}

}  // extern "C"
