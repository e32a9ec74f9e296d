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

// Where a call packs its input, and the input packed (MapCall::pack): a device store's pinned block, reserved with the records
// (the call's items), the depths (nz) and, with `extra`, triangulate_new's second halves; a host vector otherwise
int map_block(mcorb_lmap *m, bool on_device, const MapCall &mc, const MapLayout &L, size_t nz, bool extra, const double *K,
              const float *inv_sigma2, std::vector<uint8_t> &host_block, uint8_t *&base)
{
    if (on_device) {
        HIPCHK(hipSetDevice(m->device));
        (void)hipGetLastError();   // (a stale error of this thread is not this call's)
        TRY(m->map.reserve(L.p.total, mc.w.items.size(), nz, extra));
        base = m->map.in.h;
    } else {
        host_block.resize(L.p.total);
        base = host_block.data();
    }
    mc.pack(base, L, K, inv_sigma2);
    return MCORB_OK;
}

// what both entries refuse once the walk has counted the new landmarks
template <class Out>
int check_new_ids(const MapCall &mc, int32_t next_lid, int ntri, Out *out)
{
    out->n_depth = out->n_triangulated = ntri;
    if (ntri && (size_t)next_lid + (size_t)ntri > (size_t)mc.max_landmarks) return mc.fail(MCORB_E_CAP, "new landmark ids beyond max_landmarks");
    if (ntri > out->cap_depth) return mc.fail(MCORB_E_CAP, "output too small");
    if (ntri && !out->depth_vec) return mc.bad("bad argument");
    return MCORB_OK;
}

// The new landmarks into slots next_lid .. next_lid + ntri: landmark k's record is recs[rec_of[k]] on the host; a device store
// copies point, normal and ray count from record item_of[k] of d_out device to device (k_map_put)
int put_landmarks(mcorb_lmap *m, bool on_device, int32_t next_lid, int ntri, const MapOut *recs, const int32_t *rec_of, const int32_t *item_of)
{
    if (on_device && ntri) {
        hipStream_t st = m->st;
        mcorb_lmap::Mapping &b = m->map;
        TRY(b.h_put.grow((size_t)ntri, hipHostMallocDefault));
        TRY(b.d_put.grow((size_t)ntri));
        for (int k = 0; k < ntri; k++) b.h_put[k] = make_int2(item_of[k], next_lid + k);
        Submission sub(st);
        sub.copy(b.d_put, b.h_put, (size_t)ntri * sizeof(int2), hipMemcpyHostToDevice);
        sub.run([&] { launch_map_put(st, b.d_out, b.d_put, ntri, m->d_geom, m->d_nrays); });
        TRY(sub.wait());
    } else {
        for (int k = 0; k < ntri; k++) {
            double *g = &m->geom[(size_t)(next_lid + k) * 6];
            memcpy(g, recs[rec_of[k]].X, 3 * sizeof(double));
            memcpy(g + 3, recs[rec_of[k]].normal, 3 * sizeof(double));
        }
    }
    for (int k = 0; k < ntri; k++) {
        m->flags[next_lid + k] |= kSet;
        m->n_rays[next_lid + k] = recs[rec_of[k]].n_rays;
    }
    return MCORB_OK;
}

double norm3(const double a[3], const double b[3])   // cv::norm(a - b)
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) { const double d = a[k] - b[k]; s += d * d; }
    return sqrt(s);
}

// what the four hooks refuse: check_cases with the gates' prefix (the refine hooks report theirs under it too); per: the hook's
// own array per case (F, twc_cur)
int check_gate_cases(MapCases &c, const double *per, int nlevels, int n, std::vector<int32_t> &voff)
{
    if (!per) { set_error("map gates: bad argument"); return MCORB_E_ARG; }
    return check_cases("map gates", c, nlevels, n, voff);
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
    const char *const who = "lmap triangulate_neighbours";
    if (out) { out->n_matches = out->n_depth = out->n_triangulated = 0; out->next_lid = next_lid; }
    TRY(check_lmap(m, who));
    MapCall mc{who, m->max_landmarks, cur ? cur->ncams : 0, nlevels};
    if (!cur || !out || n_neigh < 0 || !K || !inv_sigma2 || nlevels < 1 || !Rcw || !tcw || next_lid < 0 || out->cap_matches < 0 ||
        out->cap_depth < 0 || (cur->nfeat && !lids_cur) || (n_neigh && (!neigh || !lids_neigh || !F21 || !match_query || !match_train ||
        !n_matches || !out->neigh_skipped)))
        return mc.bad("bad argument");
    const int C = mc.C;
    if (C < 1 || C > MCORB_MAX_CAMS) return mc.bad("1 .. MCORB_MAX_CAMS cameras");
    std::lock_guard<std::mutex> lk(m->mu);

    // ---- 1. everything that can be refused is refused before anything runs ----
    TRY(mc.check_frame(*cur));
    TRY(mc.check_lids(*cur, lids_cur));
    mc.add(*cur);
    std::vector<size_t> moff((size_t)n_neigh + 1, 0);
    size_t nz = 0;
    for (int s = 0; s < n_neigh; s++) {
        const mcorb_map_frame &f = neigh[s];
        TRY(mc.check_frame(f));
        if (n_matches[s] < 0 || (n_matches[s] && (!match_query[s] || !match_train[s])) || !F21[s] || (f.nfeat && !lids_neigh[s]))
            return mc.bad("bad argument");
        moff[s + 1] = moff[s] + (size_t)n_matches[s];
        TRY(mc.check_lids(f, lids_neigh[s]));
        mc.add(f);
        for (int i = 0; i < f.nfeat; i++) {
            const int l = lids_neigh[s][i];
            if (l == -1) continue;
            if (!(m->flags[l] & kHasPt)) return mc.fail(MCORB_E_STATE, "a neighbour's landmark was never set");
            nz++;
        }
    }
    const size_t total = moff[n_neigh];
    // the views of every match: counted once, here
    std::vector<uint8_t> nviews(total, 0);
    for (int s = 0; s < n_neigh; s++)
        for (int j = 0; j < n_matches[s]; j++) {
            uint8_t nv_cur;
            TRY(mc.count_views(neigh[s], match_query[s][j], match_train[s][j], nviews[moff[s] + j], nv_cur));
        }
    out->n_matches = (int32_t)total;
    if (total > (size_t)out->cap_matches) return mc.fail(MCORB_E_CAP, "output too small");
    if (total && (!out->inliers || !out->verdict || !out->new_lid || !out->pt3d || !out->normal || !out->dist2 || !out->cos_parallax))
        return mc.bad("bad argument");

    // ---- 2. the matches that need a record: both features are free on entry ----
    const bool dev = m->device >= 0;
    MapWork &w = mc.w;
    w.item_of.assign(total, -1);
    if (dev)
        w.order(n_neigh, match_query, match_train, n_matches, moff.data(), nviews.data(),
                [&](int s, int j) { return lids_neigh[s][match_query[s][j]] == -1 && lids_cur[match_train[s][j]] == -1; });
    const std::vector<int32_t> &item_of = w.item_of;

    // ---- 3. the packed input: the current frame, the neighbours, their F tables and the landmarks whose depth is taken ----
    TRY(mc.fits());
    const MapLayout L = mc.layout((size_t)n_neigh * C * C * 9, nz);
    std::vector<uint8_t> host_block;
    uint8_t *base;
    TRY(map_block(m, dev, mc, L, nz, false, K, inv_sigma2, host_block, base));
    int32_t *zl = (int32_t *)(base + L.zlids);
    for (int s = 0; s < n_neigh; s++) {
        memcpy(base + L.F + (size_t)s * C * C * 9 * sizeof(double), F21[s], (size_t)C * C * 9 * sizeof(double));
        for (int i = 0; i < neigh[s].nfeat; i++)
            if (lids_neigh[s][i] != -1) *zl++ = lids_neigh[s][i];
    }

    // ---- 4. the depths of the neighbours' landmarks and the records: one submission ----
    std::vector<double> z_host;
    const double *z = nullptr;
    const int nitems = (int)w.items.size();
    if (dev) {
        hipStream_t st = m->st;
        mcorb_lmap::Mapping &b = m->map;
        // (nothing returns between the first launch and the wait, so no kernel of this call still reads the pinned input when
        // the caller has its error: Submission.  The upload is the chain's first piece: nothing is queued when it fails)
        Submission sub(st);
        b.in.upload(sub, L.p.total);
        sub.run(b.neigh, b.kDepth, [&] { launch_map_depth(st, Rcw, tcw, m->d_geom, b.in.dev<const int>(L.zlids), (int)nz, b.d_z); });
        sub.run(b.neigh, b.kTriangulate,
                [&] { launch_map_triangulate(st, L.args(b.in.d, b.d_out, C), w.nblocks_small, (int)w.blocks.size() - w.nblocks_small); });
        sub.mark(b.neigh, b.kTriangulate + 1);
        sub.copy(b.h_z, b.d_z, nz * sizeof(double), hipMemcpyDeviceToHost);
        sub.copy(b.h_out, b.d_out, (size_t)nitems * sizeof(MapOut), hipMemcpyDeviceToHost);
        TRY(sub.wait());
        b.neigh.read();
        z = b.h_z;
    } else {
        z_host.resize(nz);
        zl = (int32_t *)(base + L.zlids);
        for (size_t i = 0; i < nz; i++) z_host[i] = map_depth(Rcw, tcw, &m->geom[(size_t)zl[i] * 6]);
        z = z_host.data();
    }
    m->map.last_launched = nitems;
    m->map.last_depth = (int)nz;

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
            if (dev) o = &m->map.h_out[item_of[i]];
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
    TRY(check_new_ids(mc, next_lid, ntri, out));

    // ---- 6. the new landmarks into their slots, then the caller's arrays ----
    const MapOut *recs = dev ? m->map.h_out.get() : rec_host.data();
    TRY(put_landmarks(m, dev, next_lid, ntri, recs, acc_rec.data(), acc_rec.data()));
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
    (void)hipGetLastError();   // (a stale error of this thread is not this call's)
    hipStream_t st = m->st;
    TRY(m->map.d_z.grow((size_t)n));
    TRY(m->batch.reserve((size_t)n, false, false, false, false));
    Submission sub(st);   // (its wait also covers the pageable arrays)
    m->batch.upload(sub, m->batch.d_lids, lids, (size_t)n);
    sub.run([&] { launch_map_depth(st, Rcw, tcw, m->d_geom, m->batch.d_lids, n, m->map.d_z); });
    sub.copy(z, m->map.d_z, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    return sub.wait();
}

int mcorb_lmap_last_triangulate_timing(mcorb_lmap *m, float us[2], int *n_launched, int *n_depth)
{
    TRY(check_lmap_handle(m, "lmap last_triangulate_timing"));
    if (!us) { set_error("lmap last_triangulate_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    us[0] = m->map.neigh.us[mcorb_lmap::Mapping::kTriangulate];
    us[1] = m->map.neigh.us[mcorb_lmap::Mapping::kDepth];
    if (n_launched) *n_launched = m->map.last_launched;
    if (n_depth) *n_depth = m->map.last_depth;
    return MCORB_OK;
}

int mcorb_host_map_gates(int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P, const double *K,
                         const double *centre, const float *kps, const int32_t *octave, const double *F, const float *inv_sigma2,
                         int nlevels, int32_t *verdict, int32_t *n_rays, double *vals)
{
    MapCases h{X, nv1, nv, nullptr, P, K, centre, kps, octave, inv_sigma2};
    std::vector<int32_t> voff;
    TRY(check_gate_cases(h, F, nlevels, n, voff));
    if (!verdict || !n_rays || !vals) { set_error("map gates: bad argument"); return MCORB_E_ARG; }
    const MapGateCases c{h, F};
    std::vector<MapOut> o((size_t)n);
    for (int i = 0; i < n; i++) map_gate_case(c, i, o[i]);
    gates_out(o.data(), n, verdict, n_rays, vals);
    return MCORB_OK;
}

int mcorb_dev_map_gates_selftest(int device, int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P,
                                 const double *K, const double *centre, const float *kps, const int32_t *octave, const double *F,
                                 const float *inv_sigma2, int nlevels, int32_t *verdict, int32_t *n_rays, double *vals)
{
    MapCases h{X, nv1, nv, nullptr, P, K, centre, kps, octave, inv_sigma2};
    std::vector<int32_t> voff;
    TRY(check_gate_cases(h, F, nlevels, n, voff));
    if (!verdict || !n_rays || !vals) { set_error("map gates: bad argument"); return MCORB_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { set_error("no usable HIP device"); return MCORB_E_NODEVICE; }
    HIPCHK(hipSetDevice(device));
    const size_t N = (size_t)n;
    CasesDev d;
    DevBuf<double> d_F;
    DevBuf<MapOut> d_out;
    TRY(d.upload(n, h, nlevels));
    TRY(to_device(d_F, F, N * 9));
    TRY(d_out.alloc(N));
    const MapGateCases c{d.cases(), d_F};
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
    const char *const who = "lmap triangulate_new";
    if (out) {
        out->n_matches = out->n_depth = out->n_triangulated = 0;
        out->next_lid = next_lid;
        out->avg_depth = 0.0;
        memset(out->n_rays_hist, 0, sizeof(out->n_rays_hist));
        memset(out->n_by_verdict, 0, sizeof(out->n_by_verdict));
    }
    TRY(check_lmap(m, who));
    MapCall mc{who, m->max_landmarks, cur ? cur->ncams : 0, nlevels};
    if (!cur || !prev || !out || n_matches < 0 || !K || !inv_sigma2 || nlevels < 1 || next_lid < 0 || out->cap_matches < 0 ||
        out->cap_depth < 0 || (cur->nfeat && !lids_cur) || (prev->nfeat && !lids_prev) || (n_matches && (!match_query || !match_train)))
        return mc.bad("bad argument");
    const int C = mc.C;
    if (C < 1 || C > MCORB_MAX_CAMS) return mc.bad("1 .. MCORB_MAX_CAMS cameras");
    std::lock_guard<std::mutex> lk(m->mu);

    // ---- 1. everything that can be refused is refused before anything runs ----
    TRY(mc.check_frame(*cur));
    TRY(mc.check_frame(*prev));
    TRY(mc.check_lids(*cur, lids_cur));
    TRY(mc.check_lids(*prev, lids_prev));
    mc.add(*cur);
    mc.add(*prev);
    const size_t total = (size_t)n_matches;
    std::vector<uint8_t> nviews(total, 0), nviews_cur(total, 0);
    for (int j = 0; j < n_matches; j++) TRY(mc.count_views(*prev, match_query[j], match_train[j], nviews[j], nviews_cur[j]));
    out->n_matches = n_matches;
    if (n_matches > out->cap_matches) return mc.fail(MCORB_E_CAP, "output too small");
    if (total && (!out->inliers || !out->verdict || !out->new_lid || !out->pt3d || !out->normal || !out->dist || !out->cos_parallax ||
                  !out->iterations || !out->cost_initial || !out->cost_final))
        return mc.bad("bad argument");

    // ---- 2. the matches that need a record: the current feature is free on entry ----
    const bool dev = m->device >= 0;
    MapWork &w = mc.w;
    w.item_of.assign(total, -1);
    const size_t moff[2] = {0, total};
    if (dev) w.order(1, &match_query, &match_train, &n_matches, moff, nviews.data(), [&](int, int j) { return lids_cur[match_train[j]] == -1; });
    const std::vector<int32_t> &item_of = w.item_of;
    const int nitems = (int)w.items.size();

    // ---- 3. the packed input: the current frame, then the previous keyframe ----
    TRY(mc.fits());
    const MapLayout L = mc.layout(0, 0);
    std::vector<uint8_t> host_block;
    uint8_t *base;
    TRY(map_block(m, dev && nitems, mc, L, 0, true, K, inv_sigma2, host_block, base));
    MapNewArgs na;
    for (int k = 0; k < 3; k++) { na.twc_cur[k] = cur->twc[k]; na.twc_prev[k] = prev->twc[k]; }

    // ---- 4. the records: one submission ----
    if (dev && nitems) {
        hipStream_t st = m->st;
        mcorb_lmap::Mapping &b = m->map;
        na.a = L.args(b.in.d, b.d_out, C);
        na.extra = b.d_extra;
        Submission sub(st);   // (as in mcorb_lmap_triangulate_neighbours)
        b.in.upload(sub, L.p.total);
        sub.run(b.refine_new, 0, [&] { launch_map_refine_new(st, na, w.nblocks_small, (int)w.blocks.size() - w.nblocks_small); });
        sub.mark(b.refine_new, 1);
        sub.copy(b.h_out, b.d_out, (size_t)nitems * sizeof(MapOut), hipMemcpyDeviceToHost);
        sub.copy(b.h_extra, b.d_extra, (size_t)nitems * sizeof(MapNewExtra), hipMemcpyDeviceToHost);
        TRY(sub.wait());
        b.refine_new.read();
        b.last_new_launched = nitems;
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
        if (dev) { rec[j] = m->map.h_out[item_of[j]]; ext[j] = m->map.h_extra[item_of[j]]; }
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
    TRY(check_new_ids(mc, next_lid, ntri, out));

    // ---- 6. the new landmarks into their slots, then the caller's arrays ----
    std::vector<int32_t> acc_item((size_t)ntri);
    for (int k = 0; k < ntri; k++) acc_item[k] = item_of[acc_match[k]];
    TRY(put_landmarks(m, dev, next_lid, ntri, rec.data(), acc_match.data(), acc_item.data()));
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
    us[0] = m->map.refine_new.us[0];
    if (n_launched) *n_launched = m->map.last_new_launched;
    return MCORB_OK;
}

int mcorb_host_map_refine(int n, const double *X0, const int32_t *nv1, const int32_t *nv, const double *P, const double *K,
                          const double *centre, const float *kps, const int32_t *octave, const double *twc_cur, const double *twc_prev,
                          const float *inv_sigma2, int nlevels, int32_t *verdict, int32_t *n_rays, int32_t *solves, float *cosp,
                          double *vals)
{
    MapCases h{X0, nv1, nv, nullptr, P, K, centre, kps, octave, inv_sigma2};
    std::vector<int32_t> voff;
    TRY(check_gate_cases(h, twc_cur, nlevels, n, voff));
    if (!twc_prev || !verdict || !n_rays || !solves || !cosp || !vals) { set_error("map refine: bad argument"); return MCORB_E_ARG; }
    const MapRefineCases c{h, twc_cur, twc_prev};
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
    MapCases h{X0, nv1, nv, nullptr, P, K, centre, kps, octave, inv_sigma2};
    std::vector<int32_t> voff;
    TRY(check_gate_cases(h, twc_cur, nlevels, n, voff));
    if (!twc_prev || !verdict || !n_rays || !solves || !cosp || !vals) { set_error("map refine: bad argument"); return MCORB_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { set_error("no usable HIP device"); return MCORB_E_NODEVICE; }
    HIPCHK(hipSetDevice(device));
    const size_t N = (size_t)n;
    CasesDev d;
    DevBuf<double> d_tc, d_tp;
    DevBuf<MapOut> d_out;
    DevBuf<MapNewExtra> d_ext;
    TRY(d.upload(n, h, nlevels));
    TRY(to_device(d_tc, twc_cur, N * 3));
    TRY(to_device(d_tp, twc_prev, N * 3));
    TRY(d_out.alloc(N));
    TRY(d_ext.alloc(N));
    const MapRefineCases c{d.cases(), d_tc, d_tp};
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
