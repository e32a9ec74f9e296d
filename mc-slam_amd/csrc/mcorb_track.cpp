// mcorb_track.cpp -- fast tracking: what FrontEnd::startTrackingModule (MCSlam/src/FrontEnd.cpp:1570-1689) does on every frame
// between the map-entry query and refinePose.  Tracking::project_ (MCSlam/src/Tracking.cpp:208-260) projects the gathered
// landmarks into every camera of the rig from the predicted pose; Tracking::queryCurrentFrame / querryEachFrame (:319-449) match
// each projection against the frame's keypoints by image position -- the 10 nearest, a 100 px gate, the best Hamming distance
// below 20 -- and de-duplicate per keypoint, serially.  Not restated: Tracking::queryPoints, the JSON map, refinePose (OpenGV).
//
// The arithmetic is mcorb_track.h.  A device store runs the projection in k_track_project and the neighbour search with the
// descriptor gate in k_track_match, both in one submission: the candidates, keypoints and descriptors go up as one pinned block
// in one copy, the points and the landmarks' descriptors are read from the store's slots in HBM.  The host-only store runs the
// same header serially.  The candidate walk, the compaction in candidate order and the order-dependent de-duplication run on the
// host in both.  The reference's kd-tree search (FLANN, 4 trees, 64 checks) is approximate and un-vendored: the neighbours here
// are exact.  The store's landmarks are only read: of the map object the call writes its own scratch and, as mcorb_lmap_search
// does, the per-slot stamps of the candidate walk (tick / stamp), which no call reads as state.
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

int fail(int code, const char *what) { set_error(std::string("lmap track: ") + what); return code; }

// one query on the host: the MCORB_TRACK_KNN least keys (d2, k) among the keypoints inside the radius, kept in order by
// insertion, then the descriptor gate over them in that order
TrBest query_host(float x, float y, const float *kp_xy, const uint8_t *kp_desc, int n_kp, const uint8_t *lm_desc, double max_d2,
                  int max_hamming)
{
    TrKey top[MCORB_TRACK_KNN];
    int ntop = 0;
    for (int k = 0; k < n_kp; k++) {
        uint64_t d2;
        if (!tr_d2(x, y, kp_xy[2 * (size_t)k], kp_xy[2 * (size_t)k + 1], max_d2, d2)) continue;
        if (ntop == MCORB_TRACK_KNN && !tr_less(d2, (uint32_t)k, top[ntop - 1].d2, top[ntop - 1].k)) continue;
        int at = ntop < MCORB_TRACK_KNN ? ntop++ : ntop - 1;
        for (; at > 0 && tr_less(d2, (uint32_t)k, top[at - 1].d2, top[at - 1].k); at--) top[at] = top[at - 1];
        top[at] = TrKey{d2, (uint32_t)k};
    }
    uint32_t key = kTrNoGate;
    for (int r = 0; r < ntop; r++) {
        const uint32_t g = tr_gate_key(mcorb_hamming256(lm_desc, kp_desc + (size_t)top[r].k * 32), r, max_hamming);
        if (g < key) key = g;
    }
    if (key == kTrNoGate) return TrBest{-1, kTrBest0};
    return TrBest{(int32_t)top[key & 15u].k, (int32_t)(key >> 4)};
}

struct Triple { int32_t kp, lid, dist, cand; };

size_t round32(size_t n) { return (n + 31) & ~(size_t)31; }

}  // namespace

extern "C" {

int mcorb_lmap_track(mcorb_lmap *m, const mcorb_track_view *view, const mcorb_track_frame *frame, const int32_t *lids, int n_lids,
                     double max_d2, int max_hamming, mcorb_track_out *out)
{
    TRY(check_lmap(m, "lmap track"));
    if (!view || !frame || !out || n_lids < 0 || (n_lids && !lids) || max_hamming < 0) return fail(MCORB_E_ARG, "bad argument");
    const int C = view->ncams;
    if (C < 1 || C > MCORB_MAX_CAMS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_CAMS cameras");
    if (frame->ncams != C) return fail(MCORB_E_ARG, "the frame has another camera count than the view");
    size_t total_kp = 0;
    TrFrame tf;
    memset(&tf, 0, sizeof(tf));
    for (int c = 0; c < C; c++) {
        if (frame->n_kp[c] < 0) return fail(MCORB_E_ARG, "a negative keypoint count");
        if (frame->n_kp[c] && (!frame->kp_xy[c] || !frame->desc[c])) return fail(MCORB_E_ARG, "a camera's keypoints or descriptors are NULL");
        tf.n_kp[c] = frame->n_kp[c];
        tf.first[c] = (int32_t)total_kp;
        total_kp += (size_t)frame->n_kp[c];
        if (total_kp > 0x7fffffffu) return fail(MCORB_E_ARG, "too many keypoints");
    }
    const int cap_p = out->cap_proj, cap_m = out->cap_match;
    if (cap_p < 0 || cap_m < 0 || (cap_p && (!out->proj_lid || !out->proj_xy || !out->best_kp || !out->best_dist)) ||
        (cap_m && (!out->match_kp || !out->match_lid || !out->match_dist)))
        return fail(MCORB_E_ARG, "an output array is NULL");
    memset(out->n_proj, 0, sizeof(out->n_proj));
    memset(out->n_match, 0, sizeof(out->n_match));
    out->n_candidates = 0;
    std::lock_guard<std::mutex> lk(m->mu);

    // ---- 1. the candidates; everything that can be refused is refused before anything runs ----
    for (int i = 0; i < n_lids; i++)
        if (lids[i] < -1 || lids[i] >= m->max_landmarks) return fail(MCORB_E_ARG, "landmark id outside the store");
    const int t = next_tick(m);
    std::vector<int> cand;
    for (int i = 0; i < n_lids; i++) {
        const int l = lids[i];
        if (l == -1 || m->stamp[l] == t) continue;
        m->stamp[l] = t;
        cand.push_back(l);
    }
    const int nc = (int)cand.size();
    for (int l : cand) {
        if (!(m->flags[l] & kHasPt)) return fail(MCORB_E_STATE, "a candidate landmark has no point");
        if (!(m->flags[l] & kHasDesc)) return fail(MCORB_E_STATE, "a candidate landmark has no descriptor");
    }
    if (nc > m->max_candidates) return fail(MCORB_E_CAP, "more candidates than max_candidates");
    out->n_candidates = nc;
    if (nc == 0) return MCORB_OK;

    // ---- 2. per camera and candidate: the projection, whether it is kept, the query's result ----
    const size_t rows = (size_t)C * nc;
    const float2 *xy = nullptr;
    const uint8_t *valid = nullptr;
    const TrBest *best = nullptr;
    const double *pts = nullptr;   // [nc][3] on a device store
    std::vector<float2> hxy;
    std::vector<uint8_t> hvalid;
    std::vector<TrBest> hbest;
    if (m->device < 0) {
        hxy.assign(rows, make_float2(0.f, 0.f));
        hvalid.assign(rows, 0);
        hbest.assign(rows, TrBest{-1, kTrBest0});
        for (int i = 0; i < nc; i++) {
            double p0[3];
            tr_body(view->R0, view->t0, &m->geom[(size_t)cand[i] * 6], p0);
            if (!tr_in_front(*view, p0)) continue;
            for (int c = 0; c < C; c++) {
                const size_t at = (size_t)c * nc + i;
                float x = 0.f, y = 0.f;
                if (!tr_pixel(*view, c, p0, x, y)) continue;
                hxy[at] = make_float2(x, y);
                hvalid[at] = 1;
                hbest[at] = query_host(x, y, frame->kp_xy[c], frame->desc[c], frame->n_kp[c], &m->desc[(size_t)cand[i] * 32], max_d2,
                                       max_hamming);
            }
        }
        xy = hxy.data(); valid = hvalid.data(); best = hbest.data();
    } else {
        HIPCHK(hipSetDevice(m->device));
        hipStream_t st = m->st;
        const size_t off_xy = round32((size_t)nc * sizeof(int)), off_desc = off_xy + round32(total_kp * 8);
        const size_t bytes = off_desc + total_kp * 32;
        TRY(m->h_trackin.grow(bytes, hipHostMallocDefault));
        TRY(m->d_trackin.grow(bytes));
        TRY(m->d_trackxy.grow(rows));
        TRY(m->h_trackxy.grow(rows, hipHostMallocDefault));
        TRY(m->d_trackvalid.grow(rows));
        TRY(m->h_trackvalid.grow(rows, hipHostMallocDefault));
        TRY(m->d_trackbest.grow(rows));
        TRY(m->h_trackbest.grow(rows, hipHostMallocDefault));
        const bool want_pts = out->match_pt != nullptr;
        if (want_pts) {
            TRY(m->d_trackpt.grow((size_t)nc * 3));
            TRY(m->h_trackpt.grow((size_t)nc * 3, hipHostMallocDefault));
        }
        uint8_t *in = m->h_trackin;
        memcpy(in, cand.data(), (size_t)nc * sizeof(int));
        for (int c = 0; c < C; c++) {
            if (!frame->n_kp[c]) continue;
            memcpy(in + off_xy + (size_t)tf.first[c] * 8, frame->kp_xy[c], (size_t)frame->n_kp[c] * 8);
            memcpy(in + off_desc + (size_t)tf.first[c] * 32, frame->desc[c], (size_t)frame->n_kp[c] * 32);
        }
        HIPCHK(hipMemcpyAsync(m->d_trackin, m->h_trackin, bytes, hipMemcpyHostToDevice, st));
        const int *d_cand = reinterpret_cast<const int *>(m->d_trackin.get());
        HIPCHK(hipEventRecord(m->ev8, st));
        launch_track_project(st, *view, m->d_geom, d_cand, nc, m->d_trackxy, m->d_trackvalid, want_pts ? m->d_trackpt.get() : nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(m->ev9, st));
        launch_track_match(st, tf, C, reinterpret_cast<const float2 *>(m->d_trackin.get() + off_xy), m->d_trackin.get() + off_desc,
                           m->d_desc, d_cand, nc, m->d_trackxy, m->d_trackvalid, max_d2, max_hamming, m->d_trackbest);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(m->ev10, st));
        HIPCHK(hipMemcpyAsync(m->h_trackxy, m->d_trackxy, rows * sizeof(float2), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(m->h_trackvalid, m->d_trackvalid, rows, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(m->h_trackbest, m->d_trackbest, rows * sizeof(TrBest), hipMemcpyDeviceToHost, st));
        if (want_pts) HIPCHK(hipMemcpyAsync(m->h_trackpt, m->d_trackpt, (size_t)nc * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0.f;
        ev_elapsed(&ms, m->ev8, m->ev9);
        m->us_track_project = ms * 1000.f;
        ev_elapsed(&ms, m->ev9, m->ev10);
        m->us_track_match = ms * 1000.f;
        xy = m->h_trackxy; valid = m->h_trackvalid; best = m->h_trackbest;
        if (want_pts) pts = m->h_trackpt;
    }

    // ---- 3. the projected lists in candidate order, and the de-duplication (querryEachFrame:380-415), serial per camera ----
    std::vector<std::vector<Triple>> lists((size_t)C);
    bool is_short = false;
    for (int c = 0; c < C; c++) {
        const size_t row = (size_t)c * nc;
        int np = 0;
        for (int i = 0; i < nc; i++) np += valid[row + i] ? 1 : 0;
        out->n_proj[c] = np;
        std::vector<Triple> &list = lists[c];
        const float *kps = frame->kp_xy[c];
        for (int i = 0; i < nc; i++) {
            if (!valid[row + i] || best[row + i].kp < 0) continue;
            const TrBest b = best[row + i];
            const int px = (int)kps[2 * (size_t)b.kp], py = (int)kps[2 * (size_t)b.kp + 1];
            size_t at = 0;
            for (; at < list.size(); at++)
                if ((int)kps[2 * (size_t)list[at].kp] == px && (int)kps[2 * (size_t)list[at].kp + 1] == py) break;
            if (at < list.size()) {
                if (!(list[at].dist > b.dist)) continue;
                list.erase(list.begin() + (ptrdiff_t)at);
            }
            list.push_back(Triple{b.kp, cand[i], b.dist, i});
        }
        out->n_match[c] = (int32_t)list.size();
        if (np > cap_p || (int)list.size() > cap_m) is_short = true;
    }
    if (is_short) return fail(MCORB_E_CAP, "output too small");
    for (int c = 0; c < C; c++) {
        const size_t row = (size_t)c * nc, op = (size_t)c * cap_p, om = (size_t)c * cap_m;
        int at = 0;
        for (int i = 0; i < nc; i++) {
            if (!valid[row + i]) continue;
            out->proj_lid[op + at] = cand[i];
            out->proj_xy[2 * (op + at)] = xy[row + i].x;
            out->proj_xy[2 * (op + at) + 1] = xy[row + i].y;
            out->best_kp[op + at] = best[row + i].kp;
            out->best_dist[op + at] = best[row + i].dist;
            at++;
        }
        for (size_t k = 0; k < lists[c].size(); k++) {
            const Triple &tr = lists[c][k];
            out->match_kp[om + k] = tr.kp;
            out->match_lid[om + k] = tr.lid;
            out->match_dist[om + k] = tr.dist;
            if (out->match_pt)
                memcpy(out->match_pt + 3 * (om + k), pts ? pts + 3 * (size_t)tr.cand : &m->geom[(size_t)tr.lid * 6], 3 * sizeof(double));
        }
    }
    return MCORB_OK;
}

int mcorb_lmap_last_track_timing(mcorb_lmap *m, float us[2])
{
    TRY(check_lmap(m, "lmap last_track_timing"));
    if (!us) { set_error("lmap last_track_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    us[0] = m->us_track_project;
    us[1] = m->us_track_match;
    return MCORB_OK;
}

}  // extern "C"
