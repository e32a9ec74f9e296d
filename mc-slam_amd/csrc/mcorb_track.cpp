// mcorb_track.cpp -- fast tracking: what FrontEnd::startTrackingModule (MCSlam/src/FrontEnd.cpp:1570-1689) does on every frame
// between the map-entry query and refinePose.  Tracking::project_ (MCSlam/src/Tracking.cpp:208-260) projects the gathered
// landmarks into every camera of the rig from the predicted pose; Tracking::queryCurrentFrame / querryEachFrame (:319-449) match
// each projection against the frame's keypoints by image position -- the 10 nearest, a 100 px gate, the best Hamming distance
// below 20 -- and de-duplicate per keypoint, serially.  Not restated: Tracking::queryPoints, the JSON map, refinePose (OpenGV).
//
// The arithmetic is mcorb_track.h.  A device store runs the projection in k_track_project, the neighbour search with the
// descriptor gate in k_track_match and the compaction in candidate order in k_track_compact, all in one submission: the points
// and the landmarks' descriptors are read from the store's slots in HBM, the kept rows and the matches land in host-mapped
// memory, and the one synchronisation is all the host waits for.  The frame comes from host arrays (mcorb_lmap_track: candidates, keypoints and
// descriptors go up as one pinned block in one copy) or from a rig slot (mcorb_lmap_track_rig_frame: only the candidates go up;
// k_track_points rebuilds the keypoints from the slot's packed selection words, the descriptors are read where the extraction
// job left them).  The de-duplication, serial in the reference, is a minimum per pixel and a compaction in candidate order
// (mcorb_track.h, tr_dedup_value): k_track_dedup_min / _win / _emit run it behind k_track_match in the same submission, so the
// host's part of a device call is the candidate walk in front and copies behind.  The host-only store runs the same header
// serially and keeps the reference's list as it is.  All entries share the candidate checks, the submission and
// the output.  A call is a submission and a wait: mcorb_lmap_track_submit / _rig_frame_submit return once everything is on the
// store's stream, mcorb_lmap_track_wait synchronises and writes the outputs, and the synchronous entries are the two over the
// same body.  Every call is a call of nf frames, one but for mcorb_lmap_track_rig_frames, the slot entry for up to
// MCORB_TRACK_MAX_FRAMES frames of the slot's job in one submission and one wait: every frame's candidates, one TrItem per frame
// and the views go up in one copy and the kernels take the frame from the grid's z (submit_on_device, the one function that
// launches them); a pending call has a frame count and mcorb_lmap_track_frames_wait serves any.  The reference's kd-tree search (FLANN, 4 trees, 64 checks) is approximate and un-vendored: the neighbours here are
// exact.  The store's landmarks are only read: of the map object the call writes its own scratch and, as mcorb_lmap_search
// does, the per-slot stamps of the candidate walk (tick / stamp), which no call reads as state.
#include <string.h>

#include <chrono>
#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

using TK = mcorb_lmap::Tracking;

int fail(int code, const char *what) { set_error(std::string("lmap track: ") + what); return code; }

// a camera's keypoints on the host: records of `stride` bytes that begin with pt's two floats -- the caller's packed pairs
// (mcorb_lmap_track) or a rig slot's keypoint records (mcorb_lmap_track_rig_frame)
struct KpRows {
    const uint8_t *base[MCORB_MAX_CAMS];
    size_t stride;
    const float *pt(int c, int k) const { return reinterpret_cast<const float *>(base[c] + (size_t)k * stride); }
};

// a frame of a call.  Every entry: the keypoint count per camera and the host's keypoints.  desc: the host's descriptors, which
// the host-array entry uploads and a host-only store reads.  slot (the slot entry on a device store): where the kernels find the
// frame in HBM -- image img0 + c is camera c
struct Frame {
    int32_t n_kp[MCORB_MAX_CAMS];
    KpRows kp;
    const uint8_t *desc[MCORB_MAX_CAMS];
    Rig *rig = nullptr;
    Slot *slot = nullptr;
    int img0 = 0;
};

// the host phases of a call, for scripts/track_rate.py: compiled in with -DMCORB_TRACK_PROF only (mcorb_lmap_track_phases)
struct Phases {
#ifdef MCORB_TRACK_PROF
    float *us;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    Phases(mcorb_lmap *m, bool reset) : us(m->track.us_phase)   // a submission starts the call's phases over, its wait adds to them
    {
        if (reset)
            for (int k = 0; k < 5; k++) us[k] = 0.f;
    }
    void mark(int k)
    {
        const auto now = std::chrono::steady_clock::now();
        us[k] += std::chrono::duration<float, std::micro>(now - t).count();
        t = now;
    }
#else
    Phases(mcorb_lmap *, bool) {}
    void mark(int) {}
#endif
};

// one query on the host: the MCORB_TRACK_KNN least keys (d2, k) among the keypoints inside the radius, kept in order by
// insertion, then the descriptor gate over them in that order
TrBest query_host(float x, float y, const KpRows &kp, int c, const uint8_t *kp_desc, int n_kp, const uint8_t *lm_desc, double max_d2,
                  int max_hamming)
{
    TrKey top[MCORB_TRACK_KNN];
    int ntop = 0;
    for (int k = 0; k < n_kp; k++) {
        uint64_t d2;
        const float *p = kp.pt(c, k);
        if (!tr_d2(x, y, p[0], p[1], max_d2, d2)) continue;
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

void clear_counts(mcorb_track_out *out)
{
    memset(out->n_proj, 0, sizeof(out->n_proj));
    memset(out->n_match, 0, sizeof(out->n_match));
    out->n_candidates = 0;
}

// ---- 1. what the entries refuse before anything runs, the frame apart: the arguments, then -- the caller holds the store's
// lock -- the candidates ----
int check_out(const mcorb_track_out *out)
{
    const int cap_p = out->cap_proj, cap_m = out->cap_match;
    if (cap_p < 0 || cap_m < 0 || (cap_p && (!out->proj_lid || !out->proj_xy || !out->best_kp || !out->best_dist)) ||
        (cap_m && (!out->match_kp || !out->match_lid || !out->match_dist)))
        return fail(MCORB_E_ARG, "an output array is NULL");
    return MCORB_OK;
}

// out: the synchronous entries'; a submission has none (NULL)
int check_args(const mcorb_track_view *view, const int32_t *lids, int n_lids, int max_hamming, mcorb_track_out *out, bool with_out)
{
    if (!view || (with_out && !out) || n_lids < 0 || (n_lids && !lids) || max_hamming < 0) return fail(MCORB_E_ARG, "bad argument");
    if (out) clear_counts(out);
    if (view->ncams < 1 || view->ncams > MCORB_MAX_CAMS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_CAMS cameras");
    return out ? check_out(out) : MCORB_OK;
}

// appended to cand: a batch's frames follow each other there, each walked with a stamp value of its own
int candidates_of(mcorb_lmap *m, const int32_t *lids, int n_lids, std::vector<int> &cand)
{
    const size_t from = cand.size();
    for (int i = 0; i < n_lids; i++)
        if (lids[i] < -1 || lids[i] >= m->max_landmarks) return fail(MCORB_E_ARG, "landmark id outside the store");
    const int t = next_tick(m);
    for (int i = 0; i < n_lids; i++) {
        const int l = lids[i];
        if (l == -1 || m->stamp[l] == t) continue;
        m->stamp[l] = t;
        cand.push_back(l);
    }
    for (size_t i = from; i < cand.size(); i++) {
        const int l = cand[i];
        if (!(m->flags[l] & kHasPt)) return fail(MCORB_E_STATE, "a candidate landmark has no point");
        if (!(m->flags[l] & kHasDesc)) return fail(MCORB_E_STATE, "a candidate landmark has no descriptor");
    }
    if (cand.size() - from > (size_t)m->max_candidates) return fail(MCORB_E_CAP, "more candidates than max_candidates");
    return MCORB_OK;
}

// ---- 2. per camera the kept candidates in candidate order -- the projection and the query's result -- and the de-duplicated
// matches ----
// a host-only store: mcorb_track.h serially
// (cand, rows: the frame's nc candidates and its block of C * nc rows)
void rows_on_host(const mcorb_lmap *m, const mcorb_track_view &view, const Frame &f, const int *cand, int nc, double max_d2,
                  int max_hamming, TrRow *rows, int32_t *n_proj)
{
    const int C = view.ncams;
    for (int c = 0; c < C; c++) n_proj[c] = 0;
    for (int i = 0; i < nc; i++) {
        double p0[3];
        tr_body(view.R0, view.t0, &m->geom[(size_t)cand[i] * 6], p0);
        if (!tr_in_front(view, p0)) continue;
        for (int c = 0; c < C; c++) {
            float x = 0.f, y = 0.f;
            if (!tr_pixel(view, c, p0, x, y)) continue;
            const TrBest b = query_host(x, y, f.kp, c, f.desc[c], f.n_kp[c], &m->desc[(size_t)cand[i] * 32], max_d2, max_hamming);
            rows[(size_t)c * nc + n_proj[c]++] = TrRow{i, x, y, b.kp, b.dist};
        }
    }
}

// the de-duplication (querryEachFrame:380-415) of a host-only store: the reference's list as it is, serial per camera over the rows
// with a match -> matches[c * nc + 0 .. n_match[c]).  What the search compares, the pixel of the entry's keypoint, is kept beside
// the list as one 64-bit key per entry: the scan reads 8 bytes an entry and stays in the first-level cache
void dedup_on_host(int C, int nc, const TrRow *rows, const int32_t *n_proj, const KpRows &kp, TrMatch *matches, int32_t *n_match)
{
    std::vector<TrMatch> list;
    std::vector<uint64_t> keys;   // of the camera's list, entry by entry
    for (int c = 0; c < C; c++) {
        const TrRow *row = rows + (size_t)c * nc;
        list.clear();
        keys.clear();
        for (int r = 0; r < n_proj[c]; r++) {
            if (row[r].kp < 0) continue;
            const TrRow &b = row[r];
            const float *p = kp.pt(c, b.kp);
            const uint64_t key = tr_pixel_key(p[0], p[1]);
            size_t at = 0;
            for (const size_t n = keys.size(); at < n && keys[at] != key; at++) {}
            if (at < list.size()) {
                if (!(list[at].dist > b.dist)) continue;
                list.erase(list.begin() + (ptrdiff_t)at);
                keys.erase(keys.begin() + (ptrdiff_t)at);
            }
            list.push_back(TrMatch{b.i, b.kp, b.dist});
            keys.push_back(key);
        }
        n_match[c] = (int32_t)list.size();
        std::copy(list.begin(), list.end(), matches + (size_t)c * nc);
    }
}

// The sel / nsel of the slot's last extraction as a kernel may read them: the job's own view (Slot::ctl, as launch_undistort is
// given it) -- but a later match job points ctl at the device mirror, which a small host-selected batch never filled: that
// batch's words are in the host-mapped block
void slot_sel(const Slot &s, const uint32_t *&sel, const int *&nsel)
{
    const bool host_sel = s.host_results && !s.rig->gpu_select;
    sel = host_sel ? s.hc.sel : s.ctl.sel;
    nsel = host_sel ? s.hc.nsel : s.ctl.nsel;
}

// a device store: the nf frames of a call in one submission on the store's stream -- one pinned block up in one copy (a TrItem
// and a view per frame, the frames' candidates back to back and, host arrays only, the frame), then [k_track_points,]
// k_track_project, k_track_match, k_track_compact, the tables' clear and the three kernels of the de-duplication, each once for all
// frames (the frame is the grid's z), no host step between them.  Frame f's block of every per-pair array begins at C * first[f]
// and is laid out [c * n + i] inside; its de-duplication tables have their own size and follow the frames' before it.  Once the
// stream has run them the rows, the matches and their counts are in host-mapped memory; the gathered points (want_pts) come down
// in the one result copy there is.  Nothing of the caller's is read after this returns: the arrays are in the pinned block
int submit_on_device(mcorb_lmap *m, const mcorb_track_view *views, const Frame *fr, int nf, const mcorb_lmap::TrackCall &tc, double max_d2,
                     int max_hamming, bool want_pts)
{
    const int C = tc.ncams;
    const size_t total = tc.first[nf], rows = (size_t)C * total;
    Slot *slot = fr[0].slot;   // (a call's frames are all a rig slot's or all host arrays)
    const int kcap = slot ? fr[0].rig->geom.kcap : 0;
    // (a stale error of this thread is not this call's, as in Rig::execute: whatever an earlier, unrelated HIP call left behind --
    // another object's destructor, an elapsed-time query -- would otherwise be reported by the checks behind the launches)
    TRY(use_device(m->device));
    hipStream_t st = m->st;
    size_t slots = 0, total_kp = 0;   // (total_kp: of host arrays, which go up)
    int max_n = 0;
    for (int f = 0; f < nf; f++) {
        const int n = (int)(tc.first[f + 1] - tc.first[f]);
        slots += (size_t)C << tr_dedup_log2(n);
        max_n = std::max(max_n, n);
        for (int c = 0; c < C && !slot; c++) total_kp += (size_t)fr[f].n_kp[c];
    }
    const TrackLayout L((size_t)nf, total, total_kp);
    TK &t = m->track;
    TRY(t.reserve(L.p.total, rows, (size_t)nf, slots, slot ? (size_t)nf * C * kcap : 0, want_pts ? total : 0));
    if (t.refine) TRY(m->pose.t.reserve_track((size_t)nf, rows));
    TrItem *items = t.in.host<TrItem>(L.items);
    size_t tab = 0, kp = 0;
    for (int f = 0; f < nf; f++) {
        TrItem &it = items[f];
        memset(&it, 0, sizeof(it));
        it.view = f;
        it.n = (int32_t)(tc.first[f + 1] - tc.first[f]);
        it.log2p = tr_dedup_log2(it.n);
        it.img0 = fr[f].img0;
        it.cand_first = tc.first[f];
        it.rows = (size_t)C * tc.first[f];
        it.tab = tab;
        it.kp0 = slot ? (size_t)f * C * kcap : 0;
        it.desc0 = slot ? (size_t)it.img0 * kcap : 0;
        for (int c = 0; c < C; c++) {
            const int32_t n_kp = it.frame.n_kp[c] = fr[f].n_kp[c];
            it.frame.first[c] = slot ? c * kcap : (int32_t)kp;
            if (!slot && n_kp) {
                memcpy(t.in.host<uint8_t>(L.xy) + kp * 8, fr[f].kp.base[c], (size_t)n_kp * 8);
                memcpy(t.in.host<uint8_t>(L.desc) + kp * 32, fr[f].desc[c], (size_t)n_kp * 32);
                kp += (size_t)n_kp;
            }
        }
        tab += (size_t)C << it.log2p;
        if (!it.n)   // no workgroup runs for this frame
            for (int c = 0; c < MCORB_MAX_CAMS; c++)
                t.h_nproj.get()[(size_t)f * MCORB_MAX_CAMS + c] = t.h_nmatch.get()[(size_t)f * MCORB_MAX_CAMS + c] = 0;
    }
    memcpy(t.in.host<mcorb_track_view>(L.views), views, (size_t)nf * sizeof(mcorb_track_view));
    memcpy(t.in.host<int>(L.cand), tc.cand.data(), total * sizeof(int));
    Submission sub(st);   // (from here on nothing returns before a wait: this one's after a failed piece, wait_body's otherwise)
    t.in.upload(sub, L.p.total);
    const TrItem *d_items = t.in.dev<const TrItem>(L.items);
    const mcorb_track_view *d_views = t.in.dev<const mcorb_track_view>(L.views);
    const int *d_cand = t.in.dev<const int>(L.cand);
    const float2 *kp_xy = t.in.dev<const float2>(L.xy);
    const uint8_t *kp_desc = t.in.dev<const uint8_t>(L.desc);
    if (slot) {
        const uint32_t *sel;
        const int *nsel;
        slot_sel(*slot, sel, nsel);
        sub.run(t.chain, TK::kPoints,
                [&] { launch_track_points(st, d_items, nf, max_n, sel, nsel, kcap, C, fr[0].rig->tab.scale, fr[0].rig->tab.nlevels, t.d_kp); });
        kp_xy = t.d_kp;
        kp_desc = slot->d_desc.get();
    }
    sub.run(t.chain, TK::kProject, [&] {
        launch_track_project(st, d_items, nf, max_n, d_views, m->d_geom, d_cand, t.d_xy, t.d_valid, want_pts ? t.d_pt.get() : nullptr);
    });
    sub.run(t.chain, TK::kMatch, [&] {
        launch_track_match(st, d_items, nf, max_n, C, kp_xy, kp_desc, m->d_desc, d_cand, t.d_xy, t.d_valid, max_d2, max_hamming, t.d_best);
    });
    sub.run(t.chain, TK::kCompact, [&] { launch_track_compact(st, d_items, nf, max_n, C, t.d_valid, t.d_xy, t.d_best, t.h_rows, t.h_nproj); });
    sub.mark(t.chain, TK::kDedup);
    sub.fill(t.d_owner, 0xff, slots * sizeof(uint32_t));
    sub.fill(t.d_val, 0xff, slots * sizeof(unsigned long long));
    sub.run([&] {
        launch_track_dedup(st, d_items, nf, max_n, C, kp_xy, t.d_valid, t.d_best, t.d_owner, t.d_val, t.d_slot, t.d_win, t.h_match, t.h_nmatch);
    });
    sub.mark(t.chain, TK::kDedup + 1);
    // (mcorb_lmap_set_track_refine: the pose from each frame's matches, one workgroup of k_pose_refine per frame, in the same submission)
    if (t.refine) pose_track_submit(sub, m, views, items, nf, kp_xy, d_cand);
    if (want_pts) sub.copy(t.h_pt, t.d_pt, total * 3 * sizeof(double), hipMemcpyDeviceToHost);
    return sub.failed() ? sub.wait() : MCORB_OK;
}

// ---- 3. a call's two halves, the frames checked; the caller holds the store's lock ----
// the state of a call of nf frames whose candidates (cand, first) are in place: nothing launched, every count zero
void begin_call(mcorb_lmap *m, int C, int nf, bool want_pts)
{
    mcorb_lmap::TrackCall &tc = m->track.call;
    tc.ncams = C;
    tc.nf = nf;
    tc.launched = tc.points = false;
    tc.want_pts = want_pts;
    tc.n_proj.assign((size_t)nf * MCORB_MAX_CAMS, 0);
    tc.n_match.assign((size_t)nf * MCORB_MAX_CAMS, 0);
    tc.refine = m->track.refine;
    m->track.pose_nf = 0;
    if (tc.refine) {
        tc.pose.assign((size_t)nf, mcorb_pose_result{});
        tc.pose_flags.assign((size_t)C * tc.cand.size(), 0);
    }
}

// everything up to and excluding the synchronisation: the candidates of every frame (frame f's ids are lids[lid_first[f] ..
// lid_first[f + 1])), one stamp value each, then the whole call frame by frame on a host-only store -- and when no frame has a
// candidate, which leaves the stream untouched --, the one submission on a device store.  A refusal leaves nothing behind: a
// submission with a failed piece waits for what it had queued (Submission).  outs: the synchronous entries'
int submit_body(mcorb_lmap *m, const mcorb_track_view *views, const Frame *fr, int nf, const int32_t *lids, const int32_t *lid_first,
                double max_d2, int max_hamming, bool want_pts, mcorb_track_out *outs)
{
    Phases ph(m, true);
    mcorb_lmap::TrackCall &tc = m->track.call;
    const int C = views[0].ncams;
    tc.cand.clear();
    tc.first.assign(1, 0);
    for (int f = 0; f < nf; f++) {
        TRY(candidates_of(m, lids + lid_first[f], lid_first[f + 1] - lid_first[f], tc.cand));
        tc.first.push_back(tc.cand.size());
    }
    if (outs)   // (set from here on, whatever follows)
        for (int f = 0; f < nf; f++) outs[f].n_candidates = (int)(tc.first[f + 1] - tc.first[f]);
    ph.mark(0);
    const size_t total = tc.cand.size();
    begin_call(m, C, nf, want_pts);
    if (!total || m->device < 0) {
        tc.rows.resize((size_t)C * total);
        tc.matches.resize((size_t)C * total);
        for (int f = 0; f < nf; f++) {
            const int nc = (int)(tc.first[f + 1] - tc.first[f]);
            TrMatch *matches = tc.matches.data() + (size_t)C * tc.first[f];
            int32_t *n_match = tc.n_match.data() + (size_t)f * MCORB_MAX_CAMS;
            if (nc) {
                TrRow *rows = tc.rows.data() + (size_t)C * tc.first[f];
                int32_t *n_proj = tc.n_proj.data() + (size_t)f * MCORB_MAX_CAMS;
                rows_on_host(m, views[f], fr[f], tc.cand.data() + tc.first[f], nc, max_d2, max_hamming, rows, n_proj);
                ph.mark(2);
                dedup_on_host(C, nc, rows, n_proj, fr[f].kp, matches, n_match);
                ph.mark(3);
            }
            if (tc.refine)
                pose_track_host(m, views[f], tc.cand.data() + tc.first[f], nc, matches, n_match, fr[f].kp.base, fr[f].kp.stride, tc.pose[f],
                                tc.pose_flags.data() + (size_t)C * tc.first[f]);
        }
        m->track.pose_nf = tc.refine ? nf : 0;
        return MCORB_OK;
    }
    TRY(submit_on_device(m, views, fr, nf, tc, max_d2, max_hamming, want_pts));
    tc.launched = true;
    tc.points = fr[0].slot != nullptr;
    m->track.pose_nf = tc.refine ? nf : 0;
    ph.mark(1);
    return MCORB_OK;
}

// the synchronisation, the event times and the outputs of the pending call's frames: per camera the projected lists as the rows have
// them and the matches, lid = cand[i].  pts: [nc][3] of a device store.  checked: outs are a synchronous entry's, which the
// argument checks have seen and cleared.  single: mcorb_lmap_track_wait, which serves no batch of more than one frame
int wait_body(mcorb_lmap *m, mcorb_track_out *outs, int n_outs, bool checked, bool single)
{
    Phases ph(m, false);
    const mcorb_lmap::TrackCall &tc = m->track.call;
    const int C = tc.ncams, nf = tc.nf;
    const TrRow *rows = tc.rows.data();
    const TrMatch *matches = tc.matches.data();
    const int32_t *n_proj = tc.n_proj.data(), *n_match = tc.n_match.data();
    const double *pts = nullptr;
    if (tc.launched) {
        HIPCHK(hipSetDevice(m->device));
        HIPCHK(hipStreamSynchronize(m->st));
        ph.mark(2);
        m->track.chain.read(tc.points ? TK::kPoints : TK::kProject);
        rows = m->track.h_rows;
        matches = m->track.h_match;
        n_proj = m->track.h_nproj;
        n_match = m->track.h_nmatch;
        if (tc.want_pts) pts = m->track.h_pt;
    }
    ph.mark(3);
    if (!checked) {
        if (!outs || n_outs < 1) return fail(MCORB_E_ARG, "bad argument");
        for (int f = 0; f < n_outs; f++) clear_counts(&outs[f]);
        if (single && nf != 1) return fail(MCORB_E_STATE, "the pending call is a batch: mcorb_lmap_track_frames_wait serves it");
        if (n_outs != nf) return fail(MCORB_E_ARG, "n_outs is not the pending call's frame count");
        for (int f = 0; f < nf; f++) TRY(check_out(&outs[f]));
    }
    for (int f = 0; f < nf; f++)
        if (outs[f].match_pt && !tc.want_pts) return fail(MCORB_E_ARG, "match_pt of a call that was submitted without want_pts");
    // every count of every frame, then -- unless one is short -- the arrays
    bool is_short = false;
    for (int f = 0; f < nf; f++) {
        mcorb_track_out *out = &outs[f];
        const int nc = (int)(tc.first[f + 1] - tc.first[f]);
        out->n_candidates = nc;
        if (!nc) continue;
        for (int c = 0; c < C; c++) {
            const int np = n_proj[f * MCORB_MAX_CAMS + c], nm = n_match[f * MCORB_MAX_CAMS + c];
            out->n_proj[c] = np;
            out->n_match[c] = nm;
            if (np > out->cap_proj || nm > out->cap_match) is_short = true;
        }
    }
    if (is_short) return fail(MCORB_E_CAP, "output too small");
    for (int f = 0; f < nf; f++) {
        mcorb_track_out *out = &outs[f];
        const int nc = (int)(tc.first[f + 1] - tc.first[f]);
        const int *cand = tc.cand.data() + tc.first[f];
        const size_t base = (size_t)C * tc.first[f];
        const double *fpts = pts ? pts + 3 * tc.first[f] : nullptr;
        const int cap_p = out->cap_proj, cap_m = out->cap_match;
        for (int c = 0; c < C && nc; c++) {
            const TrRow *row = rows + base + (size_t)c * nc;
            const TrMatch *mt = matches + base + (size_t)c * nc;
            const size_t op = (size_t)c * cap_p, om = (size_t)c * cap_m;
            for (int r = 0; r < out->n_proj[c]; r++) {
                out->proj_lid[op + r] = cand[row[r].i];
                out->proj_xy[2 * (op + r)] = row[r].x;
                out->proj_xy[2 * (op + r) + 1] = row[r].y;
                out->best_kp[op + r] = row[r].kp;
                out->best_dist[op + r] = row[r].dist;
            }
            for (int k = 0; k < out->n_match[c]; k++) {
                const int lid = cand[mt[k].i];
                out->match_kp[om + k] = mt[k].kp;
                out->match_lid[om + k] = lid;
                out->match_dist[om + k] = mt[k].dist;
                if (out->match_pt)
                    memcpy(out->match_pt + 3 * (om + k), fpts ? fpts + 3 * (size_t)mt[k].i : &m->geom[(size_t)lid * 6], 3 * sizeof(double));
            }
        }
    }
    ph.mark(4);
    return MCORB_OK;
}

// a call of nf checked frames from the lock on.  outs: the synchronous entries', nf of them, which wait at once; NULL: the call
// stays pending.  After a failure every count of every outs[f] is zero
int track(mcorb_lmap *m, const mcorb_track_view *views, const Frame *fr, int nf, const int32_t *lids, const int32_t *lid_first, double max_d2,
          int max_hamming, bool want_pts, mcorb_track_out *outs)
{
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track.pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");
    const int rc = submit_body(m, views, fr, nf, lids, lid_first, max_d2, max_hamming, want_pts, outs);
    if (rc != MCORB_OK) {
        for (int f = 0; f < nf && outs; f++) clear_counts(&outs[f]);
        return rc;
    }
    if (outs) return wait_body(m, outs, nf, true, false);
    m->track.pending.store(true);
    return MCORB_OK;
}

// the frame of the host-array entries
int frame_of_arrays(const mcorb_track_view *view, const mcorb_track_frame *frame, Frame &f)
{
    const int C = view->ncams;
    if (frame->ncams != C) return fail(MCORB_E_ARG, "the frame has another camera count than the view");
    f.kp.stride = 2 * sizeof(float);
    size_t total_kp = 0;
    for (int c = 0; c < C; c++) {
        if (frame->n_kp[c] < 0) return fail(MCORB_E_ARG, "a negative keypoint count");
        if (frame->n_kp[c] && (!frame->kp_xy[c] || !frame->desc[c])) return fail(MCORB_E_ARG, "a camera's keypoints or descriptors are NULL");
        f.n_kp[c] = frame->n_kp[c];
        f.kp.base[c] = reinterpret_cast<const uint8_t *>(frame->kp_xy[c]);
        f.desc[c] = frame->desc[c];
        total_kp += (size_t)frame->n_kp[c];
        if (total_kp > 0x7fffffffu) return fail(MCORB_E_ARG, "too many keypoints");
    }
    return MCORB_OK;
}

// the frame of the slot entries: the slot is idle and its last job extracted the frame
int frame_of_slot(const mcorb_lmap *m, const mcorb_track_view *view, mcorb_rig *r, int slot, int frame, Frame &f)
{
    if (!r || slot < 0 || slot >= (int)r->rig.slots.size()) return fail(MCORB_E_ARG, "no such rig slot");
    Rig &R = r->rig;
    const int C = view->ncams;
    if (R.ncams != C) return fail(MCORB_E_ARG, "the rig has another camera count than the view");
    if (m->device >= 0 && m->device != R.device) return fail(MCORB_E_ARG, "the rig lives on another device");
    Slot *s = R.slots[slot].get();
    {
        std::lock_guard<std::mutex> lk(s->m);
        if (s->busy) return fail(MCORB_E_STATE, "slot busy");
    }
    if (frame < 0 || ((long long)frame + 1) * C > s->nimg_done) return fail(MCORB_E_STATE, "frame not extracted by the slot's last job");
    f.kp.stride = sizeof(mcorb_keypoint);
    f.rig = &R;
    f.slot = m->device >= 0 ? s : nullptr;
    f.img0 = frame * C;
    for (int c = 0; c < C; c++) {
        const std::vector<mcorb_keypoint> &K = s->kps[(size_t)f.img0 + c];
        f.n_kp[c] = (int32_t)std::min(K.size(), (size_t)R.geom.kcap);
        f.kp.base[c] = reinterpret_cast<const uint8_t *>(K.data());
        f.desc[c] = s->h_desc + ((size_t)f.img0 + c) * R.geom.kcap * 32;
    }
    return MCORB_OK;
}

// the three entries, synchronous (out) or a submission (out == NULL): their own argument checks, then track()
int track_arrays(mcorb_lmap *m, const mcorb_track_view *view, const mcorb_track_frame *frame, const int32_t *lids, int n_lids,
                 double max_d2, int max_hamming, bool want_pts, mcorb_track_out *out, bool with_out)
{
    TRY(check_lmap(m, "lmap track"));
    if (!frame) return fail(MCORB_E_ARG, "bad argument");
    TRY(check_args(view, lids, n_lids, max_hamming, out, with_out));
    Frame f;
    TRY(frame_of_arrays(view, frame, f));
    const int32_t lid_first[2] = {0, n_lids};
    return track(m, view, &f, 1, lids, lid_first, max_d2, max_hamming, want_pts, out);
}

int track_slot(mcorb_lmap *m, const mcorb_track_view *view, mcorb_rig *r, int slot, int frame, const int32_t *lids, int n_lids,
               double max_d2, int max_hamming, bool want_pts, mcorb_track_out *out, bool with_out)
{
    TRY(check_lmap(m, "lmap track_rig_frame"));
    TRY(check_args(view, lids, n_lids, max_hamming, out, with_out));
    Frame f;
    TRY(frame_of_slot(m, view, r, slot, frame, f));
    const int32_t lid_first[2] = {0, n_lids};
    return track(m, view, &f, 1, lids, lid_first, max_d2, max_hamming, want_pts, out);
}

// nf frames of a slot's last extraction (mcorb_lmap_track_rig_frames)
int track_slot_frames(mcorb_lmap *m, const mcorb_track_view *views, mcorb_rig *r, int slot, const int32_t *frames, int nf,
                      const int32_t *lids, const int32_t *lid_first, double max_d2, int max_hamming, bool want_pts, mcorb_track_out *outs,
                      bool with_out)
{
    if (with_out && outs)
        for (int f = 0; f < nf; f++) clear_counts(&outs[f]);
    TRY(check_lmap(m, "lmap track_rig_frames"));
    if (nf < 1 || nf > MCORB_TRACK_MAX_FRAMES) return fail(MCORB_E_ARG, "1 .. MCORB_TRACK_MAX_FRAMES frames");
    if (!views || !frames || !lid_first || (with_out && !outs) || max_hamming < 0) return fail(MCORB_E_ARG, "bad argument");
    if (lid_first[0] < 0) return fail(MCORB_E_ARG, "a negative lid_first");
    for (int f = 0; f < nf; f++)
        if (lid_first[f + 1] < lid_first[f]) return fail(MCORB_E_ARG, "lid_first decreases");
    if (lid_first[nf] > lid_first[0] && !lids) return fail(MCORB_E_ARG, "bad argument");
    for (int f = 0; f < nf; f++)
        if (views[f].ncams < 1 || views[f].ncams > MCORB_MAX_CAMS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_CAMS cameras");
    if (with_out)
        for (int f = 0; f < nf; f++) TRY(check_out(&outs[f]));
    std::vector<Frame> fr((size_t)nf);
    for (int f = 0; f < nf; f++) TRY(frame_of_slot(m, &views[f], r, slot, frames[f], fr[f]));
    return track(m, views, fr.data(), nf, lids, lid_first, max_d2, max_hamming, want_pts, with_out ? outs : nullptr);
}

}  // namespace

extern "C" {

int mcorb_lmap_track(mcorb_lmap *m, const mcorb_track_view *view, const mcorb_track_frame *frame, const int32_t *lids, int n_lids,
                     double max_d2, int max_hamming, mcorb_track_out *out)
{
    return track_arrays(m, view, frame, lids, n_lids, max_d2, max_hamming, out && out->match_pt, out, true);
}

int mcorb_lmap_track_rig_frame(mcorb_lmap *m, const mcorb_track_view *view, mcorb_rig *r, int slot, int frame, const int32_t *lids,
                               int n_lids, double max_d2, int max_hamming, mcorb_track_out *out)
{
    return track_slot(m, view, r, slot, frame, lids, n_lids, max_d2, max_hamming, out && out->match_pt, out, true);
}

int mcorb_lmap_track_submit(mcorb_lmap *m, const mcorb_track_view *view, const mcorb_track_frame *frame, const int32_t *lids, int n_lids,
                            double max_d2, int max_hamming, int want_pts)
{
    return track_arrays(m, view, frame, lids, n_lids, max_d2, max_hamming, want_pts != 0, nullptr, false);
}

int mcorb_lmap_track_rig_frame_submit(mcorb_lmap *m, const mcorb_track_view *view, mcorb_rig *r, int slot, int frame, const int32_t *lids,
                                      int n_lids, double max_d2, int max_hamming, int want_pts)
{
    return track_slot(m, view, r, slot, frame, lids, n_lids, max_d2, max_hamming, want_pts != 0, nullptr, false);
}

// the wait of a pending call.  single: mcorb_lmap_track_wait
static int wait_pending(mcorb_lmap *m, const char *who, mcorb_track_out *outs, int n_outs, bool single)
{
    TRY(check_lmap_handle(m, who));
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->track.pending.load()) return fail(MCORB_E_STATE, "no tracking call was submitted");
    const int r = wait_body(m, outs, n_outs, false, single);
    m->track.pending.store(false);
    return r;
}

int mcorb_lmap_track_wait(mcorb_lmap *m, mcorb_track_out *out) { return wait_pending(m, "lmap track_wait", out, 1, true); }

int mcorb_lmap_track_frames_wait(mcorb_lmap *m, mcorb_track_out *outs, int n_outs)
{
    return wait_pending(m, "lmap track_frames_wait", outs, n_outs, false);
}

int mcorb_lmap_track_rig_frames_submit(mcorb_lmap *m, const mcorb_track_view *views, mcorb_rig *r, int slot, const int32_t *frames, int nf,
                                       const int32_t *lids, const int32_t *lid_first, double max_d2, int max_hamming, int want_pts)
{
    return track_slot_frames(m, views, r, slot, frames, nf, lids, lid_first, max_d2, max_hamming, want_pts != 0, nullptr, false);
}

int mcorb_lmap_track_rig_frames(mcorb_lmap *m, const mcorb_track_view *views, mcorb_rig *r, int slot, const int32_t *frames, int nf,
                                const int32_t *lids, const int32_t *lid_first, double max_d2, int max_hamming, int want_pts,
                                mcorb_track_out *outs)
{
    return track_slot_frames(m, views, r, slot, frames, nf, lids, lid_first, max_d2, max_hamming, want_pts != 0, outs, true);
}

int32_t mcorb_host_track_pixel(float v) { return tr_pixel_coord(v); }

// n spans of the last submission's chain from `first` on
static int chain_timing(mcorb_lmap *m, const char *who, float *us, int first, int n)
{
    TRY(check_lmap_handle(m, who));
    if (!us) { set_error(std::string(who) + ": bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < n; k++) us[k] = m->track.chain.us[first + k];
    return MCORB_OK;
}

int mcorb_lmap_last_track_timing(mcorb_lmap *m, float us[2]) { return chain_timing(m, "lmap last_track_timing", us, TK::kProject, 2); }
int mcorb_lmap_last_track_timing4(mcorb_lmap *m, float us[4]) { return chain_timing(m, "lmap last_track_timing4", us, TK::kPoints, 4); }
int mcorb_lmap_last_track_timing5(mcorb_lmap *m, float us[5]) { return chain_timing(m, "lmap last_track_timing5", us, TK::kPoints, 5); }

#ifdef MCORB_TRACK_PROF
// the last call's host phases in microseconds: candidate walk, submission, wait, de-duplication, output.  Not part of the
// public header: a build with -DMCORB_TRACK_PROF exports it for scripts/track_rate.py
int mcorb_lmap_track_phases(mcorb_lmap *m, float us[5])
{
    TRY(check_lmap_handle(m, "lmap track_phases"));
    if (!us) { set_error("lmap track_phases: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    memcpy(us, m->track.us_phase, sizeof(m->track.us_phase));
    return MCORB_OK;
}
#endif

}  // extern "C"
