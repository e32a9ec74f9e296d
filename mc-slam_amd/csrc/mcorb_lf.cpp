// mcorb_lf.cpp -- FrontEnd::obtainLfFeatures (MCSlam/src/FrontEnd.cpp:213-593), SURVEY.md 8f row N3: the immediate
// consumer of the IntraMatch tracks.  Host code: per-track view filtering by the segmentation masks (:262-270), N-view
// triangulation (:280-307), the depth gate (:309), representative descriptor (:349, MultiCameraFrame.cpp:530-567), and the
// response-sorted mono fill to 3000 - intramatch_size (:478-523).  The tiling / refview branches are compile-time dead in the
// reference (`bool tiling = false; bool refview = false;`, :436-437) and are not restated.
//
// Integer / ordering work is exact: the same statements in the same order, and argsorte()'s std::sort (MCSlam/utils.h:21-30)
// is called on the same sequence with the same predicate (ties between equal responses land where libstdc++'s introsort
// puts them -- that IS the reference's order).
// Triangulation: cv::sfm::triangulatePoints is un-vendored third-party code (opencv_contrib / libmv): two views -> the 4x4 DLT
// design matrix, more views -> the 3n x (4+n) "x = alpha P X" design, null vector by SVD (cv::SVD::solveZ).  Restated here with
// the smallest eigenvector of the design's Gram matrix in FP64 (inverse iteration): the null vector of a
// full-column-rank-minus-one matrix is unique up to scale, so any stable method returns the same point to ~1e-11 relative;
// parity for this step is tolerance-based (1e-9) and UNPINNED.  The per-track arithmetic (triangulation, representative
// descriptor) is in mcorb_triangulate.h, shared with k_lf_tracks (mcorb_lf_gpu.hip): the extraction job's stage (lf_job_finish,
// mcorb_rig_set_lf) gives the same bits as this host path.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

#include "mcorb_engine.h"
#include "mcorb_triangulate.h"

using namespace mcorb;

// host-stage hook for the CPU test-suite: the triangulation alone (x: nv normalised points, P: nv row-major 3x4 matrices)
extern "C" int mcorb_host_triangulate(const double *x, const double *P, int nv, double X[3])
{
    if (!x || !P || !X || nv < 2 || nv > MCORB_MAX_CAMS) return MCORB_E_ARG;
    const double *Pp[MCORB_MAX_CAMS];
    for (int i = 0; i < nv; i++) Pp[i] = P + 12 * i;
    triangulate(x, Pp, nv, X);
    return MCORB_OK;
}

// obtainLfFeatures of one frame of a slot into o (feats, words_fil, the two sizes, and in o.src the image-local keypoint of every
// feature's descriptor: m * kcap + k, m the slot's image).  parallel_tri: spread the triangulations over the worker pool (a single
// frame per call); the batched entry point runs whole frames as pool tasks instead and passes false.  pre (the extraction job's
// stage, lf_job_finish): k_lf_tracks' record of every track with two views or more, indexed like the tracks; the host then
// triangulates nothing and takes the point, uv_ref and representative view from the records (same arithmetic, same bits).
static int lf_frame_core(Rig &R, Slot *s, int slot, int frame, const int32_t *tracks, int ntracks, const uint32_t *words,
                         const mcorb_camera *cams, const float *const *seg_masks, int seg_stride, const mcorb_keypoint *const *kps_undist,
                         int total_feats, const LfTrackOut *pre, LfFrameOut &o, bool parallel_tri)
{
    o.feats.clear(); o.words_fil.clear(); o.src.clear();
    o.intramatch_size = o.mono_size = 0;
    if (ntracks < 0 || (ntracks && !tracks) || !cams) {
        set_error("obtain_lf_features: bad argument");
        return MCORB_E_ARG;
    }
    const int C = R.ncams, kcap = R.geom.kcap;
    static const bool prof = getenv("MCORB_HOST_PROF") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    const auto T0 = now();
    if (frame < 0 || (frame + 1) * C > s->nimg_done) { set_error("obtain_lf_features: frame not extracted"); return MCORB_E_STATE; }
    const int m0 = frame * C;
    auto KP = [&](int c) -> const std::vector<mcorb_keypoint> & { return s->kps[m0 + c]; };
    auto KPU = [&](int c, int k) -> const mcorb_keypoint & { return kps_undist && kps_undist[c] ? kps_undist[c][k] : s->kps[m0 + c][k]; };
    auto DESC = [&](int c, int k) -> const uint8_t * { return s->h_desc + ((size_t)(m0 + c) * kcap + k) * 32; };
    auto seg = [&](int c, float px, float py) -> float {   // segMasks[i].at<float>(p.y, p.x): float -> int conversion truncates
        if (!seg_masks || !seg_masks[c]) return 0.f;
        return seg_masks[c][(size_t)(int)py * seg_stride + (int)px];
    };
    for (int t = 0; t < ntracks; t++)
        for (int c = 0; c < C; c++) {
            const int k = tracks[(size_t)t * C + c];
            if (k < -1 || k >= (int)KP(c).size()) { set_error("obtain_lf_features: track index out of range"); return MCORB_E_ARG; }
        }
    std::vector<std::vector<uint8_t>> keypoint_mask(C);          // (:221-227)
    for (int c = 0; c < C; c++) keypoint_mask[c].assign(KP(c).size(), 1);
    std::vector<const double *> prj(C);
    for (int c = 0; c < C; c++) prj[c] = cams[c].Rt;             // build_Rt(R, t) (:224)

    // mono candidates are kept as (camera, keypoint) only: every one of them becomes the same kind of feature (:396-412 and
    // :489-512 fill the same fields), and only the best total_feats - intramatch_size are materialised after the sort
    struct MonoRef { int cam, kp; };
    std::vector<mcorb_lf_feature> &intra = o.feats;
    std::vector<MonoRef> mono_keypoints;
    std::vector<float> responses;
    std::vector<uint32_t> &wfil = o.words_fil;
    std::vector<int32_t> &src = o.src;
    size_t nkp_total = 0;
    for (int c = 0; c < C; c++) nkp_total += KP(c).size();
    intra.reserve((size_t)std::max(total_feats, ntracks) + 8); src.reserve(intra.capacity()); mono_keypoints.reserve(nkp_total + 8); responses.reserve(nkp_total + 8);
    int intramatch_size = 0, mono_size = 0;
    auto blank = [&]() {
        mcorb_lf_feature f;
        memset(&f, 0, sizeof(f));
        for (int c = 0; c < MCORB_MAX_CAMS; c++) f.match_index[c] = -1;
        return f;
    };

    // The triangulation of a track depends on nothing but the track: all of them are done up front on the worker pool
    // (a null vector by Jacobi sweeps per track was 10 of the 13 ms this call took for 2 100 tracks); the bookkeeping below
    // then walks the tracks in order, as the reference does.
    struct Tri { double X[3]; };
    std::vector<Tri> tri(pre ? 0 : (size_t)ntracks);
    if (!pre) {
        constexpr int kChunk = 64;
        const std::function<void(int, int)> tri_task = [&](int chunk, int) {
            for (int ind = chunk * kChunk; ind < std::min(ntracks, (chunk + 1) * kChunk); ind++) {
                int views[MCORB_MAX_CAMS], nv = 0;
                for (int i = 0; i < C; i++) {
                    const int k = tracks[(size_t)ind * C + i];
                    if (k != -1 && (double)seg(i, KP(i)[k].x, KP(i)[k].y) < 0.7) views[nv++] = i;
                }
                if (nv < 2) continue;
                double xx[2 * MCORB_MAX_CAMS];
                const double *PJs[MCORB_MAX_CAMS];
                for (int ii = 0; ii < nv; ii++) {
                    const int v = views[ii];
                    const mcorb_keypoint &kp = KP(v)[tracks[(size_t)ind * C + v]];
                    PJs[ii] = prj[v];
                    xx[2 * ii] = ((double)kp.x - cams[v].K[2]) / cams[v].K[0];          // (pt.x - cx) / fx (:291-293)
                    xx[2 * ii + 1] = ((double)kp.y - cams[v].K[5]) / cams[v].K[4];
                }
                triangulate(xx, PJs, nv, tri[ind].X);
            }
        };
        const int nchunks = (ntracks + kChunk - 1) / kChunk;
        if (nchunks > 1 && parallel_tri) R.pool->parallel_for(nchunks, tri_task, R.pool_threads + slot);
        else for (int ch = 0; ch < nchunks; ch++) tri_task(ch, 0);
    }

    const auto T1 = now();
    for (int ind = 0; ind < ntracks; ind++) {                    // (:250-414)
        mcorb_lf_feature temp = blank();
        for (int c = 0; c < C; c++) temp.match_index[c] = tracks[(size_t)ind * C + c];
        int view_inds[MCORB_MAX_CAMS], num_views = 0;
        const uint8_t *descs[MCORB_MAX_CAMS];
        for (int i = 0; i < C; i++) {
            const int feat_ind = temp.match_index[i];
            if (feat_ind != -1) {
                const mcorb_keypoint &kp = KP(i)[feat_ind];
                // `segMasks[i].at<float>(p.y, p.x) < 0.7` (:264): the float is promoted and compared with the DOUBLE 0.7, so a
                // mask value of exactly 0.7f (0.699999988) still counts as static
                if ((double)seg(i, kp.x, kp.y) < 0.7) {
                    descs[num_views] = DESC(i, feat_ind);
                    view_inds[num_views++] = i;
                } else {
                    temp.match_index[i] = -1;
                }
            }
        }
        if (num_views > 1) {
            const double *X = pre ? pre[ind].X : tri[ind].X;     // cv::sfm::triangulatePoints of the views kept above (:291-306)
            if (pre ? pre[ind].accept != 0 : (X[2] < 40 && X[2] > 0.5)) {   // (:309)
                // K_mats_[0] * pt3d (:339-341): the point is taken in the reference camera's frame
                const double *K0 = cams[0].K;
                const double px = K0[0] * X[0] + K0[1] * X[1] + K0[2] * X[2], py = K0[3] * X[0] + K0[4] * X[1] + K0[5] * X[2],
                             pz = K0[6] * X[0] + K0[7] * X[1] + K0[8] * X[2];
                if (words) wfil.push_back(words[ind]);
                const int rep = pre ? pre[ind].rep : representative_desc(descs, num_views);   // computeRepresentativeDesc (:349)
                memcpy(temp.desc, descs[rep], 32);
                src.push_back((m0 + view_inds[rep]) * kcap + temp.match_index[view_inds[rep]]);
                temp.point3d[0] = X[0]; temp.point3d[1] = X[1]; temp.point3d[2] = X[2];
                temp.uv_ref[0] = pre ? pre[ind].uv[0] : (float)(px / pz);   // cv::Point2f(expected_x, expected_y)
                temp.uv_ref[1] = pre ? pre[ind].uv[1] : (float)(py / pz);
                temp.mono = 0;
                temp.n_rays = num_views;
                intra.push_back(temp);
                intramatch_size++;
                for (int ii = 0; ii < num_views; ii++) keypoint_mask[view_inds[ii]][temp.match_index[view_inds[ii]]] = 0;
            }
        } else if (num_views == 1) {                             // (:396-412)
            const int v = view_inds[0], k = temp.match_index[v];
            mono_keypoints.push_back(MonoRef{v, k});
            responses.push_back(KPU(v, k).response);
            keypoint_mask[v][k] = 0;
        }
    }
    const auto T2 = now();
    // every keypoint no track used becomes a mono candidate, camera by camera (:489-512); the segmentation test is commented
    // out in this branch of the reference
    for (int i = 0; i < C; i++)
        for (int j = 0; j < (int)KP(i).size(); j++)
            if (keypoint_mask[i][j]) {
                mono_keypoints.push_back(MonoRef{i, j});
                responses.push_back(KPU(i, j).response);
                keypoint_mask[i][j] = 0;
            }
    const auto T3 = now();
    // argsorte(responses, false) (MCSlam/utils.h:21-30): std::sort of the index sequence, descending response
    std::vector<int> sorted((int)responses.size());
    std::iota(sorted.begin(), sorted.end(), 0);
    std::sort(sorted.begin(), sorted.end(), [&responses](int i, int j) -> bool { return responses[i] > responses[j]; });
    for (int i = 0; i < (int)sorted.size() && i < (total_feats - intramatch_size); ++i) {   // (:515-521)
        const MonoRef &mr = mono_keypoints[sorted[i]];
        mcorb_lf_feature f = blank();
        f.match_index[mr.cam] = mr.kp;
        memcpy(f.desc, DESC(mr.cam, mr.kp), 32);
        src.push_back((m0 + mr.cam) * kcap + mr.kp);
        f.uv_ref[0] = KPU(mr.cam, mr.kp).x; f.uv_ref[1] = KPU(mr.cam, mr.kp).y;
        f.n_rays = 1;
        f.mono = 1;
        intra.push_back(f);
        mono_size++;
    }
    const auto T4 = now();
    // words_fil is a std::set: ascending, unique
    std::sort(wfil.begin(), wfil.end());
    wfil.erase(std::unique(wfil.begin(), wfil.end()), wfil.end());

    o.intramatch_size = intramatch_size;
    o.mono_size = mono_size;
    if (prof && frame == 0)
        fprintf(stderr, "[mcorb host prof] obtain_lf_features frame 0%s: setup + triangulation %.0f us, track bookkeeping %.0f, mono pool %.0f, sort + fill %.0f, words %.0f\n",
                pre ? " (job)" : "", us(T0, T1), us(T1, T2), us(T2, T3), us(T3, T4), us(T4, now()));
    return MCORB_OK;
}

// o into the caller's arrays, with the getters' capacity convention (the counts are set either way)
static int lf_copy_out(const LfFrameOut &o, mcorb_lf_feature *out, int cap, int *n_out, int *intramatch_size_out, int *mono_size_out,
                       uint32_t *words_fil, int cap_words, int *nwords_fil_out)
{
    if (n_out) *n_out = (int)o.feats.size();
    if (intramatch_size_out) *intramatch_size_out = o.intramatch_size;
    if (mono_size_out) *mono_size_out = o.mono_size;
    if (nwords_fil_out) *nwords_fil_out = (int)o.words_fil.size();
    if ((int)o.feats.size() > cap || (words_fil && (int)o.words_fil.size() > cap_words)) { set_error("obtain_lf_features: output too small"); return MCORB_E_CAP; }
    if (!o.feats.empty()) memcpy(out, o.feats.data(), o.feats.size() * sizeof(mcorb_lf_feature));
    if (words_fil && !o.words_fil.empty()) memcpy(words_fil, o.words_fil.data(), o.words_fil.size() * sizeof(uint32_t));
    return MCORB_OK;
}

static int lf_one_frame(Rig &R, Slot *s, int slot, int frame, const int32_t *tracks, int ntracks, const uint32_t *words,
                        const mcorb_camera *cams, const float *const *seg_masks, int seg_stride, const mcorb_keypoint *const *kps_undist,
                        int total_feats, mcorb_lf_feature *out, int cap, int *n_out, int *intramatch_size_out, int *mono_size_out,
                        uint32_t *words_fil, int cap_words, int *nwords_fil_out, bool parallel_tri)
{
    if (n_out) *n_out = 0;
    if (intramatch_size_out) *intramatch_size_out = 0;
    if (mono_size_out) *mono_size_out = 0;
    if (nwords_fil_out) *nwords_fil_out = 0;
    if (!out || cap < 0) { set_error("obtain_lf_features: bad argument"); return MCORB_E_ARG; }
    LfFrameOut o;
    const int st = lf_frame_core(R, s, slot, frame, tracks, ntracks, words, cams, seg_masks, seg_stride, kps_undist, total_feats, nullptr, o,
                                 parallel_tri);
    if (st != MCORB_OK) return st;
    return lf_copy_out(o, out, cap, n_out, intramatch_size_out, mono_size_out, words_fil, cap_words, nwords_fil_out);
}

// kps_undist of frames [frame0, frame0 + nframes) with the rig's own undistorted set filled in where the caller passes NULL (as a
// whole or per entry) and some camera has undistortion set: 1 = `out` holds the merged pointers, 0 = use the caller's (nothing
// set, or every entry explicit), < 0 = error.  The frame range itself is checked by the caller's per-frame code.
static int undist_inputs(Rig &R, Slot *s, int frame0, int nframes, const mcorb_keypoint *const *kps_undist,
                         std::vector<const mcorb_keypoint *> &out)
{
    const int C = R.ncams, n = nframes * C;
    bool need = !kps_undist;
    for (int i = 0; i < n && !need; i++) need = !kps_undist[i];
    if (!need || !R.undist_on || frame0 < 0 || (frame0 + nframes) * C > s->nimg_done) return 0;
    std::vector<const mcorb_keypoint *> def;
    const int st = R.undist_default(*s, frame0 * C, n, def);
    if (st <= 0) return st;
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) out[i] = kps_undist && kps_undist[i] ? kps_undist[i] : def[i];
    return 1;
}

extern "C" int mcorb_rig_obtain_lf_features(mcorb_rig *r, int slot, int frame, const int32_t *tracks, int ntracks,
                                            const uint32_t *words, const mcorb_camera *cams, const float *const *seg_masks,
                                            int seg_stride, const mcorb_keypoint *const *kps_undist, int total_feats,
                                            mcorb_lf_feature *out, int cap, int *n_out, int *intramatch_size_out,
                                            int *mono_size_out, uint32_t *words_fil, int cap_words, int *nwords_fil_out)
{
    if (n_out) *n_out = 0;
    if (!r || slot < 0 || slot >= (int)r->rig.slots.size()) { set_error("obtain_lf_features: bad argument"); return MCORB_E_ARG; }
    Rig &R = r->rig;
    Slot *s = R.slots[slot].get();
    {
        std::lock_guard<std::mutex> lk(s->m);
        if (s->busy) { set_error("slot busy"); return MCORB_E_STATE; }
    }
    std::vector<const mcorb_keypoint *> ku;
    const int kst = undist_inputs(R, s, frame, 1, kps_undist, ku);
    if (kst < 0) return kst;
    return lf_one_frame(R, s, slot, frame, tracks, ntracks, words, cams, seg_masks, seg_stride, kst ? ku.data() : kps_undist, total_feats, out,
                        cap, n_out, intramatch_size_out, mono_size_out, words_fil, cap_words, nwords_fil_out, true);
}

// All frames [frame0, frame0 + nframes) of a slot in one call, one worker-pool task per frame (the per-frame call is 70 x the
// 0.03 ms per frame of the extraction that feeds it; FrontEnd.cpp:1024 calls obtainLfFeatures once per frame right after
// computeIntraMatches).  tracks / words: the frames' arrays back to back, ntracks[f] tracks (ncams ints each) and words per
// frame; seg_masks / kps_undist: nframes * ncams pointers (index f * ncams + cam) or NULL; out: nframes blocks of `cap` entries,
// words_fil: nframes blocks of cap_words; the four count arrays have nframes entries.  Returns the first failing frame's status.
extern "C" int mcorb_rig_obtain_lf_features_frames(mcorb_rig *r, int slot, int frame0, int nframes, const int32_t *tracks,
                                                   const int32_t *ntracks, const uint32_t *words, const mcorb_camera *cams,
                                                   const float *const *seg_masks, int seg_stride,
                                                   const mcorb_keypoint *const *kps_undist, int total_feats, mcorb_lf_feature *out,
                                                   int cap, int *n_out, int *intramatch_size_out, int *mono_size_out,
                                                   uint32_t *words_fil, int cap_words, int *nwords_fil_out)
{
    if (!r || slot < 0 || slot >= (int)r->rig.slots.size() || nframes < 1 || frame0 < 0 || !ntracks || !n_out || !intramatch_size_out ||
        !mono_size_out || !out || cap < 0 || (words_fil && !nwords_fil_out)) {
        set_error("obtain_lf_features_frames: bad argument");
        return MCORB_E_ARG;
    }
    Rig &R = r->rig;
    Slot *s = R.slots[slot].get();
    {
        std::lock_guard<std::mutex> lk(s->m);
        if (s->busy) { set_error("slot busy"); return MCORB_E_STATE; }
    }
    const int C = R.ncams;
    std::vector<const mcorb_keypoint *> ku;
    const int kst = undist_inputs(R, s, frame0, nframes, kps_undist, ku);
    if (kst < 0) return kst;
    if (kst) kps_undist = ku.data();
    std::vector<size_t> off((size_t)nframes + 1, 0);
    for (int f = 0; f < nframes; f++) {
        if (ntracks[f] < 0) { set_error("obtain_lf_features_frames: negative track count"); return MCORB_E_ARG; }
        off[f + 1] = off[f] + (size_t)ntracks[f];
    }
    std::vector<int> status((size_t)nframes, MCORB_OK);
    std::vector<std::string> errs((size_t)nframes);
    R.pool->parallel_for(nframes, [&](int f, int) {
        int nw = 0;
        status[f] = lf_one_frame(R, s, slot, frame0 + f, tracks ? tracks + off[f] * C : nullptr, ntracks[f], words ? words + off[f] : nullptr, cams,
                                 seg_masks ? seg_masks + (size_t)f * C : nullptr, seg_stride, kps_undist ? kps_undist + (size_t)f * C : nullptr,
                                 total_feats, out + (size_t)f * cap, cap, &n_out[f], &intramatch_size_out[f], &mono_size_out[f],
                                 words_fil ? words_fil + (size_t)f * cap_words : nullptr, cap_words, &nw, false);
        if (nwords_fil_out) nwords_fil_out[f] = nw;
        if (status[f] != MCORB_OK) errs[f] = get_error();   // (the error text is per thread)
    }, R.pool_threads + slot);
    for (int f = 0; f < nframes; f++)
        if (status[f] != MCORB_OK) { set_error("frame " + std::to_string(frame0 + f) + ": " + errs[f]); return status[f]; }
    return MCORB_OK;
}

// ---------------------------------------------------------------------------
// obtainLfFeatures + the LF set's transform inside the extraction job (mcorb_rig_set_lf).  FrontEnd::processFrame calls
// obtainLfFeatures right after computeIntraMatches(matches_map, words_) with words_ overwritten by ones (FrontEnd.cpp:1010) and
// all-zero segmentation masks (mc_slam_app.cpp:224): every view of a track is kept, words_fil is {1} or empty.
// ---------------------------------------------------------------------------

int mcorb::lf_job_finish(Rig &R, Slot &s, int nframes)
{
    const int C = R.ncams, kcap = R.geom.kcap;
    static const bool prof = getenv("MCORB_HOST_PROF") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    const auto T0 = now();
    if ((int)s.lf.size() < R.max_frames) { s.lf.resize(R.max_frames); s.lf_ok.assign(R.max_frames, 0); }
    // 1. k_lf_tracks' input: the tracks with two views or more, binned by view count (2, 3, 4, more) so that a wave runs one
    //    shape; record = the track's index among all tracks of the job (tbase[f] + t), the views in camera order
    constexpr int kBins = 4;
    auto bin_of = [](int nv) { return nv <= 4 ? nv - 2 : 3; };
    std::vector<int> tbase((size_t)nframes + 1, 0), vbase((size_t)nframes + 1, 0), cnt((size_t)kBins * nframes, 0);
    for (int f = 0; f < nframes; f++) {
        const BowFrameOut &b = s.bow[f];
        const int nt = (int)b.n_rays.size();
        int nvs = 0;
        for (int t = 0; t < nt; t++) {
            int nv = 0;
            for (int c = 0; c < C; c++) nv += b.tracks[(size_t)t * C + c] != -1;
            if (nv >= 2) { cnt[(size_t)bin_of(nv) * nframes + f]++; nvs += nv; }
        }
        tbase[f + 1] = tbase[f] + nt;
        vbase[f + 1] = vbase[f] + nvs;
    }
    std::vector<int> boff((size_t)kBins * nframes + 1, 0);   // bin-major, frame-minor
    for (size_t i = 0; i < cnt.size(); i++) boff[i + 1] = boff[i] + cnt[i];
    const int nsend = boff.back();
    // (the first bind sized the buffers for one track and one view per keypoint, which the BoW-guided tracks never exceed; grown
    // here all the same should a job need more)
    const size_t ntrk = (size_t)tbase[nframes], nview = (size_t)vbase[nframes];
    TRY(s.lbuf.h_lftrk.grow(ntrk, hipHostMallocDefault));
    TRY(s.lbuf.d_lftrk.grow(ntrk));
    TRY(s.lbuf.h_lfout.grow(ntrk, hipHostMallocMapped | hipHostMallocPortable));
    TRY(s.lbuf.h_lfview.grow(nview, hipHostMallocDefault));
    TRY(s.lbuf.d_lfview.grow(nview));
    R.pool->parallel_for(nframes, [&](int f, int) {
        const BowFrameOut &b = s.bow[f];
        const int nt = (int)b.n_rays.size();
        int next[kBins], vo = vbase[f];
        for (int k = 0; k < kBins; k++) next[k] = boff[(size_t)k * nframes + f];
        for (int t = 0; t < nt; t++) {
            const int32_t *tr = b.tracks.data() + (size_t)t * C;
            int nv = 0;
            for (int c = 0; c < C; c++) nv += tr[c] != -1;
            if (nv < 2) continue;
            s.lbuf.h_lftrk[next[bin_of(nv)]++] = make_int4(vo, nv, f, tbase[f] + t);
            for (int c = 0; c < C; c++)
                if (tr[c] != -1) {
                    const mcorb_keypoint &kp = s.kps[f * C + c][tr[c]];
                    s.lbuf.h_lfview[vo++] = LfView{c, tr[c], kp.x, kp.y};
                }
        }
    }, R.pool_threads + s.index);
    const auto T1 = now();
    // 2. one launch behind the descent results' copy (bow_job_finish), records straight to host-mapped memory
    if (nsend) {
        HIPCHK(hipMemcpyAsync(s.lbuf.d_lftrk, s.lbuf.h_lftrk, (size_t)nsend * sizeof(int4), hipMemcpyHostToDevice, s.st_dma));
        HIPCHK(hipMemcpyAsync(s.lbuf.d_lfview, s.lbuf.h_lfview, (size_t)vbase[nframes] * sizeof(LfView), hipMemcpyHostToDevice, s.st_dma));
        launch_lf_tracks(s.st_dma, s.lbuf.d_lftrk, s.lbuf.d_lfview, nsend, R.d_lfcams, s.d_desc, kcap, C, s.lbuf.h_lfout);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(s.lbuf.ev_lf, s.st_dma));
    HIPCHK(R.wait_event(s.lbuf.ev_lf));
    const auto T2 = now();
    // 3. per frame: the order-dependent bookkeeping on the records, then the LF set's transform from the job's descent results
    std::vector<const mcorb_keypoint *> ku;
    const int kst = undist_inputs(R, &s, 0, nframes, nullptr, ku);
    if (kst < 0) return kst;
    std::vector<int> status((size_t)nframes, MCORB_OK);
    std::vector<std::string> errs((size_t)nframes);
    const int weighting = R.bow_bind.weighting, scoring = R.bow_bind.scoring;
    R.pool->parallel_for(nframes, [&](int f, int) {
        const BowFrameOut &b = s.bow[f];
        const int nt = (int)b.n_rays.size();
        const std::vector<uint32_t> ones((size_t)nt, 1u);   // words_ (FrontEnd.cpp:1010)
        LfFrameOut &o = s.lf[f];
        status[f] = lf_frame_core(R, &s, s.index, f, b.tracks.data(), nt, ones.data(), R.lf_cams.data(), nullptr, 0,
                                  kst ? ku.data() + (size_t)f * C : nullptr, R.lf_total_feats, s.lbuf.h_lfout + tbase[f], o, false);
        if (status[f] != MCORB_OK) { errs[f] = get_error(); return; }
        std::vector<BowRes> res(o.src.size());
        for (size_t i = 0; i < o.src.size(); i++) res[i] = s.lbuf.h_lfres[o.src[i]];
        bow_assemble(weighting, scoring, res.data(), (int)res.size(), o.bow);
        s.lf_ok[f] = 1;
    }, R.pool_threads + s.index);
    if (prof)
        fprintf(stderr, "[mcorb host prof] lf stage x%d frames (%d tracks to the GPU): pack %.0f us, k_lf_tracks + wait %.0f, bookkeeping + transform %.0f\n",
                nframes, nsend, us(T0, T1), us(T1, T2), us(T2, now()));
    for (int f = 0; f < nframes; f++)
        if (status[f] != MCORB_OK) { set_error("lf stage, frame " + std::to_string(f) + ": " + errs[f]); return status[f]; }
    return MCORB_OK;
}

extern "C" int mcorb_rig_set_lf(mcorb_rig *r, const mcorb_camera *cams, int total_feats)
{
    if (!r) { set_error("set_lf: bad argument"); return MCORB_E_ARG; }
    return r->rig.set_lf(cams, total_feats);
}

// the job's LF results of one frame: MCORB_E_STATE unless the slot's last extraction ran the stage for it
static int lf_frame_of(mcorb_rig *r, int slot, int frame, const LfFrameOut **o)
{
    if (!r || slot < 0 || slot >= (int)r->rig.slots.size()) { set_error("lf getter: bad argument"); return MCORB_E_ARG; }
    Slot *s = r->rig.slots[slot].get();
    {
        std::lock_guard<std::mutex> lk(s->m);
        if (s->busy) { set_error("slot busy"); return MCORB_E_STATE; }
    }
    if (frame < 0 || frame >= (int)s->lf_ok.size() || !s->lf_ok[frame]) {
        set_error("lf getter: frame not processed by the LF stage since the slot's last extraction");
        return MCORB_E_STATE;
    }
    *o = &s->lf[frame];
    return MCORB_OK;
}

extern "C" int mcorb_rig_get_lf_features(mcorb_rig *r, int slot, int frame, mcorb_lf_feature *out, int cap, int *n_out,
                                         int *intramatch_size_out, int *mono_size_out, uint32_t *words_fil, int cap_words,
                                         int *nwords_fil_out)
{
    if (n_out) *n_out = 0;
    if (intramatch_size_out) *intramatch_size_out = 0;
    if (mono_size_out) *mono_size_out = 0;
    if (nwords_fil_out) *nwords_fil_out = 0;
    const LfFrameOut *o = nullptr;
    const int st = lf_frame_of(r, slot, frame, &o);
    if (st != MCORB_OK) return st;
    if (cap < 0 || (cap > 0 && !out)) { set_error("lf getter: bad argument"); return MCORB_E_ARG; }
    return lf_copy_out(*o, out, cap, n_out, intramatch_size_out, mono_size_out, words_fil, cap_words, nwords_fil_out);
}

extern "C" int mcorb_rig_get_lf_bow(mcorb_rig *r, int slot, int frame, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow,
                                    uint32_t *fv_nodes, int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap)
{
    if (nbow) *nbow = 0;
    if (nfv) *nfv = 0;
    const LfFrameOut *o = nullptr;
    const int st = lf_frame_of(r, slot, frame, &o);
    if (st != MCORB_OK) return st;
    const BowImageOut &b = o->bow;
    if (nbow) *nbow = (int)b.bow_ids.size();
    if (nfv) *nfv = (int)b.fv_nodes.size();
    if ((int)b.bow_ids.size() > bow_cap || (int)b.fv_nodes.size() > fv_cap || (int)b.fv_feats.size() > feat_cap) { set_error("lf bow: output too small"); return MCORB_E_CAP; }
    if (!fv_offsets || (!b.bow_ids.empty() && (!bow_ids || !bow_vals)) || (!b.fv_nodes.empty() && !fv_nodes) || (!b.fv_feats.empty() && !fv_feats)) {
        set_error("lf bow: bad argument");
        return MCORB_E_ARG;
    }
    if (!b.bow_ids.empty()) { memcpy(bow_ids, b.bow_ids.data(), b.bow_ids.size() * 4); memcpy(bow_vals, b.bow_vals.data(), b.bow_vals.size() * 8); }
    if (!b.fv_nodes.empty()) memcpy(fv_nodes, b.fv_nodes.data(), b.fv_nodes.size() * 4);
    memcpy(fv_offsets, b.fv_offsets.data(), b.fv_offsets.size() * 4);
    if (!b.fv_feats.empty()) memcpy(fv_feats, b.fv_feats.data(), b.fv_feats.size() * 4);
    return MCORB_OK;
}

// test hook: k_lf_tracks' triangulation (mcorb_triangulate.h) of n arbitrary problems on the device
extern "C" int mcorb_dev_triangulate_selftest(int device, const double *x, const double *P, const int32_t *nv, int n, double *X,
                                              int32_t *branch)
{
    if (!x || !P || !nv || !X || !branch || n < 1) { set_error("triangulate selftest: bad argument"); return MCORB_E_ARG; }
    std::vector<int> voff((size_t)n);
    size_t nviews = 0;
    for (int i = 0; i < n; i++) {
        if (nv[i] < 2 || nv[i] > MCORB_MAX_CAMS) { set_error("triangulate selftest: view count out of range"); return MCORB_E_ARG; }
        voff[i] = (int)nviews;
        nviews += (size_t)nv[i];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { set_error("no usable HIP device"); return MCORB_E_NODEVICE; }
    HIPCHK(hipSetDevice(device));
    DevBuf<double> d_x, d_P, d_X;
    DevBuf<int> d_nv, d_voff, d_br;
    TRY(d_x.alloc(nviews * 2));
    TRY(d_P.alloc(nviews * 12));
    TRY(d_X.alloc((size_t)n * 3));
    TRY(d_nv.alloc((size_t)n));
    TRY(d_voff.alloc((size_t)n));
    TRY(d_br.alloc((size_t)n));
    HIPCHK(hipMemcpy(d_x, x, nviews * 2 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_P, P, nviews * 12 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nv, nv, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_voff, voff.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    launch_tri_selftest(nullptr, d_x, d_P, d_nv, d_voff, n, d_X, d_br);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(X, d_X, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(branch, d_br, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return MCORB_OK;
}

// host twin of the self-test's branch output (the CPU suite checks the shared header against it)
extern "C" int mcorb_host_triangulate_branch(const double *x, const double *P, int nv, double X[3], int32_t *branch)
{
    if (!x || !P || !X || !branch || nv < 2 || nv > MCORB_MAX_CAMS) return MCORB_E_ARG;
    const double *Pp[MCORB_MAX_CAMS];
    for (int i = 0; i < nv; i++) Pp[i] = P + 12 * i;
    *branch = triangulate(x, Pp, nv, X);
    return MCORB_OK;
}
