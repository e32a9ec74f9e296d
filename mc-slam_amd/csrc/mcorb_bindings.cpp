// mcorb_bindings.cpp -- what a rig can have bound and every job then runs: keypoint undistortion, image undistortion, a
// vocabulary, the LF cameras.  Each is allocated at its first set call and costs a rig that never sets it nothing.
#include <string.h>

#include <cmath>

#include "mcorb_engine.h"

namespace mcorb {

// ---------------------------------------------------------------------------
// UndistortKeyPoints (MultiCameraFrame.cpp:300-347) inside the job.  Nothing of this runs, is allocated or is captured while no
// camera has undistortion set (undist_on): such a job is exactly the job without the feature.
// ---------------------------------------------------------------------------
// on the side stream, behind whatever the caller ordered it after; small batches write the host-mapped points directly and record
// ev_u1 for the caller's join, the others copy them back behind the kernel
int Rig::enqueue_undistort(Slot &s, int nimg)
{
    const bool host_out = s.host_results;
    launch_undistort(s.st_dma, s.ctl.sel, s.ctl.nsel, geom.kcap, nimg, ncams, d_undist_cams, tab.scale, tab.nlevels, host_out ? s.ubuf.h_undist : s.ubuf.d_undist);
    if (host_out || s.bow_job) HIPCHK(hipEventRecord(s.ubuf.ev_u1, s.st_dma));   // (a bound job's BoW tables read the points: enqueue_bow)
    if (!host_out) HIPCHK(hipMemcpyAsync(s.ubuf.h_undist, s.ubuf.d_undist, (size_t)nimg * geom.kcap * sizeof(float2), hipMemcpyDeviceToHost, s.st_dma));
    return MCORB_OK;
}

int Rig::lock_idle_slots(const char *who, std::vector<std::unique_lock<std::mutex>> &locks)
{
    for (auto &sp : slots) {
        locks.emplace_back(sp->m);
        if (sp->busy || sp->submitted) { set_error(std::string(who) + ": a submitted job has not been waited for"); return MCORB_E_STATE; }
    }
    return MCORB_OK;
}

int UndistBufs::alloc(size_t npoints)
{
    TRY(d_undist.alloc(npoints));
    TRY(h_undist.alloc(npoints, kHostMapped));
    TRY(ev_u0.create(hipEventDisableTiming));
    TRY(ev_u1.create(hipEventDisableTiming));
    bound = true;
    return MCORB_OK;
}

int Rig::set_undistortion(int cam, const double *K, const double *dist, int ncoeffs)
{
    if (cam < 0 || cam >= ncams) { set_error("set_undistortion: camera out of range"); return MCORB_E_ARG; }
    const bool clear = !dist || ncoeffs == 0;
    UndistCam c = {};
    if (!clear) {
        if (!K) { set_error("set_undistortion: no camera matrix"); return MCORB_E_ARG; }
        if (undist_prepare(K, dist, ncoeffs, c) != 0) { set_error("set_undistortion: 4, 5, 8 or 12 coefficients (the tilt model is not supported)"); return MCORB_E_ARG; }
        for (double f : {K[0], K[4], c.K[0], c.K[4]})
            if (!std::isfinite(f) || f == 0.) { set_error("set_undistortion: fx / fy must be finite and non-zero"); return MCORB_E_ARG; }
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    TRY(lock_idle_slots("set_undistortion", locks));
    if (imgud_on) {   // RECTIFY: image_kps_undist is the raw keypoint set (MultiCameraFrame.cpp:241-242)
        set_error("set_undistortion: image undistortion is set (mcorb_rig_set_image_undistortion); a rig is rectified or it is not");
        return MCORB_E_STATE;
    }
    HIPCHK(hipSetDevice(device));
    if (!clear && !slots[0]->ubuf.bound) {   // first set call: the device table and every slot's buffers and events
        DevBuf<UndistCam> cams;
        std::vector<UndistBufs> fresh(slots.size());
        TRY(cams.alloc((size_t)ncams));
        for (UndistBufs &b : fresh) TRY(b.alloc((size_t)max_images * geom.kcap));
        d_undist_cams = std::move(cams);   // all there: commit (nothing below fails before every slot has its bundle)
        for (size_t i = 0; i < slots.size(); i++) {
            slots[i]->ubuf = std::move(fresh[i]);
            slots[i]->kps_undist.assign(max_images, {});
            slots[i]->kps_undist_ok.assign(max_images, 0);
        }
    }
    undist_cams[cam] = c;
    undist_set[cam] = clear ? 0 : 1;
    undist_on = std::any_of(undist_set.begin(), undist_set.end(), [](uint8_t v) { return v != 0; });
    if (d_undist_cams) HIPCHK(hipMemcpy(d_undist_cams, undist_cams.data(), (size_t)ncams * sizeof(UndistCam), hipMemcpyHostToDevice));
    undist_gen++;
    return MCORB_OK;
}

// ---------------------------------------------------------------------------
// cv::undistort at the hand-off (the RECTIFY branch of setData, MultiCameraFrame.cpp:123-136).  It belongs to the upload, as it
// belongs to setData: a job, its captured graph and a re-run on resident inputs read level 0 and never know.  Nothing of this
// runs or is allocated while no camera has it set (imgud_on): an upload is then exactly the upload without the feature.
// ---------------------------------------------------------------------------
int Rig::enqueue_remap(Slot &s, int nimg)
{
    launch_remap_u8(s.st, s.d_raw, s.d_pyr, geom, d_remap_cams, ncams, nimg);
    HIPCHK(hipGetLastError());
    return MCORB_OK;
}

int Rig::set_image_undistortion(int cam, const double *K, const double *dist, int ncoeffs)
{
    if (cam < 0 || cam >= ncams) { set_error("set_image_undistortion: camera out of range"); return MCORB_E_ARG; }
    const bool clear = !dist || ncoeffs == 0;
    UndistImageCam c = {};
    if (!clear) {
        if (!K) { set_error("set_image_undistortion: no camera matrix"); return MCORB_E_ARG; }
        if (undist_image_prepare(K, dist, ncoeffs, c) != 0) { set_error("set_image_undistortion: 4, 5, 8 or 12 coefficients (the tilt model is not supported)"); return MCORB_E_ARG; }
        for (double v : c.K) if (!std::isfinite(v)) { set_error("set_image_undistortion: non-finite camera matrix"); return MCORB_E_ARG; }
        for (double v : c.k) if (!std::isfinite(v)) { set_error("set_image_undistortion: non-finite coefficient"); return MCORB_E_ARG; }
        if (c.K[0] == 0. || c.K[4] == 0.) { set_error("set_image_undistortion: fx / fy must be non-zero"); return MCORB_E_ARG; }
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    TRY(lock_idle_slots("set_image_undistortion", locks));
    if (undist_on) {   // the reference's RECTIFY is rig-wide and excludes UndistortKeyPoints (MultiCameraFrame.cpp:241-242)
        set_error("set_image_undistortion: keypoint undistortion is set (mcorb_rig_set_undistortion); a rig is rectified or it is not");
        return MCORB_E_STATE;
    }
    HIPCHK(hipSetDevice(device));
    for (auto &sp : slots) HIPCHK(hipStreamSynchronize(sp->st));   // an earlier upload's k_remap_u8 reads the tables changed below
    const size_t plane = (size_t)W * H, mp = remap_map_pitch(W);
    if (!clear) {
        if (!d_remap_cams) {   // first set call: the camera table and every slot's raw planes
            DevBuf<RemapCam> cams;
            std::vector<DevBuf<uint8_t>> fresh(slots.size());
            TRY(cams.alloc((size_t)ncams));
            for (auto &b : fresh) {
                TRY(b.alloc((size_t)max_images * plane));
                HIPCHK(hipMemset(b, 0, (size_t)max_images * plane));
            }
            d_remap_cams = std::move(cams);
            for (size_t i = 0; i < slots.size(); i++) slots[i]->d_raw = std::move(fresh[i]);
        }
        // the camera's maps: built here, once (the row loop is a serial sum), padded for the device
        std::vector<int16_t> m1(plane * 2);
        std::vector<uint16_t> m2(plane);
        undist_image_map(c, W, H, m1.data(), m2.data());
        std::vector<int16_t> p1((size_t)H * mp * 2, 0);
        std::vector<uint16_t> p2((size_t)H * mp, 0);
        for (int y = 0; y < H; y++) {
            memcpy(p1.data() + (size_t)y * mp * 2, m1.data() + (size_t)y * W * 2, (size_t)W * 4);
            memcpy(p2.data() + (size_t)y * mp, m2.data() + (size_t)y * W, (size_t)W * 2);
        }
        DevBuf<int16_t> d1;
        DevBuf<uint16_t> d2;
        TRY(d1.alloc(p1.size()));
        TRY(d2.alloc(p2.size()));
        HIPCHK(hipMemcpy(d1, p1.data(), p1.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d2, p2.data(), p2.size() * 2, hipMemcpyHostToDevice));
        d_imgud_map1[cam] = std::move(d1);   // all there: commit
        d_imgud_map2[cam] = std::move(d2);
        imgud_map1[cam] = std::move(m1);
        imgud_map2[cam] = std::move(m2);
    } else {
        d_imgud_map1[cam].reset();
        d_imgud_map2[cam].reset();
        imgud_map1[cam] = {};
        imgud_map2[cam] = {};
    }
    imgud_cams[cam] = c;
    imgud_set[cam] = clear ? 0 : 1;
    imgud_on = std::any_of(imgud_set.begin(), imgud_set.end(), [](uint8_t v) { return v != 0; });
    if (d_remap_cams) {
        std::vector<RemapCam> t((size_t)ncams);
        for (int i = 0; i < ncams; i++) t[i] = RemapCam{d_imgud_map1[i].get(), d_imgud_map2[i].get(), imgud_set[i] ? 1 : 0, 0};
        HIPCHK(hipMemcpy(d_remap_cams, t.data(), t.size() * sizeof(RemapCam), hipMemcpyHostToDevice));
    }
    return MCORB_OK;
}

// ---------------------------------------------------------------------------
// transform() (MultiCameraFrame.cpp:257) and computeIntraMatches(matches, words_) (:586-943) inside the job.  Nothing of this runs,
// is allocated or is captured while no vocabulary is bound (bow_bind.flags == 0): such a job is exactly the job without the feature.
// ---------------------------------------------------------------------------
int Rig::check_job_shape(const Job &j) const
{
    if ((j.kind == Job::EXTRACT || j.kind == Job::PROCESS) && (bow_bind.flags & MCORB_BOW_MATCH) && j.nimg % ncams != 0) {
        set_error("extract: a vocabulary bound with MCORB_BOW_MATCH needs whole rig frames (nimg a multiple of the camera count)");
        return MCORB_E_ARG;
    }
    return MCORB_OK;
}

int Rig::enqueue_bow(Slot &s, int nimg)
{
    const BowBinding &b = bow_bind;
    const uint32_t *sel = s.ctl.sel;
    const int *nsel = s.ctl.nsel;
    const bool host_out = s.host_results;
    const int kcap = geom.kcap, nframes = nimg / ncams;
    const bool match = (s.bow_job & MCORB_BOW_MATCH) && npp > 0 && nframes > 0;
    launch_bow_descend(s.st, s.d_desc, nimg * kcap, b.child_start, b.child_count, b.child_desc, b.child_id, b.word_id, b.weight,
                       b.L - b.levelsup, s.bbuf.d_bowres);
    launch_bow_fold(s.st, s.bbuf.d_bowres, nsel, kcap, nimg, b.weighting, b.scoring, s.bbuf.d_bowrec, host_out ? s.bbuf.h_bowrec : nullptr);
    if (match) {
        // the rows of the |dy| < 50 gate: the job's own undistorted points when undistortion is set (k_undistort on the side stream)
        if (undist_on && !host_out) HIPCHK(hipStreamWaitEvent(s.st, s.ubuf.ev_u1, 0));   // (small batches joined it already)
        launch_bow_tables(s.st, s.bbuf.d_bowrec, kcap, ncams, nframes, nsel, sel, tab.scale, tab.nlevels,
                          undist_on ? (host_out ? s.ubuf.h_undist : s.ubuf.d_undist) : nullptr, s.bbuf.d_bslot, s.bbuf.d_bnfeats, s.bbuf.d_bnfeat, s.bbuf.d_brgbase,
                          s.bbuf.d_byv, s.bbuf.d_brange);
        launch_bow_best2(s.st, s.d_desc, 0, kcap, ncams, nframes, s.bbuf.d_byv, s.bbuf.d_bslot, s.bbuf.d_brange, s.bbuf.d_brgbase, s.bbuf.d_bnfeats, s.bbuf.d_bnfeat,
                         host_out ? s.bbuf.h_btab : s.bbuf.d_btab);
    }
    HIPCHK(hipGetLastError());
    if (host_out) return MCORB_OK;
    HIPCHK(hipEventRecord(s.bbuf.ev_b, s.st));
    HIPCHK(hipStreamWaitEvent(s.st_dma, s.bbuf.ev_b, 0));
    HIPCHK(hipMemcpyAsync(s.bbuf.h_bowrec, s.bbuf.d_bowrec, (size_t)nimg * bow_rec_ints(kcap) * sizeof(int), hipMemcpyDeviceToHost, s.st_dma));
    if (match)
        HIPCHK(hipMemcpyAsync(s.bbuf.h_btab, s.bbuf.d_btab, (size_t)nframes * npp * kcap * sizeof(int4), hipMemcpyDeviceToHost, s.st_dma));
    return MCORB_OK;
}

int BowBufs::alloc(const Rig &R)
{
    const size_t M = (size_t)R.max_images, kc = (size_t)R.geom.kcap, F = (size_t)R.max_frames;
    const size_t tab_n = std::max<size_t>((size_t)std::max(R.npp, 1) * F * kc, 1);
    TRY(d_bowres.alloc(M * kc));
    TRY(d_bowrec.alloc(M * bow_rec_ints(R.geom.kcap)));
    TRY(h_bowrec.alloc(M * bow_rec_ints(R.geom.kcap), kHostMapped));
    TRY(d_bslot.alloc(M * kc));
    TRY(d_bnfeats.alloc(M * kc));
    TRY(d_bnfeat.alloc(M));
    TRY(d_brgbase.alloc(F + 1));
    TRY(d_byv.alloc(M * kc));
    TRY(d_brange.alloc(M * kc * (size_t)R.ncams));
    TRY(d_btab.alloc(tab_n));
    TRY(h_btab.alloc(tab_n, kHostMapped));
    TRY(ev_b.create(hipEventDisableTiming));
    bound = true;
    return MCORB_OK;
}

int Rig::set_vocabulary(const BowBinding &b)
{
    if (b.flags && geom.kcap > kBowFoldMaxKcap) {
        set_error("set_vocabulary: the rig's keypoint capacity (kcap " + std::to_string(geom.kcap) + ") exceeds MCORB_BOW_MAX_KCAP (" +
                  std::to_string(kBowFoldMaxKcap) + ")");
        return MCORB_E_ARG;
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    TRY(lock_idle_slots("set_vocabulary", locks));
    HIPCHK(hipSetDevice(device));
    if (b.flags && !slots.empty() && !slots[0]->bbuf.bound) {   // first bind: every slot's buffers
        std::vector<BowBufs> fresh(slots.size());
        for (BowBufs &f : fresh) TRY(f.alloc(*this));
        for (size_t i = 0; i < slots.size(); i++) slots[i]->bbuf = std::move(fresh[i]);   // all there: commit
    }
    bow_bind = b.flags ? b : BowBinding{};
    bow_gen++;
    return MCORB_OK;
}

int LfBufs::alloc(size_t n)
{
    TRY(h_lftrk.alloc(n, hipHostMallocDefault));
    TRY(d_lftrk.alloc(n));
    TRY(h_lfview.alloc(n, hipHostMallocDefault));
    TRY(d_lfview.alloc(n));
    TRY(h_lfout.alloc(n, kHostMapped));
    TRY(h_lfres.alloc(n, hipHostMallocDefault));
    TRY(ev_lf.create(hipEventDisableTiming));
    bound = true;
    return MCORB_OK;
}

// obtainLfFeatures inside the job (lf_job_finish).  Nothing of it runs, is allocated or is captured while no cameras are bound.
int Rig::set_lf(const mcorb_camera *cams, int total_feats)
{
    if (cams && total_feats < 0) { set_error("set_lf: total_feats must be >= 0"); return MCORB_E_ARG; }
    std::vector<std::unique_lock<std::mutex>> locks;
    TRY(lock_idle_slots("set_lf", locks));
    HIPCHK(hipSetDevice(device));
    if (cams && !slots[0]->lbuf.bound) {   // first bind: the camera table and every slot's buffers, sized for one track per keypoint
        DevBuf<LfCam> table;
        std::vector<LfBufs> fresh(slots.size());
        TRY(table.alloc(MCORB_MAX_CAMS));
        for (LfBufs &f : fresh) TRY(f.alloc((size_t)max_images * geom.kcap));
        d_lfcams = std::move(table);   // all there: commit
        for (size_t i = 0; i < slots.size(); i++) slots[i]->lbuf = std::move(fresh[i]);
    }
    if (cams) {
        std::vector<LfCam> dc((size_t)ncams);
        for (int c = 0; c < ncams; c++) {
            memcpy(dc[c].K, cams[c].K, sizeof(dc[c].K));
            memcpy(dc[c].Rt, cams[c].Rt, sizeof(dc[c].Rt));
        }
        HIPCHK(hipMemcpy(d_lfcams, dc.data(), dc.size() * sizeof(LfCam), hipMemcpyHostToDevice));
        lf_cams.assign(cams, cams + ncams);
        lf_total_feats = total_feats;
    } else {
        lf_cams.clear();
    }
    lf_on = cams != nullptr;
    lf_gen++;
    return MCORB_OK;
}

int Rig::undist_records(Slot &s, int m0, int n, std::vector<const mcorb_keypoint *> &out)
{
    if (m0 < 0 || n < 0 || m0 + n > s.nimg_done) { set_error("undistorted keypoints: image index out of range"); return MCORB_E_ARG; }
    if (s.undist_gen != undist_gen) { set_error("undistorted keypoints: image not extracted since the last mcorb_rig_set_undistortion"); return MCORB_E_STATE; }
    std::lock_guard<std::mutex> lk(s.undist_m);
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const int m = m0 + i;
        if (!s.undist_job) { out[i] = s.kps[m].data(); continue; }
        if (!s.kps_undist_ok[m]) {   // the keypoint records with pt replaced (:336-344)
            std::vector<mcorb_keypoint> &U = s.kps_undist[m];
            U = s.kps[m];
            const float2 *p = s.ubuf.h_undist + (size_t)m * geom.kcap;
            for (size_t k = 0; k < U.size(); k++) { U[k].x = p[k].x; U[k].y = p[k].y; }
            s.kps_undist_ok[m] = 1;
        }
        out[i] = s.kps_undist[m].data();
    }
    return MCORB_OK;
}

int Rig::undist_default(Slot &s, int m0, int n, std::vector<const mcorb_keypoint *> &out)
{
    if (!undist_on) return 0;
    const int st = undist_records(s, m0, n, out);
    return st == MCORB_OK ? 1 : st;
}

}  // namespace mcorb
