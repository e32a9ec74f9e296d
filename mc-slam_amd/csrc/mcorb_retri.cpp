// mcorb_retri.cpp -- mcorb_lmap_retriangulate: the landmarks seen in a moved keyframe made again from all of their observations
// (mcorb_retri.h).  The host checks the arguments, sorts the observations by (landmark, keyframe, camera)
// and names the keyframes that have one (retri_plan).  A device store then queues k_retri_views and k_retri_solve
// (mcorb_retri_gpu.hip) in one Submission and waits once; the records land in host-mapped memory.  A host-only store runs
// retri_run_serial, the same arithmetic with the same fold, so the two agree bit for bit.  In apply mode the kernel makes the
// gated stores into the points and the host then deletes the failed landmarks through mcorb_lmap_delete's body: the observations
// are host state.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_kernels.h"
#include "mcorb_lmap_store.h"
#include "mcorb_pack.h"

using namespace mcorb;

namespace {

int fail(int code, const char *what) { set_error(std::string("lmap retriangulate: ") + what); return code; }

bool failed(int verdict)
{
    return verdict == MCORB_RETRI_DEGENERATE || verdict == MCORB_RETRI_BEHIND || verdict == MCORB_RETRI_FAR || verdict == MCORB_RETRI_OUTLIER;
}

}  // namespace

extern "C" {

int mcorb_lmap_retriangulate(mcorb_lmap *m, int nkf, const double *kf_R, const double *kf_t, const uint8_t *moved, int ncams,
                             const mcorb_track_cam *cams, int nlm, const int32_t *lids, int nobs, const int32_t *obs_kf,
                             const int32_t *obs_cam, const int32_t *obs_lm, const float *uv, const mcorb_retri_params *params,
                             double *pts_out, double *diff_norm, int32_t *n_views, int32_t *verdict, mcorb_retri_result *res,
                             int32_t *kfs, int32_t *feats, int cap)
{
    TRY(check_lmap(m, "lmap retriangulate"));
    if (!kf_R || !kf_t || !moved || !cams || !params || !res) return fail(MCORB_E_ARG, "bad argument");
    if (nkf < 1 || nkf > MCORB_RETRI_MAX_KF) return fail(MCORB_E_ARG, "1 .. MCORB_RETRI_MAX_KF keyframes");
    if (ncams < 1 || ncams > MCORB_MAX_CAMS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_CAMS cameras");
    if (nlm < 0 || nlm > MCORB_BA_MAX_LANDMARKS) return fail(MCORB_E_ARG, "0 .. MCORB_BA_MAX_LANDMARKS landmarks");
    if (nobs < 0 || nobs > MCORB_BA_MAX_OBS) return fail(MCORB_E_ARG, "0 .. MCORB_BA_MAX_OBS observations");
    if (params->mode != MCORB_RETRI_REPORT && params->mode != MCORB_RETRI_APPLY) return fail(MCORB_E_ARG, "an unknown mode");
    if (params->rank_tol != params->rank_tol || params->max_diff != params->max_diff) return fail(MCORB_E_ARG, "a NaN rank_tol or max_diff");
    if (nlm && !lids) return fail(MCORB_E_ARG, "bad argument");
    if (nobs && (!obs_kf || !obs_cam || !obs_lm || !uv)) return fail(MCORB_E_ARG, "bad argument");
    if (cap < 0 || (cap && (!kfs || !feats))) return fail(MCORB_E_ARG, "bad argument");
    for (int i = 0; i < nobs; i++) {
        if (obs_kf[i] < 0 || obs_kf[i] >= nkf) return fail(MCORB_E_ARG, "a keyframe index outside the call's list");
        if (obs_cam[i] < 0 || obs_cam[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
        if (obs_lm[i] < 0 || obs_lm[i] >= nlm) return fail(MCORB_E_ARG, "a landmark index outside the call's list");
    }
    for (int j = 0; j < nlm; j++)
        if (lids[j] < 0 || lids[j] >= m->max_landmarks) return fail(MCORB_E_ARG, "landmark id outside the store");
    const bool apply = params->mode == MCORB_RETRI_APPLY;
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track.pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");
    bool twice = false;
    for (int j = 0; j < nlm; j++)
        if (m->life.occ[lids[j]]++) twice = true;
    for (int j = 0; j < nlm; j++) m->life.occ[lids[j]] = 0;
    if (twice) return fail(MCORB_E_ARG, "a landmark id twice in lids");
    for (int j = 0; j < nlm; j++) {
        if (!(m->flags[lids[j]] & kHasPt)) return fail(MCORB_E_STATE, "a landmark has no point");
        if (apply && (m->flags[lids[j]] & kSet) != kSet) return fail(MCORB_E_STATE, "apply mode: a slot that was never set");
    }

    memset(res, 0, sizeof(*res));
    RetriPlan plan;
    retri_plan(nkf, ncams, nlm, nobs, obs_lm, obs_kf, obs_cam, uv, plan);
    const int nslots = (int)plan.kf_of_slot.size();
    std::vector<PoseState> poses((size_t)nslots);
    std::vector<uint8_t> slot_moved((size_t)nslots);
    bool any_moved = false;
    for (int s = 0; s < nslots; s++) {
        const size_t k = (size_t)plan.kf_of_slot[s];
        pose_load(poses[s], kf_R + 9 * k, kf_t + 3 * k);
        slot_moved[s] = moved[k] ? 1 : 0;
        any_moved = any_moved || moved[k];
    }
    auto give = [&](const RetriOut *out) {
        for (int j = 0; j < nlm; j++) {
            if (pts_out) memcpy(pts_out + 3 * (size_t)j, out[j].X, 3 * sizeof(double));
            if (diff_norm) diff_norm[j] = out[j].diff_norm;
            if (n_views) n_views[j] = out[j].n_views;
            if (verdict) verdict[j] = out[j].verdict;
            res->counts[out[j].verdict]++;
            if (failed(out[j].verdict)) res->n_pairs += (int32_t)m->obs[lids[j]].size();
        }
    };
    if (!any_moved) {   // (no observation among them: nothing runs)
        std::vector<RetriOut> out((size_t)nlm);
        for (int j = 0; j < nlm; j++) {
            memset(&out[j], 0, sizeof(RetriOut));
            out[j].n_views = plan.obs_first[j + 1] - plan.obs_first[j];
            out[j].verdict = MCORB_RETRI_NOT_SELECTED;
        }
        give(out.data());
        return MCORB_OK;
    }

    RetriJob job;
    memset(&job, 0, sizeof(job));
    memcpy(job.cams, cams, (size_t)ncams * sizeof(mcorb_track_cam));
    job.rank_tol = params->rank_tol;
    job.far_threshold = params->landmark_distance_threshold;
    job.outlier_threshold = params->dynamic_outlier_threshold;
    job.max_diff = params->max_diff;
    job.ncams = ncams;
    job.nslots = nslots;
    job.nlm = nlm;
    job.nobs = nobs;
    std::vector<RetriOut> host_out;
    const RetriOut *out = nullptr;
    const RetriLayout L((size_t)nslots, (size_t)nlm, (size_t)nobs);
    mcorb_lmap::Retri &b = m->retri;
    if (m->device >= 0) {
        HIPCHK(hipSetDevice(m->device));
        (void)hipGetLastError();   // (a stale error of this thread is not this call's)
        TRY(b.reserve(L.p.total, (size_t)nslots * ncams, (size_t)nlm));
    } else {
        host_out.resize((size_t)nlm);
    }
    // the whole computation, the store written iff with_apply
    auto run = [&](bool with_apply) -> int {
        job.apply = with_apply ? 1 : 0;
        if (m->device < 0) {
            retri_run_serial(job, plan, poses.data(), slot_moved.data(), lids, m->geom.data(), host_out.data());
            out = host_out.data();
            return MCORB_OK;
        }
        const Staged &s = b.in;
        *s.host<RetriJob>(L.job) = job;
        memcpy(s.host<PoseState>(L.poses), poses.data(), (size_t)nslots * sizeof(PoseState));
        memcpy(s.host<uint8_t>(L.moved), slot_moved.data(), (size_t)nslots);
        memcpy(s.host<int32_t>(L.lids), lids, (size_t)nlm * sizeof(int32_t));
        memcpy(s.host<RetriObs>(L.obs), plan.obs.data(), (size_t)nobs * sizeof(RetriObs));
        memcpy(s.host<int32_t>(L.obs_first), plan.obs_first.data(), ((size_t)nlm + 1) * sizeof(int32_t));
        RetriArgs a;
        a.job = s.dev<const RetriJob>(L.job);
        a.poses = s.dev<const PoseState>(L.poses);
        a.moved = s.dev<const uint8_t>(L.moved);
        a.lids = s.dev<const int32_t>(L.lids);
        a.obs = s.dev<const RetriObs>(L.obs);
        a.obs_first = s.dev<const int32_t>(L.obs_first);
        a.views = b.d_views;
        a.geom = m->d_geom;
        a.out = b.h_out;
        a.nviews = nslots * ncams;
        a.nlm = nlm;
        hipStream_t st = m->st;
        Submission sub(st);
        b.in.upload(sub, L.p.total);
        using B = mcorb_lmap::Retri;
        sub.run(b.chain, B::kViews, [&] { launch_retri_views(st, a); });
        sub.run(b.chain, B::kSolve, [&] { launch_retri_solve(st, a); });
        sub.mark(b.chain, B::kSolve + 1);
        TRY(sub.wait());
        b.chain.read();
        out = b.h_out.get();
        return MCORB_OK;
    };
    auto count_pairs = [&] {
        size_t total = 0;
        for (int j = 0; j < nlm; j++)
            if (failed(out[j].verdict)) total += m->obs[lids[j]].size();
        return total;
    };
    res->launched = m->device >= 0 ? 1 : 0;
    if (!apply) {
        TRY(run(false));
        give(out);
        return MCORB_OK;
    }
    // apply: the pairs must fit before a point is written.  They fit whatever the verdicts are when cap holds every named
    // landmark's; otherwise a pass in report mode counts them first (the verdicts do not depend on the mode)
    size_t bound = 0;
    for (int j = 0; j < nlm; j++) bound += m->obs[lids[j]].size();
    if (bound > (size_t)cap) {
        TRY(run(false));
        const size_t total = count_pairs();
        if (total > (size_t)cap) {
            res->n_pairs = (int32_t)total;
            return fail(MCORB_E_CAP, "output too small");
        }
    }
    TRY(run(true));
    give(out);
    std::vector<int32_t> dead;
    for (int j = 0; j < nlm; j++)
        if (failed(out[j].verdict)) dead.push_back(lids[j]);
    return lmap_delete_checked(m, dead.data(), (int)dead.size(), kfs, feats);
}

int mcorb_lmap_last_retri_timing(mcorb_lmap *m, float us[MCORB_RETRI_SPANS])
{
    TRY(check_lmap_handle(m, "lmap last_retri_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < MCORB_RETRI_SPANS; k++) us[k] = m->retri.chain.us[k];
    return MCORB_OK;
}

}  // extern "C"
