// mcorb_ba.cpp -- mcorb_lmap_bundle_adjust: the local bundle adjustment over rig keyframes and landmarks (mcorb_ba.h; DESIGN.md
// section 9o).  The host checks the arguments, sorts the observations by (landmark, keyframe) and builds the per-landmark tables
// (ba_plan).  A device store then queues the whole chain of kernels (mcorb_ba_gpu.hip) in one Submission -- max_iterations
// iterations, of which those behind the loop's end return at once: the loop's record lives in device memory and no decision is
// taken on the host -- and waits once; the result lands in host-mapped memory.  A host-only store runs ba_run_serial, the same
// arithmetic in the same order, so the two agree bit for bit.  The store is read (the points of lids) and never written.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_kernels.h"
#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

int fail(int code, const char *what) { set_error(std::string("lmap bundle_adjust: ") + what); return code; }

}  // namespace

extern "C" {

int mcorb_lmap_bundle_adjust(mcorb_lmap *m, int nkf, const double *kf_R, const double *kf_t, const uint8_t *fixed, int ncams,
                             const mcorb_track_cam *cams, int nlm, const int32_t *lids, const double *pts, int nobs,
                             const int32_t *obs_kf, const int32_t *obs_cam, const int32_t *obs_lm, const float *uv,
                             const int32_t *octave, const mcorb_ba_params *params, double *R_out, double *t_out, double *pts_out,
                             mcorb_ba_result *res, uint8_t *inlier)
{
    TRY(check_lmap(m, "lmap bundle_adjust"));
    if (!kf_R || !kf_t || !fixed || !cams || !params || !R_out || !t_out || !res) return fail(MCORB_E_ARG, "bad argument");
    if (nkf < 1 || nkf > MCORB_BA_MAX_KF) return fail(MCORB_E_ARG, "1 .. MCORB_BA_MAX_KF keyframes");
    if (ncams < 1 || ncams > MCORB_MAX_CAMS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_CAMS cameras");
    if (nlm < 0 || nlm > MCORB_BA_MAX_LANDMARKS) return fail(MCORB_E_ARG, "0 .. MCORB_BA_MAX_LANDMARKS landmarks");
    if (nobs < 0 || nobs > MCORB_BA_MAX_OBS) return fail(MCORB_E_ARG, "0 .. MCORB_BA_MAX_OBS observations");
    if (params->nlevels < 1 || params->nlevels > MCORB_MAX_LEVELS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_LEVELS levels");
    if (params->max_iterations < 1 || params->max_iterations > 100) return fail(MCORB_E_ARG, "1 .. 100 iterations");
    for (int l = 0; l < params->nlevels; l++)
        if (!(params->sigma[l] > 0)) return fail(MCORB_E_ARG, "a sigma that is not > 0");
    if ((lids != nullptr) == (pts != nullptr)) return fail(MCORB_E_ARG, "exactly one of lids and pts");
    if (nlm && !pts_out) return fail(MCORB_E_ARG, "bad argument");
    if (nobs && (!obs_kf || !obs_cam || !obs_lm || !uv || !octave)) return fail(MCORB_E_ARG, "bad argument");
    for (int i = 0; i < nobs; i++) {
        if (obs_kf[i] < 0 || obs_kf[i] >= nkf) return fail(MCORB_E_ARG, "a keyframe index outside the window");
        if (obs_cam[i] < 0 || obs_cam[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
        if (obs_lm[i] < 0 || obs_lm[i] >= nlm) return fail(MCORB_E_ARG, "a landmark index outside the call's list");
        if (octave[i] < 0 || octave[i] >= params->nlevels) return fail(MCORB_E_ARG, "an octave outside the levels");
    }
    if (lids)
        for (int j = 0; j < nlm; j++)
            if (lids[j] < 0 || lids[j] >= m->max_landmarks) return fail(MCORB_E_ARG, "landmark id outside the store");
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track.pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");
    if (lids)
        for (int j = 0; j < nlm; j++)
            if (!(m->flags[lids[j]] & kHasPt)) return fail(MCORB_E_STATE, "a landmark has no point");

    BaJob job;
    memset(&job, 0, sizeof(job));
    memcpy(job.cams, cams, (size_t)ncams * sizeof(mcorb_track_cam));
    for (int l = 0; l < params->nlevels; l++) job.inv_s[l] = 1.0 / params->sigma[l];
    job.huber_k = sqrt(5.991);   // the double nearest the root: IEEE's sqrt on the host
    job.nkf = nkf;
    job.ncams = ncams;
    job.nlm = nlm;
    job.nobs = nobs;
    job.max_iterations = params->max_iterations;
    std::vector<PoseState> poses((size_t)nkf);
    for (int k = 0; k < nkf; k++) {
        memcpy(poses[k].R, kf_R + 9 * (size_t)k, sizeof(poses[k].R));
        memcpy(poses[k].t, kf_t + 3 * (size_t)k, sizeof(poses[k].t));
    }
    auto give_poses = [&](const PoseState *P) {
        for (int k = 0; k < nkf; k++) {
            memcpy(R_out + 9 * (size_t)k, P[k].R, sizeof(P[k].R));
            memcpy(t_out + 3 * (size_t)k, P[k].t, sizeof(P[k].t));
        }
    };
    if (m->device < 0 || nobs == 0) {
        // (a device store's points of lids are read here only without observations: the state goes back as it came)
        std::vector<double> X((size_t)nlm * 3);
        if (lids && m->device >= 0 && nlm) {
            HIPCHK(hipSetDevice(m->device));
            std::vector<double> geom((size_t)m->max_landmarks * 6);
            HIPCHK(hipMemcpy(geom.data(), m->d_geom, geom.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int j = 0; j < nlm; j++) memcpy(&X[3 * (size_t)j], &geom[(size_t)lids[j] * 6], 3 * sizeof(double));
        } else {
            for (int j = 0; j < nlm; j++)
                memcpy(&X[3 * (size_t)j], lids ? &m->geom[(size_t)lids[j] * 6] : pts + 3 * (size_t)j, 3 * sizeof(double));
        }
        memset(res, 0, sizeof(*res));
        res->status = MCORB_BA_NO_OBS;
        if (nobs) {
            BaPlan plan;
            ba_plan(job, fixed, obs_kf, obs_cam, obs_lm, uv, octave, plan);
            std::vector<uint8_t> flags((size_t)nobs);
            ba_run_serial(job, plan, poses.data(), X.data(), *res, flags.data());
            if (inlier) memcpy(inlier, flags.data(), (size_t)nobs);
        }
        give_poses(poses.data());
        if (nlm) memcpy(pts_out, X.data(), (size_t)nlm * 3 * sizeof(double));
        return MCORB_OK;
    }

    BaPlan plan;
    ba_plan(job, fixed, obs_kf, obs_cam, obs_lm, uv, octave, plan);
    mcorb_lmap::Ba &b = m->ba;
    HIPCHK(hipSetDevice(m->device));
    (void)hipGetLastError();   // (a stale error of this thread is not this call's)
    const BaLayout L((size_t)nkf, (size_t)nlm, (size_t)nobs, lids != nullptr);
    TRY(b.reserve(L.p.total, (size_t)nlm, (size_t)nobs, (size_t)job.nviews));
    const Staged &s = b.in;
    *s.host<BaJob>(L.job) = job;
    memcpy(s.host<PoseState>(L.poses), poses.data(), (size_t)nkf * sizeof(PoseState));
    if (lids)
        memcpy(s.host<int32_t>(L.pt), lids, (size_t)nlm * sizeof(int32_t));
    else
        memcpy(s.host<double>(L.pt), pts, (size_t)nlm * 3 * sizeof(double));
    memcpy(s.host<BaObs>(L.obs), plan.obs.data(), (size_t)nobs * sizeof(BaObs));
    memcpy(s.host<int32_t>(L.obs_first), plan.obs_first.data(), ((size_t)nlm + 1) * sizeof(int32_t));
    memcpy(s.host<int32_t>(L.view_first), plan.view_first.data(), ((size_t)nlm + 1) * sizeof(int32_t));
    memcpy(s.host<int8_t>(L.slot), plan.slot.data(), (size_t)nlm * MCORB_BA_MAX_KF);
    BaArgs a;
    a.job = s.dev<const BaJob>(L.job);
    a.poses_in = s.dev<const PoseState>(L.poses);
    a.lids = lids ? s.dev<const int32_t>(L.pt) : nullptr;
    a.pts_in = lids ? nullptr : s.dev<const double>(L.pt);
    a.geom = m->d_geom;
    a.obs = s.dev<const BaObs>(L.obs);
    a.obs_first = s.dev<const int32_t>(L.obs_first);
    a.view_first = s.dev<const int32_t>(L.view_first);
    a.slot = s.dev<const int8_t>(L.slot);
    a.poses = b.d_poses;
    a.pts = b.d_pts;
    a.V = b.d_V;
    a.gp = b.d_gp;
    a.cost = b.d_cost;
    a.views = b.d_views;
    a.diag = b.d_diag;
    a.pairs = b.d_pairs;
    a.delta = b.d_delta;
    a.rec = b.d_rec;
    a.count = b.d_count;
    a.out = b.h_out;
    a.out_pts = b.h_pts;
    a.flags = b.h_flags;
    a.nkf = nkf;
    a.nlm = nlm;
    a.nobs = nobs;
    a.nsys = job.nsys;
    a.max_iterations = job.max_iterations;
    hipStream_t st = m->st;
    Submission sub(st);
    b.in.upload(sub, L.p.total);
    using B = mcorb_lmap::Ba;
    sub.run(b.chain, B::kBegin, [&] { launch_ba_begin(st, a); });
    sub.run([&] { launch_ba_linearize(st, a); });
    sub.run([&] { launch_ba_accept(st, a, true); });
    for (int it = 0; it < job.max_iterations; it++) {
        // (the spans: the first iteration kernel by kernel, the others as one piece)
        if (it > 0) {
            if (it == 1) sub.mark(b.chain, B::kRest);
            sub.run([&] { launch_ba_linearize(st, a); });
        }
        if (it == 0) sub.mark(b.chain, B::kSchur);
        sub.run([&] { launch_ba_schur(st, a); });
        if (it == 0) sub.mark(b.chain, B::kSolve);
        sub.run([&] { launch_ba_solve(st, a); });
        if (it == 0) sub.mark(b.chain, B::kUpdate);
        sub.run([&] { launch_ba_update(st, a); });
        if (it == 0) sub.mark(b.chain, B::kAccept);
        sub.run([&] { launch_ba_accept(st, a, false); });
    }
    if (job.max_iterations == 1) sub.mark(b.chain, B::kRest);
    sub.run(b.chain, B::kFinal, [&] { launch_ba_final(st, a); });
    sub.mark(b.chain, B::kFinal + 1);
    TRY(sub.wait());
    b.chain.read();
    const BaOut &out = *b.h_out.get();
    *res = out.res;
    // an iteration is a linearization (but the first), k_ba_schur (with a system), k_ba_solve, k_ba_update and k_ba_accept
    const int idle = job.max_iterations - res->iterations;
    b.last_idle = idle * (job.nsys ? 5 : 4);
    give_poses(out.poses);
    if (nlm) memcpy(pts_out, b.h_pts.get(), (size_t)nlm * 3 * sizeof(double));
    if (inlier) memcpy(inlier, b.h_flags.get(), (size_t)nobs);
    return MCORB_OK;
}

int mcorb_lmap_last_ba_timing(mcorb_lmap *m, float us[MCORB_BA_SPANS], int32_t *launches_idle)
{
    TRY(check_lmap_handle(m, "lmap last_ba_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < MCORB_BA_SPANS; k++) us[k] = m->ba.chain.us[k];
    if (launches_idle) *launches_idle = m->ba.last_idle;
    return MCORB_OK;
}

int mcorb_ba_eval(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam, const float *uv, const double *pts,
                  const double *sigma, const double *R, const double *t, double *r, double *J, double *JX, double *w)
{
    if (n < 0 || ncams < 1 || ncams > MCORB_MAX_CAMS || !cams || !R || !t || (n && (!cam || !uv || !pts || !sigma || !r || !J || !JX || !w)))
        return fail(MCORB_E_ARG, "bad argument");
    for (int i = 0; i < n; i++) {
        if (cam[i] < 0 || cam[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
        if (!(sigma[i] > 0)) return fail(MCORB_E_ARG, "a sigma that is not > 0");
    }
    PoseState P;
    memcpy(P.R, R, sizeof(P.R));
    memcpy(P.t, t, sizeof(P.t));
    const double k = sqrt(5.991);
    for (int i = 0; i < n; i++) {
        double Ji[2][6], JXi[2][3], rho;
        ba_observation<true>(cams[cam[i]], P, pts + 3 * (size_t)i, uv[2 * i], uv[2 * i + 1], 1.0 / sigma[i], k, r[2 * (size_t)i],
                             r[2 * (size_t)i + 1], Ji, JXi, w[i], rho);
        memcpy(J + 12 * (size_t)i, Ji, sizeof(Ji));
        memcpy(JX + 6 * (size_t)i, JXi, sizeof(JXi));
    }
    return MCORB_OK;
}

}  // extern "C"
