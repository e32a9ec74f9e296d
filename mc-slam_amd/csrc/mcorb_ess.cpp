// mcorb_ess.cpp -- the pose of one camera between two frames from 2D-2D matches: mcorb_lmap_essential_pose, what the reference
// gets from cv::findEssentialMat and cv::recoverPose in the one-camera arm of its bootstrap (MCSlam/src/FrontEnd.cpp:2591-2628).
// A device store runs k_ess_hypotheses, k_ess_score, k_ess_pick and k_ess_finish (mcorb_ess_gpu.hip) in one submission on the
// store's stream with one wait; the record and the flags land in host-mapped memory.  A host-only store runs the header
// (mcorb_ess.h) serially, so the two agree bit for bit.  Recalled from OpenCV: the Sampson distance and the cheirality vote;
// stated: the draws, the five-point solver, no adaptive stop, the midpoint inside the vote, the rotations from E (DESIGN.md
// section 9m).  mcorb_lmap_essential_pose_polished is the same call (essential_pose below, with polish parameters) with
// k_ess_finish's record and flags kept in device memory and k_ess_fit behind it: the polish of the winner over its inliers
// (mcorb_ess_polish.h), stated too.  A plain call touches none of the polish's buffers.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

int fail(int code, const char *what) { set_error(std::string("lmap essential_pose: ") + what); return code; }

void fill_job(EssJob &job, const mcorb_track_cam &cam)
{
    memset(&job, 0, sizeof(job));
    job.fx = cam.fx;
    job.fy = cam.fy;
    job.s = cam.s;
    job.u0 = cam.u0;
    job.v0 = cam.v0;
}

void fill_obs(EssObs *obs, int n, const float *uv1, const float *uv2)
{
    for (int i = 0; i < n; i++) obs[i] = EssObs{uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1]};
}

int check_polish(const mcorb_ess_polish_params *pp)
{
    if (pp->rounds < 1 || pp->rounds > MCORB_ESS_POLISH_ROUNDS) return fail(MCORB_E_ARG, "1 .. MCORB_ESS_POLISH_ROUNDS rounds");
    if (pp->max_iterations < 1 || pp->max_iterations > MCORB_ESS_POLISH_MAX_ITERATIONS)
        return fail(MCORB_E_ARG, "1 .. MCORB_ESS_POLISH_MAX_ITERATIONS polish iterations");
    return MCORB_OK;
}

// the polish record of a call in which no round runs
void begin_record(EssPolish &rec, const EssOut &out)
{
    PoseState P;
    memcpy(P.R, out.R, sizeof(P.R));
    memcpy(P.t, out.t, sizeof(P.t));
    ess_polish_begin(rec, P, out.E, out.n_ransac_inliers, out.n_inliers);
}

// ess_polish_serial with its scratch, on a record: out's pose, E and counts and the flags are the current ones in, the accepted
// ones out; member: round 1's members, a copy the rounds overwrite
void polish_host(const EssPt *pts, int S, double threshold2, double distance, double inv_thr, const mcorb_ess_polish_params &pp, EssOut &out,
                 uint8_t *flags, std::vector<uint8_t> member, EssPolish &rec)
{
    std::vector<uint8_t> scratch((size_t)S);
    std::vector<double> lanes((size_t)MCORB_POSE_LANES * kEssFitSums);
    PoseState P;
    memcpy(P.R, out.R, sizeof(P.R));
    memcpy(P.t, out.t, sizeof(P.t));
    ess_polish_serial(pts, S, threshold2, distance, inv_thr, pp.rounds, pp.max_iterations, P, out.E, out.n_ransac_inliers, out.n_inliers, flags,
                      member.data(), scratch.data(), reinterpret_cast<double (*)[kEssFitSums]>(lanes.data()), rec);
    memcpy(out.R, P.R, sizeof(P.R));
    memcpy(out.t, P.t, sizeof(P.t));
}

// both entries; who: the entry's name in check_lmap's errors.  pp: the polish parameters and polish, its record, or neither: a plain
// call, whose k_ess_finish writes the host-mapped record and flags itself
int essential_pose(mcorb_lmap *m, const char *who, int n, const float *uv1, const float *uv2, const mcorb_track_cam *cam,
                   const mcorb_ess_params *params, const mcorb_ess_polish_params *pp, mcorb_ess_result *res, uint8_t *inlier,
                   mcorb_ess_polish *polish)
{
    TRY(check_lmap(m, who));
    if (!params || !res || !cam || n < 0 || (n && (!uv1 || !uv2))) return fail(MCORB_E_ARG, "bad argument");
    if (!positive(params->threshold_px)) return fail(MCORB_E_ARG, "a threshold that is not finite and positive");
    if (!positive(params->distance_thresh)) return fail(MCORB_E_ARG, "a distance that is not finite and positive");
    if (!positive(cam->fx) || !positive(cam->fy)) return fail(MCORB_E_ARG, "a focal length that is not finite and positive");
    if (params->max_iterations < 1 || params->max_iterations > MCORB_ESS_MAX_ITERATIONS)
        return fail(MCORB_E_ARG, "1 .. MCORB_ESS_MAX_ITERATIONS iterations");
    if (pp) TRY(check_polish(pp));
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track.pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");

    const int S = n, H = params->max_iterations;
    const size_t slots = (size_t)H * kEssRoots;
    EssJob job;
    fill_job(job, *cam);
    const double thr = params->threshold_px / ((cam->fx + cam->fy) / 2.0);
    job.threshold2 = thr * thr;
    job.distance = params->distance_thresh;
    job.seed = params->seed;
    job.S = S;
    job.H = H;
    const double inv_thr = ess_fit_scale(params->threshold_px, cam->fx, cam->fy);   // (the polish's)

    EssOut out;
    EssPolish rec;
    std::vector<uint8_t> flags((size_t)n);
    mcorb_lmap::Ess &b = m->ess;
    if (S == 0) {
        no_obs(out, MCORB_ESS_NO_OBS);
        out.best_hypothesis = out.best_root = -1;
        if (pp) begin_record(rec, out);
    } else if (m->device < 0) {
        std::vector<EssObs> obs((size_t)n);
        fill_obs(obs.data(), n, uv1, uv2);
        std::vector<int32_t> samples((size_t)H * kEssSample), count(slots);
        std::vector<EssPt> pts((size_t)S);
        b.host_models.resize(slots);
        ess_run_serial(job, obs.data(), b.host_models.data(), samples.data(), count.data(), pts.data(), out, flags.data());
        b.host_count.swap(count);
        b.last_hyp = H;
        if (pp && out.status == MCORB_ESS_OK)
            polish_host(pts.data(), S, job.threshold2, job.distance, inv_thr, *pp, out, flags.data(), flags, rec);
        else if (pp)
            begin_record(rec, out);
    } else {
        HIPCHK(hipSetDevice(m->device));
        (void)hipGetLastError();   // (a stale error of this thread is not this call's)
        const EssLayout L((size_t)n);
        TRY(b.reserve(L.p.total, (size_t)n, (size_t)H));
        if (pp) TRY(b.reserve_polish((size_t)n));
        *b.in.host<EssJob>(L.job) = job;
        fill_obs(b.in.host<EssObs>(L.obs), n, uv1, uv2);
        hipStream_t st = m->st;
        EssArgs a;
        a.job = b.in.dev<const EssJob>(L.job);
        a.obs = b.in.dev<const EssObs>(L.obs);
        a.models = b.d_models;
        a.samples = b.d_samples;
        a.valid = b.d_valid;
        a.count = b.d_count;
        a.cheir = b.d_count.get() + slots;
        a.pick = b.d_pick;
        // (polished: k_ess_finish's record and flags stay in device memory, k_ess_fit reads nothing across the link)
        a.out = pp ? b.d_out.get() : b.h_out.get();
        a.flags = pp ? b.d_member.get() : b.h_flags.get();
        Submission sub(st);
        b.in.upload(sub, L.p.total);
        sub.fill(b.d_count, 0, (slots + 4) * sizeof(int32_t));   // (the four votes lie behind the counts)
        sub.run(b.kernels, 0, [&] { launch_ess_hypotheses(st, a, H); });
        sub.run(b.kernels, 1, [&] { launch_ess_score(st, a, S, H); });
        sub.run(b.kernels, 2, [&] { launch_ess_pick(st, a, S); });
        sub.run(b.kernels, 3, [&] { launch_ess_finish(st, a, S); });
        sub.mark(b.kernels, 4);
        if (pp) {
            const EssFitArgs f{a.job, a.obs, b.d_out, b.d_member, pp->rounds, pp->max_iterations, inv_thr, b.h_out, b.h_flags, b.h_polish};
            sub.run(b.fit, 0, [&] { launch_ess_fit(st, f); });
            sub.mark(b.fit, 1);
        }
        TRY(sub.wait());
        b.kernels.read();
        if (pp) b.fit.read();
        b.last_hyp = H;
        out = *b.h_out.get();
        if (pp) rec = *b.h_polish.get();
        memcpy(flags.data(), b.h_flags.get(), (size_t)n);
    }

    memset(res, 0, sizeof(*res));
    memcpy(res->R, out.R, sizeof(out.R));
    memcpy(res->t, out.t, sizeof(out.t));
    memcpy(res->E, out.E, sizeof(out.E));
    res->status = out.status;
    res->n_matches = n;
    res->n_ransac_inliers = out.n_ransac_inliers;
    res->n_inliers = out.n_inliers;
    res->best_hypothesis = out.best_hypothesis;
    res->best_root = out.best_root;
    memcpy(res->sample, out.sample, sizeof(res->sample));
    res->n_models = out.n_models;
    memcpy(res->cheirality, out.cheirality, sizeof(res->cheirality));
    if (pp) *polish = rec;
    if (inlier && n) memcpy(inlier, flags.data(), (size_t)n);
    return MCORB_OK;
}

}  // namespace

extern "C" {

int mcorb_lmap_essential_pose(mcorb_lmap *m, int n, const float *uv1, const float *uv2, const mcorb_track_cam *cam,
                              const mcorb_ess_params *params, mcorb_ess_result *res, uint8_t *inlier)
{
    return essential_pose(m, "lmap essential_pose", n, uv1, uv2, cam, params, nullptr, res, inlier, nullptr);
}

int mcorb_lmap_last_essential_timing(mcorb_lmap *m, float us[4], int *n_hyp)
{
    TRY(check_lmap_handle(m, "lmap last_essential_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < 4; k++) us[k] = m->ess.kernels.us[k];
    if (n_hyp) *n_hyp = m->ess.last_hyp;
    return MCORB_OK;
}

int mcorb_lmap_essential_pose_polished(mcorb_lmap *m, int n, const float *uv1, const float *uv2, const mcorb_track_cam *cam,
                                       const mcorb_ess_params *params, const mcorb_ess_polish_params *pp, mcorb_ess_result *res,
                                       uint8_t *inlier, mcorb_ess_polish *polish)
{
    TRY(check_lmap(m, "lmap essential_pose_polished"));
    if (!pp || !polish) return fail(MCORB_E_ARG, "bad argument");
    return essential_pose(m, "lmap essential_pose_polished", n, uv1, uv2, cam, params, pp, res, inlier, polish);
}

int mcorb_lmap_last_essential_timing5(mcorb_lmap *m, float us[5], int *n_hyp)
{
    TRY(check_lmap_handle(m, "lmap last_essential_timing5"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < 4; k++) us[k] = m->ess.kernels.us[k];
    us[4] = m->ess.fit.us[0];
    if (n_hyp) *n_hyp = m->ess.last_hyp;
    return MCORB_OK;
}

int mcorb_ess_polish_run(const mcorb_track_cam *cam, int n, const double *uv1, const double *uv2, const uint8_t *member, const double *R,
                         const double *t, double threshold_px, double distance_thresh, const mcorb_ess_polish_params *pp,
                         mcorb_ess_polish *polish, double *R_out, double *t_out, double *E_out, uint8_t *inlier)
{
    if (!cam || n < 0 || !R || !t || !pp || !polish || !R_out || !t_out || !E_out || (n && (!uv1 || !uv2 || !member || !inlier)))
        return fail(MCORB_E_ARG, "bad argument");
    if (!positive(threshold_px)) return fail(MCORB_E_ARG, "a threshold that is not finite and positive");
    if (!positive(distance_thresh)) return fail(MCORB_E_ARG, "a distance that is not finite and positive");
    if (!positive(cam->fx) || !positive(cam->fy)) return fail(MCORB_E_ARG, "a focal length that is not finite and positive");
    TRY(check_polish(pp));
    EssJob job;
    fill_job(job, *cam);
    const double thr = threshold_px / ((cam->fx + cam->fy) / 2.0);
    job.threshold2 = thr * thr;
    job.distance = distance_thresh;
    std::vector<EssPt> pts((size_t)n);
    for (int i = 0; i < n; i++) ess_point(job, uv1[2 * (size_t)i], uv1[2 * (size_t)i + 1], uv2[2 * (size_t)i], uv2[2 * (size_t)i + 1], pts[i]);
    EssOut out;
    memset(&out, 0, sizeof(out));
    memcpy(out.R, R, sizeof(out.R));
    memcpy(out.t, t, sizeof(out.t));
    PoseState P;
    memcpy(P.R, R, sizeof(P.R));
    memcpy(P.t, t, sizeof(P.t));
    ess_fit_E(P, out.E);
    std::vector<uint8_t> flags((size_t)n), mem((size_t)n);
    for (int i = 0; i < n; i++) {
        bool within, flag;
        ess_fit_test(P, out.E, pts[i], job.threshold2, job.distance, within, flag);
        flags[i] = flag ? 1 : 0;
        out.n_ransac_inliers += within ? 1 : 0;
        out.n_inliers += flag ? 1 : 0;
        mem[i] = member[i] ? 1 : 0;
    }
    polish_host(pts.data(), n, job.threshold2, job.distance, ess_fit_scale(threshold_px, cam->fx, cam->fy), *pp, out, flags.data(), mem, *polish);
    memcpy(R_out, out.R, sizeof(out.R));
    memcpy(t_out, out.t, sizeof(out.t));
    memcpy(E_out, out.E, sizeof(out.E));
    if (n) memcpy(inlier, flags.data(), (size_t)n);
    return MCORB_OK;
}

int mcorb_lmap_last_essential_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, double *models, int cap, int *n_slots)
{
    const auto copy_out = [&](int s, const EssModel &M) { if (models) memcpy(models + 9 * (size_t)s, M.E, sizeof(M.E)); };
    const auto host_valid = [&](const mcorb_lmap::Ess &b, int s) { copy_out(s, b.host_models[s]); return b.host_models[s].valid; };
    return last_counts<EssModel>(m, &mcorb_lmap::ess, kEssRoots, "lmap last_essential_counts", fail, count, valid, cap, n_slots, host_valid,
                                 copy_out);
}

int mcorb_ess_solve(const mcorb_track_cam *cam, const double *uv1, const double *uv2, double *E, double *z)
{
    if (!cam || !uv1 || !uv2 || !E) return fail(MCORB_E_ARG, "bad argument");
    EssJob job;
    fill_job(job, *cam);
    double d1[kEssSample][3], d2[kEssSample][3];
    for (int j = 0; j < kEssSample; j++) {
        EssPt p;
        ess_point(job, uv1[2 * j], uv1[2 * j + 1], uv2[2 * j], uv2[2 * j + 1], p);
        ess_bearing(p.x1, p.y1, d1[j]);
        ess_bearing(p.x2, p.y2, d2[j]);
    }
    return ess_solve5(d1, d2, E, z);
}

int mcorb_dev_ess_solve_selftest(int device, int n, const mcorb_track_cam *cam, const double *uv1, const double *uv2, int32_t *count, double *E,
                                 double *z)
{
    if (n < 0 || (n && (!cam || !uv1 || !uv2 || !count || !E || !z))) return fail(MCORB_E_ARG, "bad argument");
    if (n == 0) return MCORB_OK;
    TRY(selftest_device(device));
    const size_t N = (size_t)n, slots = N * kEssRoots;
    std::vector<EssJob> jobs(N);
    for (size_t i = 0; i < N; i++) fill_job(jobs[i], cam[i]);
    DevBuf<EssJob> d_jobs;
    DevBuf<double> d_uv1, d_uv2, d_z;
    DevBuf<EssModel> d_models;
    DevBuf<int32_t> d_valid;
    TRY(to_device(d_jobs, jobs.data(), N));
    TRY(to_device(d_uv1, uv1, N * 2 * kEssSample));
    TRY(to_device(d_uv2, uv2, N * 2 * kEssSample));
    TRY(d_models.alloc(slots));
    TRY(d_valid.alloc(slots));
    TRY(d_z.alloc(slots));
    launch_ess_solve_selftest(nullptr, d_jobs, d_uv1, d_uv2, n, d_models, d_valid, d_z);
    HIPCHK(hipGetLastError());
    std::vector<EssModel> models(slots);
    std::vector<int32_t> valid(slots);
    TRY(from_device(models.data(), d_models, slots));
    TRY(from_device(valid.data(), d_valid, slots));
    TRY(from_device(z, d_z, slots));
    for (size_t i = 0; i < N; i++) {
        count[i] = 0;
        for (int c = 0; c < kEssRoots; c++) {
            const EssModel &M = models[kEssRoots * i + c];
            memcpy(E + 9 * (kEssRoots * i + c), M.E, sizeof(M.E));   // (zero without a model)
            count[i] += valid[kEssRoots * i + c] ? 1 : 0;           // (the dense flags k_ess_pick walks)
        }
    }
    return MCORB_OK;
}

int mcorb_ess_eval(const mcorb_track_cam *cam, int n, const double *uv1, const double *uv2, const double *E, double *err)
{
    if (!cam || n < 0 || !E || (n && (!uv1 || !uv2 || !err))) return fail(MCORB_E_ARG, "bad argument");
    EssJob job;
    fill_job(job, *cam);
    for (int i = 0; i < n; i++) {
        EssPt p;
        ess_point(job, uv1[2 * (size_t)i], uv1[2 * (size_t)i + 1], uv2[2 * (size_t)i], uv2[2 * (size_t)i + 1], p);
        err[i] = pose_default_nan(ess_sampson(E, p));
    }
    return MCORB_OK;
}

int mcorb_ess_decompose(const double *E, double *Rp, double *Rm, double *t, const mcorb_track_cam *cam, int n, const double *uv1,
                        const double *uv2, double *depth)
{
    if (!E || !Rp || !Rm || !t || n < 0 || (n && (!cam || !uv1 || !uv2 || !depth))) return fail(MCORB_E_ARG, "bad argument");
    EssPick P;
    memset(&P, 0, sizeof(P));
    ess_decompose(E, P.Rp, P.Rm, P.t);
    memcpy(Rp, P.Rp, sizeof(P.Rp));
    memcpy(Rm, P.Rm, sizeof(P.Rm));
    memcpy(t, P.t, sizeof(P.t));
    if (!n) return MCORB_OK;
    EssJob job;
    fill_job(job, *cam);
    for (int i = 0; i < n; i++) {
        EssPt p;
        ess_point(job, uv1[2 * (size_t)i], uv1[2 * (size_t)i + 1], uv2[2 * (size_t)i], uv2[2 * (size_t)i + 1], p);
        for (int c = 0; c < 4; c++) {
            const double tc[3] = {c < 2 ? P.t[0] : -P.t[0], c < 2 ? P.t[1] : -P.t[1], c < 2 ? P.t[2] : -P.t[2]};
            double z1, z2;
            ess_depths((c & 1) ? P.Rm : P.Rp, tc, p, z1, z2);
            depth[(4 * (size_t)i + c) * 2] = pose_default_nan(z1);
            depth[(4 * (size_t)i + c) * 2 + 1] = pose_default_nan(z2);
        }
    }
    return MCORB_OK;
}

}  // extern "C"
