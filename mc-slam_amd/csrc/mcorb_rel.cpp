// mcorb_rel.cpp -- the relative rig pose between two frames by RANSAC: mcorb_lmap_relative_pose, the consensus step of
// FrontEnd::poseFromSeventeenPt (MCSlam/src/FrontEnd.cpp:4532-4657) and LoopCloser::checkEssentialMatrix (LoopCloser.cpp:353-446).
// A device store runs k_rel_hypotheses, k_rel_score and k_rel_pick (mcorb_rel_gpu.hip) in one submission on the store's stream
// with one wait; the records land in host-mapped memory.  A host-only store runs the header (mcorb_rel.h) serially, so the two
// agree bit for bit.  Stated rather than OpenGV's: the draws, the linear solver, no adaptive stop.
// mcorb_lmap_relative_pose_polished is the same call (relative_pose below, with polish parameters) with the pick's record and
// flags kept in device memory and k_rel_fit behind it: the polish of the winner over its inliers, stated too.  A plain call
// touches none of the polish's buffers.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

int fail(int code, const char *what) { set_error(std::string("lmap relative_pose: ") + what); return code; }

int check_cams(int n, const int32_t *cam1, const int32_t *cam2, int ncams)
{
    for (int i = 0; i < n; i++)
        if (cam1[i] < 0 || cam1[i] >= ncams || cam2[i] < 0 || cam2[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
    return MCORB_OK;
}

void fill_obs(RelObs *obs, int n, const int32_t *cam1, const float *uv1, const int32_t *cam2, const float *uv2)
{
    for (int i = 0; i < n; i++) obs[i] = RelObs{uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1], cam1[i], cam2[i]};
}

int check_polish(const mcorb_rel_polish_params *pp)
{
    if (pp->rounds < 1 || pp->rounds > MCORB_REL_POLISH_ROUNDS) return fail(MCORB_E_ARG, "1 .. MCORB_REL_POLISH_ROUNDS rounds");
    if (pp->max_iterations < 1 || pp->max_iterations > MCORB_REL_POLISH_MAX_ITERATIONS)
        return fail(MCORB_E_ARG, "1 .. MCORB_REL_POLISH_MAX_ITERATIONS polish iterations");
    return MCORB_OK;
}

// rel_polish_serial with its scratch; member: round 1's members, a copy the rounds overwrite
void polish_host(const RelRays *rays, int S, double threshold, const mcorb_rel_polish_params &pp, PoseState &P, int32_t &count,
                 uint8_t *flags, std::vector<uint8_t> member, RelPolish &rec)
{
    std::vector<uint8_t> scratch((size_t)S);
    std::vector<double> lanes((size_t)MCORB_POSE_LANES * kPoseSums);
    rel_polish_serial(rays, S, threshold, pp.rounds, pp.max_iterations, P, count, flags, member.data(), scratch.data(),
                      reinterpret_cast<double (*)[kPoseSums]>(lanes.data()), rec);
}

// both entries; who: the entry's name in check_lmap's errors.  pp: the polish parameters and polish, its record, or neither: a plain
// call, whose pick writes the host-mapped record and flags itself
int relative_pose(mcorb_lmap *m, const char *who, int n, const int32_t *cam1, const float *uv1, const int32_t *cam2, const float *uv2,
                  int ncams, const mcorb_track_cam *cams, const mcorb_rel_params *params, const mcorb_rel_polish_params *pp,
                  mcorb_rel_result *res, uint8_t *inlier, mcorb_rel_polish *polish)
{
    TRY(check_lmap(m, who));
    if (!params || !res || !cams || n < 0 || ncams < 1 || ncams > MCORB_MAX_CAMS || (n && (!cam1 || !uv1 || !cam2 || !uv2)))
        return fail(MCORB_E_ARG, "bad argument");
    if (!positive(params->threshold)) return fail(MCORB_E_ARG, "a threshold that is not finite and positive");
    if (params->max_iterations < 1 || params->max_iterations > MCORB_REL_MAX_ITERATIONS)
        return fail(MCORB_E_ARG, "1 .. MCORB_REL_MAX_ITERATIONS iterations");
    if (pp) TRY(check_polish(pp));
    TRY(check_cams(n, cam1, cam2, ncams));
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track.pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");

    const int S = n, H = params->max_iterations;
    RelJob job;
    memset(&job, 0, sizeof(job));
    memcpy(job.cams, cams, (size_t)ncams * sizeof(mcorb_track_cam));
    job.threshold = params->threshold;
    job.seed = params->seed;
    job.ncams = ncams;
    job.S = S;
    job.H = H;

    RelOut out;
    RelPolish rec;
    std::vector<uint8_t> flags((size_t)n);
    mcorb_lmap::Rel &b = m->rel;
    if (S == 0) {
        no_obs(out, MCORB_REL_NO_OBS);
        out.best = -1;
        if (pp) rel_polish_begin(rec, PoseState{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}}, 0);
    } else if (m->device < 0) {
        std::vector<RelObs> obs((size_t)n);
        fill_obs(obs.data(), n, cam1, uv1, cam2, uv2);
        std::vector<RelModel> models((size_t)H);
        std::vector<int32_t> count((size_t)H);
        std::vector<RelRays> rays((size_t)S);
        rel_run_serial(job, obs.data(), models.data(), count.data(), rays.data(), out, flags.data());
        b.host_valid.resize((size_t)H);
        for (int h = 0; h < H; h++) b.host_valid[h] = models[h].valid;
        b.host_count.swap(count);
        b.last_hyp = H;
        if (pp) {
            PoseState P;
            memcpy(P.R, out.R, sizeof(P.R));
            memcpy(P.t, out.t, sizeof(P.t));
            if (out.best >= 0) {
                polish_host(rays.data(), S, job.threshold, *pp, P, out.n_inliers, flags.data(), flags, rec);
                memcpy(out.R, P.R, sizeof(P.R));
                memcpy(out.t, P.t, sizeof(P.t));
            } else {
                rel_polish_begin(rec, P, out.n_inliers);
            }
        }
    } else {
        HIPCHK(hipSetDevice(m->device));
        (void)hipGetLastError();   // (a stale error of this thread is not this call's)
        const RelLayout L((size_t)n);
        TRY(b.reserve(L.p.total, (size_t)n, (size_t)H));
        if (pp) TRY(b.reserve_polish((size_t)n));
        *b.in.host<RelJob>(L.job) = job;
        fill_obs(b.in.host<RelObs>(L.obs), n, cam1, uv1, cam2, uv2);
        hipStream_t st = m->st;
        RelArgs a;
        a.job = b.in.dev<const RelJob>(L.job);
        a.obs = b.in.dev<const RelObs>(L.obs);
        a.models = b.d_models;
        a.count = b.d_count;
        // (polished: the pick's record and flags stay in device memory, k_rel_fit reads nothing across the link)
        a.out = pp ? b.d_pick.get() : b.h_out.get();
        a.flags = pp ? b.d_member.get() : b.h_flags.get();
        Submission sub(st);
        b.in.upload(sub, L.p.total);
        sub.fill(b.d_count, 0, (size_t)H * sizeof(int32_t));
        sub.run(b.kernels, 0, [&] { launch_rel_hypotheses(st, a, H); });
        sub.run(b.kernels, 1, [&] { launch_rel_score(st, a, S, H); });
        sub.run(b.kernels, 2, [&] { launch_rel_pick(st, a, S); });
        sub.mark(b.kernels, 3);
        if (pp) {
            const RelFitArgs f{a.job, a.obs, b.d_pick, b.d_member, pp->rounds, pp->max_iterations, b.h_out, b.h_flags, b.h_polish};
            sub.run(b.fit, 0, [&] { launch_rel_fit(st, f); });
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
    res->status = out.status;
    res->n_inliers = out.n_inliers;
    res->n_matches = n;
    res->best_hypothesis = out.best;
    memcpy(res->sample, out.sample, sizeof(res->sample));
    res->n_models = out.n_models;
    if (pp) *polish = rec;
    if (inlier && n) memcpy(inlier, flags.data(), (size_t)n);
    return MCORB_OK;
}

}  // namespace

extern "C" {

int mcorb_lmap_relative_pose(mcorb_lmap *m, int n, const int32_t *cam1, const float *uv1, const int32_t *cam2, const float *uv2, int ncams,
                             const mcorb_track_cam *cams, const mcorb_rel_params *params, mcorb_rel_result *res, uint8_t *inlier)
{
    return relative_pose(m, "lmap relative_pose", n, cam1, uv1, cam2, uv2, ncams, cams, params, nullptr, res, inlier, nullptr);
}

int mcorb_lmap_last_relative_timing(mcorb_lmap *m, float us[3], int *n_hyp)
{
    TRY(check_lmap_handle(m, "lmap last_relative_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < 3; k++) us[k] = m->rel.kernels.us[k];
    if (n_hyp) *n_hyp = m->rel.last_hyp;
    return MCORB_OK;
}

int mcorb_lmap_relative_pose_polished(mcorb_lmap *m, int n, const int32_t *cam1, const float *uv1, const int32_t *cam2, const float *uv2,
                                      int ncams, const mcorb_track_cam *cams, const mcorb_rel_params *params,
                                      const mcorb_rel_polish_params *pp, mcorb_rel_result *res, uint8_t *inlier, mcorb_rel_polish *polish)
{
    TRY(check_lmap(m, "lmap relative_pose_polished"));
    if (!pp || !polish) return fail(MCORB_E_ARG, "bad argument");
    return relative_pose(m, "lmap relative_pose_polished", n, cam1, uv1, cam2, uv2, ncams, cams, params, pp, res, inlier, polish);
}

int mcorb_lmap_last_relative_timing4(mcorb_lmap *m, float us[4], int *n_hyp)
{
    TRY(check_lmap_handle(m, "lmap last_relative_timing4"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < 3; k++) us[k] = m->rel.kernels.us[k];
    us[3] = m->rel.fit.us[0];
    if (n_hyp) *n_hyp = m->rel.last_hyp;
    return MCORB_OK;
}

int mcorb_rel_polish_run(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam1, const double *uv1, const int32_t *cam2,
                         const double *uv2, const uint8_t *member, const double *R, const double *t, double threshold,
                         const mcorb_rel_polish_params *pp, mcorb_rel_polish *polish, double *R_out, double *t_out, uint8_t *inlier)
{
    if (n < 0 || ncams < 1 || ncams > MCORB_MAX_CAMS || !cams || !R || !t || !pp || !polish || !R_out || !t_out ||
        (n && (!cam1 || !uv1 || !cam2 || !uv2 || !member || !inlier)))
        return fail(MCORB_E_ARG, "bad argument");
    if (!positive(threshold)) return fail(MCORB_E_ARG, "a threshold that is not finite and positive");
    TRY(check_polish(pp));
    TRY(check_cams(n, cam1, cam2, ncams));
    std::vector<RelRays> rays((size_t)n);
    for (int i = 0; i < n; i++) rel_rays_d(cams, cam1[i], uv1 + 2 * (size_t)i, cam2[i], uv2 + 2 * (size_t)i, rays[i]);
    PoseState P;
    memcpy(P.R, R, sizeof(P.R));
    memcpy(P.t, t, sizeof(P.t));
    std::vector<uint8_t> flags((size_t)n), mem((size_t)n);
    int32_t count = 0;
    for (int i = 0; i < n; i++) {
        flags[i] = sac_is_inlier(rel_score(P, rays[i]), threshold) ? 1 : 0;
        count += flags[i];
        mem[i] = member[i] ? 1 : 0;
    }
    polish_host(rays.data(), n, threshold, *pp, P, count, flags.data(), mem, *polish);
    memcpy(R_out, P.R, sizeof(P.R));
    memcpy(t_out, P.t, sizeof(P.t));
    if (n) memcpy(inlier, flags.data(), (size_t)n);
    return MCORB_OK;
}

int mcorb_lmap_last_relative_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, int cap, int *n_hyp)
{
    return last_counts<RelModel>(m, &mcorb_lmap::rel, 1, "lmap last_relative_counts", fail, count, valid, cap, n_hyp, host_valid_array,
                                 each_nothing);
}

double mcorb_rel_threshold(double K00_02) { return 2.0 * mcorb_sac_threshold(K00_02); }

int mcorb_rel_solve(int ncams, const mcorb_track_cam *cams, const int32_t *cam1, const double *uv1, const int32_t *cam2, const double *uv2,
                    double *R, double *t)
{
    if (ncams < 1 || ncams > MCORB_MAX_CAMS || !cams || !cam1 || !uv1 || !cam2 || !uv2 || !R || !t) return fail(MCORB_E_ARG, "bad argument");
    TRY(check_cams(kRelSample, cam1, cam2, ncams));
    RelRays rays[kRelSample];
    for (int j = 0; j < kRelSample; j++) rel_rays_d(cams, cam1[j], uv1 + 2 * j, cam2[j], uv2 + 2 * j, rays[j]);
    PoseState P;
    const bool ok = rel_solve17(rays, P);
    memcpy(R, P.R, sizeof(P.R));
    memcpy(t, P.t, sizeof(P.t));
    return ok ? 1 : 0;
}

int mcorb_dev_rel_solve_selftest(int device, int n, int ncams, const mcorb_track_cam *cams, const int32_t *cam1, const double *uv1,
                                 const int32_t *cam2, const double *uv2, int32_t *count, double *R, double *t)
{
    if (n < 0 || ncams < 1 || ncams > MCORB_MAX_CAMS || (n && (!cams || !cam1 || !uv1 || !cam2 || !uv2 || !count || !R || !t)))
        return fail(MCORB_E_ARG, "bad argument");
    const size_t N = (size_t)n, M = N * kRelSample;
    for (size_t i = 0; i < N; i++) TRY(check_cams(kRelSample, cam1 + kRelSample * i, cam2 + kRelSample * i, ncams));
    if (n == 0) return MCORB_OK;
    TRY(selftest_device(device));
    DevBuf<mcorb_track_cam> d_cams;
    DevBuf<int32_t> d_cam1, d_cam2, d_count;
    DevBuf<double> d_uv1, d_uv2, d_R, d_t;
    TRY(to_device(d_cams, cams, N * (size_t)ncams));
    TRY(to_device(d_cam1, cam1, M));
    TRY(to_device(d_cam2, cam2, M));
    TRY(to_device(d_uv1, uv1, 2 * M));
    TRY(to_device(d_uv2, uv2, 2 * M));
    TRY(d_count.alloc(N));
    TRY(d_R.alloc(N * 9));
    TRY(d_t.alloc(N * 3));
    launch_rel_solve_selftest(nullptr, d_cams, ncams, d_cam1, d_uv1, d_cam2, d_uv2, n, d_R, d_t, d_count);
    HIPCHK(hipGetLastError());
    TRY(from_device(count, d_count, N));
    TRY(from_device(R, d_R, N * 9));
    return from_device(t, d_t, N * 3);
}

int mcorb_rel_eval(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam1, const double *uv1, const int32_t *cam2,
                   const double *uv2, const double *R, const double *t, double *score)
{
    if (n < 0 || ncams < 1 || ncams > MCORB_MAX_CAMS || !cams || !R || !t || (n && (!cam1 || !uv1 || !cam2 || !uv2 || !score)))
        return fail(MCORB_E_ARG, "bad argument");
    TRY(check_cams(n, cam1, cam2, ncams));
    PoseState P;
    memcpy(P.R, R, sizeof(P.R));
    memcpy(P.t, t, sizeof(P.t));
    for (int i = 0; i < n; i++) {
        RelRays r;
        rel_rays_d(cams, cam1[i], uv1 + 2 * (size_t)i, cam2[i], uv2 + 2 * (size_t)i, r);
        score[i] = pose_default_nan(rel_score(P, r));
    }
    return MCORB_OK;
}

}  // extern "C"
