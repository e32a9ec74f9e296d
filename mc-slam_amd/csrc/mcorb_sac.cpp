// mcorb_sac.cpp -- the absolute rig pose by RANSAC in front of the refinement: mcorb_lmap_ransac_pose, the consensus step of
// FrontEnd::absolutePoseFromGP3P (MCSlam/src/FrontEnd.cpp:4660-4798) with the refinement and the rule of :4771-4795 behind it.
// A device store runs k_sac_hypotheses (k_sac_hypotheses_rig with MCORB_SAC_SOLVER_RIG), k_sac_score, k_sac_pick
// (mcorb_sac_gpu.hip) and, when asked, k_pose_refine in one submission on the store's stream with one wait; the records land in
// host-mapped memory.  A host-only store runs the header
// (mcorb_sac.h) serially, so the two agree bit for bit.  Stated rather than OpenGV's: the draws, the minimal solver, no adaptive
// stop.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

int fail(int code, const char *what) { set_error(std::string("lmap ransac_pose: ") + what); return code; }

// the lists the draws index: the consensus observations in input order, and camera by camera
struct SacLists {
    std::vector<int32_t> cons, cam_first, cam_cons;
    std::vector<uint8_t> is_first;
    std::vector<int32_t> match_first;   // per match: its first observation; one more: n
};

void make_lists(int n, const int32_t *cam, const int32_t *match, int ncams, SacLists &L)
{
    L.is_first.assign((size_t)n, 0);
    L.cam_first.assign((size_t)ncams + 1, 0);
    for (int i = 0; i < n; i++) {
        if (match && i && match[i] == match[i - 1]) continue;
        L.is_first[i] = 1;
        L.cons.push_back(i);
        L.match_first.push_back(i);
        L.cam_first[cam[i] + 1]++;
    }
    L.match_first.push_back(n);
    for (int c = 0; c < ncams; c++) L.cam_first[c + 1] += L.cam_first[c];
    L.cam_cons.resize(L.cons.size());
    std::vector<int32_t> at(L.cam_first.begin(), L.cam_first.end() - 1);
    for (int32_t i : L.cons) L.cam_cons[at[cam[i]]++] = i;
}

// what the solver hooks hand to sac_solve / sac_solve_rig: the poses, appended to the caller's arrays
struct Collect {
    double *R, *t;
    int n;
    void operator()(const PoseState &P)
    {
        memcpy(R + 9 * n, P.R, sizeof(P.R));
        memcpy(t + 3 * n, P.t, sizeof(P.t));
        n++;
    }
};

}  // namespace

extern "C" {

int mcorb_lmap_ransac_pose(mcorb_lmap *m, int n, const int32_t *cam, const float *uv, const int32_t *octave, const int32_t *match,
                           const int32_t *lids, const double *pts, int ncams, const mcorb_track_cam *cams,
                           const mcorb_sac_params *params, const mcorb_pose_params *refine_params, mcorb_sac_result *res,
                           uint8_t *inlier)
{
    const char *who = "lmap ransac_pose: ";
    TRY(check_lmap(m, "lmap ransac_pose"));
    if (!params || !res) return fail(MCORB_E_ARG, "bad argument");
    if (refine_params) TRY(pose_check_params(refine_params));
    if (!positive(params->threshold)) return fail(MCORB_E_ARG, "a threshold that is not finite and positive");
    if (params->max_iterations < 1 || params->max_iterations > MCORB_SAC_MAX_ITERATIONS)
        return fail(MCORB_E_ARG, "1 .. MCORB_SAC_MAX_ITERATIONS iterations");
    if (params->solver != MCORB_SAC_SOLVER_CENTRAL && params->solver != MCORB_SAC_SOLVER_RIG)
        return fail(MCORB_E_ARG, "a solver that is not one of MCORB_SAC_SOLVER_*");
    const ObsInput in{n, cam, uv, octave, lids, pts, ncams, cams};
    TRY(obs_check(m, in, refine_params ? refine_params->nlevels : MCORB_MAX_LEVELS, match, who));
    std::lock_guard<std::mutex> lk(m->mu);
    TRY(obs_check_locked(m, in, who));

    SacLists lists;
    make_lists(n, cam, match, ncams, lists);
    const int S = (int)lists.cons.size(), H = params->max_iterations;
    SacJob job;
    memset(&job, 0, sizeof(job));
    memcpy(job.cams, cams, (size_t)ncams * sizeof(mcorb_track_cam));
    job.threshold = params->threshold;
    job.seed = params->seed;
    job.ncams = ncams;
    job.n = n;
    job.S = S;
    job.H = H;
    job.solver = params->solver;
    PoseJob pjob;
    const PoseState ident = PoseState{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
    if (refine_params) {
        pose_job_init(pjob, *refine_params, ncams, cams, ident);
        pjob.n = n;
    }

    SacOut out;
    mcorb_pose_result pres;
    memset(&pres, 0, sizeof(pres));
    std::vector<uint8_t> sac_flags((size_t)n), ref_flags((size_t)n);
    if (m->device < 0 || S == 0) {
        std::vector<PoseObs> obs;
        std::vector<double> X;
        obs_gather(m, in, obs, X);
        if (S == 0) {
            no_obs(out, MCORB_SAC_NO_OBS);
            out.best = -1;
        } else {
            std::vector<SacModel> models((size_t)H);
            std::vector<int32_t> count((size_t)H);
            std::vector<double> f((size_t)S * 3);
            sac_run_serial(job, obs.data(), X.data(), lists.cons.data(), lists.cam_first.data(), lists.cam_cons.data(), models.data(),
                           count.data(), f.data(), out, sac_flags.data());
            m->sac.host_count = count;
            m->sac.host_valid.resize((size_t)H);
            for (int h = 0; h < H; h++) m->sac.host_valid[h] = models[h].valid;
            m->sac.last_hyp = H;
        }
        if (refine_params) {
            memcpy(pjob.init.R, out.R, sizeof(out.R));
            memcpy(pjob.init.t, out.t, sizeof(out.t));
            pose_run_host(pjob, obs.data(), X.data(), n, ref_flags.data(), pres);
        }
    } else {
        mcorb_lmap::Sac &b = m->sac;
        HIPCHK(hipSetDevice(m->device));
        (void)hipGetLastError();   // (a stale error of this thread is not this call's)
        const ObsLayout L((size_t)n, lids != nullptr, true, (size_t)S, (size_t)ncams);
        TRY(b.reserve(L.p.total, (size_t)n, (size_t)H, refine_params != nullptr));
        if (refine_params) *b.in.host<PoseJob>(L.pose_job) = pjob;
        *b.in.host<SacJob>(L.sac_job) = job;
        obs_stage(in, L, b.in);
        memcpy(b.in.host<int32_t>(L.cons), lists.cons.data(), (size_t)S * sizeof(int32_t));
        memcpy(b.in.host<int32_t>(L.cam_first), lists.cam_first.data(), ((size_t)ncams + 1) * sizeof(int32_t));
        memcpy(b.in.host<int32_t>(L.cam_cons), lists.cam_cons.data(), (size_t)S * sizeof(int32_t));
        memcpy(b.in.host<uint8_t>(L.is_first), lists.is_first.data(), (size_t)n);
        hipStream_t st = m->st;
        SacArgs a;
        a.job = b.in.dev<const SacJob>(L.sac_job);
        a.obs = b.in.dev<const PoseObs>(L.obs);
        a.lids = lids ? b.in.dev<const int32_t>(L.pt) : nullptr;
        a.pts = lids ? nullptr : b.in.dev<const double>(L.pt);
        a.geom = m->d_geom;
        a.cons = b.in.dev<const int32_t>(L.cons);
        a.cam_first = b.in.dev<const int32_t>(L.cam_first);
        a.cam_cons = b.in.dev<const int32_t>(L.cam_cons);
        a.is_first = b.in.dev<const uint8_t>(L.is_first);
        a.models = b.d_models;
        a.count = b.d_count;
        a.out = b.h_out;
        a.flags = b.h_flags;
        a.pose_job = refine_params ? b.in.dev<PoseJob>(L.pose_job) : nullptr;
        Submission sub(st);
        b.in.upload(sub, L.p.total);
        sub.fill(b.d_count, 0, (size_t)H * sizeof(int32_t));
        sub.run(b.kernels, 0, [&] {
            if (job.solver == MCORB_SAC_SOLVER_RIG)
                launch_sac_hypotheses_rig(st, a, H);
            else
                launch_sac_hypotheses(st, a, H);
        });
        sub.run(b.kernels, 1, [&] { launch_sac_score(st, a, S, H); });
        sub.run(b.kernels, 2, [&] { launch_sac_pick(st, a, n); });
        sub.mark(b.kernels, 3);
        if (refine_params) sub.run([&] { obs_enqueue_refine(m, in, L, b.in, b.pose); });
        TRY(sub.wait());
        b.kernels.read();
        b.last_hyp = H;
        out = *b.h_out.get();
        memcpy(sac_flags.data(), b.h_flags.get(), (size_t)n);
        if (refine_params) {
            pres = *b.pose.h_out.get();
            memcpy(ref_flags.data(), b.pose.h_flags.get(), (size_t)n);
        }
    }

    // the fold to matches and the rule of :4786
    const int nm = S;
    memset(res, 0, sizeof(*res));
    memcpy(res->sac_R, out.R, sizeof(out.R));
    memcpy(res->sac_t, out.t, sizeof(out.t));
    res->status = out.status;
    res->n_matches = nm;
    res->n_consensus = S;
    res->sac_n_inliers = out.n_inliers;
    res->best_hypothesis = out.best;
    memcpy(res->sample, out.sample, sizeof(out.sample));
    res->n_models = out.n_models;
    res->refine = pres;
    int ref_in = 0;
    std::vector<uint8_t> ref_match((size_t)nm);
    if (refine_params)
        for (int k = 0; k < nm; k++) {
            uint8_t all = 1;
            for (int i = lists.match_first[k]; i < lists.match_first[k + 1]; i++) all &= ref_flags[i];
            ref_match[k] = all;
            ref_in += all;
        }
    const bool use_refine = refine_params && out.status == MCORB_SAC_OK && !(out.n_inliers > ref_in);
    res->used = use_refine ? 1 : 0;
    memcpy(res->R, use_refine ? pres.R : out.R, sizeof(res->R));
    memcpy(res->t, use_refine ? pres.t : out.t, sizeof(res->t));
    res->n_inliers = use_refine ? ref_in : out.n_inliers;
    if (inlier)
        for (int k = 0; k < nm; k++) inlier[k] = use_refine ? ref_match[k] : sac_flags[lists.match_first[k]];
    return MCORB_OK;
}

int mcorb_lmap_last_ransac_timing(mcorb_lmap *m, float us[3], int *n_hyp)
{
    TRY(check_lmap_handle(m, "lmap last_ransac_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < 3; k++) us[k] = m->sac.kernels.us[k];
    if (n_hyp) *n_hyp = m->sac.last_hyp;
    return MCORB_OK;
}

int mcorb_lmap_last_ransac_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, int cap, int *n_hyp)
{
    return last_counts<SacModel>(m, &mcorb_lmap::sac, 1, "lmap last_ransac_counts", fail, count, valid, cap, n_hyp, host_valid_array,
                                 each_nothing);
}

double mcorb_sac_threshold(double K00_02) { return 1.0 - cos(atan(sqrt(2.0) * 0.5 / K00_02)); }

int mcorb_sac_solve(const mcorb_track_cam *cam, const float *uv, const double *pts, double *R, double *t)
{
    if (!cam || !uv || !pts || !R || !t) return fail(MCORB_E_ARG, "bad argument");
    Collect collect{R, t, 0};
    double f[3][3];
    for (int k = 0; k < 3; k++) sac_bearing(*cam, uv[2 * k], uv[2 * k + 1], f[k]);
    sac_solve(*cam, f[0], f[1], f[2], pts, pts + 3, pts + 6, collect);
    return collect.n;
}

int mcorb_sac_solve_rig(int ncams, const mcorb_track_cam *cams, const int32_t *cam, const float *uv, const double *pts, double *R, double *t)
{
    if (ncams < 1 || ncams > MCORB_MAX_CAMS || !cams || !cam || !uv || !pts || !R || !t) return fail(MCORB_E_ARG, "bad argument");
    for (int k = 0; k < 3; k++)
        if (cam[k] < 0 || cam[k] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
    Collect collect{R, t, 0};
    double f[3][3];
    for (int k = 0; k < 3; k++) sac_bearing(cams[cam[k]], uv[2 * k], uv[2 * k + 1], f[k]);
    sac_solve_rig(cams, cam[0], cam[1], cam[2], f[0], f[1], f[2], pts, pts + 3, pts + 6, collect);
    return collect.n;
}

int mcorb_host_sac_rig_roots(int ncams, const mcorb_track_cam *cams, const int32_t *cam, const float *uv, const double *pts, double *R, double *t,
                             int32_t *mask, int32_t *best, double *best_R, double *best_t)
{
    if (ncams < 1 || ncams > MCORB_MAX_CAMS || !cams || !cam || !uv || !pts || !R || !t || !mask || !best || !best_R || !best_t)
        return fail(MCORB_E_ARG, "bad argument");
    for (int k = 0; k < 4; k++)
        if (cam[k] < 0 || cam[k] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
    const mcorb_track_cam &c0 = cams[cam[0]], &c1 = cams[cam[1]], &c2 = cams[cam[2]], &c3 = cams[cam[3]];
    double f[4][3];
    for (int k = 0; k < 4; k++) sac_bearing(cams[cam[k]], uv[2 * k], uv[2 * k + 1], f[k]);
    SacRig G;
    sac_rig_prepare(c0, c1, c2, f[0], f[1], f[2], pts, pts + 3, pts + 6, G);
    Collect collect{R, t, 0};
    PoseState Pb = PoseState{};
    bool hb = false;
    double sb = 0.0;
    int kb = 0;
    *mask = 0;
    for (int k = 0; k < 4; k++) {
        PoseState P;
        const bool root = sac_rig_root(G, k, c0, c1, c2, f[0], f[1], f[2], pts, pts + 3, pts + 6, P);
        const double score = sac_score(c3, P, pts + 9, f[3]);
        const bool has = root && score == score;
        if (root) {
            collect(P);
            *mask |= 1 << k;
        }
        if (sac_root_beats(has, score, k, hb, sb, kb)) hb = true, sb = score, kb = k, Pb = P;
    }
    *best = hb ? kb : -1;
    for (int j = 0; j < 9; j++) best_R[j] = hb ? Pb.R[j] : 0.0;
    for (int j = 0; j < 3; j++) best_t[j] = hb ? Pb.t[j] : 0.0;
    return collect.n;
}

int mcorb_dev_sac_solve_selftest(int device, int n, const mcorb_track_cam *cam, const float *uv, const double *pts, int32_t *count, double *R,
                                 double *t)
{
    if (n < 0 || (n && (!cam || !uv || !pts || !count || !R || !t))) return fail(MCORB_E_ARG, "bad argument");
    if (n == 0) return MCORB_OK;
    TRY(selftest_device(device));
    const size_t N = (size_t)n;
    DevBuf<mcorb_track_cam> d_cam;
    DevBuf<float> d_uv;
    DevBuf<double> d_pts, d_R, d_t;
    DevBuf<int32_t> d_count;
    TRY(to_device(d_cam, cam, N));
    TRY(to_device(d_uv, uv, N * 6));
    TRY(to_device(d_pts, pts, N * 9));
    TRY(zeroed(d_R, N * 36));
    TRY(zeroed(d_t, N * 12));
    TRY(d_count.alloc(N));
    launch_sac_solve_selftest(nullptr, d_cam, d_uv, d_pts, n, d_R, d_t, d_count);
    HIPCHK(hipGetLastError());
    TRY(from_device(count, d_count, N));
    TRY(from_device(R, d_R, N * 36));
    return from_device(t, d_t, N * 12);
}

int mcorb_dev_sac_solve_rig_selftest(int device, int n, int ncams, const mcorb_track_cam *cams, const int32_t *cam, const float *uv,
                                     const double *pts, int32_t *count, double *R, double *t, int32_t *mask, int32_t *best, double *best_R,
                                     double *best_t)
{
    if (n < 0 || ncams < 1 || ncams > MCORB_MAX_CAMS ||
        (n && (!cams || !cam || !uv || !pts || !count || !R || !t || !mask || !best || !best_R || !best_t)))
        return fail(MCORB_E_ARG, "bad argument");
    const size_t N = (size_t)n;
    for (size_t i = 0; i < 4 * N; i++)
        if (cam[i] < 0 || cam[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
    if (n == 0) return MCORB_OK;
    TRY(selftest_device(device));
    std::vector<PoseObs> obs(4 * N);
    for (size_t i = 0; i < 4 * N; i++) obs[i] = PoseObs{uv[2 * i], uv[2 * i + 1], cam[i], 0};
    DevBuf<mcorb_track_cam> d_cams;
    DevBuf<PoseObs> d_obs;
    DevBuf<double> d_pts, d_R, d_t;
    DevBuf<int32_t> d_count, d_mask, d_best;
    DevBuf<SacModel> d_win;
    TRY(to_device(d_cams, cams, N * (size_t)ncams));
    TRY(to_device(d_obs, obs.data(), 4 * N));
    TRY(to_device(d_pts, pts, N * 12));
    TRY(zeroed(d_R, N * 36));
    TRY(zeroed(d_t, N * 12));
    TRY(d_count.alloc(N));
    TRY(d_mask.alloc(N));
    TRY(d_best.alloc(N));
    TRY(d_win.alloc(N));
    launch_sac_solve_rig_selftest(nullptr, d_cams, ncams, d_obs, d_pts, n, d_R, d_t, d_count, d_mask, d_best, d_win);
    HIPCHK(hipGetLastError());
    std::vector<SacModel> win(N);
    TRY(from_device(win.data(), d_win, N));
    for (size_t i = 0; i < N; i++) {
        memcpy(best_R + 9 * i, win[i].R, sizeof(win[i].R));
        memcpy(best_t + 3 * i, win[i].t, sizeof(win[i].t));
    }
    TRY(from_device(count, d_count, N));
    TRY(from_device(mask, d_mask, N));
    TRY(from_device(best, d_best, N));
    TRY(from_device(R, d_R, N * 36));
    return from_device(t, d_t, N * 12);
}

int mcorb_sac_eval(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam, const float *uv, const double *pts, const double *R,
                   const double *t, double *score)
{
    if (n < 0 || ncams < 1 || ncams > MCORB_MAX_CAMS || !cams || !R || !t || (n && (!cam || !uv || !pts || !score)))
        return fail(MCORB_E_ARG, "bad argument");
    for (int i = 0; i < n; i++)
        if (cam[i] < 0 || cam[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
    PoseState P;
    memcpy(P.R, R, sizeof(P.R));
    memcpy(P.t, t, sizeof(P.t));
    for (int i = 0; i < n; i++) {
        double f[3];
        sac_bearing(cams[cam[i]], uv[2 * i], uv[2 * i + 1], f);
        score[i] = pose_default_nan(sac_score(cams[cam[i]], P, pts + 3 * (size_t)i, f));
    }
    return MCORB_OK;
}

}  // extern "C"
