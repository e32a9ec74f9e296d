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

size_t round32(size_t n) { return (n + 31) & ~(size_t)31; }

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

}  // namespace

extern "C" {

int mcorb_lmap_ransac_pose(mcorb_lmap *m, int n, const int32_t *cam, const float *uv, const int32_t *octave, const int32_t *match,
                           const int32_t *lids, const double *pts, int ncams, const mcorb_track_cam *cams,
                           const mcorb_sac_params *params, const mcorb_pose_params *refine_params, mcorb_sac_result *res,
                           uint8_t *inlier)
{
    TRY(check_lmap(m, "lmap ransac_pose"));
    if (n < 0 || !cams || !params || !res || (n && (!cam || !uv || !octave))) return fail(MCORB_E_ARG, "bad argument");
    if (ncams < 1 || ncams > MCORB_MAX_CAMS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_CAMS cameras");
    if (refine_params) TRY(pose_check_params(refine_params));
    if (!(params->threshold > 0) || !sac_finite(params->threshold)) return fail(MCORB_E_ARG, "a threshold that is not finite and positive");
    if (params->max_iterations < 1 || params->max_iterations > MCORB_SAC_MAX_ITERATIONS)
        return fail(MCORB_E_ARG, "1 .. MCORB_SAC_MAX_ITERATIONS iterations");
    if (params->solver != MCORB_SAC_SOLVER_CENTRAL && params->solver != MCORB_SAC_SOLVER_RIG)
        return fail(MCORB_E_ARG, "a solver that is not one of MCORB_SAC_SOLVER_*");
    if ((lids != nullptr) == (pts != nullptr)) return fail(MCORB_E_ARG, "exactly one of lids and pts");
    const int nlevels = refine_params ? refine_params->nlevels : MCORB_MAX_LEVELS;
    for (int i = 0; i < n; i++) {
        if (cam[i] < 0 || cam[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
        if (octave[i] < 0 || octave[i] >= nlevels) return fail(MCORB_E_ARG, "an octave outside the levels");
        if (lids && (lids[i] < 0 || lids[i] >= m->max_landmarks)) return fail(MCORB_E_ARG, "landmark id outside the store");
        if (match && (match[i] < 0 || (i && match[i] < match[i - 1]))) return fail(MCORB_E_ARG, "a match index that is negative or decreases");
    }
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track_pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");
    if (lids)
        for (int i = 0; i < n; i++)
            if (!(m->flags[lids[i]] & kHasPt)) return fail(MCORB_E_STATE, "a landmark has no point");

    SacLists L;
    make_lists(n, cam, match, ncams, L);
    const int S = (int)L.cons.size(), H = params->max_iterations;
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
        std::vector<PoseObs> obs((size_t)n);
        std::vector<double> X((size_t)n * 3);
        for (int i = 0; i < n; i++) {
            obs[i] = PoseObs{uv[2 * i], uv[2 * i + 1], cam[i], octave[i]};
            memcpy(&X[3 * (size_t)i], lids ? &m->geom[(size_t)lids[i] * 6] : pts + 3 * (size_t)i, 3 * sizeof(double));
        }
        if (S == 0) {
            memset(&out, 0, sizeof(out));
            memcpy(out.R, ident.R, sizeof(out.R));
            out.status = MCORB_SAC_NO_OBS;
            out.best = -1;
            for (int j = 0; j < 4; j++) out.sample[j] = -1;
        } else {
            std::vector<SacModel> models((size_t)H);
            std::vector<int32_t> count((size_t)H);
            std::vector<double> f((size_t)S * 3);
            sac_run_serial(job, obs.data(), X.data(), L.cons.data(), L.cam_first.data(), L.cam_cons.data(), models.data(), count.data(),
                           f.data(), out, sac_flags.data());
            m->sac_host_count = count;
            m->sac_host_valid.resize((size_t)H);
            for (int h = 0; h < H; h++) m->sac_host_valid[h] = models[h].valid;
            m->sac_last_hyp = H;
        }
        if (refine_params) {
            memcpy(pjob.init.R, out.R, sizeof(out.R));
            memcpy(pjob.init.t, out.t, sizeof(out.t));
            pose_run_host(pjob, obs.data(), X.data(), n, ref_flags.data(), pres);
        }
    } else {
        SacBufs &b = m->sac;
        HIPCHK(hipSetDevice(m->device));
        (void)hipGetLastError();   // (a stale error of this thread is not this call's)
        const size_t off_job = round32(sizeof(PoseJob)), off_obs = off_job + round32(sizeof(SacJob));
        const size_t off_pt = off_obs + round32((size_t)n * sizeof(PoseObs));
        const size_t off_cons = off_pt + round32((size_t)n * (lids ? sizeof(int32_t) : 3 * sizeof(double)));
        const size_t off_camfirst = off_cons + round32((size_t)S * sizeof(int32_t));
        const size_t off_camcons = off_camfirst + round32(((size_t)ncams + 1) * sizeof(int32_t));
        const size_t off_first = off_camcons + round32((size_t)S * sizeof(int32_t));
        const size_t bytes = off_first + (size_t)n;
        TRY(b.h_in.grow(bytes, hipHostMallocDefault));
        TRY(b.d_in.grow(bytes));
        TRY(b.d_models.grow((size_t)H));
        TRY(b.d_count.grow((size_t)H));
        TRY(b.h_out.grow(1, kHostMapped));
        TRY(b.h_flags.grow((size_t)n, kHostMapped));
        if (refine_params) {
            TRY(b.pose.d_alive.grow((size_t)n));
            TRY(b.pose.h_out.grow(1, kHostMapped));
            TRY(b.pose.h_flags.grow((size_t)n, kHostMapped));
        }
        uint8_t *in = b.h_in;
        if (refine_params) memcpy(in, &pjob, sizeof(pjob));
        memcpy(in + off_job, &job, sizeof(job));
        PoseObs *obs = reinterpret_cast<PoseObs *>(in + off_obs);
        for (int i = 0; i < n; i++) obs[i] = PoseObs{uv[2 * i], uv[2 * i + 1], cam[i], octave[i]};
        if (lids)
            memcpy(in + off_pt, lids, (size_t)n * sizeof(int32_t));
        else
            memcpy(in + off_pt, pts, (size_t)n * 3 * sizeof(double));
        memcpy(in + off_cons, L.cons.data(), (size_t)S * sizeof(int32_t));
        memcpy(in + off_camfirst, L.cam_first.data(), ((size_t)ncams + 1) * sizeof(int32_t));
        memcpy(in + off_camcons, L.cam_cons.data(), (size_t)S * sizeof(int32_t));
        memcpy(in + off_first, L.is_first.data(), (size_t)n);
        hipStream_t st = m->st;
        HIPCHK(hipMemcpyAsync(b.d_in, b.h_in, bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(b.d_count, 0, (size_t)H * sizeof(int32_t), st));
        uint8_t *d = b.d_in.get();
        SacArgs a;
        a.job = reinterpret_cast<const SacJob *>(d + off_job);
        a.obs = reinterpret_cast<const PoseObs *>(d + off_obs);
        a.lids = lids ? reinterpret_cast<const int32_t *>(d + off_pt) : nullptr;
        a.pts = lids ? nullptr : reinterpret_cast<const double *>(d + off_pt);
        a.geom = m->d_geom;
        a.cons = reinterpret_cast<const int32_t *>(d + off_cons);
        a.cam_first = reinterpret_cast<const int32_t *>(d + off_camfirst);
        a.cam_cons = reinterpret_cast<const int32_t *>(d + off_camcons);
        a.is_first = d + off_first;
        a.models = b.d_models;
        a.count = b.d_count;
        a.out = b.h_out;
        a.flags = b.h_flags;
        a.pose_job = refine_params ? reinterpret_cast<PoseJob *>(d) : nullptr;
        HIPCHK(hipEventRecord(m->ev16, st));
        if (job.solver == MCORB_SAC_SOLVER_RIG)
            launch_sac_hypotheses_rig(st, a, H);
        else
            launch_sac_hypotheses(st, a, H);
        hipError_t launched = hipGetLastError();
        HIPCHK(hipEventRecord(m->ev17, st));
        launch_sac_score(st, a, S, H);
        if (launched == hipSuccess) launched = hipGetLastError();
        HIPCHK(hipEventRecord(m->ev18, st));
        launch_sac_pick(st, a, n);
        if (launched == hipSuccess) launched = hipGetLastError();
        HIPCHK(hipEventRecord(m->ev19, st));
        if (refine_params) {
            launch_pose_refine(st, reinterpret_cast<const PoseJob *>(d), 1, reinterpret_cast<PoseObs *>(d + off_obs),
                               lids ? reinterpret_cast<int32_t *>(d + off_pt) : nullptr, a.pts, m->d_geom, b.pose.d_alive, nullptr, nullptr,
                               nullptr, nullptr, b.pose.h_out, b.pose.h_flags);
            if (launched == hipSuccess) launched = hipGetLastError();
        }
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(launched);
        float ms = 0.f;
        ev_elapsed(&ms, m->ev16, m->ev17);
        m->us_sac[0] = ms * 1000.f;
        ev_elapsed(&ms, m->ev17, m->ev18);
        m->us_sac[1] = ms * 1000.f;
        ev_elapsed(&ms, m->ev18, m->ev19);
        m->us_sac[2] = ms * 1000.f;
        m->sac_last_hyp = H;
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
            for (int i = L.match_first[k]; i < L.match_first[k + 1]; i++) all &= ref_flags[i];
            ref_match[k] = all;
            ref_in += all;
        }
    const bool use_refine = refine_params && out.status == MCORB_SAC_OK && !(out.n_inliers > ref_in);
    res->used = use_refine ? 1 : 0;
    memcpy(res->R, use_refine ? pres.R : out.R, sizeof(res->R));
    memcpy(res->t, use_refine ? pres.t : out.t, sizeof(res->t));
    res->n_inliers = use_refine ? ref_in : out.n_inliers;
    if (inlier)
        for (int k = 0; k < nm; k++) inlier[k] = use_refine ? ref_match[k] : sac_flags[L.match_first[k]];
    return MCORB_OK;
}

int mcorb_lmap_last_ransac_timing(mcorb_lmap *m, float us[3], int *n_hyp)
{
    TRY(check_lmap_handle(m, "lmap last_ransac_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < 3; k++) us[k] = m->us_sac[k];
    if (n_hyp) *n_hyp = m->sac_last_hyp;
    return MCORB_OK;
}

int mcorb_lmap_last_ransac_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, int cap, int *n_hyp)
{
    TRY(check_lmap(m, "lmap last_ransac_counts"));
    if (cap < 0 || !n_hyp || (cap && (!count || !valid))) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    const int H = m->sac_last_hyp;
    *n_hyp = H;
    if (cap < H) return fail(MCORB_E_CAP, "arrays too small");
    if (m->device < 0) {
        for (int h = 0; h < H; h++) {
            count[h] = m->sac_host_count[h];
            valid[h] = m->sac_host_valid[h];
        }
        return MCORB_OK;
    }
    if (!H) return MCORB_OK;
    HIPCHK(hipSetDevice(m->device));
    std::vector<SacModel> models((size_t)H);
    HIPCHK(hipMemcpy(count, m->sac.d_count, (size_t)H * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(models.data(), m->sac.d_models, (size_t)H * sizeof(SacModel), hipMemcpyDeviceToHost));
    for (int h = 0; h < H; h++) valid[h] = models[h].valid;
    return MCORB_OK;
}

double mcorb_sac_threshold(double K00_02) { return 1.0 - cos(atan(sqrt(2.0) * 0.5 / K00_02)); }

int mcorb_sac_solve(const mcorb_track_cam *cam, const float *uv, const double *pts, double *R, double *t)
{
    if (!cam || !uv || !pts || !R || !t) return fail(MCORB_E_ARG, "bad argument");
    struct Collect {
        double *R, *t;
        int n;
        void operator()(const PoseState &P)
        {
            memcpy(R + 9 * n, P.R, sizeof(P.R));
            memcpy(t + 3 * n, P.t, sizeof(P.t));
            n++;
        }
    } collect{R, t, 0};
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
    struct Collect {
        double *R, *t;
        int n;
        void operator()(const PoseState &P)
        {
            memcpy(R + 9 * n, P.R, sizeof(P.R));
            memcpy(t + 3 * n, P.t, sizeof(P.t));
            n++;
        }
    } collect{R, t, 0};
    double f[3][3];
    for (int k = 0; k < 3; k++) sac_bearing(cams[cam[k]], uv[2 * k], uv[2 * k + 1], f[k]);
    sac_solve_rig(cams, cam[0], cam[1], cam[2], f[0], f[1], f[2], pts, pts + 3, pts + 6, collect);
    return collect.n;
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
