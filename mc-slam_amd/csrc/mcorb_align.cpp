// mcorb_align.cpp -- the rig pose between two frames from 3D-3D pairs: mcorb_lmap_align_pose, FrontEnd::poseFromPCAlignment
// (MCSlam/src/FrontEnd.cpp:4441-4530), the PC_ALIGN estimator of FrontEnd::estimatePoseLF.  A device store runs
// k_align_hypotheses, k_align_score, k_align_pick and k_align_fit (mode 0: k_align_fit alone; mcorb_align_gpu.hip) in one
// submission on the store's stream with one wait; the record lands in host-mapped memory.  A host-only store runs the header
// (mcorb_align.h) serially, so the two agree bit for bit.  Stated rather than OpenGV's: the draws, the solver, no adaptive stop
// (DESIGN.md section 9k).
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

int fail(int code, const char *what) { set_error(std::string("lmap align_pose: ") + what); return code; }

}  // namespace

extern "C" {

int mcorb_lmap_align_pose(mcorb_lmap *m, int n, const int32_t *lids1, const double *pts1, const double *pts2,
                          const mcorb_align_params *params, mcorb_align_result *res, uint8_t *inlier)
{
    TRY(check_lmap(m, "lmap align_pose"));
    if (!params || !res || n < 0 || (n && !pts2)) return fail(MCORB_E_ARG, "bad argument");
    if ((lids1 != nullptr) == (pts1 != nullptr)) return fail(MCORB_E_ARG, "exactly one of lids1 and pts1");
    if (!positive(params->threshold) || !positive(params->inlier_dist))
        return fail(MCORB_E_ARG, "a threshold or inlier_dist that is not finite and positive");
    if (params->mode != MCORB_ALIGN_MODE_ALL && params->mode != MCORB_ALIGN_MODE_SAC) return fail(MCORB_E_ARG, "an unknown mode");
    const bool sac = params->mode == MCORB_ALIGN_MODE_SAC;
    if (sac && (params->max_iterations < 1 || params->max_iterations > MCORB_ALIGN_MAX_ITERATIONS))
        return fail(MCORB_E_ARG, "1 .. MCORB_ALIGN_MAX_ITERATIONS iterations");
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track.pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");
    if (lids1)
        for (int i = 0; i < n; i++)
            if (lids1[i] < 0 || lids1[i] >= m->max_landmarks || !(m->flags[lids1[i]] & kHasPt))
                return fail(MCORB_E_ARG, "a landmark id that is not a slot with a point");

    const int H = sac ? params->max_iterations : 0;
    AlignJob job;
    memset(&job, 0, sizeof(job));
    job.threshold = params->threshold;
    job.inlier_dist = params->inlier_dist;
    job.seed = params->seed;
    job.n = n;
    job.H = H;
    job.mode = params->mode;
    job.refit = params->refit ? 1 : 0;

    AlignOut out;
    std::vector<uint8_t> flags((size_t)n);
    mcorb_lmap::Align &b = m->align;
    if (n == 0) {
        no_obs(out, MCORB_ALIGN_NO_OBS);
        out.sac_R[0] = out.sac_R[4] = out.sac_R[8] = 1.0;
        out.best = -1;
    } else if (m->device < 0) {
        std::vector<double> gathered;
        const double *p1 = pts1;
        if (lids1) {
            gathered.resize((size_t)n * 3);
            for (int i = 0; i < n; i++) memcpy(&gathered[3 * (size_t)i], &m->geom[(size_t)lids1[i] * 6], 3 * sizeof(double));
            p1 = gathered.data();
        }
        std::vector<AlignModel> models((size_t)H);
        std::vector<int32_t> count((size_t)H);
        std::vector<uint8_t> member((size_t)n);
        memset(&out, 0, sizeof(out));
        align_run_serial(job, p1, pts2, models.data(), count.data(), member.data(), out, flags.data());
        if (sac) {
            b.host_valid.resize((size_t)H);
            for (int h = 0; h < H; h++) b.host_valid[h] = models[h].valid;
            b.host_count.swap(count);
            b.last_hyp = H;
        }
    } else {
        HIPCHK(hipSetDevice(m->device));
        (void)hipGetLastError();   // (a stale error of this thread is not this call's)
        const AlignLayout L((size_t)n, lids1 != nullptr);
        TRY(b.reserve(L.p.total, (size_t)n, (size_t)H));
        *b.in.host<AlignJob>(L.job) = job;
        if (lids1)
            memcpy(b.in.host<int32_t>(L.p1), lids1, (size_t)n * sizeof(int32_t));
        else
            memcpy(b.in.host<double>(L.p1), pts1, (size_t)n * 3 * sizeof(double));
        memcpy(b.in.host<double>(L.p2), pts2, (size_t)n * 3 * sizeof(double));
        hipStream_t st = m->st;
        AlignArgs a;
        a.job = b.in.dev<const AlignJob>(L.job);
        a.p1 = lids1 ? nullptr : b.in.dev<const double>(L.p1);
        a.p2 = b.in.dev<const double>(L.p2);
        a.lids1 = lids1 ? b.in.dev<const int32_t>(L.p1) : nullptr;
        a.geom = m->d_geom;
        a.models = b.d_models;
        a.count = b.d_count;
        a.pick = b.d_pick;
        a.member = b.d_member;
        a.out = b.h_out;
        a.flags = b.h_flags;
        Submission sub(st);
        b.in.upload(sub, L.p.total);
        if (sac) {
            sub.fill(b.d_count, 0, (size_t)H * sizeof(int32_t));
            sub.run(b.sac, 0, [&] { launch_align_hypotheses(st, a, H); });
            sub.run(b.sac, 1, [&] { launch_align_score(st, a, n, H); });
            sub.run(b.sac, 2, [&] { launch_align_pick(st, a, n); });
            sub.mark(b.sac, 3);
        }
        sub.run(b.fit, 0, [&] { launch_align_fit(st, a); });
        sub.mark(b.fit, 1);
        TRY(sub.wait());
        if (sac) {
            b.sac.read();
            b.last_hyp = H;
        }
        b.fit.read();
        out = *b.h_out.get();
        memcpy(flags.data(), b.h_flags.get(), (size_t)n);
    }

    memset(res, 0, sizeof(*res));
    memcpy(res->R, out.R, sizeof(out.R));
    memcpy(res->t, out.t, sizeof(out.t));
    memcpy(res->sac_R, out.sac_R, sizeof(out.sac_R));
    memcpy(res->sac_t, out.sac_t, sizeof(out.sac_t));
    res->mean_error = out.mean_error;
    res->status = out.status;
    res->used = out.used;
    res->n_inliers = out.n_inliers;
    res->n_matches = n;
    res->sac_n_inliers = out.sac_n_inliers;
    res->best_hypothesis = out.best;
    memcpy(res->sample, out.sample, sizeof(res->sample));
    res->n_models = out.n_models;
    if (inlier && n) memcpy(inlier, flags.data(), (size_t)n);
    return MCORB_OK;
}

int mcorb_lmap_last_align_timing(mcorb_lmap *m, float us[4], int *n_hyp)
{
    TRY(check_lmap_handle(m, "lmap last_align_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < 3; k++) us[k] = m->align.sac.us[k];
    us[3] = m->align.fit.us[0];
    if (n_hyp) *n_hyp = m->align.last_hyp;
    return MCORB_OK;
}

int mcorb_lmap_last_align_counts(mcorb_lmap *m, int32_t *count, int32_t *valid, int cap, int *n_hyp)
{
    return last_counts<AlignModel>(m, &mcorb_lmap::align, 1, "lmap last_align_counts", fail, count, valid, cap, n_hyp, host_valid_array,
                                   each_nothing);
}

int mcorb_align_solve(int n, const double *p1, const double *p2, const uint8_t *member, double *R, double *t, double *gap)
{
    if (n < 0 || !R || !t || (n && (!p1 || !p2))) return fail(MCORB_E_ARG, "bad argument");
    PoseState P;
    int cnt;
    const bool ok = align_fit_host(n, p1, p2, member, P, cnt, gap);
    if (gap) *gap = pose_default_nan(*gap);   // (returned to the caller: the device twin's bits)
    memcpy(R, P.R, sizeof(P.R));
    memcpy(t, P.t, sizeof(P.t));
    return ok ? 1 : 0;
}

int mcorb_dev_align_solve_selftest(int device, int n, const int32_t *npairs, const double *p1, const double *p2, const uint8_t *member,
                                   int32_t *valid, double *R, double *t, double *gap)
{
    if (n < 0 || (n && (!npairs || !valid || !R || !t || !gap))) return fail(MCORB_E_ARG, "bad argument");
    const size_t N = (size_t)n;
    std::vector<int32_t> first(N);
    size_t total = 0;
    for (size_t i = 0; i < N; i++) {
        if (npairs[i] < 0 || total + (size_t)npairs[i] > 0x7fffffffu) return fail(MCORB_E_ARG, "a pair count out of range");
        first[i] = (int32_t)total;
        total += (size_t)npairs[i];
    }
    if (total && (!p1 || !p2 || !member)) return fail(MCORB_E_ARG, "bad argument");
    if (n == 0) return MCORB_OK;
    TRY(selftest_device(device));
    const size_t T = total ? total : 1;   // (problems without pairs read nothing)
    DevBuf<double> d_p1, d_p2, d_R, d_t, d_gap;
    DevBuf<uint8_t> d_member;
    DevBuf<int32_t> d_first, d_cnt, d_valid;
    TRY(zeroed(d_p1, 3 * T));
    TRY(zeroed(d_p2, 3 * T));
    TRY(zeroed(d_member, T));
    if (total) {
        HIPCHK(hipMemcpy(d_p1, p1, 3 * total * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_p2, p2, 3 * total * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_member, member, total, hipMemcpyHostToDevice));
    }
    TRY(to_device(d_first, first.data(), N));
    TRY(to_device(d_cnt, npairs, N));
    TRY(d_valid.alloc(N));
    TRY(d_R.alloc(N * 9));
    TRY(d_t.alloc(N * 3));
    TRY(d_gap.alloc(N));
    launch_align_solve_selftest(nullptr, d_p1, d_p2, d_member, d_first, d_cnt, n, d_R, d_t, d_gap, d_valid);
    HIPCHK(hipGetLastError());
    TRY(from_device(valid, d_valid, N));
    TRY(from_device(R, d_R, N * 9));
    TRY(from_device(t, d_t, N * 3));
    return from_device(gap, d_gap, N);
}

int mcorb_align_eval(int n, const double *p1, const double *p2, const double *R, const double *t, double *dist)
{
    if (n < 0 || !R || !t || (n && (!p1 || !p2 || !dist))) return fail(MCORB_E_ARG, "bad argument");
    PoseState P;
    memcpy(P.R, R, sizeof(P.R));
    memcpy(P.t, t, sizeof(P.t));
    for (int i = 0; i < n; i++) dist[i] = pose_default_nan(align_dist(P, p1 + 3 * (size_t)i, p2 + 3 * (size_t)i));
    return MCORB_OK;
}

}  // extern "C"
