// mcorb_pose.cpp -- the rig pose from a frame's 2D-3D matches: the cost function and outlier rule of FrontEnd::OptimizePose
// (MCSlam/src/FrontEnd.cpp:4272-4409) around a stated Levenberg-Marquardt (mcorb_pose.h).  mcorb_lmap_refine_pose takes the
// observations as arrays; mcorb_lmap_set_track_refine appends the same refinement to every tracking submission of the store
// (mcorb_track.cpp calls pose_track_submit / pose_track_host), whose kernel builds the observations from the frame's matches on
// the device.  A device store runs a problem in one launch of k_pose_refine (mcorb_pose_gpu.hip), the result in host-mapped
// memory: one synchronisation, no copy down.  A host-only store runs the header serially, lane by lane in the order the
// workgroup adds, so the two agree bit for bit.  Not restated: gtsam's optimizer.  The RANSAC in front of it is mcorb_sac.cpp.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

int fail(int code, const char *what) { set_error(std::string("lmap pose: ") + what); return code; }

size_t round32(size_t n) { return (n + 31) & ~(size_t)31; }

int check_params(const mcorb_pose_params *p)
{
    if (!p) return fail(MCORB_E_ARG, "bad argument");
    if (p->nlevels < 1 || p->nlevels > MCORB_MAX_LEVELS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_LEVELS levels");
    if (p->max_iterations < 1 || p->max_iterations > 100) return fail(MCORB_E_ARG, "1 .. 100 iterations");
    return MCORB_OK;
}

// the serial pass of a host-only store: lane l adds observations l, l + 256, .. and the lanes fold as the workgroup does
struct HostPass {
    const PoseJob &job;
    const PoseObs *obs;
    const double *pts;   // [n][3], gathered
    const uint8_t *alive;
    int n;
    void operator()(const PoseState &P, double S[kPoseSums])
    {
        static thread_local double s[MCORB_POSE_LANES][kPoseSums];
        for (int l = 0; l < MCORB_POSE_LANES; l++) {
            for (int k = 0; k < kPoseSums; k++) s[l][k] = 0.0;
            for (int i = l; i < n; i += MCORB_POSE_LANES) {
                if (!alive[i]) continue;
                pose_add(job.cams[obs[i].cam], P, pts + 3 * (size_t)i, obs[i].u, obs[i].v, job.huber_k, s[l]);
            }
        }
        pose_fold(s, S);
    }
};

}  // namespace

namespace mcorb {

int pose_check_params(const mcorb_pose_params *p) { return check_params(p); }

void pose_job_init(PoseJob &job, const mcorb_pose_params &p, int ncams, const mcorb_track_cam *cams, const PoseState &init)
{
    memset(&job, 0, sizeof(job));
    job.init = init;
    memcpy(job.inv_sigma2, p.inv_sigma2, sizeof(job.inv_sigma2));
    job.huber_k = sqrt(5.991);   // the double nearest the root: IEEE's sqrt on the host
    memcpy(job.cams, cams, (size_t)ncams * sizeof(mcorb_track_cam));
    job.ncams = ncams;
    job.nlevels = p.nlevels;
    job.max_iterations = p.max_iterations;
}

// a problem on the host: what k_pose_refine does, serially.  alive: n flags, written
void pose_run_host(const PoseJob &job, const PoseObs *obs, const double *pts, int n, uint8_t *alive, mcorb_pose_result &res)
{
    memset(&res, 0, sizeof(res));
    memcpy(res.R, job.init.R, sizeof(res.R));
    memcpy(res.t, job.init.t, sizeof(res.t));
    res.status = MCORB_POSE_NO_OBS;
    res.n_obs = n;
    if (n < 1) return;
    memset(alive, 1, (size_t)n);
    HostPass pass{job, obs, pts, alive, n};
    PoseState pose = job.init;
    for (int round = 0; round < 2; round++) {
        double c0, c1;
        pose_round(pass, job.init, job.max_iterations, pose, res.iterations[round], res.status, c0, c1);
        if (round == 0) res.cost_initial = pose_default_nan(c0);
        res.cost_final = pose_default_nan(c1);
        for (int i = 0; i < n; i++)
            if (alive[i] && pose_is_outlier(job.cams[obs[i].cam], pose, pts + 3 * (size_t)i, obs[i].u, obs[i].v, job.inv_sigma2[obs[i].octave]))
                alive[i] = 0;
    }
    memcpy(res.R, pose.R, sizeof(res.R));
    memcpy(res.t, pose.t, sizeof(res.t));
    for (int i = 0; i < n; i++) res.n_inliers += alive[i];
}

// ---- behind a tracking call (mcorb_track.cpp; the caller holds the store's lock) ----
// the job of frame f of the pending call: the rig and the initial pose of its view
static void track_job(const mcorb_lmap *m, const mcorb_track_view &view, PoseJob &job)
{
    PoseState init;
    pose_of_view(view.R0, view.t0, init);
    pose_job_init(job, m->track_refine_params, view.ncams, view.cams, init);
}

// a host-only store, or a frame for which nothing was launched: the observations from the frame's matches (cand, matches and
// n_match: the frame's; kp: its keypoints), the cameras back to back in match order
void pose_track_host(mcorb_lmap *m, const mcorb_track_view &view, const int *cand, int nc, const TrMatch *matches, const int32_t *n_match,
                     const uint8_t *const *kp_base, size_t kp_stride, mcorb_pose_result &res, uint8_t *flags)
{
    PoseJob job;
    track_job(m, view, job);
    std::vector<PoseObs> obs;
    std::vector<double> pts;
    for (int c = 0; c < view.ncams && nc; c++)
        for (int k = 0; k < n_match[c]; k++) {
            const TrMatch &mt = matches[(size_t)c * nc + k];
            const float *p = reinterpret_cast<const float *>(kp_base[c] + (size_t)mt.kp * kp_stride);
            obs.push_back(PoseObs{p[0], p[1], c, 0});
            const double *X = &m->geom[(size_t)cand[mt.i] * 6];
            pts.insert(pts.end(), X, X + 3);
        }
    pose_run_host(job, obs.data(), pts.data(), (int)obs.size(), flags, res);
}

// a device store: k_pose_refine for the nf frames of the submission, behind its de-duplication on the store's stream.  first:
// the frames' places in the call's candidate list (nf + 1); frames: per frame its TrFrame and keypoint base (kp0) in kp_xy
int pose_track_submit(mcorb_lmap *m, const mcorb_track_view *views, int nf, const size_t *first, const TrFrame *frames, const size_t *kp0,
                      const float2 *kp_xy, const int *d_cand)
{
    PoseBufs &b = m->pose_t;
    const int C = views[0].ncams;
    const size_t rows = (size_t)C * first[nf];
    const size_t bytes = (size_t)nf * sizeof(PoseJob);
    TRY(b.h_in.grow(bytes, hipHostMallocDefault));
    TRY(b.d_in.grow(bytes));
    TRY(b.d_obs.grow(rows));
    TRY(b.d_lids.grow(rows));
    TRY(b.d_alive.grow(rows));
    TRY(b.h_out.grow((size_t)nf, kHostMapped));
    TRY(b.h_flags.grow(rows, kHostMapped));
    PoseJob *jobs = reinterpret_cast<PoseJob *>(b.h_in.get());
    for (int f = 0; f < nf; f++) {
        PoseJob &job = jobs[f];
        track_job(m, views[f], job);
        job.from_track = 1;
        job.n_cand = (int32_t)(first[f + 1] - first[f]);
        job.n = C * job.n_cand;
        job.cand_first = first[f];
        job.obs0 = job.rows = (size_t)C * first[f];
        job.kp0 = kp0[f];
        job.frame = frames[f];
    }
    HIPCHK(hipMemcpyAsync(b.d_in, b.h_in, bytes, hipMemcpyHostToDevice, m->st));
    launch_pose_refine(m->st, reinterpret_cast<const PoseJob *>(b.d_in.get()), nf, b.d_obs, b.d_lids, nullptr, m->d_geom, b.d_alive,
                       m->d_trackwin, m->d_trackbest, d_cand, kp_xy, b.h_out, b.h_flags);
    HIPCHK(hipGetLastError());
    return MCORB_OK;
}

}  // namespace mcorb

extern "C" {

int mcorb_lmap_refine_pose(mcorb_lmap *m, int n, const int32_t *cam, const float *uv, const int32_t *octave, const int32_t *lids,
                           const double *pts, int ncams, const mcorb_track_cam *cams, const double *R, const double *t,
                           const mcorb_pose_params *params, mcorb_pose_result *res, uint8_t *inlier)
{
    TRY(check_lmap(m, "lmap refine_pose"));
    if (n < 0 || !cams || !R || !t || !res || (n && (!cam || !uv || !octave))) return fail(MCORB_E_ARG, "bad argument");
    if (ncams < 1 || ncams > MCORB_MAX_CAMS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_CAMS cameras");
    TRY(check_params(params));
    if ((lids != nullptr) == (pts != nullptr)) return fail(MCORB_E_ARG, "exactly one of lids and pts");
    for (int i = 0; i < n; i++) {
        if (cam[i] < 0 || cam[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
        if (octave[i] < 0 || octave[i] >= params->nlevels) return fail(MCORB_E_ARG, "an octave outside the levels");
        if (lids && (lids[i] < 0 || lids[i] >= m->max_landmarks)) return fail(MCORB_E_ARG, "landmark id outside the store");
    }
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track_pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");
    if (lids)
        for (int i = 0; i < n; i++)
            if (!(m->flags[lids[i]] & kHasPt)) return fail(MCORB_E_STATE, "a landmark has no point");
    PoseJob job;
    PoseState init;
    memcpy(init.R, R, sizeof(init.R));
    memcpy(init.t, t, sizeof(init.t));
    pose_job_init(job, *params, ncams, cams, init);
    job.n = n;
    if (m->device < 0 || n == 0) {
        std::vector<PoseObs> obs((size_t)n);
        std::vector<double> X((size_t)n * 3);
        std::vector<uint8_t> alive((size_t)n);
        for (int i = 0; i < n; i++) {
            obs[i] = PoseObs{uv[2 * i], uv[2 * i + 1], cam[i], octave[i]};
            memcpy(&X[3 * (size_t)i], lids ? &m->geom[(size_t)lids[i] * 6] : pts + 3 * (size_t)i, 3 * sizeof(double));
        }
        pose_run_host(job, obs.data(), X.data(), n, alive.data(), *res);
        if (inlier && n) memcpy(inlier, alive.data(), (size_t)n);
        return MCORB_OK;
    }
    PoseBufs &b = m->pose_x;
    HIPCHK(hipSetDevice(m->device));
    (void)hipGetLastError();   // (a stale error of this thread is not this call's)
    const size_t off_obs = round32(sizeof(PoseJob)), off_pt = off_obs + round32((size_t)n * sizeof(PoseObs));
    const size_t bytes = off_pt + (size_t)n * (lids ? sizeof(int32_t) : 3 * sizeof(double));
    TRY(b.h_in.grow(bytes, hipHostMallocDefault));
    TRY(b.d_in.grow(bytes));
    TRY(b.d_alive.grow((size_t)n));
    TRY(b.h_out.grow(1, kHostMapped));
    TRY(b.h_flags.grow((size_t)n, kHostMapped));
    uint8_t *in = b.h_in;
    memcpy(in, &job, sizeof(job));
    PoseObs *obs = reinterpret_cast<PoseObs *>(in + off_obs);
    for (int i = 0; i < n; i++) obs[i] = PoseObs{uv[2 * i], uv[2 * i + 1], cam[i], octave[i]};
    if (lids)
        memcpy(in + off_pt, lids, (size_t)n * sizeof(int32_t));
    else
        memcpy(in + off_pt, pts, (size_t)n * 3 * sizeof(double));
    hipStream_t st = m->st;
    HIPCHK(hipMemcpyAsync(b.d_in, b.h_in, bytes, hipMemcpyHostToDevice, st));
    uint8_t *d = b.d_in.get();
    HIPCHK(hipEventRecord(m->ev14, st));
    launch_pose_refine(st, reinterpret_cast<const PoseJob *>(d), 1, reinterpret_cast<PoseObs *>(d + off_obs),
                       lids ? reinterpret_cast<int32_t *>(d + off_pt) : nullptr, lids ? nullptr : reinterpret_cast<const double *>(d + off_pt),
                       m->d_geom, b.d_alive, nullptr, nullptr, nullptr, nullptr, b.h_out, b.h_flags);
    const hipError_t launched = hipGetLastError();
    HIPCHK(hipEventRecord(m->ev15, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(launched);
    float ms = 0.f;
    ev_elapsed(&ms, m->ev14, m->ev15);
    m->us_pose = ms * 1000.f;
    *res = *b.h_out.get();
    if (inlier) memcpy(inlier, b.h_flags.get(), (size_t)n);
    return MCORB_OK;
}

int mcorb_lmap_last_pose_timing(mcorb_lmap *m, float us[1])
{
    TRY(check_lmap_handle(m, "lmap last_pose_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    us[0] = m->us_pose;
    return MCORB_OK;
}

int mcorb_lmap_set_track_refine(mcorb_lmap *m, const mcorb_pose_params *params)
{
    TRY(check_lmap(m, "lmap set_track_refine"));
    if (params) TRY(check_params(params));
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track_pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");
    m->track_refine = params != nullptr;
    if (params) m->track_refine_params = *params;
    return MCORB_OK;
}

int mcorb_lmap_last_track_pose(mcorb_lmap *m, int f, mcorb_pose_result *out, uint8_t *flags, int cap)
{
    TRY(check_lmap_handle(m, "lmap last_track_pose"));
    if (!out || cap < 0 || (cap && !flags)) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track_pending.load()) return fail(MCORB_E_STATE, "the tracking call has not been waited for");
    if (!m->track_pose_nf) return fail(MCORB_E_STATE, "the last tracking call ran without mcorb_lmap_set_track_refine, or there was none");
    const mcorb_lmap::TrackCall &tc = m->track_call;
    if (f < 0 || f >= m->track_pose_nf) return fail(MCORB_E_ARG, "a frame outside the call");
    const size_t at = (size_t)tc.ncams * tc.first[f];
    const uint8_t *src;
    if (tc.launched) {
        *out = m->pose_t.h_out.get()[f];
        src = m->pose_t.h_flags.get() + at;
    } else {
        *out = tc.pose[f];
        src = tc.pose_flags.data() + at;
    }
    if (flags && cap < out->n_obs) return fail(MCORB_E_CAP, "flags too small");
    if (flags && out->n_obs) memcpy(flags, src, (size_t)out->n_obs);
    return MCORB_OK;
}

void mcorb_pose_of_view(const mcorb_track_view *view, double R[9], double t[3])
{
    PoseState P;
    pose_of_view(view->R0, view->t0, P);
    memcpy(R, P.R, sizeof(P.R));
    memcpy(t, P.t, sizeof(P.t));
}

int mcorb_pose_eval(int ncams, const mcorb_track_cam *cams, int n, const int32_t *cam, const float *uv, const double *pts, const double *R,
                    const double *t, double *r, double *J, double *w)
{
    if (n < 0 || ncams < 1 || ncams > MCORB_MAX_CAMS || !cams || !R || !t || (n && (!cam || !uv || !pts || !r || !J || !w)))
        return fail(MCORB_E_ARG, "bad argument");
    for (int i = 0; i < n; i++)
        if (cam[i] < 0 || cam[i] >= ncams) return fail(MCORB_E_ARG, "a camera index outside the rig");
    PoseState P;
    memcpy(P.R, R, sizeof(P.R));
    memcpy(P.t, t, sizeof(P.t));
    const double k = sqrt(5.991);
    for (int i = 0; i < n; i++) {
        double Ji[2][6], rho;
        pose_residual<true>(cams[cam[i]], P, pts + 3 * (size_t)i, uv[2 * i], uv[2 * i + 1], r[2 * (size_t)i], r[2 * (size_t)i + 1], Ji);
        memcpy(J + 12 * (size_t)i, Ji, sizeof(Ji));
        pose_huber(r[2 * (size_t)i], r[2 * (size_t)i + 1], k, w[i], rho);
    }
    return MCORB_OK;
}

}  // extern "C"
