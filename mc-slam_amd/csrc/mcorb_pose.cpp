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

int pose_check_params(const mcorb_pose_params *p)
{
    if (!p) return fail(MCORB_E_ARG, "bad argument");
    if (p->nlevels < 1 || p->nlevels > MCORB_MAX_LEVELS) return fail(MCORB_E_ARG, "1 .. MCORB_MAX_LEVELS levels");
    if (p->max_iterations < 1 || p->max_iterations > 100) return fail(MCORB_E_ARG, "1 .. 100 iterations");
    return MCORB_OK;
}

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

// ---- the observation input of the two explicit entries (mcorb_lmap_refine_pose, mcorb_lmap_ransac_pose) ----
static int obs_fail(const char *who, int code, const char *what) { set_error(std::string(who) + what); return code; }

int obs_check(const mcorb_lmap *m, const ObsInput &in, int nlevels, const int32_t *match, const char *who)
{
    const int n = in.n;
    if (n < 0 || !in.cams || (n && (!in.cam || !in.uv || !in.octave))) return obs_fail(who, MCORB_E_ARG, "bad argument");
    if (in.ncams < 1 || in.ncams > MCORB_MAX_CAMS) return obs_fail(who, MCORB_E_ARG, "1 .. MCORB_MAX_CAMS cameras");
    if ((in.lids != nullptr) == (in.pts != nullptr)) return obs_fail(who, MCORB_E_ARG, "exactly one of lids and pts");
    for (int i = 0; i < n; i++) {
        if (in.cam[i] < 0 || in.cam[i] >= in.ncams) return obs_fail(who, MCORB_E_ARG, "a camera index outside the rig");
        if (in.octave[i] < 0 || in.octave[i] >= nlevels) return obs_fail(who, MCORB_E_ARG, "an octave outside the levels");
        if (in.lids && (in.lids[i] < 0 || in.lids[i] >= m->max_landmarks)) return obs_fail(who, MCORB_E_ARG, "landmark id outside the store");
        if (match && (match[i] < 0 || (i && match[i] < match[i - 1])))
            return obs_fail(who, MCORB_E_ARG, "a match index that is negative or decreases");
    }
    return MCORB_OK;
}

int obs_check_locked(const mcorb_lmap *m, const ObsInput &in, const char *who)
{
    if (m->track.pending.load()) return obs_fail(who, MCORB_E_STATE, "a submitted tracking call has not been waited for");
    if (in.lids)
        for (int i = 0; i < in.n; i++)
            if (!(m->flags[in.lids[i]] & kHasPt)) return obs_fail(who, MCORB_E_STATE, "a landmark has no point");
    return MCORB_OK;
}

static void obs_rows(const ObsInput in, PoseObs *obs)   // (by value: the stores to obs cannot be stores to its fields)
{
    for (int i = 0; i < in.n; i++) obs[i] = PoseObs{in.uv[2 * i], in.uv[2 * i + 1], in.cam[i], in.octave[i]};
}

void obs_gather(const mcorb_lmap *m, const ObsInput &in, std::vector<PoseObs> &obs, std::vector<double> &X)
{
    obs.resize((size_t)in.n);
    X.resize((size_t)in.n * 3);
    obs_rows(in, obs.data());
    for (int i = 0; i < in.n; i++)
        memcpy(&X[3 * (size_t)i], in.lids ? &m->geom[(size_t)in.lids[i] * 6] : in.pts + 3 * (size_t)i, 3 * sizeof(double));
}

void obs_stage(const ObsInput &in, const ObsLayout &L, const Staged &s)
{
    obs_rows(in, s.host<PoseObs>(L.obs));
    if (in.lids)
        memcpy(s.host<int32_t>(L.pt), in.lids, (size_t)in.n * sizeof(int32_t));
    else
        memcpy(s.host<double>(L.pt), in.pts, (size_t)in.n * 3 * sizeof(double));
}

void obs_enqueue_refine(const mcorb_lmap *m, const ObsInput &in, const ObsLayout &L, const Staged &s, const PoseBufs &b)
{
    launch_pose_refine(m->st, s.dev<const PoseJob>(L.pose_job), 1, s.dev<PoseObs>(L.obs), in.lids ? s.dev<int32_t>(L.pt) : nullptr,
                       in.lids ? nullptr : s.dev<const double>(L.pt), m->d_geom, b.d_alive, nullptr, nullptr, nullptr, nullptr, b.h_out,
                       b.h_flags);
}

// ---- behind a tracking call (mcorb_track.cpp; the caller holds the store's lock) ----
// the job of frame f of the pending call: the rig and the initial pose of its view
static void track_job(const mcorb_lmap *m, const mcorb_track_view &view, PoseJob &job)
{
    PoseState init;
    pose_of_view(view.R0, view.t0, init);
    pose_job_init(job, m->track.refine_params, view.ncams, view.cams, init);
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

// a device store: k_pose_refine for the nf frames of the submission sub, behind its de-duplication on the store's stream; the
// buffers are reserved (PoseBufs::reserve_track).  items:
// the submission's, on the host -- a frame's candidates, block of the per-pair arrays and keypoints in kp_xy are where they say
void pose_track_submit(Submission &sub, mcorb_lmap *m, const mcorb_track_view *views, const TrItem *items, int nf, const float2 *kp_xy,
                       const int *d_cand)
{
    const PoseBufs &b = m->pose.t;
    const int C = views[0].ncams;
    PoseJob *jobs = b.in.host<PoseJob>(0);
    for (int f = 0; f < nf; f++) {
        PoseJob &job = jobs[f];
        const TrItem &it = items[f];
        track_job(m, views[f], job);
        job.from_track = 1;
        job.n_cand = it.n;
        job.n = C * job.n_cand;
        job.cand_first = it.cand_first;
        job.obs0 = job.rows = it.rows;
        job.kp0 = it.kp0;
        job.frame = it.frame;
    }
    b.in.upload(sub, (size_t)nf * sizeof(PoseJob));
    sub.run([&] {
        launch_pose_refine(m->st, b.in.dev<const PoseJob>(0), nf, b.d_obs, b.d_lids, nullptr, m->d_geom, b.d_alive, m->track.d_win,
                           m->track.d_best, d_cand, kp_xy, b.h_out, b.h_flags);
    });
}

}  // namespace mcorb

extern "C" {

int mcorb_lmap_refine_pose(mcorb_lmap *m, int n, const int32_t *cam, const float *uv, const int32_t *octave, const int32_t *lids,
                           const double *pts, int ncams, const mcorb_track_cam *cams, const double *R, const double *t,
                           const mcorb_pose_params *params, mcorb_pose_result *res, uint8_t *inlier)
{
    const char *who = "lmap pose: ";
    TRY(check_lmap(m, "lmap refine_pose"));
    if (!R || !t || !res) return fail(MCORB_E_ARG, "bad argument");
    TRY(pose_check_params(params));
    const ObsInput in{n, cam, uv, octave, lids, pts, ncams, cams};
    TRY(obs_check(m, in, params->nlevels, nullptr, who));
    std::lock_guard<std::mutex> lk(m->mu);
    TRY(obs_check_locked(m, in, who));
    PoseJob job;
    PoseState init;
    memcpy(init.R, R, sizeof(init.R));
    memcpy(init.t, t, sizeof(init.t));
    pose_job_init(job, *params, ncams, cams, init);
    job.n = n;
    if (m->device < 0 || n == 0) {
        std::vector<PoseObs> obs;
        std::vector<double> X;
        std::vector<uint8_t> alive((size_t)n);
        obs_gather(m, in, obs, X);
        pose_run_host(job, obs.data(), X.data(), n, alive.data(), *res);
        if (inlier && n) memcpy(inlier, alive.data(), (size_t)n);
        return MCORB_OK;
    }
    PoseBufs &b = m->pose.x;
    HIPCHK(hipSetDevice(m->device));
    (void)hipGetLastError();   // (a stale error of this thread is not this call's)
    const ObsLayout L((size_t)n, lids != nullptr, false, 0, 0);
    TRY(b.in.reserve(L.p.total));
    TRY(b.reserve((size_t)n));
    *b.in.host<PoseJob>(L.pose_job) = job;
    obs_stage(in, L, b.in);
    hipStream_t st = m->st;
    Submission sub(st);
    b.in.upload(sub, L.p.total);
    sub.run(m->pose.refine, 0, [&] { obs_enqueue_refine(m, in, L, b.in, b); });
    sub.mark(m->pose.refine, 1);
    TRY(sub.wait());
    m->pose.refine.read();
    *res = *b.h_out.get();
    if (inlier) memcpy(inlier, b.h_flags.get(), (size_t)n);
    return MCORB_OK;
}

int mcorb_lmap_last_pose_timing(mcorb_lmap *m, float us[1])
{
    TRY(check_lmap_handle(m, "lmap last_pose_timing"));
    if (!us) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    us[0] = m->pose.refine.us[0];
    return MCORB_OK;
}

int mcorb_lmap_set_track_refine(mcorb_lmap *m, const mcorb_pose_params *params)
{
    TRY(check_lmap(m, "lmap set_track_refine"));
    if (params) TRY(pose_check_params(params));
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track.pending.load()) return fail(MCORB_E_STATE, "a submitted tracking call has not been waited for");
    m->track.refine = params != nullptr;
    if (params) m->track.refine_params = *params;
    return MCORB_OK;
}

int mcorb_lmap_last_track_pose(mcorb_lmap *m, int f, mcorb_pose_result *out, uint8_t *flags, int cap)
{
    TRY(check_lmap_handle(m, "lmap last_track_pose"));
    if (!out || cap < 0 || (cap && !flags)) return fail(MCORB_E_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->track.pending.load()) return fail(MCORB_E_STATE, "the tracking call has not been waited for");
    if (!m->track.pose_nf) return fail(MCORB_E_STATE, "the last tracking call ran without mcorb_lmap_set_track_refine, or there was none");
    const mcorb_lmap::TrackCall &tc = m->track.call;
    if (f < 0 || f >= m->track.pose_nf) return fail(MCORB_E_ARG, "a frame outside the call");
    const size_t at = (size_t)tc.ncams * tc.first[f];
    const uint8_t *src;
    if (tc.launched) {
        *out = m->pose.t.h_out.get()[f];
        src = m->pose.t.h_flags.get() + at;
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
