// mcorb_sac_gpu.hip -- the absolute rig pose by RANSAC of mcorb_sac.h on a device store (mcorb_sac.cpp): three launches on the
// store's stream, no workgroup waits on another.
//   k_sac_hypotheses   one lane per hypothesis: the draws, the four points (from the store's geometry by id, or given), the
//                      central minimal solver and the disambiguation; a model record per hypothesis
//   k_sac_hypotheses_rig   the same with the rig solver (MCORB_SAC_SOLVER_RIG), four lanes per hypothesis: the lanes of a quad
//                      compute the sample, the points and the quartic redundantly, then lane k takes root k -- Newton, pose,
//                      self-check, the fourth point's score -- and two xor-shuffle steps over the quad pick by (score, k) with
//                      the header's rule; the winning lane, or lane 0 without a model, writes the record.  Everything behind the
//                      sample is sac_rig_quad, which k_sac_solve_rig_selftest (mcorb_dev_sac_solve_rig_selftest) runs on
//                      caller-given problems in the same launch shape; k_sac_solve_selftest is the central solver's twin
//   k_sac_score        the hot path, H x S reprojections: a workgroup owns a tile of kSacTile consensus observations, whose
//                      bearing, point and camera each lane computes once and keeps in registers, and a block of kSacHypBlock
//                      hypotheses, whose models it reads at uniform addresses: consensus_count (mcorb_consensus.h)
//   k_sac_pick         every workgroup finds the arg-max of count[H] for itself (consensus_best_wg) and writes the winner's flags
//                      for its tile of all n observations (0 outside the consensus set); workgroup 0 writes the record to host-mapped memory
//                      and, when a refinement follows, the pose into the PoseJob k_pose_refine reads
// The arithmetic is the header's, so the host-only store gives the same bits.  No extraction job runs this and no benchmark leg
// times it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"
#include "mcorb_sac.h"

namespace mcorb {

static_assert(kSacTile == kWgLanes, "the workgroup of mcorb_device.h's reductions");

// an observation's point: given, or the store's of its id
struct SacPoint {
    const int32_t *lids;
    const double *pts, *geom;
    __device__ __forceinline__ void operator()(int i, double X[3]) const
    {
        const double *p = pts ? pts + 3 * (size_t)i : geom + 6 * (size_t)lids[i];
        X[0] = p[0];
        X[1] = p[1];
        X[2] = p[2];
    }
};

__global__ __launch_bounds__(64) void k_sac_hypotheses(const SacJob *__restrict__ job, const PoseObs *__restrict__ obs,
                                                       const int32_t *__restrict__ lids, const double *__restrict__ pts,
                                                       const double *__restrict__ geom, const int32_t *__restrict__ cons,
                                                       const int32_t *__restrict__ cam_first, const int32_t *__restrict__ cam_cons,
                                                       SacModel *__restrict__ models)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= job->H) return;
    const SacPoint point{lids, pts, geom};
    sac_hypothesis_central(*job, h, obs, point, cons, cam_first, cam_cons, models[h]);
}

// Everything of a rig hypothesis behind its sample, for lane k of its quad: the observations obs[s0 .. s3] of cameras of cams,
// their points through point, sac_rig_prepare, root k, the fourth point's score, and the two xor-shuffle steps over the quad
// with the header's rule -> whether this lane writes the record: the winning lane, or lane 0 without a model.  P: root k's pose;
// root: whether root k has one (before the fourth point is asked); hb, kb: whether the quad has a winner, and its root.  All
// four lanes of a quad call it with the same arguments but k, and all 64 lanes of the wave call it: the shuffles name lanes.
// k_sac_hypotheses_rig feeds it from sac_sample_rig, k_sac_solve_rig_selftest from problem h of a table
template <class Point>
__device__ __forceinline__ bool sac_rig_quad(const mcorb_track_cam *cams, const PoseObs *__restrict__ obs, const Point &point, bool ok,
                                             int32_t s0, int32_t s1, int32_t s2, int32_t s3, int k, PoseState &P, bool &root, int &hb,
                                             int &kb)
{
    P = PoseState{};
    double score = 0.0;
    bool has = false;
    root = false;
    if (ok) {
        const PoseObs o0 = obs[s0], o1 = obs[s1], o2 = obs[s2], o3 = obs[s3];
        const mcorb_track_cam &c0 = cams[o0.cam], &c1 = cams[o1.cam], &c2 = cams[o2.cam], &c3 = cams[o3.cam];
        double X0[3], X1[3], X2[3], X3[3], f1[3], f2[3], f3[3], f4[3];
        point(s0, X0);
        point(s1, X1);
        point(s2, X2);
        point(s3, X3);
        sac_bearing(c0, o0.u, o0.v, f1);
        sac_bearing(c1, o1.u, o1.v, f2);
        sac_bearing(c2, o2.u, o2.v, f3);
        sac_bearing(c3, o3.u, o3.v, f4);
        SacRig G;
        sac_rig_prepare(c0, c1, c2, f1, f2, f3, X0, X1, X2, G);
        root = sac_rig_root(G, k, c0, c1, c2, f1, f2, f3, X0, X1, X2, P);
        score = sac_score(c3, P, X3, f4);
        has = root && score == score;   // (a NaN never wins)
    }
    kb = k, hb = has ? 1 : 0;
    double sb = score;
#pragma unroll
    for (int step = 1; step <= 2; step <<= 1) {
        const int ko = __shfl_xor(kb, step, 64), ho = __shfl_xor(hb, step, 64);
        const double so = __shfl_xor(sb, step, 64);
        const bool beats = sac_root_beats(ho != 0, so, ko, hb != 0, sb, kb);
        kb = beats ? ko : kb;
        hb = beats ? ho : hb;
        sb = beats ? so : sb;
    }
    return hb ? k == kb : k == 0;
}

// Four lanes per hypothesis, 16 hypotheses per wave.  A quad's lanes hold the same h, so everything up to the quartic is the same
// in all four and every branch on it is uniform over the quad; the shuffles stay inside the quad.  Quads beyond H compute
// hypothesis H - 1 again and write nothing.
__global__ __launch_bounds__(64) void k_sac_hypotheses_rig(const SacJob *__restrict__ job, const PoseObs *__restrict__ obs,
                                                           const int32_t *__restrict__ lids, const double *__restrict__ pts,
                                                           const double *__restrict__ geom, const int32_t *__restrict__ cons,
                                                           SacModel *__restrict__ models)
{
    const int t = blockIdx.x * 64 + threadIdx.x, k = t & 3, H = job->H;
    const bool live = (t >> 2) < H;
    const int h = live ? t >> 2 : H - 1;
    const SacPoint point{lids, pts, geom};
    int32_t s0, s1, s2, s3;
    const bool ok = sac_sample_rig(job->seed, h, job->S, cons, s0, s1, s2, s3);
    PoseState P;
    bool root;
    int hb, kb;
    const bool writer = sac_rig_quad(job->cams, obs, point, ok, s0, s1, s2, s3, k, P, root, hb, kb);
    if (live && writer) sac_write_model(models[h], hb != 0, P, s0, s1, s2, s3);
}

// mcorb_dev_sac_solve_rig_selftest: problem h of a table in place of a hypothesis's sample -- its rig at cams + ncams h, its four
// observations obs[4 h ..] and points pts[4 h ..] -- in k_sac_hypotheses_rig's launch shape, so neighbouring problems share a
// wave as neighbouring hypotheses do.  The writer leaves the record k_sac_hypotheses_rig would (win[h]) and the winner's root
// (best[h], -1: none); every lane whose root has a pose leaves it in the problem's next free slot in root order, as
// sac_solve_rig visits them (R, t: four slots a problem, zeroed before the launch), lane 0 their count and the roots' mask
__global__ __launch_bounds__(64) void k_sac_solve_rig_selftest(const mcorb_track_cam *__restrict__ cams, int ncams,
                                                               const PoseObs *__restrict__ obs, const double *__restrict__ pts, int n,
                                                               double *__restrict__ R, double *__restrict__ tr, int32_t *__restrict__ count,
                                                               int32_t *__restrict__ mask, int32_t *__restrict__ best,
                                                               SacModel *__restrict__ win)
{
    const int t = blockIdx.x * 64 + threadIdx.x, k = t & 3;
    const bool live = (t >> 2) < n;
    const int h = live ? t >> 2 : n - 1;
    const SacPoint point{nullptr, pts, nullptr};
    const int32_t s0 = 4 * h, s1 = 4 * h + 1, s2 = 4 * h + 2, s3 = 4 * h + 3;
    PoseState P;
    bool root;
    int hb, kb;
    const bool writer = sac_rig_quad(cams + (size_t)ncams * h, obs, point, true, s0, s1, s2, s3, k, P, root, hb, kb);
    const int roots = (int)((__ballot(root) >> (threadIdx.x & 60)) & 15ull);   // (the quad's four)
    if (!live) return;
    if (writer) {
        sac_write_model(win[h], hb != 0, P, s0, s1, s2, s3);
        best[h] = hb ? kb : -1;
    }
    if (k == 0) {
        count[h] = __popc(roots);
        mask[h] = roots;
    }
    if (root) {
        const size_t at = 4 * (size_t)h + __popc(roots & ((1 << k) - 1));
        for (int j = 0; j < 9; j++) R[9 * at + j] = P.R[j];
        for (int j = 0; j < 3; j++) tr[3 * at + j] = P.t[j];
    }
}

// mcorb_dev_sac_solve_selftest: the central solver, sac_solve of the header as k_sac_hypotheses' sac_model calls it, on problem
// h of a table, one lane each: camera cams[h], keypoints uv[3 h ..], points pts[3 h ..]; R, t: four slots a problem, zeroed
// before the launch
struct SacCollectDev {
    double *R, *t;
    int n;
    __device__ void operator()(const PoseState &P)
    {
        if (n >= 4) return;   // (a quartic has four roots: the slots are never exceeded, whatever the solver visits)
        for (int j = 0; j < 9; j++) R[9 * n + j] = P.R[j];
        for (int j = 0; j < 3; j++) t[3 * n + j] = P.t[j];
        n++;
    }
};

__global__ __launch_bounds__(64) void k_sac_solve_selftest(const mcorb_track_cam *__restrict__ cams, const float *__restrict__ uv,
                                                           const double *__restrict__ pts, int n, double *__restrict__ R,
                                                           double *__restrict__ tr, int32_t *__restrict__ count)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= n) return;
    const mcorb_track_cam cam = cams[h];
    const float *q = uv + 6 * (size_t)h;
    const double *X = pts + 9 * (size_t)h;
    double f[3][3];
    for (int k = 0; k < 3; k++) sac_bearing(cam, q[2 * k], q[2 * k + 1], f[k]);
    SacCollectDev collect{R + 36 * (size_t)h, tr + 12 * (size_t)h, 0};
    sac_solve(cam, f[0], f[1], f[2], X, X + 3, X + 6, collect);
    count[h] = collect.n;
}

#ifdef MCORB_SAC_RIG_ONE_LANE
// the experiment k_sac_hypotheses_rig was measured against: one lane per hypothesis, the four roots in turn
__global__ __launch_bounds__(64) void k_sac_hypotheses_rig1(const SacJob *__restrict__ job, const PoseObs *__restrict__ obs,
                                                            const int32_t *__restrict__ lids, const double *__restrict__ pts,
                                                            const double *__restrict__ geom, const int32_t *__restrict__ cons,
                                                            SacModel *__restrict__ models)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= job->H) return;
    const SacPoint point{lids, pts, geom};
    sac_hypothesis_rig(*job, h, obs, point, cons, models[h]);
}
#endif

__global__ __launch_bounds__(kSacTile) void k_sac_score(const SacJob *__restrict__ job, const PoseObs *__restrict__ obs,
                                                        const int32_t *__restrict__ lids, const double *__restrict__ pts,
                                                        const double *__restrict__ geom, const int32_t *__restrict__ cons,
                                                        const SacModel *__restrict__ models, int32_t *__restrict__ count)
{
    __shared__ int32_t cnt[kSacHypBlock];
    const int S = job->S;
    const int k = blockIdx.x * kSacTile + threadIdx.x;
    const bool in = k < S;
    const int i = cons[in ? k : 0];   // (S >= 1: a lane beyond the set scores observation cons[0] and counts nothing)
    const PoseObs o = obs[i];
    const mcorb_track_cam cam = job->cams[o.cam];
    const double threshold = job->threshold;
    double f[3], X[3];
    sac_bearing(cam, o.u, o.v, f);
    SacPoint{lids, pts, geom}(i, X);
    consensus_count<kSacHypBlock>(
        job->H, count, cnt, [&](int h) { return models[h].valid; },   // (uniform over the workgroup: scalar loads)
        [&](int h) {
            PoseState P;
            pose_load(P, models[h].R, models[h].t);
            return in && sac_is_inlier(sac_score(cam, P, X, f), threshold);
        });
}

__global__ __launch_bounds__(kSacTile) void k_sac_pick(const SacJob *__restrict__ job, const PoseObs *__restrict__ obs,
                                                       const int32_t *__restrict__ lids, const double *__restrict__ pts,
                                                       const double *__restrict__ geom, const uint8_t *__restrict__ is_first,
                                                       const SacModel *__restrict__ models, const int32_t *__restrict__ count,
                                                       SacOut *out, uint8_t *flags, PoseJob *pose_job)
{
    __shared__ unsigned long long wkey[4];
    __shared__ int32_t wmodels[4];
    const int t = threadIdx.x;
    const int n = job->n;
    int32_t n_models;
    const int best = consensus_best_wg<kSacKeyBits, 1>(   // (the same in every lane)
        job->H, [&](int h) { return models[h].valid; }, [&](int h) { return count[h]; }, wkey, wmodels, n_models);
    PoseState P;
    pose_identity(P);
    if (best >= 0) pose_load(P, models[best].R, models[best].t);
    const int i = blockIdx.x * kSacTile + t;
    if (i < n) {
        uint8_t flag = 0;
        if (best >= 0 && is_first[i]) {
            const PoseObs o = obs[i];
            double f[3], X[3];
            sac_bearing(job->cams[o.cam], o.u, o.v, f);
            SacPoint{lids, pts, geom}(i, X);
            flag = sac_is_inlier(sac_score(job->cams[o.cam], P, X, f), job->threshold) ? 1 : 0;
        }
        flags[i] = flag;
    }
    if (blockIdx.x == 0 && t == 0) {
        for (int j = 0; j < 9; j++) out->R[j] = P.R[j];
        for (int j = 0; j < 3; j++) out->t[j] = P.t[j];
        out->status = best >= 0 ? MCORB_SAC_OK : MCORB_SAC_NO_MODEL;
        out->n_inliers = best >= 0 ? count[best] : 0;
        out->best = best;
        out->n_models = n_models;
        for (int j = 0; j < 4; j++) out->sample[j] = best >= 0 ? models[best].sample[j] : -1;
        if (pose_job) {
            for (int j = 0; j < 9; j++) pose_job->init.R[j] = P.R[j];
            for (int j = 0; j < 3; j++) pose_job->init.t[j] = P.t[j];
        }
    }
}

void launch_sac_hypotheses(hipStream_t st, const SacArgs &a, int H)
{
    hipLaunchKernelGGL(k_sac_hypotheses, dim3((H + 63) / 64), dim3(64), 0, st, a.job, a.obs, a.lids, a.pts, a.geom, a.cons, a.cam_first,
                       a.cam_cons, a.models);
}

void launch_sac_hypotheses_rig(hipStream_t st, const SacArgs &a, int H)
{
#ifdef MCORB_SAC_RIG_ONE_LANE
    hipLaunchKernelGGL(k_sac_hypotheses_rig1, dim3((H + 63) / 64), dim3(64), 0, st, a.job, a.obs, a.lids, a.pts, a.geom, a.cons, a.models);
#else
    hipLaunchKernelGGL(k_sac_hypotheses_rig, dim3((4 * H + 63) / 64), dim3(64), 0, st, a.job, a.obs, a.lids, a.pts, a.geom, a.cons, a.models);
#endif
}

void launch_sac_solve_selftest(hipStream_t st, const mcorb_track_cam *cams, const float *uv, const double *pts, int n, double *R, double *t,
                                int32_t *count)
{
    hipLaunchKernelGGL(k_sac_solve_selftest, dim3((n + 63) / 64), dim3(64), 0, st, cams, uv, pts, n, R, t, count);
}

void launch_sac_solve_rig_selftest(hipStream_t st, const mcorb_track_cam *cams, int ncams, const PoseObs *obs, const double *pts, int n, double *R,
                                    double *t, int32_t *count, int32_t *mask, int32_t *best, SacModel *win)
{
    hipLaunchKernelGGL(k_sac_solve_rig_selftest, dim3((4 * n + 63) / 64), dim3(64), 0, st, cams, ncams, obs, pts, n, R, t, count, mask, best, win);
}

void launch_sac_score(hipStream_t st, const SacArgs &a, int S, int H)
{
    hipLaunchKernelGGL(k_sac_score, dim3((S + kSacTile - 1) / kSacTile, (H + kSacHypBlock - 1) / kSacHypBlock), dim3(kSacTile), 0, st, a.job,
                       a.obs, a.lids, a.pts, a.geom, a.cons, a.models, a.count);
}

void launch_sac_pick(hipStream_t st, const SacArgs &a, int n)
{
    hipLaunchKernelGGL(k_sac_pick, dim3((n + kSacTile - 1) / kSacTile), dim3(kSacTile), 0, st, a.job, a.obs, a.lids, a.pts, a.geom,
                       a.is_first, a.models, a.count, a.out, a.flags, a.pose_job);
}

}  // namespace mcorb
