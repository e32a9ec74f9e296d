// mcorb_rel_gpu.hip -- the relative rig pose between two frames by RANSAC of mcorb_rel.h on a device store (mcorb_rel.cpp): three
// launches on the store's stream, no workgroup waits on another.
//   k_rel_hypotheses   one lane per hypothesis: the 17 draws, the rays of the sample, the linear solver (its designs, the
//                      Gram-Schmidt basis and null_vector's factorisation are private arrays, so they live in scratch); a model
//                      record per hypothesis
//   k_rel_score        the hot path, H x S two-view midpoint triangulations with two angles each: a workgroup owns a tile of
//                      kRelTile matches, whose four ray vectors each lane computes once and keeps in registers, and a block of
//                      kRelHypBlock hypotheses, whose models it reads at uniform addresses: consensus_count (mcorb_consensus.h)
//   k_rel_pick         every workgroup finds the arg-max of count[H] for itself (consensus_best_wg) and writes the winner's flags
//                      for its tile of matches; workgroup 0 writes the record to host-mapped memory
//   k_rel_fit          the polished call only, behind a k_rel_pick whose record and flags stay in device memory: ONE workgroup of
//                      256 -- the rounds of the header's polish (pose_round over the members, the 28 sums folded by wg_fold of
//                      mcorb_device.h, then all S matches scored at the result), and the accepted record, its flags and the polish
//                      record to host-mapped memory
// The arithmetic is the header's, so the host-only store gives the same bits.  No extraction job runs this and no benchmark leg
// times it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"
#include "mcorb_rel.h"

namespace mcorb {

static_assert(kRelTile == kWgLanes && kRelTile == MCORB_POSE_LANES, "mcorb_device.h's workgroup, a lane of pose_fold each");

__global__ __launch_bounds__(64) void k_rel_hypotheses(const RelJob *__restrict__ job, const RelObs *__restrict__ obs,
                                                       RelModel *__restrict__ models)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= job->H) return;
    rel_hypothesis(*job, h, obs, models[h]);
}

// mcorb_dev_rel_solve_selftest: rel_solve17 of the header, as k_rel_hypotheses' rel_hypothesis calls it, on problem h of a table,
// one lane each: its rig at cams + ncams h, its 17 matches with keypoints as doubles (rel_rays_d, as mcorb_rel_solve forms the
// rays).  Without a model the slot is zero
__global__ __launch_bounds__(64) void k_rel_solve_selftest(const mcorb_track_cam *__restrict__ cams, int ncams, const int32_t *__restrict__ cam1,
                                                           const double *__restrict__ uv1, const int32_t *__restrict__ cam2,
                                                           const double *__restrict__ uv2, int n, double *__restrict__ R,
                                                           double *__restrict__ tr, int32_t *__restrict__ count)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= n) return;
    const size_t at = (size_t)kRelSample * h;
    RelRays rays[kRelSample];
    for (int j = 0; j < kRelSample; j++)
        rel_rays_d(cams + (size_t)ncams * h, cam1[at + j], uv1 + 2 * (at + j), cam2[at + j], uv2 + 2 * (at + j), rays[j]);
    PoseState P;
    const bool ok = rel_solve17(rays, P);
    for (int j = 0; j < 9; j++) R[9 * (size_t)h + j] = ok ? P.R[j] : 0.0;
    for (int j = 0; j < 3; j++) tr[3 * (size_t)h + j] = ok ? P.t[j] : 0.0;
    count[h] = ok ? 1 : 0;
}

void launch_rel_solve_selftest(hipStream_t st, const mcorb_track_cam *cams, int ncams, const int32_t *cam1, const double *uv1, const int32_t *cam2,
                                const double *uv2, int n, double *R, double *t, int32_t *count)
{
    hipLaunchKernelGGL(k_rel_solve_selftest, dim3((n + 63) / 64), dim3(64), 0, st, cams, ncams, cam1, uv1, cam2, uv2, n, R, t, count);
}

__global__ __launch_bounds__(kRelTile) void k_rel_score(const RelJob *__restrict__ job, const RelObs *__restrict__ obs,
                                                        const RelModel *__restrict__ models, int32_t *__restrict__ count)
{
    __shared__ int32_t cnt[kRelHypBlock];
    const int S = job->S;
    const int k = blockIdx.x * kRelTile + threadIdx.x;
    const bool in = k < S;
    const double threshold = job->threshold;
    RelRays r;
    rel_rays(job->cams, obs[in ? k : 0], r);   // (S >= 1: a lane beyond the matches scores match 0 and counts nothing)
    consensus_count<kRelHypBlock>(
        job->H, count, cnt, [&](int h) { return models[h].valid; },   // (uniform over the workgroup)
        [&](int h) {
            PoseState P;
            pose_load(P, models[h].R, models[h].t);
            return in && sac_is_inlier(rel_score(P, r), threshold);
        });
}

__global__ __launch_bounds__(kRelTile) void k_rel_pick(const RelJob *__restrict__ job, const RelObs *__restrict__ obs,
                                                       const RelModel *__restrict__ models, const int32_t *__restrict__ count, RelOut *out,
                                                       uint8_t *flags)
{
    __shared__ unsigned long long wkey[4];
    __shared__ int32_t wmodels[4];
    const int t = threadIdx.x;
    const int S = job->S;
    int32_t n_models;
    const int best = consensus_best_wg<kRelKeyBits, 1>(   // (the same in every lane)
        job->H, [&](int h) { return models[h].valid; }, [&](int h) { return count[h]; }, wkey, wmodels, n_models);
    PoseState P;
    pose_identity(P);
    if (best >= 0) pose_load(P, models[best].R, models[best].t);
    const int i = blockIdx.x * kRelTile + t;
    if (i < S) {
        uint8_t flag = 0;
        if (best >= 0) {
            RelRays r;
            rel_rays(job->cams, obs[i], r);
            flag = sac_is_inlier(rel_score(P, r), job->threshold) ? 1 : 0;
        }
        flags[i] = flag;
    }
    if (blockIdx.x == 0 && t == 0) {
        for (int j = 0; j < 9; j++) out->R[j] = P.R[j];
        for (int j = 0; j < 3; j++) out->t[j] = P.t[j];
        out->status = best >= 0 ? MCORB_REL_OK : MCORB_REL_NO_MODEL;
        out->n_inliers = best >= 0 ? count[best] : 0;
        out->best = best;
        out->n_models = n_models;
        for (int j = 0; j < kRelSample; j++) out->sample[j] = best >= 0 ? models[best].sample[j] : -1;
        for (int j = 0; j < 3; j++) out->pad[j] = 0;
    }
}

// a lane's 28 sums while it walks its members: column threadIdx.x of acc[28][256] in LDS, touched by that lane alone.  In
// registers they would be live through the seven residual evaluations of every member and the kernel would spill
struct RelFitLaneSums {
    double *base;
    __device__ __forceinline__ double &operator[](int k) const { return base[k * kRelTile]; }
};

// a pass of k_rel_fit: the 28 sums at P over the members, the same bits in every lane.  Lanes 0 .. 6 leave P and its six
// perturbations in LDS, every lane reads them at uniform addresses; lane l adds members l, l + 256, .. into its column of acc,
// takes the 28 into registers, and the workgroup folds them (wg_fold).  Both barriers are met by every lane; poses and part are
// written again only behind a barrier that every lane reaches after it has read them: the next pass's first
struct RelFitPass {
    const RelJob *job;
    const RelObs *obs;
    const uint8_t *member;
    int S;
    double scale;
    PoseState *poses;
    double (*part)[kPoseSums];
    double (*acc)[kRelTile];
    __device__ __forceinline__ void operator()(const PoseState &P, double sums[kPoseSums])
    {
        const int t = threadIdx.x;
        if (t < kRelFitPoses) {
            PoseState Q;
            rel_fit_pose(P, t, Q);
            pose_load(poses[t], Q.R, Q.t);
        }
        __syncthreads();
        const RelFitLaneSums mine{&acc[0][t]};
#pragma unroll
        for (int k = 0; k < kPoseSums; k++) mine[k] = 0.0;
        for (int i = t; i < S; i += kRelTile) {
            if (!member[i]) continue;
            RelRays r;
            rel_rays(job->cams, obs[i], r);
            rel_fit_add(poses, r, scale, mine);
        }
        double s[kPoseSums];
#pragma unroll
        for (int k = 0; k < kPoseSums; k++) s[k] = mine[k];
        wg_fold<kPoseSums>(s, part, sums);
    }
};

// ONE workgroup, for k_align_fit's reason: the sums are floating-point and their order is part of the definition.  pick and
// member[0 .. S) are what k_rel_pick left in device memory; nothing host-mapped is read.  Every lane holds the same pose, count
// and verdicts, so the rounds' control flow is uniform; a match's flags are read and written by the one lane that serves it
__global__ __launch_bounds__(kRelTile) void k_rel_fit(const RelJob *__restrict__ job, const RelObs *__restrict__ obs, const RelOut *pick,
                                                      uint8_t *member, int rounds, int max_iterations, RelOut *out, uint8_t *flags,
                                                      RelPolish *polish)
{
    __shared__ PoseState poses[kRelFitPoses];
    __shared__ double part[kPoseBlocks][kPoseSums];
    __shared__ double acc[kPoseSums][kRelTile];
    __shared__ int32_t wcnt[kPoseBlocks];
    const int t = threadIdx.x;
    const int S = job->S;
    const double threshold = job->threshold;
    PoseState cur;
#pragma unroll
    for (int j = 0; j < 9; j++) cur.R[j] = pick->R[j];   // (not pose_load: at 256 VGPRs the kernel spilled with it)
#pragma unroll
    for (int j = 0; j < 3; j++) cur.t[j] = pick->t[j];
    int32_t count = pick->n_inliers;
    uint8_t *curf = member, *other = member + S;
    if (t == 0) rel_polish_begin(*polish, cur, count);
    if (pick->best >= 0) {   // (uniform over the workgroup)
        RelFitPass pass{job, obs, curf, S, rel_fit_scale(threshold), poses, part, acc};
        for (int round = 0; round < rounds; round++) {
            pass.member = curf;
            int mine = 0;
            for (int i = t; i < S; i += kRelTile) mine += curf[i] ? 1 : 0;
            const int members = wg_total(mine, wcnt);
            PoseState cand;
            double c0, c1;
            int32_t its, status;
            pose_round(pass, cur, max_iterations, cand, its, status, c0, c1);
            int in = 0;
            for (int i = t; i < S; i += kRelTile) {
                RelRays r;
                rel_rays(job->cams, obs[i], r);
                const uint8_t flag = sac_is_inlier(rel_score(cand, r), threshold) ? 1 : 0;
                other[i] = flag;
                in += flag;
            }
            const int n = wg_total(in, wcnt);
            const bool accepted = n >= count;
            if (t == 0) {
                mcorb_rel_polish_round &q = polish->round[round];
                q.cost_initial = pose_default_nan(c0);
                q.cost_final = pose_default_nan(c1);
                q.n_members = members;
                q.iterations = its;
                q.status = status;
                q.n_inliers = n;
                q.accepted = accepted ? 1 : 0;
                polish->rounds_run = round + 1;
            }
            if (!accepted) break;
            cur = cand;
            count = n;
            uint8_t *swap = curf;
            curf = other;
            other = swap;
        }
    }
    for (int i = t; i < S; i += kRelTile) flags[i] = curf[i];
    if (t == 0) {
        for (int j = 0; j < 9; j++) out->R[j] = cur.R[j];
        for (int j = 0; j < 3; j++) out->t[j] = cur.t[j];
        out->status = pick->status;
        out->n_inliers = count;
        out->best = pick->best;
        out->n_models = pick->n_models;
        for (int j = 0; j < kRelSample; j++) out->sample[j] = pick->sample[j];
        for (int j = 0; j < 3; j++) out->pad[j] = 0;
    }
}

void launch_rel_fit(hipStream_t st, const RelFitArgs &a)
{
    hipLaunchKernelGGL(k_rel_fit, dim3(1), dim3(kRelTile), 0, st, a.job, a.obs, a.pick, a.member, a.rounds, a.max_iterations, a.out, a.flags,
                       a.polish);
}

void launch_rel_hypotheses(hipStream_t st, const RelArgs &a, int H)
{
    hipLaunchKernelGGL(k_rel_hypotheses, dim3((H + 63) / 64), dim3(64), 0, st, a.job, a.obs, a.models);
}

void launch_rel_score(hipStream_t st, const RelArgs &a, int S, int H)
{
    hipLaunchKernelGGL(k_rel_score, dim3((S + kRelTile - 1) / kRelTile, (H + kRelHypBlock - 1) / kRelHypBlock), dim3(kRelTile), 0, st, a.job,
                       a.obs, a.models, a.count);
}

void launch_rel_pick(hipStream_t st, const RelArgs &a, int S)
{
    hipLaunchKernelGGL(k_rel_pick, dim3((S + kRelTile - 1) / kRelTile), dim3(kRelTile), 0, st, a.job, a.obs, a.models, a.count, a.out, a.flags);
}

}  // namespace mcorb
