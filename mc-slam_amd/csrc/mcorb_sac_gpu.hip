// mcorb_sac_gpu.hip -- the absolute rig pose by RANSAC of mcorb_sac.h on a device store (mcorb_sac.cpp): three launches on the
// store's stream, no workgroup waits on another.
//   k_sac_hypotheses   one lane per hypothesis: the draws, the four points (from the store's geometry by id, or given), the
//                      minimal solver and the disambiguation; a model record per hypothesis
//   k_sac_score        the hot path, H x S reprojections: a workgroup owns a tile of kSacTile consensus observations, whose
//                      bearing, point and camera each lane computes once and keeps in registers, and a block of kSacHypBlock
//                      hypotheses, whose models it reads at uniform addresses; per model a ballot and a population count per
//                      wave into integer counts in LDS, then one integer atomicAdd per (workgroup, hypothesis) into count[H].
//                      The additions are integer: the result does not depend on their order
//   k_sac_pick         every workgroup finds the arg-max of count[H] for itself and writes the winner's flags for its tile of
//                      all n observations (0 outside the consensus set); workgroup 0 writes the record to host-mapped memory
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

static_assert(kSacTile == 4 * 64, "four waves");
static_assert(kSacHypBlock <= kSacTile, "a lane per hypothesis of the block adds its count");

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
    sac_hypothesis(*job, h, obs, point, cons, cam_first, cam_cons, models[h]);
}

__global__ __launch_bounds__(kSacTile) void k_sac_score(const SacJob *__restrict__ job, const PoseObs *__restrict__ obs,
                                                        const int32_t *__restrict__ lids, const double *__restrict__ pts,
                                                        const double *__restrict__ geom, const int32_t *__restrict__ cons,
                                                        const SacModel *__restrict__ models, int32_t *__restrict__ count)
{
    __shared__ int32_t cnt[kSacHypBlock];
    const int t = threadIdx.x, lane = t & 63;
    const int S = job->S, H = job->H;
    const int k = blockIdx.x * kSacTile + t;
    const bool in = k < S;
    const int i = cons[in ? k : 0];   // (S >= 1: a lane beyond the set scores observation cons[0] and counts nothing)
    const PoseObs o = obs[i];
    const mcorb_track_cam cam = job->cams[o.cam];
    const double threshold = job->threshold;
    double f[3], X[3];
    sac_bearing(cam, o.u, o.v, f);
    SacPoint{lids, pts, geom}(i, X);
    if (t < kSacHypBlock) cnt[t] = 0;
    __syncthreads();
    const int h0 = blockIdx.y * kSacHypBlock, h1 = min(H, h0 + kSacHypBlock);
    for (int h = h0; h < h1; h++) {
        const SacModel &M = models[h];   // (uniform over the workgroup: scalar loads)
        if (!M.valid) continue;
        PoseState P;
#pragma unroll
        for (int j = 0; j < 9; j++) P.R[j] = M.R[j];
#pragma unroll
        for (int j = 0; j < 3; j++) P.t[j] = M.t[j];
        const bool inl = in && sac_is_inlier(sac_score(cam, P, X, f), threshold);
        const unsigned long long mask = __ballot(inl);
        if (lane == 0 && mask) atomicAdd(&cnt[h - h0], __popcll(mask));
    }
    __syncthreads();
    if (t < h1 - h0 && cnt[t]) atomicAdd(&count[h0 + t], cnt[t]);
}

__global__ __launch_bounds__(kSacTile) void k_sac_pick(const SacJob *__restrict__ job, const PoseObs *__restrict__ obs,
                                                       const int32_t *__restrict__ lids, const double *__restrict__ pts,
                                                       const double *__restrict__ geom, const uint8_t *__restrict__ is_first,
                                                       const SacModel *__restrict__ models, const int32_t *__restrict__ count,
                                                       SacOut *out, uint8_t *flags, PoseJob *pose_job)
{
    __shared__ unsigned long long wkey[4];
    __shared__ int32_t wmodels[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = job->n, H = job->H;
    unsigned long long key = 0;
    int32_t nm = 0;
    for (int h = t; h < H; h += kSacTile) {
        const int32_t valid = models[h].valid;
        const unsigned long long kh = sac_key(valid, count[h], h);
        key = kh > key ? kh : key;
        nm += valid;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long other = __shfl_xor(key, s, 64);
        key = other > key ? other : key;
        nm += __shfl_xor(nm, s, 64);
    }
    if (lane == 0) {
        wkey[wave] = key;
        wmodels[wave] = nm;
    }
    __syncthreads();
    key = wkey[0];
    for (int w = 1; w < 4; w++) key = wkey[w] > key ? wkey[w] : key;
    const int best = sac_key_hypothesis(key);   // (the same in every lane)
    PoseState P;
#pragma unroll
    for (int j = 0; j < 9; j++) P.R[j] = (j % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) P.t[j] = 0.0;
    if (best >= 0) {
        const SacModel &M = models[best];
#pragma unroll
        for (int j = 0; j < 9; j++) P.R[j] = M.R[j];
#pragma unroll
        for (int j = 0; j < 3; j++) P.t[j] = M.t[j];
    }
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
        out->n_models = (wmodels[0] + wmodels[1]) + (wmodels[2] + wmodels[3]);
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
