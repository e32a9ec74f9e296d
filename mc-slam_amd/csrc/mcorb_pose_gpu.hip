// mcorb_pose_gpu.hip -- k_pose_refine: the rig pose refinement of mcorb_pose.h on a device store (mcorb_pose.cpp), both rounds of
// FrontEnd::OptimizePose (MCSlam/src/FrontEnd.cpp:4361-4400) in one launch.  One workgroup of MCORB_POSE_LANES lanes per problem.
// A pass over the observations re-reads them from L2: lane l adds observations l, l + 256, .. into its 28 sums and the workgroup
// folds them by wg_fold of mcorb_device.h -- the tree mcorb_pose.h states, so the host-only store gives the same bits.  Every
// lane then solves the 6 x 6 system and retracts for itself: all lanes hold the same pose, take the same branches and meet at the
// same barriers.  The barrier is the only synchronisation: no workgroup waits on another, no atomics, no scratch.  An
// observation's flag is read and written by the one lane that serves it.  No extraction job runs this and no benchmark leg
// times it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"
#include "mcorb_pose.h"

namespace mcorb {

constexpr int kPoseT = MCORB_POSE_LANES;
static_assert(kPoseT == kWgLanes, "the workgroup of mcorb_device.h's reductions");

// the observations of one problem as a lane reads them
struct PoseSrc {
    const PoseJob *job;
    const PoseObs *obs;
    const int32_t *lids;
    const double *pts, *geom;
    uint8_t *alive;
    int n;
    __device__ __forceinline__ void point(int i, double X[3]) const
    {
        const double *p = pts ? pts + 3 * (size_t)i : geom + 6 * (size_t)lids[i];
        X[0] = p[0];
        X[1] = p[1];
        X[2] = p[2];
    }
};

// a pass: the 28 sums at P, the same bits in every lane.  Pass p leaves the waves' sums in half p & 1 of the LDS: a wave writes
// half h again only behind the barrier of the pass between, which every wave reaches after it has read h
struct PosePass {
    const PoseSrc &src;
    double (*part)[kPoseBlocks][kPoseSums];
    int half;
    __device__ __forceinline__ void operator()(const PoseState &P, double S[kPoseSums])
    {
        double s[kPoseSums];
#pragma unroll
        for (int k = 0; k < kPoseSums; k++) s[k] = 0.0;
        for (int i = threadIdx.x; i < src.n; i += kPoseT) {
            if (!src.alive[i]) continue;
            const PoseObs o = src.obs[i];
            double X[3];
            src.point(i, X);
            pose_add(src.job->cams[o.cam], P, X, o.u, o.v, src.job->huber_k, s);
        }
        wg_fold<kPoseSums>(s, part[half], S);
        half ^= 1;
    }
};

// The observations of a tracking submission's frame: per camera the candidates that won their pixel (win), in candidate order,
// the cameras back to back -- the order of the frame's match lists -- ranked by a ballot per wave and a running count.  -> the
// count.  Reads win / best / cand and the keypoint rows on the device, nothing of the host-mapped rows
__device__ __forceinline__ int pose_gather(const PoseJob &job, int *cnt, const uint8_t *__restrict__ win, const TrBest *__restrict__ best,
                                           const int *__restrict__ cand, const float2 *__restrict__ kp_xy, PoseObs *__restrict__ obs,
                                           int32_t *__restrict__ lids)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nc = job.n_cand;
    int off = 0;
    for (int c = 0; c < job.ncams; c++) {
        const size_t row = job.rows + (size_t)c * nc;
        const float2 *kp = kp_xy + job.kp0 + job.frame.first[c];
        for (int i0 = 0; i0 < nc; i0 += kPoseT) {
            const int i = i0 + t;
            const bool keep = i < nc && win[row + i] != 0;
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) cnt[wave] = __popcll(mask);
            __syncthreads();
            int at = off, total = 0;
            for (int w = 0; w < kPoseBlocks; w++) {
                at += w < wave ? cnt[w] : 0;
                total += cnt[w];
            }
            if (keep) {
                const int k = best[row + i].kp;   // (a winner has a match: 0 <= k < n_kp[c])
                const float2 p = kp[k];
                const int r = lane_rank(mask, at);
                obs[r] = PoseObs{p.x, p.y, c, 0};
                lids[r] = cand[job.cand_first + i];
            }
            off += total;
            __syncthreads();   // cnt is written again
        }
    }
    return off;
}

__device__ __forceinline__ void pose_write(mcorb_pose_result &res, const PoseState &P, double cost_initial, double cost_final, int32_t status,
                                           int32_t its0, int32_t its1, int32_t n_inliers, int32_t n)
{
    for (int k = 0; k < 9; k++) res.R[k] = P.R[k];
    for (int k = 0; k < 3; k++) res.t[k] = P.t[k];
    res.cost_initial = cost_initial;
    res.cost_final = cost_final;
    res.status = status;
    res.iterations[0] = its0;
    res.iterations[1] = its1;
    res.n_inliers = n_inliers;
    res.n_obs = n;
    res.reserved = 0;
}

__global__ __launch_bounds__(kPoseT) void k_pose_refine(const PoseJob *__restrict__ jobs, PoseObs *obs, int32_t *lids,
                                                        const double *__restrict__ pts, const double *__restrict__ geom, uint8_t *alive,
                                                        const uint8_t *__restrict__ win, const TrBest *__restrict__ best,
                                                        const int *__restrict__ cand, const float2 *__restrict__ kp_xy,
                                                        mcorb_pose_result *out, uint8_t *flags)
{
    __shared__ double part[2][kPoseBlocks][kPoseSums];
    __shared__ int cnt[kPoseBlocks];
    const PoseJob &job = jobs[blockIdx.x];
    const int t = threadIdx.x;
    obs += job.obs0;
    lids = lids ? lids + job.obs0 : nullptr;
    alive += job.obs0;
    flags += job.obs0;
    int n = job.n;
    if (job.from_track) {
        n = pose_gather(job, cnt, win, best, cand, kp_xy, obs, lids);   // (ends behind a barrier: the list is the workgroup's)
        pts = nullptr;
    } else if (pts) {
        pts += 3 * job.obs0;
        lids = nullptr;
    }
    const PoseState init = job.init;
    mcorb_pose_result &res = out[blockIdx.x];   // (written by lane 0, member by member: a local copy's tail would live in scratch)
    if (n < 1) {   // (uniform over the workgroup)
        if (t == 0) pose_write(res, init, 0.0, 0.0, MCORB_POSE_NO_OBS, 0, 0, 0, n);
        return;
    }
    for (int i = t; i < n; i += kPoseT) alive[i] = 1;
    const PoseSrc src{&job, obs, lids, pts, geom, alive, n};
    PosePass pass{src, part, 0};
    PoseState pose = init;
    double cost_initial = 0.0, cost_final = 0.0;
    int32_t status = MCORB_POSE_NO_OBS, its0 = 0, its1 = 0;
    for (int round = 0; round < 2; round++) {
        double c0, c1;
        int32_t its;
        pose_round(pass, init, job.max_iterations, pose, its, status, c0, c1);
        if (round == 0) {
            cost_initial = c0;
            its0 = its;
        } else {
            its1 = its;
        }
        cost_final = c1;
        for (int i = t; i < n; i += kPoseT) {
            if (!alive[i]) continue;
            const PoseObs o = obs[i];
            double X[3];
            src.point(i, X);
            if (pose_is_outlier(job.cams[o.cam], pose, X, o.u, o.v, job.inv_sigma2[o.octave])) alive[i] = 0;
        }
    }
    int in = 0;
    for (int i = t; i < n; i += kPoseT) {
        const uint8_t a = alive[i];
        flags[i] = a;
        in += a;
    }
    in = wave_total(in);
    if ((t & 63) == 0) cnt[t >> 6] = in;
    __syncthreads();
    if (t == 0)
        pose_write(res, pose, pose_default_nan(cost_initial), pose_default_nan(cost_final), status, its0, its1, wg_combine(cnt), n);
}

void launch_pose_refine(hipStream_t st, const PoseJob *jobs, int njobs, PoseObs *obs, int32_t *lids, const double *pts, const double *geom,
                        uint8_t *alive, const uint8_t *win, const TrBest *best, const int *cand, const float2 *kp_xy,
                        mcorb_pose_result *out, uint8_t *flags)
{
    if (njobs < 1) return;
    hipLaunchKernelGGL(k_pose_refine, dim3(njobs), dim3(kPoseT), 0, st, jobs, obs, lids, pts, geom, alive, win, best, cand, kp_xy, out,
                       flags);
}

}  // namespace mcorb
