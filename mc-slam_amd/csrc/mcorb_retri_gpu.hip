// mcorb_retri_gpu.hip -- the kernels of mcorb_lmap_retriangulate on a device store (mcorb_retri.cpp; the arithmetic is
// mcorb_retri.h's).  The host queues both behind one another on the store's stream and waits once.
//
//   k_retri_views   one lane per (keyframe, camera) of the keyframes that have an observation: P = K [R_cw | t_cw] and the camera
//                   centre, 15 doubles
//   k_retri_solve   16 lanes per landmark, 4 landmarks per wave, 256-lane workgroups.  The group reads its landmark's span, folds
//                   the selection with an OR, accumulates G over its observations (lane l: l, l + 16, ..) and folds the 16 sums by
//                   xor-shuffles with strides 8, 4, 2, 1 -- an addition commutes, so every lane of the group ends with the bits
//                   lane 0 has and the Jacobi runs redundantly in all 16 without a broadcast.  The check pass over the same
//                   observations folds an integer minimum and an fp64 maximum; lane 0 makes the gated store into the HBM point
//                   and writes the record into host-mapped memory.  A group whose landmark is not selected or has fewer than two
//                   observations leaves after the span read
//
// No LDS, no atomics, no workgroup waits on another; every loop is bounded by a count from the arguments and every index comes
// from a table the host checked or built.  A landmark appears once per launch, so no two groups touch one slot.  No extraction
// job runs this and no benchmark leg times it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"
#include "mcorb_retri.h"

namespace mcorb {

constexpr int kRetriT = 256;
static_assert(kRetriT % kRetriLanes == 0 && 64 % kRetriLanes == 0, "a group of lanes lies inside one wave");

__global__ __launch_bounds__(kRetriT) void k_retri_views(const RetriArgs a)
{
    const int i = blockIdx.x * kRetriT + threadIdx.x;
    if (i >= a.nviews) return;
    const int ncams = a.job->ncams, s = i / ncams, c = i - s * ncams;
    double v[kRetriView];
    retri_view(a.job->cams[c], a.poses[s], v);
#pragma unroll
    for (int k = 0; k < kRetriView; k++) a.views[(size_t)kRetriView * i + k] = v[k];
}

__global__ __launch_bounds__(kRetriT) void k_retri_solve(const RetriArgs a)
{
    const int g = (blockIdx.x * kRetriT + threadIdx.x) / kRetriLanes, l = threadIdx.x & (kRetriLanes - 1);
    if (g >= a.nlm) return;
    const int o0 = a.obs_first[g], o1 = a.obs_first[g + 1], n = o1 - o0;
    int sel = 0;
    for (int i = o0 + l; i < o1; i += kRetriLanes) sel |= a.moved[a.obs[i].slot];
#pragma unroll
    for (int stride = kRetriLanes / 2; stride >= 1; stride >>= 1) sel |= __shfl_xor(sel, stride, kRetriLanes);
    RetriOut &out = a.out[g];
    if (!sel || n < 2) {
        if (l == 0) {
            out.X[0] = out.X[1] = out.X[2] = out.diff_norm = 0.0;
            out.n_views = n;
            out.verdict = !sel ? MCORB_RETRI_NOT_SELECTED : MCORB_RETRI_FEW_VIEWS;
        }
        return;
    }
    const RetriJob &job = *a.job;
    double G[kRetriG];
#pragma unroll
    for (int k = 0; k < kRetriG; k++) G[k] = 0.0;
    for (int i = o0 + l; i < o1; i += kRetriLanes) {
        const RetriObs o = a.obs[i];
        retri_add(a.views + (size_t)kRetriView * o.view, o.u, o.v, G);
    }
#pragma unroll
    for (int stride = kRetriLanes / 2; stride >= 1; stride >>= 1)
#pragma unroll
        for (int k = 0; k < kRetriG; k++) G[k] = G[k] + __shfl_xor(G[k], stride, kRetriLanes);
    double X[3];
    const bool degenerate = retri_solve(G, job.rank_tol, X);
    int32_t key = kRetriNoKey;
    double emax = 0.0;
    const double far_threshold = job.far_threshold;
    for (int i = o0 + l; i < o1; i += kRetriLanes) {
        const RetriObs o = a.obs[i];
        retri_check(a.views + (size_t)kRetriView * o.view, X, o.u, o.v, far_threshold, i - o0, key, emax);
    }
#pragma unroll
    for (int stride = kRetriLanes / 2; stride >= 1; stride >>= 1) {
        const int32_t other = __shfl_xor(key, stride, kRetriLanes);
        const double e = __shfl_xor(emax, stride, kRetriLanes);
        key = other < key ? other : key;
        emax = e > emax ? e : emax;
    }
    if (l) return;
    int verdict = retri_verdict(degenerate, key, emax, job.outlier_threshold);
    double diff_norm = 0.0;
    if (verdict == MCORB_RETRI_VALID_UPDATED) verdict = retri_update(a.geom + 6 * (size_t)a.lids[g], X, job.max_diff, job.apply != 0, diff_norm);
    out.X[0] = X[0];
    out.X[1] = X[1];
    out.X[2] = X[2];
    out.diff_norm = diff_norm;
    out.n_views = n;
    out.verdict = verdict;
}

void launch_retri_views(hipStream_t st, const RetriArgs &a)
{
    hipLaunchKernelGGL(k_retri_views, dim3((a.nviews + kRetriT - 1) / kRetriT), dim3(kRetriT), 0, st, a);
}
void launch_retri_solve(hipStream_t st, const RetriArgs &a)
{
    constexpr int per = kRetriT / kRetriLanes;
    hipLaunchKernelGGL(k_retri_solve, dim3((a.nlm + per - 1) / per), dim3(kRetriT), 0, st, a);
}

}  // namespace mcorb
