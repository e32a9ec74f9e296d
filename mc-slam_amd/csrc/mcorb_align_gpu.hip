// mcorb_align_gpu.hip -- the rig pose between two frames from 3D-3D pairs of mcorb_align.h on a device store (mcorb_align.cpp):
// four launches on the store's stream in mode 1, one in mode 0, no workgroup waits on another.
//   k_align_hypotheses  one lane per hypothesis: the three draws, Horn's closed form on the three pairs (the Jacobi pairs and the
//                       4 x 4 indices are compile-time constants: N and V are registers); a model record per hypothesis
//   k_align_score       H x n distances: a workgroup owns a tile of kAlignTile pairs, which each lane keeps in registers, and a
//                       block of kAlignHypBlock hypotheses, whose models it reads at uniform addresses: consensus_count
//                       (mcorb_consensus.h)
//   k_align_pick        every workgroup finds the arg-max of count[H] for itself (consensus_best_wg) and writes the winner's flags
//                       at the threshold for its tile of pairs into member[n]; workgroup 0 writes the winner's record, both to
//                       device memory
//   k_align_fit         ONE workgroup of 256: the two passes over the members (mode 0: all pairs), folded in order by wg_fold of
//                       mcorb_device.h, lane 0 solves, then the workgroup strides over the n pairs for the verdict's flags, count
//                       and mean distance and writes the record to host-mapped memory.  One workgroup is deliberate: the sums are
//                       floating-point and their order is part of the definition; a grid-wide reduction would need a wait between
//                       workgroups or an atomic whose order the hardware picks
// The arithmetic is the header's, so the host-only store gives the same bits.  No extraction job runs this and no benchmark leg
// times it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"
#include "mcorb_align.h"

namespace mcorb {

static_assert(kAlignTile == kWgLanes && kAlignTile == kAlignLanes, "mcorb_device.h's workgroup, a lane of pose_fold each");

// the pairs as a lane reads them: frame 1's point is given or the store's landmark's
struct AlignSrc {
    const double *p1, *p2;
    const int32_t *lids1;
    const double *geom;
    __device__ __forceinline__ void operator()(int i, double a[3], double b[3]) const
    {
        const double *p = p1 ? p1 + 3 * (size_t)i : geom + 6 * (size_t)lids1[i];
        const double *q = p2 + 3 * (size_t)i;
        a[0] = p[0], a[1] = p[1], a[2] = p[2];
        b[0] = q[0], b[1] = q[1], b[2] = q[2];
    }
};

__global__ __launch_bounds__(64) void k_align_hypotheses(const AlignJob *__restrict__ job, AlignSrc src, AlignModel *__restrict__ models)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= job->H) return;
    align_hypothesis(*job, h, src, models[h]);
}

__global__ __launch_bounds__(kAlignTile) void k_align_score(const AlignJob *__restrict__ job, AlignSrc src,
                                                            const AlignModel *__restrict__ models, int32_t *__restrict__ count)
{
    __shared__ int32_t cnt[kAlignHypBlock];
    const int n = job->n;
    const int i = blockIdx.x * kAlignTile + threadIdx.x;
    const bool in = i < n;
    const double threshold = job->threshold;
    double p1[3], p2[3];
    src(in ? i : 0, p1, p2);   // (n >= 1: a lane beyond the pairs scores pair 0 and counts nothing)
    consensus_count<kAlignHypBlock>(
        job->H, count, cnt, [&](int h) { return models[h].valid; },   // (uniform over the workgroup)
        [&](int h) {
            PoseState P;
            pose_load(P, models[h].R, models[h].t);
            return in && sac_is_inlier(align_dist(P, p1, p2), threshold);
        });
}

__global__ __launch_bounds__(kAlignTile) void k_align_pick(const AlignJob *__restrict__ job, AlignSrc src,
                                                           const AlignModel *__restrict__ models, const int32_t *__restrict__ count,
                                                           AlignPick *__restrict__ pick, uint8_t *__restrict__ member)
{
    __shared__ unsigned long long wkey[4];
    __shared__ int32_t wmodels[4];
    const int t = threadIdx.x;
    const int n = job->n;
    int32_t n_models;
    const int best = consensus_best_wg<kRelKeyBits, 1>(   // (the same in every lane)
        job->H, [&](int h) { return models[h].valid; }, [&](int h) { return count[h]; }, wkey, wmodels, n_models);
    PoseState P;
    pose_identity(P);
    if (best >= 0) pose_load(P, models[best].R, models[best].t);
    const int i = blockIdx.x * kAlignTile + t;
    if (i < n) {
        uint8_t flag = 0;
        if (best >= 0) {
            double p1[3], p2[3];
            src(i, p1, p2);
            flag = sac_is_inlier(align_dist(P, p1, p2), job->threshold) ? 1 : 0;
        }
        member[i] = flag;
    }
    if (blockIdx.x == 0 && t == 0) {
        for (int j = 0; j < 9; j++) pick->R[j] = P.R[j];
        for (int j = 0; j < 3; j++) pick->t[j] = P.t[j];
        pick->best = best;
        pick->count = best >= 0 ? count[best] : 0;
        pick->n_models = n_models;
        for (int j = 0; j < kAlignSample; j++) pick->sample[j] = best >= 0 ? models[best].sample[j] : -1;
    }
}

// The two passes of a fit by one workgroup of kAlignTile over the members of n pairs (member null: all of them) -> their count;
// M: the nine sums of pass 2 and c1, c2: the centroids, the same bits in every lane, for align_from_sums.  The folds are wg_fold's
// (mcorb_device.h), with a barrier behind each before part and wcnt are written again.  k_align_fit and k_align_solve_selftest
// both fit through this
__device__ __forceinline__ int align_fit_sums(const AlignSrc &src, int n, const uint8_t *member, double (*part)[kAlignSums2], int32_t *wcnt,
                                              double M[kAlignSums2], double c1[3], double c2[3])
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // pass 1: the coordinate sums and the members
    double s[kAlignSums2];
#pragma unroll
    for (int k = 0; k < kAlignSums2; k++) s[k] = 0.0;
    int mine = 0;
    for (int i = t; i < n; i += kAlignTile) {
        if (member && !member[i]) continue;
        double p1[3], p2[3];
        src(i, p1, p2);
        align_add1(p1, p2, s);
        mine++;
    }
    mine = wave_total(mine);
    if (lane == 0) wcnt[wave] = mine;
    wg_fold<kAlignSums1>(s, part, M);   // (its barrier and the next cover wcnt)
    __syncthreads();
    const int cnt = wg_combine(wcnt);
    align_centroids(M, cnt, c1, c2);
    // pass 2: M
#pragma unroll
    for (int k = 0; k < kAlignSums2; k++) s[k] = 0.0;
    for (int i = t; i < n; i += kAlignTile) {
        if (member && !member[i]) continue;
        double p1[3], p2[3];
        src(i, p1, p2);
        align_add2(p1, p2, c1, c2, s);
    }
    wg_fold<kAlignSums2>(s, part, M);
    __syncthreads();
    return cnt;
}

// mcorb_dev_align_solve_selftest: a workgroup of k_align_fit's shape per problem -- problem b has cnt[b] pairs from pair first[b]
// on in p1, p2 and member -- the fit's two passes, then lane 0's align_from_sums with the gap.  R and t are zero without a
// valid fit; the gap is written either way, a NaN as the default quiet NaN
__global__ __launch_bounds__(kAlignTile) void k_align_solve_selftest(const double *__restrict__ p1, const double *__restrict__ p2,
                                                                     const uint8_t *__restrict__ member, const int32_t *__restrict__ first,
                                                                     const int32_t *__restrict__ cnt, double *__restrict__ R,
                                                                     double *__restrict__ tr, double *__restrict__ gap,
                                                                     int32_t *__restrict__ valid)
{
    __shared__ double part[kWgWaves][kAlignSums2];
    __shared__ int32_t wcnt[kWgWaves];
    const int b = blockIdx.x;
    const size_t at = (size_t)first[b];
    const AlignSrc src{p1 + 3 * at, p2 + 3 * at, nullptr, nullptr};
    double S[kAlignSums2], c1[3], c2[3];
    const int members = align_fit_sums(src, cnt[b], member + at, part, wcnt, S, c1, c2);
    if (threadIdx.x == 0) {
        PoseState P;
        double g = 0.0;
        const bool ok = align_from_sums(S, c1, c2, members, P, &g);
        for (int j = 0; j < 9; j++) R[9 * (size_t)b + j] = ok ? P.R[j] : 0.0;
        for (int j = 0; j < 3; j++) tr[3 * (size_t)b + j] = ok ? P.t[j] : 0.0;
        gap[b] = pose_default_nan(g);
        valid[b] = ok ? 1 : 0;
    }
}

void launch_align_solve_selftest(hipStream_t st, const double *p1, const double *p2, const uint8_t *member, const int32_t *first,
                                  const int32_t *cnt, int n, double *R, double *t, double *gap, int32_t *valid)
{
    hipLaunchKernelGGL(k_align_solve_selftest, dim3(n), dim3(kAlignTile), 0, st, p1, p2, member, first, cnt, R, t, gap, valid);
}

__global__ __launch_bounds__(kAlignTile) void k_align_fit(const AlignJob *__restrict__ job, AlignSrc src, const AlignPick *pick,
                                                          const uint8_t *member, AlignOut *out, uint8_t *flags)
{
    __shared__ double part[kWgWaves][kAlignSums2];
    __shared__ int32_t wcnt[kWgWaves];
    __shared__ double fitted[12];
    __shared__ int32_t fit_ok;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = job->n;
    const bool all = job->mode == MCORB_ALIGN_MODE_ALL;
    PoseState win, ans;
    pose_identity(win);
    int best = -1, sac_count = 0, n_models = 0;
    if (!all) {
        pose_load(win, pick->R, pick->t);
        best = pick->best;
        sac_count = pick->count;
        n_models = pick->n_models;
    }
    ans = win;
    bool have = best >= 0;
    int used = MCORB_ALIGN_USED_SAC;
    if (all || (have && job->refit)) {   // (uniform over the workgroup)
        double S[kAlignSums2], c1[3], c2[3];
        const int cnt = align_fit_sums(src, n, all ? nullptr : member, part, wcnt, S, c1, c2);
        if (t == 0) {
            PoseState P;
            const bool ok = align_from_sums(S, c1, c2, cnt, P, nullptr);
#pragma unroll
            for (int j = 0; j < 9; j++) fitted[j] = P.R[j];
#pragma unroll
            for (int j = 0; j < 3; j++) fitted[9 + j] = P.t[j];
            fit_ok = ok ? 1 : 0;
        }
        __syncthreads();
        if (fit_ok) {
            pose_load(ans, fitted, fitted + 9);
            used = MCORB_ALIGN_USED_FIT;
            have = true;
        }
    }
    // the verdict: the flags, their count, the fold-ordered sum of the distances
    double d[1] = {0.0}, D[1];
    int inl = 0;
    const double inlier_dist = job->inlier_dist;
    for (int i = t; i < n; i += kAlignTile) {
        uint8_t flag = 0;
        if (have) {
            double p1[3], p2[3];
            src(i, p1, p2);
            const double di = align_dist(ans, p1, p2);
            flag = sac_is_inlier(di, inlier_dist) ? 1 : 0;
            d[0] = d[0] + di;
        }
        flags[i] = flag;
        inl += flag;
    }
    inl = wave_total(inl);
    if (lane == 0) wcnt[wave] = inl;
    wg_fold<1>(d, part, D);   // (its barrier covers wcnt; nothing in LDS is written again)
    if (t == 0) {
        for (int j = 0; j < 9; j++) out->R[j] = ans.R[j], out->sac_R[j] = win.R[j];
        for (int j = 0; j < 3; j++) out->t[j] = ans.t[j], out->sac_t[j] = win.t[j];
        out->mean_error = have ? pose_default_nan(D[0] / (double)n) : 0.0;
        out->status = have ? MCORB_ALIGN_OK : MCORB_ALIGN_NO_MODEL;
        out->used = used;
        out->n_inliers = wg_combine(wcnt);
        out->sac_n_inliers = sac_count;
        out->best = best;
        out->n_models = n_models;
        for (int j = 0; j < kAlignSample; j++) out->sample[j] = all ? -1 : pick->sample[j];
        out->pad = 0;
    }
}

static AlignSrc src_of(const AlignArgs &a) { return AlignSrc{a.p1, a.p2, a.lids1, a.geom}; }

void launch_align_hypotheses(hipStream_t st, const AlignArgs &a, int H)
{
    hipLaunchKernelGGL(k_align_hypotheses, dim3((H + 63) / 64), dim3(64), 0, st, a.job, src_of(a), a.models);
}

void launch_align_score(hipStream_t st, const AlignArgs &a, int n, int H)
{
    hipLaunchKernelGGL(k_align_score, dim3((n + kAlignTile - 1) / kAlignTile, (H + kAlignHypBlock - 1) / kAlignHypBlock), dim3(kAlignTile), 0,
                       st, a.job, src_of(a), a.models, a.count);
}

void launch_align_pick(hipStream_t st, const AlignArgs &a, int n)
{
    hipLaunchKernelGGL(k_align_pick, dim3((n + kAlignTile - 1) / kAlignTile), dim3(kAlignTile), 0, st, a.job, src_of(a), a.models, a.count,
                       a.pick, a.member);
}

void launch_align_fit(hipStream_t st, const AlignArgs &a)
{
    hipLaunchKernelGGL(k_align_fit, dim3(1), dim3(kAlignTile), 0, st, a.job, src_of(a), a.pick, a.member, a.out, a.flags);
}

}  // namespace mcorb
