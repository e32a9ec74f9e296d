// mcorb_ba_gpu.hip -- the kernels of mcorb_lmap_bundle_adjust on a device store (mcorb_ba.cpp; the arithmetic is mcorb_ba.h's,
// DESIGN.md section 9o).  The host queues the whole chain behind one another on the store's stream and waits once.  The loop's
// record (lambda, the cost, the solves, which half of the state is current, whether the loop is over) lives in device memory:
// k_ba_accept updates it once per iteration, every kernel reads it at a uniform address, and the kernels of the iterations
// queued behind the loop's end return at once.
//
//   k_ba_begin       the points (given, or gathered from the store) and the poses into half 0 of the state; the record
//   k_ba_linearize   one lane per landmark: its observations in order -> V, gp, cost and its views (45 sums each); a lane holds
//                    one view's sums in registers at a time.  Returns at once when the state has not moved since the last one
//   k_ba_schur       one workgroup of 256 lanes per keyframe pair a <= b of the system (E_ab, 36 sums) and one per keyframe
//                    (U_a and rhs_a, 27 sums): fold_j by wg_fold_waves and wg_combine of mcorb_device.h, k_pose_refine's tree
//   k_ba_solve       one workgroup: S in LDS as a packed triangle, the LDL^T column by column (lane i computes L[i][j], every dot
//                    product in ascending k), the forward substitution the same way, the backward one by lane 0 (its dot
//                    products ascend while its rows descend); then the free poses retract into the trial half
//   k_ba_update      one lane per landmark: the back-substitution into the trial half, then the trial's cost
//   k_ba_accept      one workgroup: the fold of the cost and ba_decide on the record
//   k_ba_flags, k_ba_result   the flags per observation, the points and the result into host-mapped memory
//
// No workgroup waits on another, no atomics, no grid-wide synchronisation; every loop is bounded by a count from the arguments.
// No extraction job runs this and no benchmark leg times it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"
#include "mcorb_ba.h"

namespace mcorb {

constexpr int kBaT = MCORB_POSE_LANES;   // the fold's workgroup
constexpr int kBaLmT = 64;               // the per-landmark kernels: one wave per workgroup, so that few landmarks still spread
constexpr int kBaSolveT = 128;           // k_ba_solve: a lane per unknown (96 at most)
static_assert(kBaT == kWgLanes && kBaSolveT >= kBaMaxN, "the workgroup of mcorb_device.h's reductions; a lane per unknown");

__global__ __launch_bounds__(kBaT) void k_ba_begin(const BaArgs a)
{
    const int i = blockIdx.x * kBaT + threadIdx.x;
    if (i < 3 * a.nlm) {
        const int j = i / 3, c = i - 3 * j;
        a.pts[i] = a.pts_in ? a.pts_in[i] : a.geom[6 * (size_t)a.lids[j] + c];
    }
    if (blockIdx.x) return;
    constexpr int kPoseDoubles = sizeof(PoseState) / sizeof(double);
    if (threadIdx.x < kPoseDoubles * a.nkf) {   // (double by double: a PoseState copied whole would pass through scratch)
        const double v = reinterpret_cast<const double *>(a.poses_in)[threadIdx.x];
        reinterpret_cast<double *>(a.poses)[threadIdx.x] = v;
        reinterpret_cast<double *>(a.poses + MCORB_BA_MAX_KF)[threadIdx.x] = v;
    }
    if (threadIdx.x == 0) {
        BaRecord r;
        r.lambda = 1e-4;
        r.cost = r.cost_initial = 0.0;
        r.solves = r.any = r.converged = r.done = r.cur = r.step_ok = r.reserved = 0;
        r.relin = 1;
        *a.rec = r;
    }
}

__global__ __launch_bounds__(kBaLmT) void k_ba_linearize(const BaArgs a)
{
    const BaRecord &r = *a.rec;
    if (r.done || !r.relin) return;
    const int j = blockIdx.x * kBaLmT + threadIdx.x;
    if (j >= a.nlm) return;
    const int cur = r.cur;
    const double *Xp = a.pts + 3 * ((size_t)cur * a.nlm + j);
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    double V[6], gp[3], cost;
    ba_linearize_lm(*a.job, a.poses + MCORB_BA_MAX_KF * cur, a.obs, a.obs_first[j], a.obs_first[j + 1], X, V, gp, cost,
                    a.views + (size_t)kBaView * a.view_first[j]);
#pragma unroll
    for (int k = 0; k < 6; k++) a.V[6 * (size_t)j + k] = V[k];
#pragma unroll
    for (int k = 0; k < 3; k++) a.gp[3 * (size_t)j + k] = gp[k];
    a.cost[j] = cost;
}

// the lanes' K sums -> out[K]: wg_fold's tree, but behind the barrier lane k < K alone combines the four waves' sum k
template <int K>
__device__ __forceinline__ void ba_fold_out(double s[K], double (*part)[K], double *out)
{
    wg_fold_waves<K>(s, part);
    if (threadIdx.x < K) out[threadIdx.x] = wg_combine(part, threadIdx.x);
}

__global__ __launch_bounds__(kBaT) void k_ba_schur(const BaArgs a)
{
    __shared__ double part[4][kBaPair];
    const BaRecord &r = *a.rec;
    if (r.done) return;
    const double lambda = r.lambda;
    const int nsys = a.nsys, npairs = nsys * (nsys + 1) / 2, t = threadIdx.x;
    if ((int)blockIdx.x < npairs) {
        int ka = 0, rem = blockIdx.x;
        for (int k = 0; k < nsys && rem >= nsys - ka; k++) {   // (row ka of the pairs has nsys - ka entries)
            rem -= nsys - ka;
            ka++;
        }
        const int kb = ka + rem;
        double s[kBaPair];
#pragma unroll
        for (int k = 0; k < kBaPair; k++) s[k] = 0.0;
        for (int j = t; j < a.nlm; j += kBaT) {
            const int sa = a.slot[(size_t)j * MCORB_BA_MAX_KF + ka], sb = a.slot[(size_t)j * MCORB_BA_MAX_KF + kb];
            if (sa < 0 || sb < 0) continue;
            const BaLdl L = ba_ldl3(a.V + 6 * (size_t)j, lambda);
            if (!L.ok) continue;
            const double *views = a.views + (size_t)kBaView * a.view_first[j];
            double term[kBaPair];
            ba_pair_term(L, views + kBaView * sa, views + kBaView * sb, term);
#pragma unroll
            for (int k = 0; k < kBaPair; k++) s[k] = s[k] + term[k];
        }
        ba_fold_out<kBaPair>(s, part, a.pairs + (size_t)kBaPair * blockIdx.x);
    } else {
        const int ka = blockIdx.x - npairs;
        double s[kBaDiag];
#pragma unroll
        for (int k = 0; k < kBaDiag; k++) s[k] = 0.0;
        for (int j = t; j < a.nlm; j += kBaT) {
            const int sa = a.slot[(size_t)j * MCORB_BA_MAX_KF + ka];
            if (sa < 0) continue;
            const BaLdl L = ba_ldl3(a.V + 6 * (size_t)j, lambda);
            if (!L.ok) continue;
            double term[kBaDiag];
            ba_diag_term(L, a.views + (size_t)kBaView * (a.view_first[j] + sa), a.gp + 3 * (size_t)j, term);
#pragma unroll
            for (int k = 0; k < kBaDiag; k++) s[k] = s[k] + term[k];
        }
        ba_fold_out<kBaDiag>(s, reinterpret_cast<double(*)[kBaDiag]>(&part[0][0]), a.diag + (size_t)kBaDiag * ka);
    }
}

__global__ __launch_bounds__(kBaSolveT) void k_ba_solve(const BaArgs a)
{
    __shared__ double A[kBaTri], D[kBaMaxN], y[kBaMaxN], x[kBaMaxN];
    BaRecord &r = *a.rec;
    if (r.done) return;
    const double lambda = r.lambda;
    const int nsys = a.nsys, n = 6 * nsys, npairs = nsys * (nsys + 1) / 2, t = threadIdx.x, cur = r.cur;
    for (int q = t; q < npairs * kBaPair; q += kBaSolveT) {
        const int p = q / kBaPair, ik = q - kBaPair * p, i = ik / 6, k = ik - 6 * i;
        int ka = 0, rem = p;
        for (int c = 0; c < nsys && rem >= nsys - ka; c++) {
            rem -= nsys - ka;
            ka++;
        }
        const int kb = ka + rem;
        if (ka == kb && k < i) continue;
        A[ba_tri(6 * ka + i, 6 * kb + k, n)] = ba_system_entry(a.diag, a.pairs, nsys, lambda, ka, kb, i, k);
    }
    __syncthreads();
    // the LDL^T: lane t owns row t of L.  In column j lane t >= j subtracts (L[t][k] L[j][k]) D[k], k ascending, from entry (j, t):
    // lane j's is the pivot (its two factors are the same entry), the others' divide by it behind the barrier.  Entry (k, t) lies
    // n - k - 1 behind entry (k - 1, t) of the packed triangle
    bool ok = true;
    for (int j = 0; j < n; j++) {
        double v = 0.0;
        if (t >= j && t < n) {
            v = A[ba_tri(j, t, n)];
            int at_t = t, at_j = j;
#pragma unroll 4
            for (int k = 0; k < j; k++) {
                v = v - (A[at_t] * A[at_j]) * D[k];
                at_t += n - k - 1;
                at_j += n - k - 1;
            }
        }
        if (t == j) D[j] = v;
        __syncthreads();
        const double dj = D[j];
        if (!(dj > 0)) ok = false;
        if (t > j && t < n) A[ba_tri(j, t, n)] = v / dj;
        __syncthreads();
    }
    if (ok) {   // (the same in every lane)
        double v = t < n ? -a.diag[(size_t)kBaDiag * (t / 6) + kBaG + (t - 6 * (t / 6))] : 0.0;
        for (int k = 0; k < n; k++) {
            if (t == k) y[k] = v;
            __syncthreads();
            if (t > k && t < n) v = v - A[ba_tri(k, t, n)] * y[k];
        }
        if (t == 0)   // (row i of the packed triangle is contiguous: the loads and products run ahead of the chain of subtractions)
            for (int i = n - 1; i >= 0; i--) {
                double u = y[i] / D[i];
                const double *row = A + ba_tri(i, i, n) - i;
#pragma unroll 8
                for (int k = i + 1; k < n; k++) u = u - row[k] * x[k];
                x[i] = u;
            }
        __syncthreads();
        if (t < n) a.delta[t] = x[t];
        if (t < a.nkf) {
            const PoseState *from = a.poses + MCORB_BA_MAX_KF * cur;
            PoseState *to = a.poses + MCORB_BA_MAX_KF * (cur ^ 1);
            const int s = a.job->sys_of_kf[t];
            const PoseState P = from[t];
            if (s < 0) {
                to[t] = P;
            } else {
                const double d[6] = {x[6 * s], x[6 * s + 1], x[6 * s + 2], x[6 * s + 3], x[6 * s + 4], x[6 * s + 5]};
                PoseState Q;
                pose_retract(P, d, Q);
                to[t] = Q;
            }
        }
    }
    if (t == 0) r.step_ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(kBaLmT) void k_ba_update(const BaArgs a)
{
    const BaRecord &r = *a.rec;
    if (r.done || !r.step_ok) return;
    const int j = blockIdx.x * kBaLmT + threadIdx.x;
    if (j >= a.nlm) return;
    const int cur = r.cur;
    const double *Xp = a.pts + 3 * ((size_t)cur * a.nlm + j);
    double *Xt = a.pts + 3 * ((size_t)(cur ^ 1) * a.nlm + j);
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    double Xn[3] = {X[0], X[1], X[2]};
    const BaLdl L = ba_ldl3(a.V + 6 * (size_t)j, r.lambda);
    if (L.ok)
        ba_backsub_lm(L, a.gp + 3 * (size_t)j, a.slot + (size_t)j * MCORB_BA_MAX_KF, a.views + (size_t)kBaView * a.view_first[j], a.nsys,
                      a.delta, X, Xn);
    Xt[0] = Xn[0];
    Xt[1] = Xn[1];
    Xt[2] = Xn[2];
    a.cost[j] = ba_cost_lm(*a.job, a.poses + MCORB_BA_MAX_KF * (cur ^ 1), a.obs, a.obs_first[j], a.obs_first[j + 1], Xn);
}

__global__ __launch_bounds__(kBaT) void k_ba_accept(const BaArgs a, int first)
{
    __shared__ double part[4][1];
    __shared__ double total;
    BaRecord &r = *a.rec;
    if (r.done) return;
    double s[1] = {0.0};
    for (int j = threadIdx.x; j < a.nlm; j += kBaT) s[0] = s[0] + a.cost[j];
    ba_fold_out<1>(s, part, &total);
    __syncthreads();
    if (threadIdx.x) return;
    BaRecord q = r;
    if (first)
        q.cost = q.cost_initial = total;
    else
        ba_decide(q, total, a.max_iterations);
    r = q;
}

__global__ __launch_bounds__(kBaT) void k_ba_flags(const BaArgs a)
{
    __shared__ int cnt[4];
    const int cur = a.rec->cur, i = blockIdx.x * kBaT + threadIdx.x;
    const double *pts = a.pts + 3 * (size_t)cur * a.nlm;
    if (i < 3 * a.nlm) a.out_pts[i] = pts[i];
    int in = 0;
    if (i < a.nobs) {
        const BaObs o = a.obs[i];
        const double X[3] = {pts[3 * (size_t)o.lm], pts[3 * (size_t)o.lm + 1], pts[3 * (size_t)o.lm + 2]};
        in = ba_inlier(*a.job, a.poses + MCORB_BA_MAX_KF * cur, o, X);
        a.flags[o.orig] = (uint8_t)in;
    }
    in = wave_total(in);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = in;
    __syncthreads();
    if (threadIdx.x == 0) a.count[blockIdx.x] = wg_combine(cnt);
}

__global__ __launch_bounds__(kBaT) void k_ba_result(const BaArgs a, int nblocks)
{
    __shared__ int cnt[4];
    const BaRecord &r = *a.rec;
    const int t = threadIdx.x;
    int in = 0;
    for (int b = t; b < nblocks; b += kBaT) in += a.count[b];
    in = wave_total(in);
    if ((t & 63) == 0) cnt[t >> 6] = in;
    __syncthreads();
    if (t < a.nkf) {   // (member by member: a local copy's tail would live in scratch)
        const PoseState &P = a.poses[MCORB_BA_MAX_KF * r.cur + t];
        for (int k = 0; k < 9; k++) a.out->poses[t].R[k] = P.R[k];
        for (int k = 0; k < 3; k++) a.out->poses[t].t[k] = P.t[k];
    }
    if (t) return;
    mcorb_ba_result &res = a.out->res;
    res.cost_initial = pose_default_nan(r.cost_initial);
    res.cost_final = pose_default_nan(r.cost);
    res.status = ba_status(r);
    res.iterations = r.solves;
    res.n_inliers = wg_combine(cnt);
    res.n_obs = a.nobs;
}

static inline int ba_blocks(int n, int per) { return n > 0 ? (n + per - 1) / per : 1; }

void launch_ba_begin(hipStream_t st, const BaArgs &a)
{
    hipLaunchKernelGGL(k_ba_begin, dim3(ba_blocks(3 * a.nlm, kBaT)), dim3(kBaT), 0, st, a);
}
void launch_ba_linearize(hipStream_t st, const BaArgs &a)
{
    hipLaunchKernelGGL(k_ba_linearize, dim3(ba_blocks(a.nlm, kBaLmT)), dim3(kBaLmT), 0, st, a);
}
void launch_ba_schur(hipStream_t st, const BaArgs &a)
{
    if (a.nsys < 1) return;   // (no free keyframe: the step is the points' alone)
    hipLaunchKernelGGL(k_ba_schur, dim3(a.nsys * (a.nsys + 1) / 2 + a.nsys), dim3(kBaT), 0, st, a);
}
void launch_ba_solve(hipStream_t st, const BaArgs &a) { hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(kBaSolveT), 0, st, a); }
void launch_ba_update(hipStream_t st, const BaArgs &a)
{
    hipLaunchKernelGGL(k_ba_update, dim3(ba_blocks(a.nlm, kBaLmT)), dim3(kBaLmT), 0, st, a);
}
void launch_ba_accept(hipStream_t st, const BaArgs &a, bool first)
{
    hipLaunchKernelGGL(k_ba_accept, dim3(1), dim3(kBaT), 0, st, a, first ? 1 : 0);
}
void launch_ba_final(hipStream_t st, const BaArgs &a)
{
    const int nblocks = ba_blocks(a.nobs > 3 * a.nlm ? a.nobs : 3 * a.nlm, kBaT);
    hipLaunchKernelGGL(k_ba_flags, dim3(nblocks), dim3(kBaT), 0, st, a);
    hipLaunchKernelGGL(k_ba_result, dim3(1), dim3(kBaT), 0, st, a, nblocks);
}

}  // namespace mcorb
