// mcorb_ess_gpu.hip -- the pose of one camera between two frames by five-point RANSAC of mcorb_ess.h on a device store
// (mcorb_ess.cpp): four launches on the store's stream, no workgroup waits on another, no result depends on the launch shape.
//   k_ess_hypotheses   kEssLanes = 16 lanes per hypothesis, four hypotheses per wave, a workgroup of one wave.  The lanes of a
//                      group only move values through LDS; every chain of operations is one function of the header, so the
//                      host-only store gives the same bits.  Lane 0: the draws, the bearings, the null-space basis.  Lane k <
//                      10: cubic k into the group's 10 x 20 table.  Lane j < 11: det C(z) at node j -- the pivoted LU indexes
//                      its rows at run time, so its 10 x 10 matrix is a private array in scratch --, then coefficient j of the
//                      polynomial.  The derivative chain: per level, lane i takes bracket i and lane 0 gathers the roots found.
//                      Lane r < 10: the model of root r into its slot.  Everything behind the sample is ess_group_models, which
//                      k_ess_solve_selftest (mcorb_dev_ess_solve_selftest) runs on caller-given problems in the same launch shape
//   k_ess_score        the hot path, 10 H x S Sampson distances: a workgroup owns a tile of kEssTile matches, whose normalised
//                      points each lane computes once, and a block of kEssSlotBlock slots, whose models it reads at uniform
//                      addresses: consensus_count (mcorb_consensus.h).  Slots without a model are skipped uniformly
//   k_ess_pick         every workgroup finds the arg-max of the slots' keys for itself (consensus_best_wg), forms the four candidates
//                      from the winner -- the same bits in every workgroup -- and adds its matches' four votes to four integers;
//                      workgroup 0 leaves the winner and its candidates for k_ess_finish
//   k_ess_finish       reads the four votes, writes the flags of its tile; workgroup 0 writes the record to host-mapped memory
//   k_ess_fit          the polished call only, behind a k_ess_finish whose record and flags stay in device memory: ONE workgroup of
//                      256 -- the rounds of mcorb_ess_polish.h (ess_fit_round over the members, the 21 sums folded by wg_fold of
//                      mcorb_device.h, then all S matches tested at the result), and the accepted record, its flags
//                      and the polish record to host-mapped memory
// No extraction job runs this and no benchmark leg times it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_ess.h"
#include "mcorb_kernels.h"

namespace mcorb {

static_assert(kEssTile == kWgLanes && kEssTile == MCORB_POSE_LANES, "mcorb_device.h's workgroup, a lane of pose_fold each");
static_assert(kEssLanes >= kEssNodes && kEssLanes >= kEssRoots + 1 && 64 % kEssLanes == 0, "a lane per node, per bracket and per root");

// what the lanes of one hypothesis share
struct EssGroup {
    double B[36], table[200], d1[kEssSample][3], d2[kEssSample][3];
    double det[kEssNodes], poly[kEssNodes], crit[kEssRoots], found[kEssRoots + 1], E[9 * kEssRoots];
    int32_t has[kEssRoots + 1], sample[kEssSample], m, ok;
};

// Everything of a hypothesis behind its sample, for the sixteen lanes of its group: G.d1, G.d2 and G.ok are lane 0's, written
// before the call (the first barrier here covers them).  The slots go to models and valid at kEssRoots * h; z (null in a call):
// the root each kept model began from, rho * G.crit[lane], compacted by the same prefix as its E, 0 behind the models.
// k_ess_hypotheses feeds it from ess_sample, k_ess_solve_selftest from problem h of a table.  Every lane of the workgroup calls
// it -- a group beyond the hypotheses (act false) goes through every barrier and touches nothing
__device__ __forceinline__ void ess_group_models(EssGroup &G, int lane, int h, bool act, EssModel *__restrict__ models,
                                                 int32_t *__restrict__ valid, double *__restrict__ z)
{
    if (act && lane == 0) {
        ess_basis(G.d1, G.d2, G.B);
        G.m = 0;
    }
    __syncthreads();
    if (act && lane < 10) ess_cubic(G.B, lane, G.table + 20 * lane);
    __syncthreads();
    if (act && lane < kEssNodes) G.det[lane] = ess_det_at(G.table, lane, 1.0);
    __syncthreads();
    if (act && lane < kEssNodes) G.poly[lane] = ess_coefficient(G.det, lane);
    __syncthreads();
    // the second pass at the roots' scale, which every lane works out for itself
    double rho = 1.0;
    if (act) {
        const double ends[kEssNodes] = {G.poly[0], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, G.poly[10]};
        rho = ess_scale(ends);
    }
    if (act && lane < kEssNodes) G.det[lane] = ess_det_at(G.table, lane, rho);
    __syncthreads();
    if (act && lane < kEssNodes) G.poly[lane] = ess_coefficient(G.det, lane);
    __syncthreads();
    // ess_real_roots, a bracket per lane
    const bool chain = act && G.ok && sac_finite(G.poly[10]) && G.poly[10] != 0.0;
    for (int L = 9; L >= 0; L--) {
        const int n = 10 - L;
        const int m = chain ? G.m : 0;   // (<= n - 1: level L + 1 had at most n - 1 brackets)
        if (chain && lane <= m) {
            double p[kEssNodes], q[kEssNodes], crit[kEssRoots], bound, r;
            for (int j = 0; j < kEssNodes; j++) p[j] = G.poly[j];
            for (int j = 0; j < kEssRoots; j++) crit[j] = j < m ? G.crit[j] : 0.0;
            ess_level(p, L, q, bound);
            const bool got = ess_interval(q, n, crit, m, bound, lane, r);
            G.has[lane] = got ? 1 : 0;
            G.found[lane] = r;
        }
        __syncthreads();
        if (chain && lane == 0) {
            int found = 0;
            for (int i = 0; i <= m; i++)
                if (G.has[i]) G.crit[found++] = G.found[i];
            G.m = found;
        }
        __syncthreads();
    }
    const int nr = chain ? G.m : 0;
    // the models, compacted in root order as ess_hypothesis leaves them: lane r keeps its E, lane 0 writes the slots
    double E[9];
    bool kept = false;
    if (act && lane < nr) kept = ess_root_model(G.table, G.B, G.d1, G.d2, rho * G.crit[lane], E);
    if (act && lane < kEssRoots) {
        G.has[lane] = kept ? 1 : 0;
        for (int k = 0; k < 9; k++) G.E[9 * lane + k] = 0.0;
    }
    __syncthreads();
    if (act && lane < kEssRoots && kept) {
        int at = 0;
        for (int i = 0; i < lane; i++) at += G.has[i];
        for (int k = 0; k < 9; k++) G.E[9 * at + k] = E[k];
        if (z) z[(size_t)kEssRoots * h + at] = rho * G.crit[lane];
    }
    __syncthreads();
    if (act && lane < kEssRoots) {
        int n = 0;
        for (int i = 0; i < kEssRoots; i++) n += G.has[i];
        double M[9];
        for (int k = 0; k < 9; k++) M[k] = G.E[9 * (lane < n ? lane : 0) + k];
        ess_write_model(models[(size_t)kEssRoots * h + lane], lane < n, M);
        valid[(size_t)kEssRoots * h + lane] = lane < n ? 1 : 0;
        if (z && lane >= n) z[(size_t)kEssRoots * h + lane] = 0.0;
    }
}

__global__ __launch_bounds__(64) void k_ess_hypotheses(const EssJob *__restrict__ job, const EssObs *__restrict__ obs,
                                                       EssModel *__restrict__ models, int32_t *__restrict__ valid,
                                                       int32_t *__restrict__ samples)
{
    constexpr int kGroups = 64 / kEssLanes;
    __shared__ EssGroup groups[kGroups];
    EssGroup &G = groups[threadIdx.x / kEssLanes];
    const int lane = threadIdx.x % kEssLanes;
    const int h = blockIdx.x * kGroups + threadIdx.x / kEssLanes;
    const bool act = h < job->H;

    if (act && lane == 0) {
        int32_t smp[kEssSample];
        G.ok = ess_sample(*job, h, obs, smp, G.d1, G.d2) ? 1 : 0;
        for (int j = 0; j < kEssSample; j++) G.sample[j] = smp[j];
    }
    ess_group_models(G, lane, h, act, models, valid, nullptr);
    if (act && lane < kEssSample) samples[(size_t)kEssSample * h + lane] = G.sample[lane];
}

// mcorb_dev_ess_solve_selftest: problem h of a table in place of a hypothesis's sample -- its camera in jobs[h], its five matches
// as doubles, the bearings as mcorb_ess_solve forms them -- in k_ess_hypotheses' launch shape, so neighbouring problems share a
// workgroup and its EssGroup array as neighbouring hypotheses do
__global__ __launch_bounds__(64) void k_ess_solve_selftest(const EssJob *__restrict__ jobs, const double *__restrict__ uv1,
                                                           const double *__restrict__ uv2, int n, EssModel *__restrict__ models,
                                                           int32_t *__restrict__ valid, double *__restrict__ z)
{
    constexpr int kGroups = 64 / kEssLanes;
    __shared__ EssGroup groups[kGroups];
    EssGroup &G = groups[threadIdx.x / kEssLanes];
    const int lane = threadIdx.x % kEssLanes;
    const int h = blockIdx.x * kGroups + threadIdx.x / kEssLanes;
    const bool act = h < n;

    if (act && lane == 0) {
        const double *a = uv1 + 2 * (size_t)kEssSample * h, *b = uv2 + 2 * (size_t)kEssSample * h;
        for (int j = 0; j < kEssSample; j++) {
            EssPt p;
            ess_point(jobs[h], a[2 * j], a[2 * j + 1], b[2 * j], b[2 * j + 1], p);
            ess_bearing(p.x1, p.y1, G.d1[j]);
            ess_bearing(p.x2, p.y2, G.d2[j]);
        }
        G.ok = 1;
    }
    ess_group_models(G, lane, h, act, models, valid, z);
}

__device__ __forceinline__ void ess_point_of(const EssJob &job, const EssObs &o, EssPt &p)
{
    ess_point(job, (double)o.u1, (double)o.v1, (double)o.u2, (double)o.v2, p);
}

__global__ __launch_bounds__(kEssTile) void k_ess_score(const EssJob *__restrict__ job, const EssObs *__restrict__ obs,
                                                        const EssModel *__restrict__ models, int32_t *__restrict__ count)
{
    __shared__ int32_t cnt[kEssSlotBlock];
    const int S = job->S;
    const int k = blockIdx.x * kEssTile + threadIdx.x;
    const bool in = k < S;
    const double threshold2 = job->threshold2;
    EssPt p;
    ess_point_of(*job, obs[in ? k : 0], p);   // (S >= 1: a lane beyond the matches scores match 0 and counts nothing)
    consensus_count<kEssSlotBlock>(
        job->H * kEssRoots, count, cnt, [&](int s) { return models[s].valid; },   // (uniform over the workgroup)
        [&](int s) {
            double E[9];
#pragma unroll
            for (int j = 0; j < 9; j++) E[j] = models[s].E[j];
            return in && sac_is_inlier(ess_sampson(E, p), threshold2);
        });
}

__global__ __launch_bounds__(kEssTile) void k_ess_pick(const EssJob *__restrict__ job, const EssObs *__restrict__ obs,
                                                       const EssModel *__restrict__ models, const int32_t *__restrict__ valid,
                                                       const int32_t *__restrict__ count,
                                                       int32_t *__restrict__ cheir, EssPick *__restrict__ pick)
{
    __shared__ unsigned long long wkey[4];
    __shared__ int32_t wmodels[4], votes[4];
    __shared__ EssPick P;
    const int t = threadIdx.x, lane = t & 63;
    const int S = job->S;
    if (t < 4) votes[t] = 0;
    // (eight trips' loads at a time: a trip alone waits out two loads' latency, 390 times at 10 000 hypotheses)
    int32_t n_models;
    const int slot = consensus_best_wg<kEssKeyBits, 8>(
        job->H * kEssRoots, [&](int s) { return valid[s]; },   // (models[s].valid, read densely)
        [&](int s) { return count[s]; }, wkey, wmodels, n_models);
    if (t == 0) ess_pick(models, count, slot, n_models, P);
    __syncthreads();
    const int i = blockIdx.x * kEssTile + t;
    bool pass[4] = {false, false, false, false};
    if (i < S && P.slot >= 0) {
        EssPt p;
        ess_point_of(*job, obs[i], p);
        if (sac_is_inlier(ess_sampson(P.E, p), job->threshold2)) {
#pragma unroll
            for (int c = 0; c < 4; c++) pass[c] = ess_candidate_passes(P, c, p, job->distance);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const unsigned long long mask = __ballot(pass[c]);
        if (lane == 0 && mask) atomicAdd(&votes[c], __popcll(mask));
    }
    __syncthreads();
    if (t < 4 && votes[t]) atomicAdd(&cheir[t], votes[t]);
    if (blockIdx.x == 0 && t == 0) *pick = P;
}

__global__ __launch_bounds__(kEssTile) void k_ess_finish(const EssJob *__restrict__ job, const EssObs *__restrict__ obs,
                                                         const EssPick *__restrict__ pick, const int32_t *__restrict__ cheir,
                                                         const int32_t *__restrict__ samples, EssOut *out, uint8_t *flags)
{
    __shared__ EssPick P;
    const int t = threadIdx.x;
    if (t == 0) P = *pick;
    __syncthreads();
    const int32_t votes[4] = {cheir[0], cheir[1], cheir[2], cheir[3]};
    const int w = ess_vote(votes);
    const int i = blockIdx.x * kEssTile + t;
    if (i < job->S) {
        uint8_t flag = 0;
        if (P.slot >= 0) {
            EssPt p;
            ess_point_of(*job, obs[i], p);
            flag = sac_is_inlier(ess_sampson(P.E, p), job->threshold2) && ess_candidate_passes(P, w, p, job->distance) ? 1 : 0;
        }
        flags[i] = flag;
    }
    if (blockIdx.x == 0 && t == 0) ess_finish(P, votes, samples, *out);
}

// a pass of k_ess_fit: the 21 sums at P over the members, the same bits in every lane.  Lanes 0 .. 5 leave E of P and of its five
// perturbations in LDS; every lane takes the 54 numbers into registers at uniform addresses (broadcasts), walks members t, t + 256,
// .. with its 21 sums in registers, and the workgroup folds them (wg_fold).  A member's EssPt is computed again from its
// EssObs in every pass, as k_ess_score does it: four divisions next to the six residuals' six divisions and six square roots,
// against a buffer of 32 bytes per match that would follow n and be read back in its place.  Both barriers are met by every lane;
// Es and part are written again only behind a barrier that every lane reaches after it has read them: the next pass's first
struct EssFitPass {
    const EssJob *job;
    const EssObs *obs;
    const uint8_t *member;
    int S;
    double inv_thr;
    double (*Es)[9];
    double (*part)[kEssFitSums];
    __device__ __forceinline__ void operator()(const PoseState &P, double sums[kEssFitSums])
    {
        const int t = threadIdx.x;
        if (t < kEssFitPoses) {
            PoseState Q;
            double E[9];
            ess_fit_pose(P, t, Q);
            ess_fit_E(Q, E);
#pragma unroll
            for (int j = 0; j < 9; j++) Es[t][j] = E[j];
        }
        __syncthreads();
        double E[kEssFitPoses][9], s[kEssFitSums];
#pragma unroll
        for (int k = 0; k < kEssFitPoses; k++)
#pragma unroll
            for (int j = 0; j < 9; j++) E[k][j] = Es[k][j];
#pragma unroll
        for (int k = 0; k < kEssFitSums; k++) s[k] = 0.0;
        for (int i = t; i < S; i += kEssTile) {
            if (!member[i]) continue;
            EssPt p;
            ess_point_of(*job, obs[i], p);
            ess_fit_add(E, p, inv_thr, s);
        }
        wg_fold<kEssFitSums>(s, part, sums);
    }
};

// The polished call only, behind a k_ess_finish whose record and flags stay in device memory.  ONE workgroup, for k_align_fit's
// reason: the sums are floating-point and their order is part of the definition.  pick and member[0 .. S) are what k_ess_finish
// left; nothing host-mapped is read.  Every lane holds the same pose, counts and verdicts, so the rounds' control flow is uniform;
// a match's flags are read and written by the one lane that serves it, in member[0 .. S) and member[S .. 2 S), which swap on
// acceptance
__global__ __launch_bounds__(kEssTile) void k_ess_fit(const EssJob *__restrict__ job, const EssObs *__restrict__ obs, const EssOut *pick,
                                                      uint8_t *member, int rounds, int max_iterations, double inv_thr, EssOut *out,
                                                      uint8_t *flags, EssPolish *polish)
{
    __shared__ double Es[kEssFitPoses][9];
    __shared__ double part[kPoseBlocks][kEssFitSums];
    __shared__ int32_t wcnt[kPoseBlocks];
    const int t = threadIdx.x;
    const int S = job->S;
    const double threshold2 = job->threshold2, distance = job->distance;
    PoseState cur;
    double E[9];
#pragma unroll
    for (int j = 0; j < 9; j++) cur.R[j] = pick->R[j];   // (not pose_load, as in k_rel_fit)
#pragma unroll
    for (int j = 0; j < 3; j++) cur.t[j] = pick->t[j];
#pragma unroll
    for (int j = 0; j < 9; j++) E[j] = pick->E[j];
    int32_t n_ransac = pick->n_ransac_inliers, count = pick->n_inliers;
    uint8_t *curf = member, *other = member + S;
    if (t == 0) ess_polish_begin(*polish, cur, E, n_ransac, count);
    if (pick->status == MCORB_ESS_OK) {   // (uniform over the workgroup)
        EssFitPass pass{job, obs, curf, S, inv_thr, Es, part};
        for (int round = 0; round < rounds; round++) {
            pass.member = curf;
            int mine = 0;
            for (int i = t; i < S; i += kEssTile) mine += curf[i] ? 1 : 0;
            const int members = wg_total(mine, wcnt);
            PoseState cand;
            double c0, c1, Ec[9];
            int32_t its, status;
            ess_fit_round(pass, cur, members, max_iterations, cand, its, status, c0, c1);
            ess_fit_E(cand, Ec);
            int within_mine = 0, in = 0;
            for (int i = t; i < S; i += kEssTile) {
                EssPt p;
                ess_point_of(*job, obs[i], p);
                bool within, flag;
                ess_fit_test(cand, Ec, p, threshold2, distance, within, flag);
                other[i] = flag ? 1 : 0;
                within_mine += within ? 1 : 0;
                in += flag ? 1 : 0;
            }
            const int nr = wg_total(within_mine, wcnt);
            const int n = wg_total(in, wcnt);
            const bool accepted = n >= count;
            if (t == 0) {
                mcorb_ess_polish_round &q = polish->round[round];
                q.cost_initial = pose_default_nan(c0);
                q.cost_final = pose_default_nan(c1);
                q.n_members = members;
                q.iterations = its;
                q.status = status;
                q.n_ransac_inliers = nr;
                q.n_inliers = n;
                q.accepted = accepted ? 1 : 0;
                polish->rounds_run = round + 1;
            }
            if (!accepted) break;
            cur = cand;
#pragma unroll
            for (int j = 0; j < 9; j++) E[j] = Ec[j];
            n_ransac = nr;
            count = n;
            uint8_t *swap = curf;
            curf = other;
            other = swap;
        }
    }
    for (int i = t; i < S; i += kEssTile) flags[i] = curf[i];
    if (t == 0) {
        for (int j = 0; j < 9; j++) out->R[j] = cur.R[j];
        for (int j = 0; j < 3; j++) out->t[j] = cur.t[j];
        for (int j = 0; j < 9; j++) out->E[j] = E[j];
        out->status = pick->status;
        out->n_ransac_inliers = n_ransac;
        out->n_inliers = count;
        out->best_hypothesis = pick->best_hypothesis;
        out->best_root = pick->best_root;
        for (int j = 0; j < kEssSample; j++) out->sample[j] = pick->sample[j];
        out->n_models = pick->n_models;
        for (int c = 0; c < 4; c++) out->cheirality[c] = pick->cheirality[c];
        out->pad = 0;
    }
}

void launch_ess_fit(hipStream_t st, const EssFitArgs &a)
{
    hipLaunchKernelGGL(k_ess_fit, dim3(1), dim3(kEssTile), 0, st, a.job, a.obs, a.pick, a.member, a.rounds, a.max_iterations, a.inv_thr, a.out,
                       a.flags, a.polish);
}

void launch_ess_hypotheses(hipStream_t st, const EssArgs &a, int H)
{
    constexpr int kGroups = 64 / kEssLanes;
    hipLaunchKernelGGL(k_ess_hypotheses, dim3((H + kGroups - 1) / kGroups), dim3(64), 0, st, a.job, a.obs, a.models, a.valid, a.samples);
}

void launch_ess_solve_selftest(hipStream_t st, const EssJob *jobs, const double *uv1, const double *uv2, int n, EssModel *models, int32_t *valid,
                                double *z)
{
    constexpr int kGroups = 64 / kEssLanes;
    hipLaunchKernelGGL(k_ess_solve_selftest, dim3((n + kGroups - 1) / kGroups), dim3(64), 0, st, jobs, uv1, uv2, n, models, valid, z);
}

void launch_ess_score(hipStream_t st, const EssArgs &a, int S, int H)
{
    hipLaunchKernelGGL(k_ess_score, dim3((S + kEssTile - 1) / kEssTile, (H * kEssRoots + kEssSlotBlock - 1) / kEssSlotBlock), dim3(kEssTile), 0,
                       st, a.job, a.obs, a.models, a.count);
}

void launch_ess_pick(hipStream_t st, const EssArgs &a, int S)
{
    hipLaunchKernelGGL(k_ess_pick, dim3((S + kEssTile - 1) / kEssTile), dim3(kEssTile), 0, st, a.job, a.obs, a.models, a.valid, a.count, a.cheir, a.pick);
}

void launch_ess_finish(hipStream_t st, const EssArgs &a, int S)
{
    hipLaunchKernelGGL(k_ess_finish, dim3((S + kEssTile - 1) / kEssTile), dim3(kEssTile), 0, st, a.job, a.obs, a.pick, a.cheir, a.samples, a.out,
                       a.flags);
}

}  // namespace mcorb
