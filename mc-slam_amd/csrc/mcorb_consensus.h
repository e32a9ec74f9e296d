// mcorb_consensus.h -- what the pose RANSACs (mcorb_sac.h, mcorb_rel.h, mcorb_ess.h, mcorb_align.h) share behind their hypotheses:
// the winner's key, its arg-max, and on the device the consensus count and the arg-max of a workgroup.  The counts are integers,
// so no result depends on the order of an addition here.
#pragma once
#include <stdint.h>

#include "mcorb_pose.h"
#if defined(__HIPCC__)
#include "mcorb_device.h"
#endif

namespace mcorb {

// The winner among indexed models: the largest count of those that are valid, a tie to the lowest index.  As a key that a maximum
// picks: (count + 1) << kBits | (2^kBits - 1 - index) for a model, 0 without one; 0 <= index < 2^kBits.  A key never leaves a
// kernel or a serial run: the records hold indices and counts
template <int kBits>
MCORB_POSE_HD uint64_t consensus_key(int32_t valid, int32_t count, int index)
{
    return valid ? (((uint64_t)count + 1) << kBits) | (uint64_t)((1 << kBits) - 1 - index) : 0;
}
template <int kBits>
MCORB_POSE_HD int consensus_key_index(uint64_t key) { return key ? (1 << kBits) - 1 - (int)(key & ((1 << kBits) - 1)) : -1; }

// the arg-max over N models, serially (the *_run_serial of a host-only store).  valid_of(i), count_of(i): model i's
struct ConsensusBest {
    uint64_t key;
    int n_models;
};
template <int kBits, class ValidOf, class CountOf>
inline ConsensusBest consensus_best(int N, const ValidOf &valid_of, const CountOf &count_of)
{
    ConsensusBest b{0, 0};
    for (int i = 0; i < N; i++) {
        const int32_t valid = valid_of(i);
        const uint64_t ki = consensus_key<kBits>(valid, count_of(i), i);
        b.key = ki > b.key ? ki : b.key;
        b.n_models += valid;
    }
    return b;
}

#if defined(__HIPCC__)
// The body of a score kernel.  A workgroup of kWgLanes owns a tile of observations, one per lane, and block blockIdx.y of kBlock
// models out of N, which it reads at uniform addresses: per valid model a ballot and a population count per wave into the integer
// counts cnt[kBlock] of LDS, then one atomicAdd per (workgroup, model) into count[N].  valid_of(h) must be uniform over the
// workgroup; inlier_of(h) is the lane's verdict (false in a lane beyond the observations).  Every lane reaches both barriers: a
// functor must never return around them
template <int kBlock, class ValidOf, class InlierOf>
__device__ __forceinline__ void consensus_count(int N, int32_t *__restrict__ count, int32_t *cnt, const ValidOf &valid_of,
                                                const InlierOf &inlier_of)
{
    static_assert(kBlock <= kWgLanes, "a lane per model of the block adds its count");
    const int t = threadIdx.x, lane = t & 63;
    if (t < kBlock) cnt[t] = 0;
    __syncthreads();
    const int h0 = blockIdx.y * kBlock, h1 = min(N, h0 + kBlock);
    for (int h = h0; h < h1; h++) {
        if (!valid_of(h)) continue;
        const unsigned long long mask = __ballot(inlier_of(h));
        if (lane == 0 && mask) atomicAdd(&cnt[h - h0], __popcll(mask));
    }
    __syncthreads();
    if (t < h1 - h0 && cnt[t]) atomicAdd(&count[h0 + t], cnt[t]);
}

// The arg-max of a pick kernel: every workgroup of kWgLanes finds it for itself -> the winner's index, -1 without a model, and
// the number of models, the same in every lane.  A lane walks models t, t + 256, .., kTrips of them at a time with their loads
// issued together (k_ess_pick walks 100 000 slots: DESIGN.md section 9m); a wave reduces by xor-shuffles, the four waves through
// wkey[4] and wmodels[4] of LDS, which are free again at the caller's next barrier
template <int kBits, int kTrips, class ValidOf, class CountOf>
__device__ __forceinline__ int consensus_best_wg(int N, const ValidOf &valid_of, const CountOf &count_of, unsigned long long *wkey,
                                                 int32_t *wmodels, int32_t &n_models)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long key = 0;
    int32_t nm = 0;
    for (int i0 = t; i0 < N; i0 += kTrips * kWgLanes) {
        int32_t v[kTrips], c[kTrips];
#pragma unroll
        for (int u = 0; u < kTrips; u++) {
            const int i = i0 + u * kWgLanes;
            v[u] = i < N ? valid_of(i) : 0;
            c[u] = i < N ? count_of(i) : 0;
        }
#pragma unroll
        for (int u = 0; u < kTrips; u++) {
            const unsigned long long ki = consensus_key<kBits>(v[u], c[u], i0 + u * kWgLanes);
            key = ki > key ? ki : key;
            nm += v[u];
        }
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
    for (int w = 1; w < kWgWaves; w++) key = wkey[w] > key ? wkey[w] : key;
    n_models = wg_combine(wmodels);
    return consensus_key_index<kBits>(key);
}
#endif

}  // namespace mcorb
