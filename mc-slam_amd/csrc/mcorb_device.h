// mcorb_device.h -- device-side helpers shared by every .hip file (wave64, gfx950).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"

namespace mcorb {

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
// number of set bits of a wave mask below this lane, plus acc (v_mbcnt_lo/hi: two instructions)
__device__ __forceinline__ int lane_rank(unsigned long long mask, int acc = 0)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, (uint32_t)acc));
}
// a value every lane of the wave holds alike, moved to a scalar register
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// LDS written by some lanes of this wave, read by others of the SAME wave (a wave only ever reads what it wrote itself): no s_barrier
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The workgroup reductions of the pose estimators' kernels: a workgroup of kWgLanes = four waves of 64.  The LDS is the caller's and
// is passed in.  The order of the additions below is part of the numeric contract (mcorb_pose.h's pose_fold states it for the host):
// this is its one place on the device.
constexpr int kWgLanes = 256, kWgWaves = 4;

// the four waves' values of slot k, combined as (b0 + b1) + (b2 + b3)
template <int KP>
__device__ __forceinline__ double wg_combine(double (*part)[KP], int k) { return (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]); }
__device__ __forceinline__ int wg_combine(const int32_t *w) { return (w[0] + w[1]) + (w[2] + w[3]); }

// a wave's fold of its lanes' K sums by shuffles with strides 32 .. 1: lane 0 holds s[l] + s[l + stride] of pose_fold
template <int K>
__device__ __forceinline__ void wave_fold(double s[K])
{
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1)
#pragma unroll
        for (int k = 0; k < K; k++) s[k] = s[k] + __shfl_down(s[k], stride, 64);
}
// wave_fold, then lane 0 of each wave leaves the wave's sums in part[wave][0 .. K) and the workgroup meets at a barrier.
// part: [4][KP] of LDS, KP >= K
template <int K, int KP>
__device__ __forceinline__ void wg_fold_waves(double s[K], double (*part)[KP])
{
    static_assert(K <= KP, "part holds a wave's K sums");
    wave_fold<K>(s);
    if (lane_id() == 0)
#pragma unroll
        for (int k = 0; k < K; k++) part[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
}
// the fold of the lanes' K sums -> S, the same bits in every lane.  No barrier behind the reads of part: the caller writes part
// again only behind a barrier that every lane reaches after this returns
template <int K, int KP>
__device__ __forceinline__ void wg_fold(double s[K], double (*part)[KP], double S[K])
{
    wg_fold_waves<K>(s, part);
#pragma unroll
    for (int k = 0; k < K; k++) S[k] = wg_combine(part, k);
}

// the wave's sum of an integer, in every lane
__device__ __forceinline__ int wave_total(int v)
{
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
// the workgroup's sum of an integer, the same in every lane; wcnt: [4] of LDS, free again on return
__device__ __forceinline__ int wg_total(int v, int32_t *wcnt)
{
    v = wave_total(v);
    if (lane_id() == 0) wcnt[threadIdx.x >> 6] = v;
    __syncthreads();
    const int total = wg_combine(wcnt);
    __syncthreads();
    return total;
}

// XCD-aware work index: workgroups b and b+8 share an XCD (and its L2) under the observed round-robin
// placement, so give each XCD one contiguous eighth of the work items -- spatial neighbours (cells or
// tiles that re-read the same 64-B lines for their halos) then hit in the same L2.  Bijective for any n;
// placement only changes speed, never results.
__device__ __forceinline__ int xcd_remap(int b, int n)
{
    const int q = n >> 3, r = n & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}
__device__ __forceinline__ int reflect101(int p, int len)
{
    // cv::borderInterpolate(BORDER_REFLECT_101); |overshoot| < len here
    if (p < 0) p = -p;
    if (p >= len) p = 2 * len - 2 - p;
    return p;
}

// pt of a selected keypoint from its packed selection word (level, x, y of the level), as the host's keypoint records build it:
// (float)x, (float)y, times the float scale factor above level 0 (k_undistort, k_bow_tables)
struct UndistScales {
    float s[kMaxLevels];
    UndistScales(const float *scale, int nlevels) : s{}
    {
        for (int l = 0; l < nlevels && l < kMaxLevels; l++) s[l] = scale[l];
    }
};
__device__ __forceinline__ float2 sel_point(uint32_t v, const UndistScales &sc)
{
    int l, xl, yl;
    unpack_sel(v, l, xl, yl);
    float x = (float)xl, y = (float)yl;
    if (l != 0) { x *= sc.s[l]; y *= sc.s[l]; }
    return make_float2(x, y);
}

// popcount(x) + acc in one instruction; chaining the eight words of a 256-bit XOR through the
// accumulator operand saves the separate adds the compiler otherwise emits
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc)
{
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}
__device__ __forceinline__ uint32_t hamming256(const ulonglong4 &a, const ulonglong4 &b)
{
    const unsigned long long x0 = a.x ^ b.x, x1 = a.y ^ b.y, x2 = a.z ^ b.z, x3 = a.w ^ b.w;
    uint32_t d = __builtin_popcount((uint32_t)x0);
    d = bcnt_acc((uint32_t)(x0 >> 32), d);
    d = bcnt_acc((uint32_t)x1, d);
    d = bcnt_acc((uint32_t)(x1 >> 32), d);
    d = bcnt_acc((uint32_t)x2, d);
    d = bcnt_acc((uint32_t)(x2 >> 32), d);
    d = bcnt_acc((uint32_t)x3, d);
    d = bcnt_acc((uint32_t)(x3 >> 32), d);
    return d;
}

}  // namespace mcorb
