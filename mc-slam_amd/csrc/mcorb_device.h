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
