// mcorb_init_gpu.hip -- the kernels of mcorb_lmap_initialize (mcorb_init.cpp): FrontEnd::initialization from the pose between the
// first two rig frames to the first landmarks (FrontEnd.cpp:2633-2839; the arithmetic is mcorb_init.h).  One submission on the
// store's stream: k_init_triangulate (both instances), k_init_select, k_init_put.  No workgroup waits on another and no result
// depends on the launch shape.  No extraction job runs them and no benchmark leg times them.
//
// k_init_triangulate: k_map_triangulate's shape -- one wave per workgroup, the host cuts the flagged matches into blocks of up to
// 64 ordered by view count, matches of at most 4 views in the instance without the run-time-shaped solver -- and init_item per
// lane: the views, the DLT, the per-view gates, cos and dist2, an 80-byte record at the match's own index.
//
// k_init_select: one workgroup.  Pass 1 walks the matches in order, 1024 at a time: a ballot and 16 wave totals in LDS give every
// match the number of parllaxVec and depthVec members before it, so the keys (init_key) are compacted in match order and the
// depthVec prefix is the match's id offset.  Pass 2 is the selection of the key of rank count / 2, a radix select over the keys
// (init_radix_median).  Integer counts only; no float is ever summed across lanes.  The form that lost: every lane ranking its own
// member against all members staged through LDS tiles, which is quadratic (DESIGN.md section 9l has both measurements).
//
// k_init_put: every workgroup forms the verdict and the scale from *sel alike (init_verdict); a lane finishes its match
// (init_finish), stores an accepted one into its slot and writes the match's record to host-mapped memory with plain vector
// stores; lane 0 of workgroup 0 writes the call's record.
#include <hip/hip_runtime.h>

#include "mcorb_common.h"
#include "mcorb_kernels.h"

namespace mcorb {

template <bool kAnyViews>
__global__ __launch_bounds__(kMapBlock) void k_init_triangulate(MapArgs a, int block0)
{
    MapBlock b;
    if (map_lane(a, block0, b)) init_item<kAnyViews>(a, a.items[b.first + threadIdx.x]);
}

void launch_init_triangulate(hipStream_t st, const MapArgs &a, int nblocks_small, int nblocks_any)
{
    if (nblocks_small > 0) hipLaunchKernelGGL(k_init_triangulate<false>, dim3(nblocks_small), dim3(kMapBlock), 0, st, a, 0);
    if (nblocks_any > 0) hipLaunchKernelGGL(k_init_triangulate<true>, dim3(nblocks_any), dim3(kMapBlock), 0, st, a, nblocks_small);
}

// The key of rank count / 2 among keys[0 .. count), by a radix select in the workgroup: eight passes of eight bits from the top.
// A pass counts, in 256 LDS integers, the next byte of every key that still carries the prefix found so far; a scan over the 256
// counts (a shuffle scan per wave and four wave totals) names the one byte whose range holds the rank, which becomes part of the
// prefix, and the rank becomes the rank inside that range.  Equal keys are one value, so no index is needed.  hist: 256, tot: 4,
// pick: 2 integers of LDS.  Every lane of the workgroup takes part
__device__ inline void init_radix_median(const uint64_t *__restrict__ keys, int count, int *hist, int *tot, int *pick, double *median)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t prefix = 0, mask = 0;
    int rank = count / 2;
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();   // (pick of the pass before has been read)
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < count; j += kInitSelectT) {
            const uint64_t k = keys[j];
            if ((k & mask) == prefix) atomicAdd(&hist[(int)((k >> shift) & 255u)], 1);
        }
        __syncthreads();
        int mine = 0, incl = 0;
        if (tid < 256) {
            mine = incl = hist[tid];
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            if (lane == 63) tot[wave] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < wave; w++) incl += tot[w];
            const int excl = incl - mine;
            if (excl <= rank && rank < incl) { pick[0] = tid; pick[1] = rank - excl; }
        }
        __syncthreads();
        prefix |= (uint64_t)pick[0] << shift;
        mask |= (uint64_t)255u << shift;
        rank = pick[1];
    }
    if (tid == 0) *median = init_unkey(prefix);
}

__global__ __launch_bounds__(kInitSelectT) void k_init_select(const MapOut *__restrict__ rec, const uint8_t *__restrict__ flags, int n,
                                                              uint64_t *__restrict__ keys, int32_t *__restrict__ offset,
                                                              InitSel *__restrict__ sel)
{
    constexpr int kWaves = kInitSelectT / 64;
    __shared__ int hist[256], tot[4], pick[2];
    __shared__ int wave_p[kWaves], wave_d[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t *keys_p = keys, *keys_d = keys + n;
    int base_p = 0, base_d = 0;
    for (int i0 = 0; i0 < n; i0 += kInitSelectT) {
        const int i = i0 + tid;
        bool in_p = false, in_d = false;
        double cosp = 0.0, dist2 = 0.0;
        if (i < n) {
            if (flags[i]) {   // (a match whose flag is clear has no record)
                const int verdict = rec[i].verdict;
                in_p = init_in_parallax(1, verdict);
                in_d = init_in_depth(1, verdict);
                if (in_p) { cosp = rec[i].cos; dist2 = rec[i].dist2; }
            }
        }
        const unsigned long long bp = __ballot(in_p), bd = __ballot(in_d), below = (1ull << lane) - 1ull;
        __syncthreads();   // (the totals of the chunk before have been read)
        if (lane == 0) { wave_p[wave] = __popcll(bp); wave_d[wave] = __popcll(bd); }
        __syncthreads();
        int before_p = base_p + __popcll(bp & below), before_d = base_d + __popcll(bd & below);
        for (int w = 0; w < kWaves; w++) {
            const int tp = wave_p[w], td = wave_d[w];
            if (w < wave) { before_p += tp; before_d += td; }
            base_p += tp;
            base_d += td;
        }
        if (i < n) offset[i] = before_d;
        if (in_p) keys_p[before_p] = init_key(cosp);
        if (in_d) keys_d[before_d] = init_key(dist2);
    }
    if (tid == 0) {
        sel->n_parallax = base_p;
        sel->n_depth = base_d;
        sel->parallax = 0.0;
        sel->depth = 0.0;
    }
    __syncthreads();   // the keys and the zeros are visible to the workgroup
    if (base_p > 0 && base_d > 0) {
        init_radix_median(keys_p, base_p, hist, tot, pick, &sel->parallax);
        init_radix_median(keys_d, base_d, hist, tot, pick, &sel->depth);
    }
}

void launch_init_select(hipStream_t st, const MapOut *rec, const uint8_t *flags, int n, uint64_t *keys, int32_t *offset, InitSel *sel)
{
    hipLaunchKernelGGL(k_init_select, dim3(1), dim3(kInitSelectT), 0, st, rec, flags, n, keys, offset, sel);
}

template <bool kCases>
__global__ __launch_bounds__(kInitPutT) void k_init_put(InitPutArgs p)
{
    const int i = blockIdx.x * kInitPutT + threadIdx.x;
    InitCall call;
    double s;
    init_verdict(p.job, *p.sel, call, s);
    if (i == 0) *p.h_call = call;
    if (i >= p.job.n) return;
    const int flag = p.flags[i];
    MapOut o;
    map_clear(o);
    MapViews v;
    v.nv = v.nv1 = 0;
    if (flag) {
        o = p.rec[i];
        if (o.verdict == kMapLandmark && call.status == kInitDone) {
            if (kCases) map_case_views(p.cases, i, v);
            else map_gather_pair(p.a, p.query[i], p.train[i], v);
        }
    }
    if (init_finish(v, p.job, call, s, flag, o)) {
        const size_t slot = (size_t)p.job.next_lid + (size_t)p.offset[i];
        double *g = p.geom + slot * 6;
        for (int k = 0; k < 3; k++) { g[k] = o.X[k]; g[3 + k] = o.normal[k]; }
        p.nrays[slot] = o.n_rays;
    }
    p.h_rec[i] = o;
}

void launch_init_put(hipStream_t st, const InitPutArgs &p, bool from_cases)
{
    const int nb = (max(p.job.n, 1) + kInitPutT - 1) / kInitPutT;   // (n == 0 still writes the call's record)
    if (from_cases) hipLaunchKernelGGL(k_init_put<true>, dim3(nb), dim3(kInitPutT), 0, st, p);
    else hipLaunchKernelGGL(k_init_put<false>, dim3(nb), dim3(kInitPutT), 0, st, p);
}

__global__ __launch_bounds__(kMapBlock) void k_init_gates(MapCases c, int n, MapOut *__restrict__ out)
{
    const int i = blockIdx.x * kMapBlock + threadIdx.x;
    if (i >= n) return;
    MapOut o;
    init_gate_case(c, i, o);
    out[i] = o;
}

void launch_init_gates(hipStream_t st, const MapCases &c, int n, MapOut *out)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_init_gates, dim3((n + kMapBlock - 1) / kMapBlock), dim3(kMapBlock), 0, st, c, n, out);
}

}  // namespace mcorb
