// mcorb_track_gpu.hip -- the kernels of fast tracking on a device store (mcorb_track.cpp): k_track_project (Tracking::project_,
// MCSlam/src/Tracking.cpp:208-260, for every candidate landmark and camera) and k_track_match (the per-query part of
// Tracking::querryEachFrame, :329-377: the 10 nearest keypoints by image position, the radius gate, the best Hamming distance).
// The arithmetic is mcorb_track.h, the code the host-only store runs.  k_track_points (the rig slot entries only) rebuilds a
// rig slot's keypoints from their packed selection words; k_track_compact leaves each camera's kept candidates in candidate
// order, in host-mapped memory; k_track_dedup_min / _win / _emit leave each camera's de-duplicated matches there (querryEachFrame
// :380-415 in closed form).  Each kernel's body is a __device__ function that takes the view or frame by reference, the base pointers
// and n; its one k_track_* entry calls it with what the TrItem of frame blockIdx.z says (mcorb_track.h), for every tracking call:
// a single call is a call of one frame, a grid whose z is 1.  No extraction job runs them and no benchmark leg times them.
//
// blockIdx.z is the frame, whose TrItem -- and, in k_track_project, view -- is read from device memory at an address that is
// uniform over the wave, so it stays in scalar registers as a kernel argument does.  The grid's x is sized by the frame with the
// most candidates: a workgroup beyond its own frame's n leaves, uniformly (none does in a call of one frame).  A frame's block of
// every per-pair array begins at item.rows and has the layout [c * n + i] inside, which is all a body sees.
//
// They go out in one submission: k_track_match reads the validity bytes k_track_project wrote and the points k_track_points
// wrote, k_track_compact and the de-duplication read the rows of the kernels before them, and the host copies rows and matches
// out after the one synchronisation.  No scratch, no workgroup waits on another; up to k_track_compact no atomics, and a query's
// result depends on that query alone, so the launch shape cannot change it.  The de-duplication's atomics are a claim and a
// minimum, whose results do not depend on arrival order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"
#include "mcorb_track.h"

namespace mcorb {

// One lane per candidate, the cameras looped inside.  The view is uniform for the workgroup: its 12 + 17 doubles per camera come
// through the scalar cache.  A lane's own traffic is its 24 bytes of point, gathered by landmark id, and per
// camera the plain stores of (x, y) and the validity byte, camera-major, so that a camera's row is contiguous for k_track_match;
// pts (may be NULL) receives the gathered point, for bestMatchLandmarks.
__device__ __forceinline__ void track_project(const mcorb_track_view &view, const double *__restrict__ geom, const int *__restrict__ cand,
                                              int n, float2 *__restrict__ xy, uint8_t *__restrict__ valid, double *__restrict__ pts)
{
    const int i = blockIdx.x * kTrackProjectT + threadIdx.x;
    if (i >= n) return;
    const double *g = geom + (size_t)cand[i] * 6;
    const double X[3] = {g[0], g[1], g[2]};
    if (pts)
        for (int k = 0; k < 3; k++) pts[3 * (size_t)i + k] = X[k];
    double p0[3];
    tr_body(view.R0, view.t0, X, p0);
    const bool front = tr_in_front(view, p0);
    for (int c = 0; c < view.ncams; c++) {
        float x = 0.f, y = 0.f;
        const bool keep = front && tr_pixel(view, c, p0, x, y);
        const size_t at = (size_t)c * n + i;
        xy[at] = make_float2(x, y);
        valid[at] = keep ? 1 : 0;
    }
}

__global__ __launch_bounds__(kTrackProjectT) void k_track_project(const TrItem *__restrict__ items, const mcorb_track_view *__restrict__ views,
                                                                  const double *__restrict__ geom, const int *__restrict__ cand,
                                                                  float2 *__restrict__ xy, uint8_t *__restrict__ valid,
                                                                  double *__restrict__ pts)
{
    const TrItem &it = items[blockIdx.z];
    if ((int)(blockIdx.x * kTrackProjectT) >= it.n) return;
    track_project(views[it.view], geom, cand + it.cand_first, it.n, xy + it.rows, valid + it.rows,
                  pts ? pts + 3 * it.cand_first : nullptr);
}

void launch_track_project(hipStream_t st, const TrItem *items, int nf, int max_n, const mcorb_track_view *views, const double *geom,
                          const int *cand, float2 *xy, uint8_t *valid, double *pts)
{
    if (nf < 1 || max_n < 1) return;
    hipLaunchKernelGGL(k_track_project, dim3((max_n + kTrackProjectT - 1) / kTrackProjectT, 1, nf), dim3(kTrackProjectT), 0, st, items,
                       views, geom, cand, xy, valid, pts);
}

// A workgroup of kTrackMatchWaves waves serves camera blockIdx.y; a wave serves kTrackMatchQ consecutive candidates.  The
// camera's keypoints stream through LDS in tiles of MCORB_TRACK_TILE x 8 bytes, each tile read once per workgroup and used by
// all its queries, so a camera may have any number of keypoints.
//
// The 10 nearest of a query under the total order (d2, k) live in lanes 0 .. 9 of its wave, lane r holding rank r (every other
// lane, and an unfilled rank, holds `none`, which is greater than any key): no register is indexed dynamically.  For 64 keypoints
// of the tile at a time every lane takes one distance; a keypoint inside the radius whose key is less than rank 9's is inserted --
// one at a time over the ballot, each a shift by one lane of the ranks above it.  The set that results is the 10 least keys
// whatever the order of insertion.  Then lanes 0 .. 9 take one neighbour's Hamming distance each (8 dwords xor + popcount,
// against the landmark's descriptor gathered by id) and the wave reduces min(dist * 16 + rank) over those below max_hamming.
struct TrTop { uint64_t d2; uint32_t k; };

__device__ __forceinline__ void track_tile_query(const float2 *tile, int tile_n, int first_k, float qx, float qy, double max_d2, int lane,
                                                 TrTop &top)
{
    for (int j0 = 0; j0 < tile_n; j0 += 64) {
        const int j = j0 + lane;
        uint64_t d2 = kTrNoneD2;
        const uint32_t k = (uint32_t)(first_k + j);
        bool cand = false;
        if (j < tile_n) {
            const float2 kp = tile[j];
            cand = tr_d2(qx, qy, kp.x, kp.y, max_d2, d2);
        }
        uint64_t thr_d2 = __shfl(top.d2, MCORB_TRACK_KNN - 1, 64);
        uint32_t thr_k = __shfl(top.k, MCORB_TRACK_KNN - 1, 64);
        cand = cand && tr_less(d2, k, thr_d2, thr_k);
        unsigned long long todo = __ballot(cand);
        while (todo) {
            const int src = __ffsll(todo) - 1;
            const uint64_t nd2 = __shfl(d2, src, 64);
            const uint32_t nk = __shfl(k, src, 64);
            const uint64_t pd2 = __shfl_up(top.d2, 1, 64);
            const uint32_t pk = __shfl_up(top.k, 1, 64);
            if (lane < MCORB_TRACK_KNN && tr_less(nd2, nk, top.d2, top.k)) {
                // this rank moves up: it takes the new key when the rank below stays, that rank's key otherwise
                const bool here = lane == 0 || tr_less(pd2, pk, nd2, nk);
                top.d2 = here ? nd2 : pd2;
                top.k = here ? nk : pk;
            }
            thr_d2 = __shfl(top.d2, MCORB_TRACK_KNN - 1, 64);
            thr_k = __shfl(top.k, MCORB_TRACK_KNN - 1, 64);
            cand = cand && lane != src && tr_less(d2, k, thr_d2, thr_k);
            todo = __ballot(cand);
        }
    }
}

__device__ __forceinline__ void track_match(float2 *tile, const TrFrame &frame, const float2 *__restrict__ kp_xy,
                                            const uint32_t *__restrict__ kp_desc, const uint32_t *__restrict__ lm_desc,
                                            const int *__restrict__ cand, int n, const float2 *__restrict__ xy,
                                            const uint8_t *__restrict__ valid, double max_d2, int max_hamming, TrBest *__restrict__ best)
{
    const int c = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_kp = frame.n_kp[c], first = frame.first[c];
    const int q0 = (blockIdx.x * kTrackMatchWaves + wave) * kTrackMatchQ;
    const size_t row = (size_t)c * n;

    bool live[kTrackMatchQ];
    float qx[kTrackMatchQ], qy[kTrackMatchQ];
    TrTop top[kTrackMatchQ];
#pragma unroll
    for (int q = 0; q < kTrackMatchQ; q++) {
        const int i = q0 + q;
        live[q] = i < n && valid[row + i] != 0;   // (uniform over the wave)
        const float2 p = live[q] ? xy[row + i] : make_float2(0.f, 0.f);
        qx[q] = p.x;
        qy[q] = p.y;
        top[q].d2 = kTrNoneD2;
        top[q].k = kTrNoneK;
    }

    for (int t0 = 0; t0 < n_kp; t0 += MCORB_TRACK_TILE) {
        const int tile_n = min(MCORB_TRACK_TILE, n_kp - t0);
        __syncthreads();   // the tile before has been read by every wave
        for (int j = threadIdx.x; j < tile_n; j += kTrackMatchT) tile[j] = kp_xy[(size_t)first + t0 + j];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kTrackMatchQ; q++)
            if (live[q]) track_tile_query(tile, tile_n, t0, qx[q], qy[q], max_d2, lane, top[q]);
    }

#pragma unroll
    for (int q = 0; q < kTrackMatchQ; q++) {
        if (!live[q]) continue;
        const int i = q0 + q;
        uint32_t key = kTrNoGate;
        if (top[q].k != kTrNoneK) {   // lanes 0 .. 9 that hold a neighbour
            const uint32_t *a = lm_desc + (size_t)cand[i] * 8;
            const uint32_t *b = kp_desc + ((size_t)first + top[q].k) * 8;
            int dist = 0;
            for (int w = 0; w < 8; w++) dist += __popc(a[w] ^ b[w]);
            key = tr_gate_key(dist, lane, max_hamming);
        }
        for (int s = 8; s >= 1; s >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, s, 64));   // lanes 0 .. 15
        key = (uint32_t)__shfl((int)key, 0, 64);
        if (key == kTrNoGate) {
            if (lane == 0) best[row + i] = TrBest{-1, kTrBest0};
        } else {
            const int kp = (int)__shfl((int)top[q].k, (int)(key & 15u), 64);
            if (lane == 0) best[row + i] = TrBest{kp, (int)(key >> 4)};
        }
    }
}

__global__ __launch_bounds__(kTrackMatchT) void k_track_match(const TrItem *__restrict__ items, const float2 *__restrict__ kp_xy,
                                                              const uint32_t *__restrict__ kp_desc, const uint32_t *__restrict__ lm_desc,
                                                              const int *__restrict__ cand, const float2 *__restrict__ xy,
                                                              const uint8_t *__restrict__ valid, double max_d2, int max_hamming,
                                                              TrBest *__restrict__ best)
{
    __shared__ float2 tile[MCORB_TRACK_TILE];
    const TrItem &it = items[blockIdx.z];
    if ((int)(blockIdx.x * (kTrackMatchWaves * kTrackMatchQ)) >= it.n) return;
    track_match(tile, it.frame, kp_xy + it.kp0, kp_desc + it.desc0 * 8, lm_desc, cand + it.cand_first, it.n, xy + it.rows,
                valid + it.rows, max_d2, max_hamming, best + it.rows);
}

void launch_track_match(hipStream_t st, const TrItem *items, int nf, int max_n, int ncams, const float2 *kp_xy, const uint8_t *kp_desc,
                        const uint8_t *lm_desc, const int *cand, const float2 *xy, const uint8_t *valid, double max_d2, int max_hamming,
                        TrBest *best)
{
    if (nf < 1 || max_n < 1) return;
    const int per_block = kTrackMatchWaves * kTrackMatchQ;
    hipLaunchKernelGGL(k_track_match, dim3((max_n + per_block - 1) / per_block, ncams, nf), dim3(kTrackMatchT), 0, st, items, kp_xy,
                       reinterpret_cast<const uint32_t *>(kp_desc), reinterpret_cast<const uint32_t *>(lm_desc), cand, xy, valid, max_d2,
                       max_hamming, best);
}

// One lane per keypoint of a row of kcap, camera c's image being img0 + c of the slot: pt as the host's keypoint record has it
// (sel_point), for k_track_match's tiles.  A pass of its own: on a small batch sel / nsel are host-mapped memory, which is read
// here once and not once per workgroup of k_track_match.  The padding of a row (k >= nsel) is not written and never read.
__device__ __forceinline__ void track_points(const uint32_t *__restrict__ sel, const int *__restrict__ nsel, int kcap, int img0,
                                             const UndistScales &sc, float2 *__restrict__ out)
{
    const int c = blockIdx.y, m = img0 + c, k = blockIdx.x * kTrackPointsT + threadIdx.x;
    if (k >= min(nsel[m], kcap)) return;
    out[(size_t)c * kcap + k] = sel_point(sel[(size_t)m * kcap + k], sc);
}

// frame f's images img0 .. img0 + ncams -> rows (f * ncams + c) * kcap of out, f's kp0 on: a frame named twice is converted twice
__global__ __launch_bounds__(kTrackPointsT) void k_track_points(const TrItem *__restrict__ items, const uint32_t *__restrict__ sel,
                                                                const int *__restrict__ nsel, int kcap, UndistScales sc,
                                                                float2 *__restrict__ out)
{
    const TrItem &it = items[blockIdx.z];
    if (it.n < 1) return;   // (no kernel reads the keypoints of a frame without candidates)
    track_points(sel, nsel, kcap, it.img0, sc, out + it.kp0);
}

// (rig slots' frames only: the keypoints of a host-array frame are uploaded)
void launch_track_points(hipStream_t st, const TrItem *items, int nf, int max_n, const uint32_t *sel, const int *nsel, int kcap, int ncams,
                         const float *scale, int nlevels, float2 *out)
{
    if (kcap < 1 || ncams < 1 || nf < 1 || max_n < 1) return;
    hipLaunchKernelGGL(k_track_points, dim3((kcap + kTrackPointsT - 1) / kTrackPointsT, ncams, nf), dim3(kTrackPointsT), 0, st, items,
                       sel, nsel, kcap, UndistScales(scale, nlevels), out);
}

// The ordered stream compaction of a row of n flags (each 0 or 1), the part k_track_compact and k_track_dedup_emit share.
// Workgroup b serves flags b * 256 .. b * 256 + 255 and counts the set ones before them itself: p[0 .. b * 256) in 16-byte loads
// from the first 16-byte boundary of the row on (the up to 15 bytes in front of it and as many behind the last whole load byte by
// byte), a wave reduction and four partials through LDS (before, kept: one int per wave) -- at most n bytes, from L2, so
// n * n / 512 per row.  Its own 256 flags are ranked by a ballot per wave.  No workgroup waits on another.  -> keep: this lane's
// flag i = b * 256 + t is set; at: its place among the row's set flags; total: the set flags up to and including this
// workgroup's, the row's count in its last workgroup.  Every lane of the workgroup calls it (it synchronises)
static_assert(kTrackCompactT == kTrackDedupT, "track_rank serves both with one workgroup size");
struct TrRank { bool keep; int at, total; };

__device__ __forceinline__ TrRank track_rank(const uint8_t *__restrict__ p, int n, int *before, int *kept)
{
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int end = b * kTrackCompactT;    // a multiple of 16: the head and the tail below are 16 bytes together, or none
    const int head = end ? (int)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) : 0;
    const int nvec = (end - head) >> 4, tail = head + (nvec << 4);
    int s = 0;
    if (t < head) s = p[t];
    const uint4 *v = reinterpret_cast<const uint4 *>(p + head);
    for (int j = t; j < nvec; j += kTrackCompactT) {
        const uint4 q = v[j];
        s += __popc(q.x) + __popc(q.y) + __popc(q.z) + __popc(q.w);
    }
    if (tail + t < end) s += p[tail + t];
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);

    const int i = end + t;
    const bool keep = i < n && p[i] != 0;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) {
        before[wave] = s;
        kept[wave] = __popcll(mask);
    }
    __syncthreads();
    int at = 0, total = 0;
    for (int w = 0; w < kTrackCompactT / 64; w++) {
        at += before[w] + (w < wave ? kept[w] : 0);
        total += before[w] + kept[w];
    }
    return TrRank{keep, lane_rank(mask, at), total};
}

// camera blockIdx.y's validity bytes (as k_track_project writes them) -> its kept candidates in candidate order; the last
// workgroup of a camera has the camera's total.
__device__ __forceinline__ void track_compact(int *before, int *kept, int n, const uint8_t *__restrict__ valid,
                                              const float2 *__restrict__ xy, const TrBest *__restrict__ best, TrRow *__restrict__ rows,
                                              int32_t *__restrict__ n_proj)
{
    const int c = blockIdx.y, b = blockIdx.x;
    if (b * kTrackCompactT >= n) return;   // (uniform over the workgroup)
    const size_t row = (size_t)c * n;
    const TrRank k = track_rank(valid + row, n, before, kept);
    if (k.keep) {
        const int i = b * kTrackCompactT + threadIdx.x;
        const float2 q = xy[row + i];
        const TrBest r = best[row + i];
        rows[row + k.at] = TrRow{i, q.x, q.y, r.kp, r.dist};
    }
    if (b == (n - 1) / kTrackCompactT && threadIdx.x == 0) n_proj[c] = k.total;   // (the last workgroup of n, whatever the grid)
}

// n_proj: MCORB_MAX_CAMS counts per frame
__global__ __launch_bounds__(kTrackCompactT) void k_track_compact(const TrItem *__restrict__ items, const uint8_t *__restrict__ valid,
                                                                  const float2 *__restrict__ xy, const TrBest *__restrict__ best,
                                                                  TrRow *__restrict__ rows, int32_t *__restrict__ n_proj)
{
    __shared__ int before[kTrackCompactT / 64], kept[kTrackCompactT / 64];
    const TrItem &it = items[blockIdx.z];
    track_compact(before, kept, it.n, valid + it.rows, xy + it.rows, best + it.rows, rows + it.rows,
                  n_proj + (size_t)blockIdx.z * MCORB_MAX_CAMS);
}

void launch_track_compact(hipStream_t st, const TrItem *items, int nf, int max_n, int ncams, const uint8_t *valid, const float2 *xy,
                          const TrBest *best, TrRow *rows, int32_t *n_proj)
{
    if (nf < 1 || max_n < 1) return;
    hipLaunchKernelGGL(k_track_compact, dim3((max_n + kTrackCompactT - 1) / kTrackCompactT, ncams, nf), dim3(kTrackCompactT), 0, st, items,
                       valid, xy, best, rows, n_proj);
}

// ---- the de-duplication (mcorb_track.h, tr_dedup_value): per camera a segmented arg-min over the matched candidates, grouped by
// the pixel of the matched keypoint, then the winners in candidate order.  Three kernels behind k_track_match in the same
// submission, on the uncompacted rows (valid, best), one lane per (camera, candidate).
//
// Camera c's table is slots [c << log2p, (c + 1) << log2p) of owner / val, 1 << log2p >= 2 * n, both cleared to all ones by one
// hipMemsetAsync each in front of k_track_dedup_min.  A pixel's slot is the first one of its probe sequence that a candidate of
// that pixel claimed: the claim is a 32-bit compare-and-swap of kTrNoOwner against the candidate's index (an index is never all
// ones), a slot is never given back, and a slot's pixel is read through its owner's keypoint, which no kernel here writes -- so no
// pixel key is stored and none serves as "empty".  Which slot a pixel gets depends on arrival order; what the slot's val ends as,
// the 64-bit atomicMin over the pixel's values, does not.  The probe loop runs at most 1 << log2p trips whatever memory holds, an
// owner is followed only to a candidate index and a keypoint index inside their arrays, and a lane that found no slot (the table
// cannot fill: it has twice the slots there are candidates) takes no part, it does not spin.
// No workgroup waits on another, no scratch.
constexpr uint32_t kTrNoOwner = ~0u;

__device__ __forceinline__ void track_dedup_min(const TrFrame &frame, const float2 *__restrict__ kp_xy, int n,
                                                const uint8_t *__restrict__ valid, const TrBest *__restrict__ best, int log2p,
                                                uint32_t *__restrict__ owner, unsigned long long *__restrict__ val,
                                                int32_t *__restrict__ slot)
{
    const int c = blockIdx.y, i = blockIdx.x * kTrackDedupT + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)c * n, tab = (size_t)c << log2p;
    int mine = -1;
    if (valid[row + i] != 0 && best[row + i].kp >= 0) {   // (k_track_match wrote best for the valid ones only)
        const TrBest b = best[row + i];
        const float2 *kp = kp_xy + frame.first[c];
        const uint64_t key = tr_pixel_key(kp[b.kp].x, kp[b.kp].y);
        const uint32_t slots = 1u << log2p;
        uint32_t s = (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> (64 - log2p));
        for (uint32_t trip = 0; trip < slots; trip++, s = (s + 1) & (slots - 1)) {
            const uint32_t o = atomicCAS(&owner[tab + s], kTrNoOwner, (uint32_t)i);
            if (o != kTrNoOwner) {   // claimed before: by this pixel?
                // (only a table that was not cleared holds an owner that is no candidate, or one without a match in this call)
                if (o >= (uint32_t)n) continue;
                const int okp = best[row + o].kp;
                if (okp < 0 || okp >= frame.n_kp[c]) continue;
                const float2 q = kp[okp];
                if (tr_pixel_key(q.x, q.y) != key) continue;
            }
            atomicMin(&val[tab + s], (unsigned long long)tr_dedup_value(b.dist, i));
            mine = (int)s;
            break;
        }
    }
    slot[row + i] = mine;
}

// frame f's tables are slots [tab, tab + (ncams << log2p)) of owner / val, a table per (frame, camera) of its own size
__global__ __launch_bounds__(kTrackDedupT) void k_track_dedup_min(const TrItem *__restrict__ items, const float2 *__restrict__ kp_xy,
                                                                  const uint8_t *__restrict__ valid, const TrBest *__restrict__ best,
                                                                  uint32_t *__restrict__ owner, unsigned long long *__restrict__ val,
                                                                  int32_t *__restrict__ slot)
{
    const TrItem &it = items[blockIdx.z];
    if ((int)(blockIdx.x * kTrackDedupT) >= it.n) return;
    track_dedup_min(it.frame, kp_xy + it.kp0, it.n, valid + it.rows, best + it.rows, it.log2p, owner + it.tab, val + it.tab,
                    slot + it.rows);
}

// a candidate is its pixel's entry iff the slot's minimum is its own value
__device__ __forceinline__ void track_dedup_win(int n, const TrBest *__restrict__ best, const int32_t *__restrict__ slot,
                                                const unsigned long long *__restrict__ val, int log2p, uint8_t *__restrict__ win)
{
    const int c = blockIdx.y, i = blockIdx.x * kTrackDedupT + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)c * n;
    const int s = slot[row + i];
    win[row + i] = s >= 0 && val[((size_t)c << log2p) + s] == tr_dedup_value(best[row + i].dist, i) ? 1 : 0;
}

__global__ __launch_bounds__(kTrackDedupT) void k_track_dedup_win(const TrItem *__restrict__ items, const TrBest *__restrict__ best,
                                                                  const int32_t *__restrict__ slot,
                                                                  const unsigned long long *__restrict__ val, uint8_t *__restrict__ win)
{
    const TrItem &it = items[blockIdx.z];
    if ((int)(blockIdx.x * kTrackDedupT) >= it.n) return;
    track_dedup_win(it.n, best + it.rows, slot + it.rows, val + it.tab, it.log2p, win + it.rows);
}

// The winners in candidate order, ranked the way k_track_compact ranks the validity bytes (track_rank); the last workgroup of a
// camera has the camera's total.  matches and n_match are host-mapped.
__device__ __forceinline__ void track_dedup_emit(int *before, int *kept, int n, const uint8_t *__restrict__ win,
                                                 const TrBest *__restrict__ best, TrMatch *__restrict__ matches,
                                                 int32_t *__restrict__ n_match)
{
    const int c = blockIdx.y, b = blockIdx.x;
    if (b * kTrackDedupT >= n) return;   // (uniform over the workgroup)
    const size_t row = (size_t)c * n;
    const TrRank k = track_rank(win + row, n, before, kept);
    if (k.keep) {
        const int i = b * kTrackDedupT + threadIdx.x;
        const TrBest r = best[row + i];
        matches[row + k.at] = TrMatch{i, r.kp, r.dist};
    }
    if (b == (n - 1) / kTrackDedupT && threadIdx.x == 0) n_match[c] = k.total;   // (the last workgroup of n, whatever the grid)
}

// n_match: MCORB_MAX_CAMS counts per frame
__global__ __launch_bounds__(kTrackDedupT) void k_track_dedup_emit(const TrItem *__restrict__ items, const uint8_t *__restrict__ win,
                                                                   const TrBest *__restrict__ best, TrMatch *__restrict__ matches,
                                                                   int32_t *__restrict__ n_match)
{
    __shared__ int before[kTrackDedupT / 64], kept[kTrackDedupT / 64];
    const TrItem &it = items[blockIdx.z];
    track_dedup_emit(before, kept, it.n, win + it.rows, best + it.rows, matches + it.rows, n_match + (size_t)blockIdx.z * MCORB_MAX_CAMS);
}

void launch_track_dedup(hipStream_t st, const TrItem *items, int nf, int max_n, int ncams, const float2 *kp_xy, const uint8_t *valid,
                        const TrBest *best, uint32_t *owner, unsigned long long *val, int32_t *slot, uint8_t *win, TrMatch *matches,
                        int32_t *n_match)
{
    if (nf < 1 || max_n < 1) return;
    const dim3 grid((max_n + kTrackDedupT - 1) / kTrackDedupT, ncams, nf), block(kTrackDedupT);
    hipLaunchKernelGGL(k_track_dedup_min, grid, block, 0, st, items, kp_xy, valid, best, owner, val, slot);
    hipLaunchKernelGGL(k_track_dedup_win, grid, block, 0, st, items, best, slot, val, win);
    hipLaunchKernelGGL(k_track_dedup_emit, grid, block, 0, st, items, win, best, matches, n_match);
}

}  // namespace mcorb
