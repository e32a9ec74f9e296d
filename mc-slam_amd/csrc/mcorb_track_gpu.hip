// mcorb_track_gpu.hip -- the kernels of fast tracking on a device store (mcorb_track.cpp): k_track_project (Tracking::project_,
// MCSlam/src/Tracking.cpp:208-260, for every candidate landmark and camera) and k_track_match (the per-query part of
// Tracking::querryEachFrame, :329-377: the 10 nearest keypoints by image position, the radius gate, the best Hamming distance).
// The arithmetic is mcorb_track.h, the code the host-only store runs.  No extraction job runs them and no benchmark leg times them.
//
// The two go out in one submission: k_track_match reads the validity bytes k_track_project wrote, and the host compacts in
// candidate order after the one synchronisation.  No atomics, no scratch, no workgroup waits on another, and a query's result
// depends on that query alone, so the launch shape cannot change it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_kernels.h"
#include "mcorb_track.h"

namespace mcorb {

// One lane per candidate, the cameras looped inside.  The view is a kernel argument, uniform for the launch: its 12 + 17 doubles
// per camera come through the scalar cache.  A lane's own traffic is its 24 bytes of point, gathered by landmark id, and per
// camera the plain stores of (x, y) and the validity byte, camera-major, so that a camera's row is contiguous for k_track_match;
// pts (may be NULL) receives the gathered point, for bestMatchLandmarks.
__global__ __launch_bounds__(kTrackProjectT) void k_track_project(mcorb_track_view view, const double *__restrict__ geom,
                                                                  const int *__restrict__ cand, int n, float2 *__restrict__ xy,
                                                                  uint8_t *__restrict__ valid, double *__restrict__ pts)
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

void launch_track_project(hipStream_t st, const mcorb_track_view &view, const double *geom, const int *cand, int n, float2 *xy,
                          uint8_t *valid, double *pts)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_track_project, dim3((n + kTrackProjectT - 1) / kTrackProjectT), dim3(kTrackProjectT), 0, st, view, geom, cand,
                       n, xy, valid, pts);
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

__global__ __launch_bounds__(kTrackMatchT) void k_track_match(TrFrame frame, const float2 *__restrict__ kp_xy,
                                                              const uint32_t *__restrict__ kp_desc, const uint32_t *__restrict__ lm_desc,
                                                              const int *__restrict__ cand, int n, const float2 *__restrict__ xy,
                                                              const uint8_t *__restrict__ valid, double max_d2, int max_hamming,
                                                              TrBest *__restrict__ best)
{
    __shared__ float2 tile[MCORB_TRACK_TILE];
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

void launch_track_match(hipStream_t st, const TrFrame &frame, int ncams, const float2 *kp_xy, const uint8_t *kp_desc, const uint8_t *lm_desc,
                        const int *cand, int n, const float2 *xy, const uint8_t *valid, double max_d2, int max_hamming, TrBest *best)
{
    if (n < 1) return;
    const int per_block = kTrackMatchWaves * kTrackMatchQ;
    hipLaunchKernelGGL(k_track_match, dim3((n + per_block - 1) / per_block, ncams), dim3(kTrackMatchT), 0, st, frame, kp_xy,
                       reinterpret_cast<const uint32_t *>(kp_desc), reinterpret_cast<const uint32_t *>(lm_desc), cand, n, xy, valid,
                       max_d2, max_hamming, best);
}

}  // namespace mcorb
