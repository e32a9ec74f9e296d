// mcorb_kfdb_gpu.hip -- the keyframe database's kernels (mcorb_kfdb.cpp): k_kfdb_score (DBoW2 TemplatedDatabase::queryL1 and
// TemplatedVocabulary::score over the stored BowVectors), k_kfdb_best2 (the best / second-best search of getMatches_distRatio as
// LoopCloser::featureMatchesBow calls it, and for one entry against many probe frames in one launch: FrontEnd::InterMatchingBow,
// Relocalization::featureMatchesBow) and k_kfdb_gather (a rig frame's LF descriptors into an entry or a probe slot).  No
// extraction job runs them and no benchmark leg times them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"

namespace mcorb {

constexpr int kScoreT = 256, kScoreWaves = kScoreT / 64;

// ---------------------------------------------------------------------------
// queryL1, entry-major.  blockIdx.y = query, blockIdx.x = a run of kKfdbEntriesPerBlock entries.  The query's (word id, value)
// list is staged once per workgroup in LDS (kKfdbMaxWords x 12 B = 48 KB); a wave takes an entry and walks its ascending ids 64 at
// a time, every lane binary-searching its id in the query.  The terms of the shared words, (|q - d| - |q|) - |d| in fp64, are
// added to the wave's one accumulator in ascending lane order (the ballot's set bits, lowest first), batch after batch: the sum
// DBoW2's `pit->second += value` builds while it iterates the query's std::map, whose first term is the first shared word's.
// No contraction (the file is built with -ffp-contract=off), no reassociation, no atomics.
// Only entries below the query's limit (max_id, clamped to the size) are touched.  Per (query, entry): the raw sum and the number
// of shared words; the host lists the entries whose count is > 0.
// A query is a stored vector: q_sel[q] indexes (q_ids, q_vals, q_n) with the same stride -- the store itself (query_entries,
// score) or the one-vector scratch a host query was uploaded to.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kScoreT) void k_kfdb_score(const uint32_t *__restrict__ ids, const double *__restrict__ vals,
                                                        const int *__restrict__ nbow, int stride, const uint32_t *__restrict__ q_ids,
                                                        const double *__restrict__ q_vals, const int *__restrict__ q_n,
                                                        const int *__restrict__ q_sel, const int *__restrict__ q_limit,
                                                        const int *__restrict__ e_list, int out_stride, double *__restrict__ raw,
                                                        int *__restrict__ shared)
{
    __shared__ uint32_t s_id[kKfdbMaxWords];
    __shared__ double s_val[kKfdbMaxWords];
    const int q = blockIdx.y, limit = q_limit[q];
    const int e0 = blockIdx.x * kKfdbEntriesPerBlock;
    if (e0 >= limit) return;   // (uniform over the workgroup: before the barrier)
    const int qs = q_sel[q], nq = min(q_n[qs], kKfdbMaxWords);
    for (int i = threadIdx.x; i < nq; i += kScoreT) {
        s_id[i] = q_ids[(size_t)qs * stride + i];
        s_val[i] = q_vals[(size_t)qs * stride + i];
    }
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int e1 = min(e0 + kKfdbEntriesPerBlock, limit);
    for (int x = e0 + wave; x < e1; x += kScoreWaves) {
        const int e = e_list ? e_list[(size_t)q * out_stride + x] : x;   // (score: the one entry a query is held against)
        const int n = min(nbow[e], stride);
        const uint32_t *eid = ids + (size_t)e * stride;
        const double *eval = vals + (size_t)e * stride;
        double acc = 0.0;
        int cnt = 0;
        for (int b = 0; b < n; b += 64) {
            const int i = b + lane;
            double term = 0.0;
            bool hit = false;
            if (i < n) {
                const uint32_t w = eid[i];
                int lo = 0, hi = nq;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_id[mid] < w) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < nq && s_id[lo] == w) {
                    const double qv = s_val[lo], dv = eval[i];
                    term = (fabs(qv - dv) - fabs(qv)) - fabs(dv);
                    hit = true;
                }
            }
            unsigned long long mask = __ballot(hit);
            while (mask) {
                const int j = __builtin_ctzll(mask);
                const double t = __shfl(term, j);
                acc = cnt == 0 ? t : acc + t;
                cnt++;
                mask &= mask - 1;
            }
        }
        if (lane == 0) {
            raw[(size_t)q * out_stride + x] = acc;
            shared[(size_t)q * out_stride + x] = cnt;
        }
    }
}

void launch_kfdb_score(hipStream_t st, const uint32_t *ids, const double *vals, const int *nbow, int stride, const uint32_t *q_ids,
                       const double *q_vals, const int *q_n, const int *q_sel, const int *q_limit, const int *e_list, int nq,
                       int max_limit, int out_stride, double *raw, int *shared)
{
    if (nq < 1 || max_limit < 1) return;
    dim3 grid((max_limit + kKfdbEntriesPerBlock - 1) / kKfdbEntriesPerBlock, nq);
    hipLaunchKernelGGL(k_kfdb_score, grid, dim3(kScoreT), 0, st, ids, vals, nbow, stride, q_ids, q_vals, q_n, q_sel, q_limit, e_list,
                       out_stride, raw, shared);
}

// ---------------------------------------------------------------------------
// getMatches_distRatio's search (ORBextractor.cpp:1240-1263) for every A feature of every node that frame A shares with one or
// more frames B, in one launch: LoopCloser::featureMatchesBow (one B), FrontEnd::InterMatchingBow / Relocalization::
// featureMatchesBow of a slot's worth of probe frames (many B's), the local map's search (one B).  item i = {position of the A
// feature in A's feature list, shared-node record}; record k = {B's set, first position, count, -} of the node's B list in that
// B's feature list (feats_b + set * feats_stride ints; its descriptors at desc_b + set * desc_stride bytes -- a single pair passes
// B's own base and set 0).  One lane per item loops over the B list in list order with strict '<' (the first minimum wins) and
// emits {the best B feature or -1, best, second best (0x7fffffff: none), the A feature}.  The acceptance and the one-to-one
// bookkeeping stay on the host, in record order (Best2Search, mcorb_kfdb_store.h).
// The host lists the items B by B (probe by probe) and, within a B, node by node: the lanes of a wave mostly share a record, so a
// step of the B loop is one 32-byte row for the whole wave (the same address in every lane), and the rows of a node, which every
// item of it walks, stay in L2.  The A descriptor is loaded once and stays in registers.  No LDS, no atomics: the work is tens of
// candidates per item; what a many-probe launch saves is np - 1 submissions and synchronisations.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kfdb_best2(const uint8_t *__restrict__ desc_a, const int *__restrict__ feats_a,
                                                    const uint8_t *__restrict__ desc_p, size_t desc_stride,
                                                    const int *__restrict__ feats_p, size_t feats_stride,
                                                    const int2 *__restrict__ items, int nitems, const int4 *__restrict__ nodes,
                                                    int4 *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nitems) return;
    const int2 it = items[i];
    const int4 rg = nodes[it.y];   // {B's set, first, count, -}
    const int a = feats_a[it.x];
    const ulonglong4 q = *reinterpret_cast<const ulonglong4 *>(desc_a + (size_t)a * 32);
    const uint8_t *desc_b = desc_p + (size_t)rg.x * desc_stride;
    const int *feats_b = feats_p + (size_t)rg.x * feats_stride + rg.y;
    int4 r = int4{-1, 0x7fffffff, 0x7fffffff, a};
    for (int j = 0; j < rg.z; j++) {
        const int b = feats_b[j];
        const int d = (int)hamming256(q, *reinterpret_cast<const ulonglong4 *>(desc_b + (size_t)b * 32));
        if (d < r.y) { r.x = b; r.z = r.y; r.y = d; }
        else if (d < r.z) r.z = d;
    }
    out[i] = r;
}

void launch_kfdb_best2(hipStream_t st, const uint8_t *desc_a, const int *feats_a, const uint8_t *desc_b, size_t desc_stride,
                       const int *feats_b, size_t feats_stride, const int2 *items, int nitems, const int4 *recs, int4 *out)
{
    if (nitems < 1) return;
    hipLaunchKernelGGL(k_kfdb_best2, dim3((nitems + 255) / 256), dim3(256), 0, st, desc_a, feats_a, desc_b, desc_stride, feats_b,
                       feats_stride, items, nitems, recs, out);
}

// dst[i] = the slot's descriptor src[i] (image * kcap + keypoint), 32 bytes each: the LF set of a rig frame, device to device
__global__ __launch_bounds__(256) void k_kfdb_gather(const uint8_t *__restrict__ desc, const int *__restrict__ src, int n, uint8_t *__restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    *reinterpret_cast<ulonglong4 *>(dst + (size_t)i * 32) = *reinterpret_cast<const ulonglong4 *>(desc + (size_t)src[i] * 32);
}

void launch_kfdb_gather(hipStream_t st, const uint8_t *desc, const int *src, int n, uint8_t *dst)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_kfdb_gather, dim3((n + 255) / 256), dim3(256), 0, st, desc, src, n, dst);
}

}  // namespace mcorb
