// mcorb_bow_gpu.hip -- the DBoW2 rows of an extraction job with a vocabulary bound to the rig (mcorb_rig_set_vocabulary):
// k_bow_descend (the vocabulary-tree descent of every descriptor), k_bow_fold (transform()'s FeatureVector and BowVector),
// k_bow_tables and k_bow_best2 (BoW-guided intra-rig matching).  No benchmark leg times them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"

namespace mcorb {

// ---------------------------------------------------------------------------
// DBoW2 vocabulary-tree descent (TemplatedVocabulary::transform's per-feature part, used by
// MultiCameraFrame::extractFeatureSingle, MultiCameraFrame.cpp:257): from the root, move to the child
// with the smallest Hamming distance (strict '<': the first child wins ties) until a leaf; remember the
// node reached at depth `nid_level`.  One descriptor per lane; the children of a node are stored
// contiguously (descriptor + node id), k*32 bytes per step.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bow_descend(const uint8_t *__restrict__ desc, int n, const int *__restrict__ child_start,
                                                     const int *__restrict__ child_count, const ulonglong4 *__restrict__ child_desc,
                                                     const int *__restrict__ child_id, const int *__restrict__ word_id,
                                                     const double *__restrict__ weight, int nid_level, BowRes *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ulonglong4 q = *reinterpret_cast<const ulonglong4 *>(desc + (size_t)i * 32);
    int node = 0, nid = 0, level = 0;
    int cc = child_count[0];
    while (cc > 0) {
        ++level;
        const int cs = child_start[node];
        uint32_t best = 0xffffffffu;
        int bj = 0;
        for (int j = 0; j < cc; j++) {
            const uint32_t d = hamming256(q, child_desc[cs + j]);
            if (d < best) { best = d; bj = j; }
        }
        node = child_id[cs + bj];
        if (level == nid_level) nid = node;
        cc = child_count[node];
    }
    out[i] = BowRes{word_id[node], nid, weight[node]};
}

// ---------------------------------------------------------------------------
// BoW-guided intra-rig matching, the data-parallel half (MultiCameraFrame::computeIntraMatches(matches,
// words_), MultiCameraFrame.cpp:708-745): for feature a of camera c1 and every camera c2 > c1, the best
// and second-best Hamming distance among c2's features that fell into the same vocabulary node, skipping
// candidates whose row differs by 50 px or more; strict '<' so the first minimum wins.  The serial
// track bookkeeping that consumes this table stays on the host.
// All frames of a batch in one launch: blockIdx.z = frame, blockIdx.y = camera pair (c1 < c2).  Per frame f the
// index tables are laid out for image index m = f * ncams + c: slot_of / node_feats / yv at m * kcap,
// node_range at (rg_base[f] + slot) * ncams + c; out at ((f * npairs + pair) * kcap + a).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bow_best2(const uint8_t *__restrict__ desc, int img0, int kcap, int ncams,
                                                   const float *__restrict__ yv, const int *__restrict__ slot_of,
                                                   const int2 *__restrict__ node_range, const int *__restrict__ rg_base,
                                                   const int *__restrict__ node_feats, const int *__restrict__ nfeat,
                                                   int4 *__restrict__ out)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    const int f = blockIdx.z, npairs = ncams * (ncams - 1) / 2;
    int c1 = 0, rem = blockIdx.y;   // pair index -> (c1, c2), pairs in (0,1), (0,2), .., (1,2), .. order
    while (rem >= ncams - 1 - c1) { rem -= ncams - 1 - c1; c1++; }
    const int c2 = c1 + 1 + rem;
    const int m1 = f * ncams + c1, m2 = f * ncams + c2;
    if (a >= nfeat[m1]) return;
    int4 r = int4{-1, 0x7fffffff, 0x7fffffff, 0};
    const int slot = slot_of[(size_t)m1 * kcap + a];
    if (slot >= 0) {
        const int2 rg = node_range[(size_t)(rg_base[f] + slot) * ncams + c2];
        const ulonglong4 q = *reinterpret_cast<const ulonglong4 *>(desc + ((size_t)(img0 + m1) * kcap + a) * 32);
        const float y1 = yv[(size_t)m1 * kcap + a];
        for (int j = 0; j < rg.y; j++) {
            const int b = node_feats[(size_t)m2 * kcap + rg.x + j];
            if (fabsf(__fsub_rn(y1, yv[(size_t)m2 * kcap + b])) >= 50.f) continue;
            const int d = (int)hamming256(q, *reinterpret_cast<const ulonglong4 *>(desc + ((size_t)(img0 + m2) * kcap + b) * 32));
            if (d < r.y) { r.x = j; r.z = r.y; r.y = d; }
            else if (d < r.z) r.z = d;
        }
    }
    out[((size_t)f * npairs + blockIdx.y) * kcap + a] = r;
}

void launch_bow_best2(hipStream_t st, const uint8_t *desc, int img0, int kcap, int ncams, int nframes, const float *yv,
                      const int *slot_of, const int2 *node_range, const int *rg_base, const int *node_feats, const int *nfeat, int4 *out)
{
    if (ncams < 2 || nframes < 1) return;
    dim3 grid((kcap + 255) / 256, ncams * (ncams - 1) / 2, nframes);
    hipLaunchKernelGGL(k_bow_best2, grid, dim3(256), 0, st, desc, img0, kcap, ncams, yv, slot_of, node_range, rg_base, node_feats, nfeat, out);
}

void launch_bow_descend(hipStream_t st, const uint8_t *desc, int n, const int *child_start, const int *child_count,
                        const void *child_desc, const int *child_id, const int *word_id, const double *weight, int nid_level,
                        BowRes *out)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bow_descend, dim3((n + 255) / 256), dim3(256), 0, st, desc, n, child_start, child_count,
                       reinterpret_cast<const ulonglong4 *>(child_desc), child_id, word_id, weight, nid_level, out);
}

// ---------------------------------------------------------------------------
// transform()'s order-defined half inside the extraction job (mcorb_rig_set_vocabulary): k_bow_fold turns one image's descent
// results into its FeatureVector and BowVector exactly as the host's assemble() does (mcorb_bow.cpp), k_bow_tables turns one
// frame's FeatureVectors into the index tables k_bow_best2 reads (node_feats: the feature lists, kcap-strided).  Nothing crosses to the host in between.
// ---------------------------------------------------------------------------
constexpr int kFoldT = 512;
static_assert(kBowFoldMaxKcap % kFoldT == 0, "k_bow_fold: whole keys per lane");

// ascending bitonic sort of K[0, N), N a power of two, by the whole workgroup
__device__ void fold_sort(uint64_t *K, int N)
{
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < N; i += kFoldT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = K[i], b = K[ixj];
                    if ((a > b) == ((i & k) == 0)) { K[i] = b; K[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

// exclusive prefix sum of one value per lane over the workgroup; *total = the sum
__device__ int fold_scan(int v, int *sh, int *total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < kFoldT; o <<= 1) {
        const int x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[kFoldT - 1];
    __syncthreads();
    return incl - v;
}

// runs of equal high words in the sorted keys K[0, m): heads[0, nruns) = their first positions, ascending; heads[nruns] = m
__device__ int fold_runs(const uint64_t *K, int m, int *heads, int *sh)
{
    const int t = threadIdx.x, chunk = (m + kFoldT - 1) / kFoldT;
    const int p0 = min(m, t * chunk), p1 = min(m, p0 + chunk);
    int c = 0;
    for (int p = p0; p < p1; p++) c += p == 0 || (K[p] >> 32) != (K[p - 1] >> 32);
    int total = 0;
    int j = fold_scan(c, sh, &total);
    for (int p = p0; p < p1; p++)
        if (p == 0 || (K[p] >> 32) != (K[p - 1] >> 32)) heads[j++] = p;
    if (t == 0) heads[total] = m;
    __syncthreads();
    return total;
}

// One workgroup per image.  Stable sorts are sorts of (key << 32 | feature index): unique keys, so any sort is stable.  Each word's
// run is folded left to right by one lane and the norm is one lane's sum over the words in ascending order: the host's additions in
// the host's order (no contraction, correctly rounded '/' and sqrt), so the doubles are bit-equal.
__global__ __launch_bounds__(kFoldT) void k_bow_fold(const BowRes *__restrict__ res, const int *__restrict__ nsel, int kcap, int weighting,
                                                     int scoring, int *__restrict__ out_dev, int *__restrict__ out_host)
{
    __shared__ uint64_t K[kBowFoldMaxKcap];
    __shared__ int heads[kBowFoldMaxKcap + 1];
    __shared__ int sh[kFoldT];
    __shared__ int nvalid;
    __shared__ double norm_sh;
    const int m = blockIdx.x, t = threadIdx.x;
    const int n = min(nsel[m], kcap);
    const BowRes *r = res + (size_t)m * kcap;
    int N = 1;
    while (N < n) N <<= 1;
    const BowRecView od = bow_rec(out_dev, kcap, m);
    const BowRecView oh = bow_rec(out_host ? out_host : out_dev, kcap, m);
    const bool both = out_host != nullptr;
    // FeatureVector: the non-stopped features by node id, feature order within a node
    if (t == 0) nvalid = 0;
    __syncthreads();
    for (int i = t; i < N; i += kFoldT) {
        uint64_t k = ~0ull;
        if (i < n && r[i].weight > 0) { k = ((uint64_t)(uint32_t)r[i].nodeup << 32) | (uint32_t)i; atomicAdd(&nvalid, 1); }
        K[i] = k;
    }
    __syncthreads();
    const int nv = nvalid;
    fold_sort(K, N);
    const int nfv = fold_runs(K, nv, heads, sh);
    for (int j = t; j <= nfv; j += kFoldT) {
        const int h = heads[j];
        od.offs[j] = h;
        if (both) oh.offs[j] = h;
        if (j < nfv) {
            const uint32_t node = (uint32_t)(K[h] >> 32);
            od.nodes[j] = node;
            if (both) oh.nodes[j] = node;
        }
    }
    for (int p = t; p < nv; p += kFoldT) {
        const int fi = (int)(uint32_t)K[p];
        od.feats[p] = fi;
        if (both) oh.feats[p] = fi;
    }
    __syncthreads();
    // BowVector: the same features by word id, each word's weights folded in feature order
    for (int i = t; i < N; i += kFoldT)
        K[i] = i < n && r[i].weight > 0 ? ((uint64_t)(uint32_t)r[i].word << 32) | (uint32_t)i : ~0ull;
    __syncthreads();
    fold_sort(K, N);
    const int nbow = fold_runs(K, nv, heads, sh);
    const bool tf_like = weighting == 0 || weighting == 1;   // TF_IDF, TF accumulate; IDF, BINARY keep the first
    constexpr int kPer = kBowFoldMaxKcap / kFoldT;
    double v[kPer];
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        const int j = t + q * kFoldT;
        v[q] = 0.0;
        if (j < nbow) {
            const int p = heads[j], e = heads[j + 1];
            const uint32_t word = (uint32_t)(K[p] >> 32);
            od.ids[j] = word;
            if (both) oh.ids[j] = word;
            double s = r[(uint32_t)K[p]].weight;
            if (tf_like)
                for (int x = p + 1; x < e; x++) s += r[(uint32_t)K[x]].weight;
            v[q] = s;
        }
    }
    __syncthreads();   // K is free: the values take its place
    double *V = reinterpret_cast<double *>(K);
#pragma unroll
    for (int q = 0; q < kPer; q++)
        if (t + q * kFoldT < nbow) V[t + q * kFoldT] = v[q];
    __syncthreads();
    const bool must = scoring != 5;   // L1_NORM, CHI_SQUARE, KL, BHATTACHARYYA -> L1; L2_NORM -> L2; DOT_PRODUCT -> none
    if (must) {
        if (t == 0) {
            double s = 0.0;
            if (scoring == 1) {
                for (int j = 0; j < nbow; j++) s += V[j] * V[j];
                s = sqrt(s);
            } else {
                for (int j = 0; j < nbow; j++) s += fabs(V[j]);
            }
            norm_sh = s;
        }
        __syncthreads();
    }
    const double norm = must ? norm_sh : 0.0, nd = (double)nbow;
    for (int j = t; j < nbow; j += kFoldT) {
        double x = V[j];
        if (tf_like && !must) x /= nd;
        if (must && norm > 0.0) x /= norm;
        od.vals[j] = x;
        if (both) oh.vals[j] = x;
    }
    if (t == 0) {
        od.cnt[0] = nbow; od.cnt[1] = nfv; od.cnt[2] = nv; od.cnt[3] = 0;
        if (both) { oh.cnt[0] = nbow; oh.cnt[1] = nfv; oh.cnt[2] = nv; oh.cnt[3] = 0; }
    }
}

// binary search of `node` in the ascending list a[0, n): its index, or -1
__device__ __forceinline__ int fv_find(const uint32_t *a, int n, uint32_t node)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < node) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && a[lo] == node ? lo : -1;
}

// One workgroup per frame: the tables of k_bow_best2 from the frame's FeatureVectors (k_bow_fold's device records).  A node's slot
// is (first camera holding it) * kcap + its index there: unique per node, the same for every camera, fewer than ncams * kcap per
// frame (rg_base[f] = f * ncams * kcap).  Only the slots that exist are written; k_bow_best2 reads no other.  yv: the rows of the
// |dy| < 50 gate, the undistorted points' y when undist is given, else the keypoint records' y rebuilt from sel.
__global__ __launch_bounds__(256) void k_bow_tables(const int *__restrict__ fold, int kcap, int ncams, const int *__restrict__ nsel,
                                                    const uint32_t *__restrict__ sel, UndistScales sc, const float2 *__restrict__ undist,
                                                    int *__restrict__ slot_of, int *__restrict__ node_feats, int *__restrict__ nfeat,
                                                    int *__restrict__ rg_base, float *__restrict__ yv, int2 *__restrict__ node_range)
{
    const int f = blockIdx.x, t = threadIdx.x, C = ncams;
    const size_t base = (size_t)f * C * kcap;
    for (int c = 0; c < C; c++) {
        const int m = f * C + c, n = min(nsel[m], kcap);
        for (int k = t; k < n; k += 256) {
            const size_t i = (size_t)m * kcap + k;
            slot_of[i] = -1;
            yv[i] = undist ? undist[i].y : sel_point(sel[i], sc).y;
        }
        if (t == 0) nfeat[m] = n;
    }
    if (t == 0) rg_base[f] = (int)base;
    __syncthreads();
    for (int c = 0; c < C; c++) {
        const int m = f * C + c;
        const BowRecView a = bow_rec(const_cast<int *>(fold), kcap, m);
        const int nfv = a.cnt[1];
        for (int e = t; e < nfv; e += 256) {
            const uint32_t node = a.nodes[e];
            int oc = c, oe = e;
            for (int c2 = 0; c2 < c; c2++) {
                const BowRecView b = bow_rec(const_cast<int *>(fold), kcap, f * C + c2);
                const int i = fv_find(b.nodes, b.cnt[1], node);
                if (i >= 0) { oc = c2; oe = i; break; }
            }
            const int slot = oc * kcap + oe;
            const int beg = a.offs[e], end = a.offs[e + 1];
            for (int p = beg; p < end; p++) {
                node_feats[(size_t)m * kcap + p] = a.feats[p];
                slot_of[(size_t)m * kcap + a.feats[p]] = slot;
            }
            if (oc != c) continue;   // the slot's ranges are written by its first camera
            int2 *rg = node_range + (base + slot) * C;
            for (int c2 = 0; c2 < C; c2++) {
                if (c2 == c) { rg[c2] = make_int2(beg, end - beg); continue; }
                const BowRecView b = bow_rec(const_cast<int *>(fold), kcap, f * C + c2);
                const int i = c2 < c ? -1 : fv_find(b.nodes, b.cnt[1], node);
                rg[c2] = i < 0 ? make_int2(0, 0) : make_int2(b.offs[i], b.offs[i + 1] - b.offs[i]);
            }
        }
    }
}

void launch_bow_fold(hipStream_t st, const BowRes *res, const int *nsel, int kcap, int nimg, int weighting, int scoring, int *out_dev,
                     int *out_host)
{
    hipLaunchKernelGGL(k_bow_fold, dim3(nimg), dim3(kFoldT), 0, st, res, nsel, kcap, weighting, scoring, out_dev, out_host);
}

void launch_bow_tables(hipStream_t st, const int *fold, int kcap, int ncams, int nframes, const int *nsel, const uint32_t *sel,
                       const float *scale, int nlevels, const float2 *undist, int *slot_of, int *node_feats, int *nfeat, int *rg_base,
                       float *yv, int2 *node_range)
{
    hipLaunchKernelGGL(k_bow_tables, dim3(nframes), dim3(256), 0, st, fold, kcap, ncams, nsel, sel, UndistScales(scale, nlevels), undist,
                       slot_of, node_feats, nfeat, rg_base, yv, node_range);
}
}  // namespace mcorb
