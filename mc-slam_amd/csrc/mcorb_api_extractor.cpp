// mcorb_api_extractor.cpp -- the extern "C" entry points (include/mcorb.h) that need no rig of the caller's: the single-camera
// extractor, matching on host arrays, and the host-side helpers the tests compare against.
#include <string.h>

#include <algorithm>
#include <new>

#include "mcorb_engine.h"

using namespace mcorb;

struct mcorb_extractor {
    mcorb_params params;
    std::unique_ptr<Rig> rig;   // rebuilt when the image size changes
    int w = 0, h = 0;
    // scratch for mcorb_knn2 on host arrays, sized for kc descriptors a side (0: to be allocated)
    DevBuf<uint8_t> d_desc, d_exp;
    DevBuf<int> d_lcounts;
    DevBuf<uint2> d_part;
    HostBuf<KnnRow> h_rows;
    HostBuf<uint32_t> h_mlist;
    HostBuf<int> h_mcount, h_counts;
    HostBuf<int2> h_pair;
    int kc = 0;
};

extern "C" {

// ---------------------------------------------------------------------------
// single-camera extractor
// ---------------------------------------------------------------------------
int mcorb_create(const mcorb_params *p, int max_width, int max_height, mcorb_t **out)
{
    if (!p || !out) { set_error("null argument"); return MCORB_E_ARG; }
    *out = nullptr;
    Tables t;
    int st = compute_tables(*p, t);
    if (st != MCORB_OK) return st;
    mcorb_t *e = new (std::nothrow) mcorb_extractor;
    if (!e) return MCORB_E_ARG;
    e->params = *p;
    if (max_width > 0 && max_height > 0) {
        e->rig.reset(new Rig);
        st = e->rig->init(*p, 1, max_width, max_height, 1, 1);
        if (st != MCORB_OK) {
            const std::string keep = get_error();
            delete e;
            set_error(keep);
            return st;
        }
        e->w = max_width; e->h = max_height;
    } else if (mcorb_device_count() < 1) {
        delete e;
        set_error("no usable gfx950 device (libmcorb has no CPU path)");
        return MCORB_E_NODEVICE;
    }
    *out = e;
    return MCORB_OK;
}

void mcorb_destroy(mcorb_t *e) { delete e; }

static int ensure_rig(mcorb_t *e, int w, int h)
{
    if (e->rig && e->w == w && e->h == h) return MCORB_OK;
    e->rig.reset();
    e->rig.reset(new Rig);
    const int st = e->rig->init(e->params, 1, w, h, 1, 1);
    if (st != MCORB_OK) {
        const std::string keep = get_error();
        e->rig.reset();
        set_error(keep);
        return st;
    }
    e->w = w; e->h = h;
    return MCORB_OK;
}

static int finish_extract(mcorb_t *e, int lap_x0, int lap_x1, mcorb_keypoint *kps, uint8_t *desc, int cap, int *n_out,
                          int *mono_index_out)
{
    Job j;
    j.kind = Job::EXTRACT; j.nimg = 1; j.lap0 = lap_x0; j.lap1 = lap_x1;
    int st = e->rig->submit(0, j);
    if (st == MCORB_OK) st = e->rig->wait(0);
    if (st != MCORB_OK) return st;
    Slot *s = e->rig->slots[0].get();
    const int n = (int)s->kps[0].size();
    if (n_out) *n_out = n;
    if (mono_index_out) *mono_index_out = s->mono[0];
    if (n > cap) { set_error("keypoint buffer too small"); return MCORB_E_CAP; }
    if (kps && n) memcpy(kps, s->kps[0].data(), (size_t)n * sizeof(mcorb_keypoint));
    if (desc && n) memcpy(desc, s->h_desc, (size_t)n * 32);
    return MCORB_OK;
}

int mcorb_extract(mcorb_t *e, const uint8_t *gray, int w, int h, int stride_bytes, int lap_x0, int lap_x1,
                  mcorb_keypoint *kps, uint8_t *desc, int cap, int *n_out, int *mono_index_out)
{
    if (!e) { set_error("null extractor"); return MCORB_E_ARG; }
    if (n_out) *n_out = 0;
    if (!gray || w <= 0 || h <= 0) { set_error("empty image"); return MCORB_E_EMPTY; }
    int st = ensure_rig(e, w, h);
    if (st != MCORB_OK) return st;
    const uint8_t *imgs[1] = {gray};
    st = e->rig->upload_u8(0, imgs, 1, stride_bytes);
    if (st != MCORB_OK) return st;
    return finish_extract(e, lap_x0, lap_x1, kps, desc, cap, n_out, mono_index_out);
}

int mcorb_extract_f32(mcorb_t *e, const float *img01, int w, int h, int stride_bytes, int channels, int lap_x0,
                      int lap_x1, mcorb_keypoint *kps, uint8_t *desc, int cap, int *n_out, int *mono_index_out)
{
    if (!e) { set_error("null extractor"); return MCORB_E_ARG; }
    if (n_out) *n_out = 0;
    if (!img01 || w <= 0 || h <= 0) { set_error("empty image"); return MCORB_E_EMPTY; }
    int st = ensure_rig(e, w, h);
    if (st != MCORB_OK) return st;
    const float *imgs[1] = {img01};
    st = e->rig->upload_f32(0, imgs, 1, stride_bytes, channels);
    if (st != MCORB_OK) return st;
    return finish_extract(e, lap_x0, lap_x1, kps, desc, cap, n_out, mono_index_out);
}

int mcorb_get_tables(const mcorb_params *p, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2,
                     int *features_per_level)
{
    if (!p) return MCORB_E_ARG;
    Tables t;
    const int st = compute_tables(*p, t);
    if (st != MCORB_OK) return st;
    for (int i = 0; i < t.nlevels; i++) {
        if (scale) scale[i] = t.scale[i];
        if (inv_scale) inv_scale[i] = t.inv_scale[i];
        if (sigma2) sigma2[i] = t.sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = t.inv_sigma2[i];
        if (features_per_level) features_per_level[i] = t.quota[i];
    }
    return MCORB_OK;
}

int mcorb_get_pyramid_level(mcorb_t *e, int level, uint8_t *dst, int dst_stride, int *w, int *h)
{
    if (!e || !e->rig) { set_error("no image processed yet"); return MCORB_E_STATE; }
    const Geom &g = e->rig->geom;
    if (level < 0 || level >= g.nlevels) return MCORB_E_ARG;
    if (w) *w = g.lv[level].w;
    if (h) *h = g.lv[level].h;
    if (!dst) return MCORB_OK;
    if (dst_stride < g.lv[level].w) return MCORB_E_ARG;
    Slot *s = e->rig->slots[0].get();
    HIPCHK(hipSetDevice(e->rig->device));
    HIPCHK(hipStreamSynchronize(s->st));
    HIPCHK(hipMemcpy2D(dst, dst_stride, s->d_pyr + g.lv[level].off, g.lv[level].pitch, g.lv[level].w, g.lv[level].h,
                       hipMemcpyDeviceToHost));
    return MCORB_OK;
}

// ORBextractor::DescriptorDistance (ORBextractor.cpp:1202-1218)
int mcorb_hamming256(const uint8_t a[32], const uint8_t b[32])
{
    uint64_t x[4], y[4];
    memcpy(x, a, 32);
    memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) +
           __builtin_popcountll(x[3] ^ y[3]);
}

// MultiCameraFrame::computeRepresentativeDesc (MultiCameraFrame.cpp:530-567): among n (<= 16) descriptors
// of one track, the one with the least median Hamming distance to the others; first minimum wins.
int mcorb_representative_desc(const uint8_t *descs, int n)
{
    if (!descs || n < 1 || n > 64) { set_error("representative_desc: bad argument"); return MCORB_E_ARG; }
    int best_median = 0x7fffffff, best_idx = 0;
    std::vector<int> row(n);
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < n; j++) row[j] = i == j ? 0 : mcorb_hamming256(descs + (size_t)i * 32, descs + (size_t)j * 32);
        std::sort(row.begin(), row.end());
        const int median = row[(size_t)(0.5 * (n - 1))];
        if (median < best_median) { best_median = median; best_idx = i; }
    }
    return best_idx;
}

static int knn2_host_arrays(mcorb_t *e, const uint8_t *q, int nq, const uint8_t *t, int nt, float thr, float ratio)
{
    if (!e || nq < 0 || nt < 0 || (nq && !q) || (nt && !t)) { set_error("knn2: bad argument"); return MCORB_E_ARG; }
    if (nq > 65535 || nt > 65535) { set_error("knn2: more than 65535 descriptors"); return MCORB_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || e->params.device_id >= ndev) {
        set_error("no usable HIP device (libmcorb has no CPU path)");
        return MCORB_E_NODEVICE;
    }
    HIPCHK(hipSetDevice(e->params.device_id));
    const int need = (std::max(std::max(nq, nt), 1) + 63) / 64 * 64;
    if (need > e->kc) {
        e->kc = 0;   // (each alloc releases what it held; a failure on the way leaves kc 0, and the next call allocates all again)
        TRY(e->d_desc.alloc((size_t)2 * need * 32));
        TRY(e->d_part.alloc(knn_part_entries(1, need)));
        TRY(e->d_exp.alloc((size_t)2 * need * kKnnExpandBytes));
        TRY(e->d_lcounts.alloc(2));
        TRY(e->h_rows.alloc((size_t)need, hipHostMallocMapped));
        TRY(e->h_mlist.alloc(knn_mlist_stride(need), hipHostMallocMapped));
        TRY(e->h_mcount.alloc((size_t)knn_qblocks(need), hipHostMallocMapped));
        TRY(e->h_counts.alloc(2, hipHostMallocMapped));
        TRY(e->h_pair.alloc(1, hipHostMallocMapped));
        e->kc = need;
    }
    if (nq) HIPCHK(hipMemcpy(e->d_desc, q, (size_t)nq * 32, hipMemcpyHostToDevice));
    if (nt) HIPCHK(hipMemcpy(e->d_desc + (size_t)e->kc * 32, t, (size_t)nt * 32, hipMemcpyHostToDevice));
    e->h_counts[0] = nq;
    e->h_counts[1] = nt;
    e->h_pair[0] = int2{0, 1};
    launch_knn2(nullptr, e->d_desc, e->h_counts, nullptr, 2, e->h_pair, 1, e->kc, e->d_exp, e->d_lcounts, e->d_part, thr, ratio, e->h_rows,
                e->h_mlist, e->h_mcount, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    return MCORB_OK;
}

int mcorb_knn2(mcorb_t *e, const uint8_t *q, int nq, const uint8_t *t, int nt, int32_t *idx, int32_t *dist)
{
    if (!idx || !dist) { set_error("null output"); return MCORB_E_ARG; }
    const int st = knn2_host_arrays(e, q, nq, t, nt, 75.f, 0.85f);
    if (st != MCORB_OK) return st;
    decode_rows(e->h_rows, nq, idx, dist);
    return MCORB_OK;
}

int mcorb_match_ratio(mcorb_t *e, const uint8_t *q, int nq, const uint8_t *t, int nt, float dist_thresh, float ratio,
                      uint32_t *idx1, uint32_t *idx2, int cap, int *n_out)
{
    const int st = knn2_host_arrays(e, q, nq, t, nt, dist_thresh, ratio);
    if (st != MCORB_OK) return st;
    int n = 0;
    for (int i = 0; i < nq; i++) {
        const KnnRow &r = e->h_rows[i];
        if (knn_accept(r)) {
            if (n < cap) { idx1[n] = (uint32_t)i; idx2[n] = (uint32_t)knn_idx0(r); }
            n++;
        }
    }
    if (n_out) *n_out = n;
    if (n > cap) { set_error("match buffer too small"); return MCORB_E_CAP; }
    return MCORB_OK;
}

int mcorb_host_select(const uint32_t *packed, int n, int minX, int maxX, int minY, int maxY, int nfeatures_level,
                      int wCell, int hCell, int32_t *out_idx, int cap)
{
    if (n < 0 || (n && !packed) || !out_idx) { set_error("host_select: bad argument"); return MCORB_E_ARG; }
    if (n == 0) return 0;
    const SelectParams P = make_select_params(minX, maxX, minY, maxY, nfeatures_level, wCell, hCell);
    if (P.nIni < 1) { set_error("host_select: level too tall"); return MCORB_E_SIZE; }
    static thread_local SelectScratch sc;
    std::vector<uint32_t> sorted;
    std::vector<int> perm, bstart;
    std::vector<mcorb::BucketBest> bbest;
    host_bucket_sort(packed, n, P, sorted, perm, bstart, bbest);   // what k_compact does on the device
    std::vector<int> out((size_t)std::max(nfeatures_level, 0) + 64 + 8);
    std::vector<uint32_t> outv(out.size());
    const int r = select_octree(sorted.data(), bstart.data(), bbest.data(), n, P, out.data(), outv.data(), sc);
    if (r == -4) { set_error("host_select: 2^20 candidates or a level 4096 px wide: beyond the packed (count, UL.x) sort key"); return MCORB_E_SIZE; }
    if (r < 0) { set_error("host_select: level too tall"); return MCORB_E_SIZE; }
    if (r > cap) { set_error("host_select: output too small"); return MCORB_E_CAP; }
    for (int i = 0; i < r; i++) {
        out_idx[i] = perm[out[i]];
        if (outv[i] != packed[out_idx[i]]) { set_error("host_select: value/index mismatch"); return MCORB_E_STATE; }
    }
    return r;
}

int mcorb_host_resize_axis(int ssize, int dsize, int is_x, int32_t *quads)
{
    if (ssize < 1 || dsize < 1 || !quads) return MCORB_E_ARG;
    std::vector<ResizeTap> t;
    build_resize_axis(ssize, dsize, is_x != 0, t, 1);
    for (int d = 0; d < dsize; d++) {
        quads[4 * d] = t[d].s0; quads[4 * d + 1] = t[d].s1; quads[4 * d + 2] = t[d].c0; quads[4 * d + 3] = t[d].c1;
    }
    return MCORB_OK;
}

int mcorb_host_geometry(const mcorb_params *p, int w, int h, int32_t *six)
{
    if (!p || !six) return MCORB_E_ARG;
    Tables t;
    int st = compute_tables(*p, t);
    if (st != MCORB_OK) return st;
    Geom g;
    std::vector<ResizeTap> taps;
    st = build_geometry(*p, t, w, h, g, taps);
    if (st != MCORB_OK) return st;
    for (int l = 0; l < g.nlevels; l++) {
        const LevelGeom &L = g.lv[l];
        int32_t *o = six + 6 * l;
        o[0] = L.w; o[1] = L.h; o[2] = L.nCols; o[3] = L.nRows; o[4] = L.wCell; o[5] = L.hCell;
    }
    return MCORB_OK;
}

}  // extern "C"
