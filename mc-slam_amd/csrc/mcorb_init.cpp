// mcorb_init.cpp -- the first map from two rig frames: mcorb_lmap_initialize, FrontEnd::initialization from the baseline gate to
// the inserted landmarks (MCSlam/src/FrontEnd.cpp:2633-2839).  The arithmetic is mcorb_init.h.  A device store runs
// k_init_triangulate, k_init_select and k_init_put (mcorb_init_gpu.hip) in one submission on the store's stream with one wait:
// the records of all matches and the call's record land in host-mapped memory, the accepted points, normals and ray counts go
// into their slots on the device.  A host-only store runs init_run_serial, so the two agree bit for bit.  What is left to the
// host in both: the refusals, the two lIds arrays (a walk in match order) and the slots' host-side flags.  Not restated: the
// arms in front of :2633, insertKeyFrame, the observation lists (mcorb_lmap_observe) and the 4x4 inverses.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

void call_out(const InitCall &c, int n, mcorb_init_result *out)
{
    out->status = c.status;
    out->parallax = c.parallax;
    out->median_scene_depth = c.depth;
    memcpy(out->t_out, c.t_out, sizeof(c.t_out));
    out->n_matches = n;
    out->n_initial_inliers = c.n_initial;
    out->n_parallax = c.n_parallax;
    out->n_triangulated = c.n_triangulated;
    out->scaled = c.scaled;
    out->next_lid = c.next_lid;
}

// what both hooks refuse: their own arguments, then check_cases
int check_init_cases(MapCases &c, int nlevels, int n, int ncams, const double *R, const double *t, const uint8_t *inliers,
                     const int32_t *verdict, const int32_t *n_rays, const int32_t *lid_offset, const double *vals,
                     const mcorb_init_result *res, std::vector<int32_t> &voff)
{
    if (n > MCORB_INIT_MAX_MATCHES || ncams < 1 || ncams > MCORB_MAX_CAMS || !R || !t || !inliers || !verdict || !n_rays || !lid_offset ||
        !vals || !res) {
        set_error("init cases: bad argument");
        return MCORB_E_ARG;
    }
    return check_cases("init cases", c, nlevels, n, voff);
}

// the chain of both device entries on st with its wait, behind what the caller has queued on sub: `records` (k_init_triangulate, or the cases' k_init_gates), k_init_select
// and k_init_put on the records p.rec of n matches, the events of `kernels` around them
template <class Records>
int submit(Submission &sub, hipStream_t st, Spans<3> &kernels, Records records, const InitPutArgs &p, int n, uint64_t *keys, int32_t *offset, InitSel *sel,
           bool from_cases)
{
    typedef mcorb_lmap::Init I;
    sub.run(kernels, I::kTriangulate, records);
    sub.run(kernels, I::kSelect, [&] { launch_init_select(st, p.rec, p.flags, n, keys, offset, sel); });
    sub.run(kernels, I::kPut, [&] { launch_init_put(st, p, from_cases); });
    sub.mark(kernels, I::kPut + 1);
    return sub.wait();
}

void job_init(InitJob &job, const double *R, const double *t, int n, int ncams, int32_t next_lid, const uint8_t *flags)
{
    memset(&job, 0, sizeof(job));
    memcpy(job.R, R, sizeof(job.R));
    memcpy(job.t, t, sizeof(job.t));
    job.n = n;
    job.ncams = ncams;
    job.next_lid = next_lid;
    for (int i = 0; i < n; i++) job.n_initial += flags[i] ? 1 : 0;
}

void baseline_out(const double *t, int n, int32_t next_lid, mcorb_init_result *res)
{
    res->status = kInitBaseline;
    res->n_matches = n;
    memcpy(res->t_out, t, 3 * sizeof(double));
    res->next_lid = next_lid;
}

void cases_out(const MapOut *recs, const InitCall &call, int n, uint8_t *inliers, int32_t *verdict, int32_t *n_rays, int32_t *lid_offset,
               double *vals, mcorb_init_result *res)
{
    int32_t id = 0;
    for (int i = 0; i < n; i++) {
        const MapOut &o = recs[i];
        const bool stored = call.status == kInitDone && o.verdict == kMapLandmark;
        inliers[i] = o.verdict == kMapLandmark;
        verdict[i] = o.verdict;
        n_rays[i] = o.n_rays;
        lid_offset[i] = stored ? id++ : -1;
        double *v = vals + 8 * (size_t)i;
        for (int k = 0; k < 3; k++) { v[k] = o.X[k]; v[3 + k] = o.normal[k]; }
        v[6] = o.dist2; v[7] = o.cos;
    }
    call_out(call, n, res);
}

}  // namespace

extern "C" {

int mcorb_lmap_initialize(mcorb_lmap *m, const mcorb_map_frame *prev, int32_t *lids_prev, const mcorb_map_frame *cur, int32_t *lids_cur,
                          const double R[9], const double t[3], const double *cam_centre_body, const int32_t *match_query,
                          const int32_t *match_train, int n, const double *K, const float *inv_sigma2, int nlevels, int32_t next_lid,
                          double min_baseline, mcorb_init_result *out)
{
    const char *const who = "lmap initialize";
    TRY(check_lmap(m, who));
    MapCall mc{who, m->max_landmarks, cur ? cur->ncams : 0, nlevels};
    if (!prev || !cur || !out || !R || !t || !cam_centre_body || n < 0 || !K || !inv_sigma2 || nlevels < 1 || next_lid < 0 ||
        out->cap_matches < 0 || (cur->nfeat && !lids_cur) || (prev->nfeat && !lids_prev) || (n && (!match_query || !match_train)))
        return mc.bad("bad argument");
    const int C = mc.C;
    if (C < 1 || C > MCORB_MAX_CAMS) return mc.bad("1 .. MCORB_MAX_CAMS cameras");
    if (n > MCORB_INIT_MAX_MATCHES) return mc.bad("more than MCORB_INIT_MAX_MATCHES matches");
    std::lock_guard<std::mutex> lk(m->mu);

    // ---- 1. everything that can be refused is refused before anything runs ----
    TRY(mc.check_frame(*cur));
    TRY(mc.check_lids(*cur, lids_cur));
    TRY(mc.check_frame(*prev));
    TRY(mc.check_lids(*prev, lids_prev));
    mc.add(*cur);
    mc.add(*prev);
    std::vector<uint8_t> nviews((size_t)n, 0);
    for (int j = 0; j < n; j++) {
        uint8_t nv_cur;
        TRY(mc.count_views(*prev, match_query[j], match_train[j], nviews[j], nv_cur));
    }
    out->n_matches = n;
    if (n > out->cap_matches) return mc.fail(MCORB_E_CAP, "output too small");
    if (n && (!out->inliers || !out->verdict || !out->new_lid || !out->pt3d || !out->normal || !out->dist2 || !out->cos_parallax))
        return mc.bad("bad argument");
    InitJob job;
    job_init(job, R, t, n, C, next_lid, out->inliers);
    if ((size_t)next_lid + (size_t)job.n_initial > (size_t)m->max_landmarks) return mc.fail(MCORB_E_CAP, "new landmark ids beyond max_landmarks");

    // ---- 2. the baseline gate (:2633) ----
    if (!init_baseline(t, min_baseline)) {
        baseline_out(t, n, next_lid, out);
        return MCORB_OK;
    }

    // ---- 3. the matches that need a record: the flag is set on entry; a record lies at its match's index ----
    const bool dev = m->device >= 0;
    std::vector<uint8_t> flags(out->inliers, out->inliers + n);
    for (uint8_t &f : flags) f = f ? 1 : 0;
    MapWork &w = mc.w;
    w.item_of.assign((size_t)n, -1);
    const size_t moff[2] = {0, (size_t)n};
    if (dev) {
        w.order(1, &match_query, &match_train, &n, moff, nviews.data(), [&](int, int j) { return flags[j] != 0; });
        for (int j = 0; j < n; j++)
            if (w.item_of[j] >= 0) w.items[w.item_of[j]].rec = j;
    }

    // ---- 4. the packed input: the current frame (its centres: cam_centre_body), then prev; the flags and the matches ----
    TRY(mc.fits());
    const InitLayout L((size_t)C, (size_t)nlevels, mc.nmi, mc.nkp, w.blocks.size(), w.items.size(), (size_t)n);
    mcorb_lmap::Init &b = m->init;
    std::vector<uint8_t> host_block;
    uint8_t *base;
    if (dev) {
        HIPCHK(hipSetDevice(m->device));
        (void)hipGetLastError();   // (a stale error of this thread is not this call's)
        TRY(b.reserve(L.m.p.total, (size_t)std::max(n, 1)));
        base = b.in.h;
    } else {
        host_block.resize(L.m.p.total);
        base = host_block.data();
    }
    mc.pack(base, L.m, K, inv_sigma2);
    mc.pack_init(base, L, cam_centre_body, flags.data(), match_query, match_train, (size_t)n);

    // ---- 5. the records, the medians, the verdict and the landmarks ----
    std::vector<MapOut> host_recs;
    const MapOut *recs;
    InitCall call;
    if (dev) {
        hipStream_t st = m->st;
        InitPutArgs p;
        memset(&p, 0, sizeof(p));
        p.job = job;
        p.a = L.m.args(b.in.d, b.d_rec, C);
        p.query = b.in.dev<const int32_t>(L.query);
        p.train = b.in.dev<const int32_t>(L.train);
        p.rec = b.d_rec;
        p.flags = b.in.dev<const uint8_t>(L.flags);
        p.offset = b.d_offset;
        p.sel = b.d_sel;
        p.h_rec = b.h_rec;
        p.h_call = b.h_call;
        p.geom = m->d_geom;
        p.nrays = m->d_nrays;
        // (nothing returns between the first launch and the wait, so no kernel of this call still writes the store or the
        // host-mapped records when the caller has its error: Submission)
        const auto triangulate = [&] { launch_init_triangulate(st, p.a, w.nblocks_small, (int)w.blocks.size() - w.nblocks_small); };
        Submission sub(st);
        b.in.upload(sub, L.m.p.total);
        TRY(submit(sub, st, b.kernels, triangulate, p, n, b.d_keys, b.d_offset, b.d_sel, false));
        b.kernels.read();
        b.last_launched = (int)w.items.size();
        call = *b.h_call.get();
        recs = b.h_rec.get();
    } else {
        host_recs.resize((size_t)n);
        const MapArgs a = L.m.args(base, nullptr, C);
        init_run_serial(job, a, match_query, match_train, flags.data(), host_recs.data(), call, m->geom.data(), m->n_rays.data());
        recs = host_recs.data();
    }

    // ---- 6. the caller's arrays; with DONE the ids in match order (:2807-2832) ----
    int32_t id = next_lid;
    for (int i = 0; i < n; i++) {
        const MapOut &o = recs[i];
        const bool stored = call.status == kInitDone && o.verdict == kMapLandmark;
        out->inliers[i] = o.verdict == kMapLandmark;
        out->verdict[i] = (uint8_t)o.verdict;
        out->new_lid[i] = -1;
        out->dist2[i] = o.dist2;
        out->cos_parallax[i] = o.cos;
        for (int k = 0; k < 3; k++) { out->pt3d[3 * (size_t)i + k] = o.X[k]; out->normal[3 * (size_t)i + k] = o.normal[k]; }
        if (!stored) continue;
        out->new_lid[i] = id;
        lids_prev[match_query[i]] = lids_cur[match_train[i]] = id;
        m->flags[id] |= kSet;
        m->n_rays[id] = o.n_rays;
        id++;
    }
    call_out(call, n, out);
    return MCORB_OK;
}

int mcorb_lmap_last_initialize_timing(mcorb_lmap *m, float us[3], int *n_launched)
{
    TRY(check_lmap_handle(m, "lmap last_initialize_timing"));
    if (!us) { set_error("lmap last_initialize_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    for (int k = 0; k < 3; k++) us[k] = m->init.kernels.us[k];
    if (n_launched) *n_launched = m->init.last_launched;
    return MCORB_OK;
}

int mcorb_host_init_cases(int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P, const double *K,
                          const double *centre, const float *kps, const int32_t *octave, const float *inv_sigma2, int nlevels,
                          int ncams, const double R[9], const double t[3], double min_baseline, uint8_t *inliers, int32_t *verdict,
                          int32_t *n_rays, int32_t *lid_offset, double *vals, mcorb_init_result *res)
{
    MapCases c{X, nv1, nv, nullptr, P, K, centre, kps, octave, inv_sigma2};
    std::vector<int32_t> voff;
    TRY(check_init_cases(c, nlevels, n, ncams, R, t, inliers, verdict, n_rays, lid_offset, vals, res, voff));
    if (!init_baseline(t, min_baseline)) { baseline_out(t, n, 0, res); return MCORB_OK; }
    InitJob job;
    job_init(job, R, t, n, ncams, 0, inliers);
    std::vector<MapOut> recs((size_t)n);
    std::vector<uint8_t> flags((size_t)n);
    for (int i = 0; i < n; i++) {
        flags[i] = inliers[i] ? 1 : 0;
        map_clear(recs[i]);
        if (flags[i]) init_gate_case(c, i, recs[i]);
    }
    std::vector<double> geom((size_t)n * 6);
    std::vector<int32_t> rays((size_t)n);
    InitCall call;
    init_finish_serial(job, flags.data(), recs.data(), [&](int i, MapViews &v) { map_case_views(c, i, v); }, call, geom.data(), rays.data());
    cases_out(recs.data(), call, n, inliers, verdict, n_rays, lid_offset, vals, res);
    return MCORB_OK;
}

int mcorb_dev_init_cases_selftest(int device, int n, const double *X, const int32_t *nv1, const int32_t *nv, const double *P,
                                  const double *K, const double *centre, const float *kps, const int32_t *octave,
                                  const float *inv_sigma2, int nlevels, int ncams, const double R[9], const double t[3],
                                  double min_baseline, uint8_t *inliers, int32_t *verdict, int32_t *n_rays, int32_t *lid_offset,
                                  double *vals, mcorb_init_result *res)
{
    MapCases c{X, nv1, nv, nullptr, P, K, centre, kps, octave, inv_sigma2};
    std::vector<int32_t> voff;
    TRY(check_init_cases(c, nlevels, n, ncams, R, t, inliers, verdict, n_rays, lid_offset, vals, res, voff));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { set_error("no usable HIP device"); return MCORB_E_NODEVICE; }
    if (!init_baseline(t, min_baseline)) { baseline_out(t, n, 0, res); return MCORB_OK; }
    HIPCHK(hipSetDevice(device));
    InitJob job;
    job_init(job, R, t, n, ncams, 0, inliers);
    const size_t N = (size_t)n;
    std::vector<uint8_t> flags(N);
    for (int i = 0; i < n; i++) flags[i] = inliers[i] ? 1 : 0;
    CasesDev d;
    DevBuf<double> d_geom;
    DevBuf<int32_t> d_offset, d_nrays;
    DevBuf<uint8_t> d_flags;
    DevBuf<MapOut> d_rec;
    DevBuf<uint64_t> d_keys;
    DevBuf<InitSel> d_sel;
    HostBuf<MapOut> h_rec;
    HostBuf<InitCall> h_call;
    TRY(d.upload(n, c, nlevels));
    TRY(to_device(d_flags, flags.data(), N));
    TRY(d_rec.alloc(N));
    TRY(d_keys.alloc(2 * N));
    TRY(d_offset.alloc(N));
    TRY(d_sel.alloc(1));
    TRY(d_geom.alloc(N * 6));
    TRY(d_nrays.alloc(N));
    TRY(h_rec.alloc(N, kHostMapped));
    TRY(h_call.alloc(1, kHostMapped));
    // (a case whose flag is clear gets a record too: k_init_select and k_init_put read the flag first)
    InitPutArgs p;
    memset(&p, 0, sizeof(p));
    p.job = job;
    p.cases = d.cases();
    p.rec = d_rec;
    p.flags = d_flags;
    p.offset = d_offset;
    p.sel = d_sel;
    p.h_rec = h_rec;
    p.h_call = h_call;
    p.geom = d_geom;
    p.nrays = d_nrays;
    Spans<3> kernels;
    TRY(kernels.create());
    Submission sub(nullptr);
    TRY(submit(sub, nullptr, kernels, [&] { launch_init_gates(nullptr, p.cases, n, d_rec); }, p, n, d_keys, d_offset, d_sel, true));
    cases_out(h_rec.get(), *h_call.get(), n, inliers, verdict, n_rays, lid_offset, vals, res);
    return MCORB_OK;
}

}  // extern "C"
