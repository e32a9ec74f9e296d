// mcorb_lmap.cpp -- the local map: FrontEnd::searchLocalMap2 (MCSlam/src/FrontEnd.cpp:4901-5223) from the landmarks of the
// neighbouring keyframes to the camera-filtered matches (:4953-5171), the consumer of the probe slot that holds the current frame
// (mcorb_kfdb.cpp).  Not restated: the fbow block (:5062-5095), OptimizePose (:5198) and the 4x4 inverses, which are the caller's.
//
// A landmark's slot is its lId.  Two stores, as the keyframe database has two:
//   device >= 0   points and normals (6 doubles per slot) and descriptors in HBM; the frustum test is k_lmap_cull, the accepted
//                 rows are gathered (k_kfdb_gather) and descended (k_bow_descend), the best / second-best search is k_kfdb_best2
//                 with the gathered rows as A and the probe's rows in the database's descriptor store as B, followed by the
//                 database's accept() per shared node (Best2Search, the database's own path);
//   device == -1  host only, written the way the reference is: a small cv::Mat-like product per landmark and camera, the host
//                 descent of a host-only vocabulary, and the literal getMatches_distRatio loop (matches_host).
// The candidate walk, the compaction of the accepted landmarks (in candidate order), the FeatureVector's assembly, the shared-node
// walk and the camera filter run on the host in both.  The flags of a slot (has a point, a normal, a descriptor; mono) are
// host state in both: the filter and the state checks read them, no kernel does.
//
// cv::Mat's arithmetic is un-vendored (the eighth unpinned third-party piece): the restated order is that of its small
// matrix product -- per output element the sum over k ascending, from 0.0, of separately rounded products, then the addend --
// of Mat::dot and cv::norm over three elements in order, and of MatExpr's `/ scalar`, a multiplication by the reciprocal.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

// what set and set_desc_from_entry share: ids inside the store, and of an id that occurs twice only the last entry kept (keep[i])
static int check_set_ids(mcorb_lmap *m, const int32_t *lids, int n, const char *who, std::vector<int> &keep)
{
    for (int i = 0; i < n; i++)
        if (lids[i] < 0 || lids[i] >= m->max_landmarks) { set_error(std::string(who) + ": landmark id outside the store"); return MCORB_E_ARG; }
    keep.assign(lids, lids + n);
    const int t = next_tick(m);
    for (int i = n - 1; i >= 0; i--) {
        if (m->stamp[lids[i]] == t) keep[i] = -1;
        m->stamp[lids[i]] = t;
    }
    return MCORB_OK;
}

// a batch into the device store: keep (the slots), the host arrays that are given, or rows `rows` of src_desc (device memory)
static int put_device(mcorb_lmap *m, const std::vector<int> &keep, const double *pt3d, const double *normal, const uint8_t *desc,
                      const uint8_t *src_desc, const int32_t *rows)
{
    const size_t n = keep.size();
    TRY(use_device(m->device));
    hipStream_t st = m->st;
    mcorb_lmap::Batch &b = m->batch;
    TRY(b.reserve(n, pt3d, normal, desc, rows));
    Submission sub(st);   // (its wait also covers the pageable host arrays; an absent array is a copy of 0 bytes)
    b.upload(sub, b.d_lids, keep.data(), n);
    b.upload(sub, b.d_pt, pt3d, pt3d ? n * 3 : 0);
    b.upload(sub, b.d_normal, normal, normal ? n * 3 : 0);
    b.upload(sub, b.d_desc, desc, desc ? n * 32 : 0);
    b.upload(sub, b.d_rows, rows, rows ? n : 0);
    sub.run([&] {
        launch_lmap_put(st, b.d_lids, (int)n, pt3d ? b.d_pt.get() : nullptr, normal ? b.d_normal.get() : nullptr, desc ? b.d_desc.get() : src_desc,
                        rows ? b.d_rows.get() : nullptr, m->d_geom, m->d_desc);
    });
    return sub.wait();
}

// the frustum test of one landmark on the host (:5000-5027), with 3x3 * 3x1 products as cv::Mat's gemm evaluates them
static void mat_mul_add(const double A[9], const double b[3], const double *c, double out[3])
{
    for (int r = 0; r < 3; r++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s += A[3 * r + k] * b[k];
        out[r] = c ? s + c[r] : s;
    }
}

static uint32_t cull_host(const mcorb_lmap_view &v, const double *pt3D, const double *normal)
{
    double pt3d_body[3];
    mat_mul_add(v.Rcw, pt3D, v.tcw, pt3d_body);
    uint32_t cmids = 0;
    for (int camID = 0; camID < v.ncams; camID++) {
        const mcorb_lmap_cam &cam = v.cams[camID];
        double pt3d_c[3];
        mat_mul_add(cam.R, pt3d_body, cam.t, pt3d_c);
        const double z = pt3d_c[2];
        if (z < 0) continue;
        double curDir[3];
        for (int k = 0; k < 3; k++) curDir[k] = pt3D[k] - cam.centre_w[k];
        double dot = 0.0, norm2 = 0.0;
        for (int k = 0; k < 3; k++) dot += normal[k] * curDir[k];
        for (int k = 0; k < 3; k++) norm2 += curDir[k] * curDir[k];
        if (dot < 0.5 * sqrt(norm2)) continue;
        double tmp[3];
        mat_mul_add(cam.K, pt3d_c, nullptr, tmp);
        const double scale = 1.0 / tmp[2];   // tmp / tmp.at<double>(2, 0): MatExpr multiplies by the reciprocal
        for (int k = 0; k < 3; k++) tmp[k] = tmp[k] * scale;
        if (tmp[0] < 30 || tmp[0] > (v.width - 30)) continue;
        if (tmp[1] < 30 || tmp[1] > (v.height - 30)) continue;
        cmids |= 1u << camID;
    }
    return cmids;
}

extern "C" {

int mcorb_lmap_create(mcorb_vocab *v, int device, int max_landmarks, int max_candidates, mcorb_lmap **out)
{
    if (out) *out = nullptr;
    if (!v || !out || device < -1 || max_landmarks < 1 || max_candidates < 1) { set_error("lmap create: bad argument"); return MCORB_E_ARG; }
    int scoring = 0, vdev = 0;
    vocab_props(v, scoring, vdev);
    if (vdev != device) { set_error("lmap create: the vocabulary lives on another device (a host-only store needs a host-only vocabulary)"); return MCORB_E_ARG; }
    std::unique_ptr<mcorb_lmap> m(new mcorb_lmap);
    m->device = device; m->max_landmarks = max_landmarks; m->max_candidates = max_candidates; m->voc = v;
    m->flags.assign((size_t)max_landmarks, 0);
    m->stamp.assign((size_t)max_landmarks, 0);
    m->n_rays.assign((size_t)max_landmarks, 0);
    m->obs.resize((size_t)max_landmarks);
    m->life.occ.assign((size_t)max_landmarks, 0);
    if (device < 0) {
        m->geom.assign((size_t)max_landmarks * 6, 0.0);
        m->desc.assign((size_t)max_landmarks * 32, 0);
    } else {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { set_error("lmap create: no such HIP device"); return MCORB_E_NODEVICE; }
        HIPCHK(hipSetDevice(device));
        const size_t N = (size_t)max_landmarks, C = (size_t)max_candidates;
        TRY(m->st.create(hipStreamNonBlocking));
        TRY(m->search.create(C));
        TRY(m->map.neigh.create());
        TRY(m->map.refine_new.create());
        TRY(m->life.observe.create());
        TRY(m->life.update.create());
        TRY(m->track.chain.create());
        TRY(m->pose.refine.create());
        TRY(m->ba.chain.create());
        TRY(m->retri.chain.create());
        TRY(m->sac.kernels.create());
        TRY(m->rel.kernels.create());
        TRY(m->rel.fit.create());
        TRY(m->ess.kernels.create());
        TRY(m->ess.fit.create());
        TRY(m->align.sac.create());
        TRY(m->align.fit.create());
        TRY(m->init.kernels.create());
        TRY(m->d_geom.alloc(N * 6));
        TRY(m->d_desc.alloc(N * 32));
        HIPCHK(hipMemset(m->d_geom, 0, N * 6 * sizeof(double)));
        HIPCHK(hipMemset(m->d_desc, 0, N * 32));
        TRY(m->d_nrays.alloc(N));
        HIPCHK(hipMemset(m->d_nrays, 0, N * sizeof(int32_t)));
        // the fills run on the null stream and the store's stream is non-blocking, i.e. NOT ordered against it: without this a fill
        // that is still queued can zero what the first set() after the create has just put (seen once in a whole run of the GPU
        // suite as a neighbour skipped for its depths on a store created, filled and used at once: test_gpu_mapping.py, 1 match)
        HIPCHK(hipStreamSynchronize(nullptr));
    }
    *out = m.release();
    return MCORB_OK;
}

void mcorb_lmap_destroy(mcorb_lmap *m)
{
    if (!m) return;
    if (m->device >= 0 && hipSetDevice(m->device) == hipSuccess && m->st.get()) (void)hipStreamSynchronize(m->st);
    delete m;
}

int mcorb_lmap_set(mcorb_lmap *m, const int32_t *lids, int n, const double *pt3d, const double *normal, const uint8_t *desc,
                   const uint8_t *mono)
{
    TRY(check_lmap(m, "lmap set"));
    if (n < 0 || (n && !lids)) { set_error("lmap set: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    std::vector<int> keep;
    TRY(check_set_ids(m, lids, n, "lmap set", keep));
    const uint8_t given = (pt3d ? kHasPt : 0) | (normal ? kHasNormal : 0);
    for (int i = 0; i < n; i++)
        if (((m->flags[lids[i]] | given) & kSet) != kSet) {
            set_error("lmap set: a slot that was never set needs a point and a normal");
            return MCORB_E_STATE;
        }
    if (n == 0) return MCORB_OK;
    if (m->device < 0) {
        for (int i = 0; i < n; i++) {
            const size_t s = (size_t)lids[i];
            if (pt3d) memcpy(&m->geom[s * 6], pt3d + 3 * (size_t)i, 3 * sizeof(double));
            if (normal) memcpy(&m->geom[s * 6 + 3], normal + 3 * (size_t)i, 3 * sizeof(double));
            if (desc) memcpy(&m->desc[s * 32], desc + 32 * (size_t)i, 32);
        }
    } else if (pt3d || normal || desc) {
        TRY(put_device(m, keep, pt3d, normal, desc, nullptr, nullptr));
    }
    for (int i = 0; i < n; i++) {
        uint8_t &f = m->flags[lids[i]];
        f |= given | (desc ? kHasDesc : 0);
        if (mono) f = (uint8_t)((f & ~kMono) | (mono[i] ? kMono : 0));
    }
    return MCORB_OK;
}

int mcorb_lmap_set_desc_from_entry(mcorb_lmap *m, mcorb_kfdb *db, int entry, const int32_t *lids, const int32_t *feats, int n,
                                   const uint8_t *mono)
{
    TRY(check_lmap(m, "lmap set_desc_from_entry"));
    if (!db || n < 0 || (n && (!lids || !feats))) { set_error("lmap set_desc_from_entry: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    std::lock_guard<std::mutex> lkdb(db->mu);
    if (db->device != m->device) { set_error("lmap set_desc_from_entry: the database lives on another device"); return MCORB_E_ARG; }
    if (entry < 0 || entry >= db->n) { set_error("lmap set_desc_from_entry: no such entry"); return MCORB_E_ARG; }
    const int ndesc = m->device < 0 ? (int)(db->entries[entry].desc.size() / 32) : db->mirror[entry].ndesc;
    for (int i = 0; i < n; i++)
        if (feats[i] < 0 || feats[i] >= ndesc) { set_error("lmap set_desc_from_entry: feature index outside the entry"); return MCORB_E_ARG; }
    std::vector<int> keep;
    TRY(check_set_ids(m, lids, n, "lmap set_desc_from_entry", keep));
    if (n == 0) return MCORB_OK;
    if (m->device < 0) {
        const uint8_t *src = db->entries[entry].desc.data();
        for (int i = 0; i < n; i++) memcpy(&m->desc[(size_t)lids[i] * 32], src + (size_t)feats[i] * 32, 32);
    } else {
        TRY(put_device(m, keep, nullptr, nullptr, nullptr, place_of(db, entry, false).desc, feats));
    }
    for (int i = 0; i < n; i++) {
        uint8_t &f = m->flags[lids[i]];
        f |= kHasDesc;
        if (mono) f = (uint8_t)((f & ~kMono) | (mono[i] ? kMono : 0));
    }
    return MCORB_OK;
}

int mcorb_lmap_get(mcorb_lmap *m, int lid, double pt3d[3], double normal[3], uint8_t desc[32], int *mono, int *has_desc)
{
    TRY(check_lmap(m, "lmap get"));
    std::lock_guard<std::mutex> lk(m->mu);
    if (lid < 0 || lid >= m->max_landmarks) { set_error("lmap get: landmark id outside the store"); return MCORB_E_ARG; }
    const uint8_t f = m->flags[lid];
    if ((f & kSet) != kSet) { set_error("lmap get: the slot was never set"); return MCORB_E_STATE; }
    if (mono) *mono = (f & kMono) ? 1 : 0;
    if (has_desc) *has_desc = (f & kHasDesc) ? 1 : 0;
    const bool want_desc = desc && (f & kHasDesc);
    if (m->device < 0) {
        if (pt3d) memcpy(pt3d, &m->geom[(size_t)lid * 6], 3 * sizeof(double));
        if (normal) memcpy(normal, &m->geom[(size_t)lid * 6 + 3], 3 * sizeof(double));
        if (want_desc) memcpy(desc, &m->desc[(size_t)lid * 32], 32);
        return MCORB_OK;
    }
    HIPCHK(hipSetDevice(m->device));
    if (pt3d) HIPCHK(hipMemcpy(pt3d, m->d_geom + (size_t)lid * 6, 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (normal) HIPCHK(hipMemcpy(normal, m->d_geom + (size_t)lid * 6 + 3, 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (want_desc) HIPCHK(hipMemcpy(desc, m->d_desc + (size_t)lid * 32, 32, hipMemcpyDeviceToHost));
    return MCORB_OK;
}

int mcorb_lmap_search(mcorb_lmap *m, const mcorb_lmap_view *view, const int32_t *neighbour_lids, int n_lids,
                      const int32_t *matched_lids, int n_matched, mcorb_kfdb *db, int probe, const uint8_t *matched_cur,
                      const uint8_t *mono_cur, const int32_t *cam_cur, int levelsup, double max_neighbor_ratio, int32_t *new_lids,
                      uint32_t *cam_masks, int cap_new, int *n_new, uint32_t *ind1, uint32_t *ind2, int cap_ind, int *n_ind,
                      int32_t *match_query, int32_t *match_train, int cap_matches, int *n_matches)
{
    if (n_new) *n_new = 0;
    if (n_ind) *n_ind = 0;
    if (n_matches) *n_matches = 0;
    TRY(check_lmap(m, "lmap search"));
    if (!view || !db || n_lids < 0 || n_matched < 0 || (n_lids && !neighbour_lids) || (n_matched && !matched_lids) || cap_new < 0 ||
        cap_ind < 0 || cap_matches < 0 || (cap_new && (!new_lids || !cam_masks)) || (cap_ind && (!ind1 || !ind2)) ||
        (cap_matches && (!match_query || !match_train))) {
        set_error("lmap search: bad argument");
        return MCORB_E_ARG;
    }
    if (view->ncams < 1 || view->ncams > MCORB_MAX_CAMS) { set_error("lmap search: 1 .. MCORB_MAX_CAMS cameras"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    std::lock_guard<std::mutex> lkdb(db->mu);
    if (db->device != m->device) { set_error("lmap search: the database lives on another device"); return MCORB_E_ARG; }
    TRY(check_probe(db, probe, "lmap search"));
    const int nb = m->device < 0 ? (int)(db->probes[probe].desc.size() / 32) : db->pmirror[probe].ndesc;
    if (nb && (!matched_cur || !mono_cur || !cam_cur)) { set_error("lmap search: bad argument"); return MCORB_E_ARG; }
    for (int i = 0; i < n_lids; i++)
        if (neighbour_lids[i] < -1 || neighbour_lids[i] >= m->max_landmarks) { set_error("lmap search: landmark id outside the store"); return MCORB_E_ARG; }
    for (int i = 0; i < n_matched; i++)
        if (matched_lids[i] < 0 || matched_lids[i] >= m->max_landmarks) { set_error("lmap search: landmark id outside the store"); return MCORB_E_ARG; }

    // 1. the candidates (:4990-4998): lmSet and matchedlmset are one stamp per slot
    const int t = next_tick(m);
    for (int i = 0; i < n_matched; i++) m->stamp[matched_lids[i]] = t;
    std::vector<int> cand;
    for (int i = 0; i < n_lids; i++) {
        const int l = neighbour_lids[i];
        if (l == -1 || m->stamp[l] == t) continue;
        m->stamp[l] = t;
        cand.push_back(l);
    }
    const int nc = (int)cand.size();
    if (nc > m->max_candidates) { set_error("lmap search: more candidates than max_candidates"); return MCORB_E_CAP; }
    for (int l : cand)
        if ((m->flags[l] & kSet) != kSet) { set_error("lmap search: a candidate landmark was never set"); return MCORB_E_STATE; }
    m->search.last_candidates = nc;

    // 2. the frustum test (:5000-5027) and the accepted landmarks in candidate order
    std::vector<int> acc;          // slots
    std::vector<uint32_t> masks;   // lm_projected_cam_ids
    hipStream_t st = m->st;
    if (m->device < 0) {
        for (int l : cand) {
            const uint32_t cmids = cull_host(*view, &m->geom[(size_t)l * 6], &m->geom[(size_t)l * 6 + 3]);
            if (cmids) { acc.push_back(l); masks.push_back(cmids); }
        }
    } else if (nc) {
        TRY(use_device(m->device));
        Submission sub(st);   // (its wait also covers the pageable view and candidate list)
        sub.copy(m->search.d_view, view, sizeof(mcorb_lmap_view), hipMemcpyHostToDevice);
        sub.copy(m->search.d_cand, cand.data(), (size_t)nc * sizeof(int), hipMemcpyHostToDevice);
        sub.run(m->search.cull, 0, [&] { launch_lmap_cull(st, m->search.d_view, m->d_geom, m->search.d_cand, nc, m->search.d_masks); });
        sub.mark(m->search.cull, 1);
        sub.copy(m->search.h_masks, m->search.d_masks, (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToHost);
        TRY(sub.wait());
        m->search.cull.read();
        for (int i = 0; i < nc; i++)
            if (m->search.h_masks[i]) { acc.push_back(cand[i]); masks.push_back(m->search.h_masks[i]); }
    }
    const int na = (int)acc.size();
    for (int l : acc)
        if (!(m->flags[l] & kHasDesc)) { set_error("lmap search: an accepted landmark has no descriptor yet"); return MCORB_E_STATE; }

    // 3. transform(newlm_vecDescs, levelsup) (:5106) and 4. InterMatchingBow (:5111)
    std::vector<uint32_t> i1, i2;
    BowImageOut fv;
    if (m->device < 0) {
        HostEntry A;
        A.desc.resize((size_t)na * 32);
        for (int i = 0; i < na; i++) memcpy(&A.desc[(size_t)i * 32], &m->desc[(size_t)acc[i] * 32], 32);
        TRY(vocab_feature_vector(m->voc, A.desc.data(), na, levelsup, nullptr, fv));
        A.nodes = fv.fv_nodes; A.offs = fv.fv_offsets; A.feats = fv.fv_feats;
        matches_host(A, db->probes[probe], max_neighbor_ratio, i1, i2);
    } else if (na) {
        TRY(vocab_feature_vector(m->voc, m->search.d_adesc, na, levelsup, st, fv, [&](Submission &sub) {
            sub.copy(m->search.d_cand, acc.data(), (size_t)na * sizeof(int), hipMemcpyHostToDevice);
            sub.run([&] { launch_kfdb_gather(st, m->d_desc, m->search.d_cand, na, m->search.d_adesc); });
        }));
        // A: the gathered rows and their FeatureVector; B: the probe, with its own base as set 0
        const Place pb = place_of(db, probe, true);
        std::vector<std::vector<uint32_t>> r1, r2;
        m->search.best2.reset();
        m->search.best2.add_b(fv.fv_nodes, fv.fv_offsets, db->pmirror[probe], 0);
        const Pieces afeats = [&](Submission &sub) {   // (none without items; the run's wait covers the pageable list)
            sub.copy(m->search.d_afeats, fv.fv_feats.data(), fv.fv_feats.size() * sizeof(int), hipMemcpyHostToDevice);
        };
        TRY(m->search.best2.run(st, m->search.d_adesc, m->search.d_afeats, pb.desc, 0, pb.feats, 0, max_neighbor_ratio, r1, r2, &m->search.us_best2, afeats));
        i1.swap(r1[0]); i2.swap(r2[0]);
    }

    // 5. the filter by viewing camera (:5122-5171)
    std::vector<int32_t> mq, mt;
    for (size_t i = 0; i < i1.size(); i++) {
        const uint32_t a = i1[i], b = i2[i];
        if (matched_cur[b]) continue;
        const bool im1_mono = (m->flags[acc[a]] & kMono) != 0, im2_mono = mono_cur[b] != 0;
        if (!(im1_mono && im2_mono)) continue;
        const int ii2 = cam_cur[b];
        if (ii2 < 0 || ii2 >= MCORB_MAX_CAMS || !((masks[a] >> ii2) & 1u)) continue;
        mq.push_back((int32_t)a);
        mt.push_back((int32_t)b);
    }

    if (n_new) *n_new = na;
    if (n_ind) *n_ind = (int)i1.size();
    if (n_matches) *n_matches = (int)mq.size();
    if (na > cap_new || (int)i1.size() > cap_ind || (int)mq.size() > cap_matches) { set_error("lmap search: output too small"); return MCORB_E_CAP; }
    for (int i = 0; i < na; i++) { new_lids[i] = acc[i]; cam_masks[i] = masks[i]; }
    if (!i1.empty()) { memcpy(ind1, i1.data(), i1.size() * 4); memcpy(ind2, i2.data(), i2.size() * 4); }
    if (!mq.empty()) { memcpy(match_query, mq.data(), mq.size() * 4); memcpy(match_train, mt.data(), mt.size() * 4); }
    return MCORB_OK;
}

int mcorb_lmap_last_timing(mcorb_lmap *m, float us[2], int *n_candidates)
{
    TRY(check_lmap_handle(m, "lmap last_timing"));
    if (!us) { set_error("lmap last_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    us[0] = m->search.cull.us[0];
    us[1] = m->search.us_best2;
    if (n_candidates) *n_candidates = m->search.last_candidates;
    return MCORB_OK;
}

}  // extern "C"
