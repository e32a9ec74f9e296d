// mcorb_landmark.cpp -- the local map kept up to date as keyframes are inserted: Landmark::addLfFrame with
// Landmark::updateNormal(frame, featInd) (MCSlam/src/GlobalMap.cpp:24-74, constructor :6-14; called at FrontEnd.cpp:6326-6335,
// :6680-6682 and :2819-2821), GlobalMap::updateLandmark (:162-185; Backend.cpp:3835-3864, :3594-3663), GlobalMap::deleteLandmark
// (:151-160; Backend.cpp:3442-3449) and the keys of searchLocalMap2's kfMap (FrontEnd.cpp:4925-4933).  Not restated: insertKeyFrame,
// the pose estimation, the optimisations and the cv::Mat inverses; the caller passes W_T_cur's translation per camera.
//
// A slot's ray count lives beside its point and normal (HBM for a device store, with a copy on the host: it is integer arithmetic
// on what the host packs, so the copy needs no read-back); its observation list (KFs / featInds) is host state in both stores, like
// the flags.  The arithmetic is mcorb_landmark.h.  A device store runs it in k_lmap_observe / k_lmap_update, one lane per item; the
// host-only store runs the same header serially in batch order.  A landmark named more than once in a batch depends on its own
// earlier result: the host cuts a batch into rounds -- round r holds every landmark's r-th occurrence, in batch order -- and
// launches them in order on the store's stream, so no two lanes of a launch touch one slot.  Everything that can be refused is
// refused before anything runs.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "mcorb_lmap_store.h"

using namespace mcorb;

namespace {

int fail(int code, const char *who, const char *what) { set_error(std::string(who) + ": " + what); return code; }

int check_ids(const mcorb_lmap *m, const int32_t *lids, int n, const char *who)
{
    for (int i = 0; i < n; i++)
        if (lids[i] < 0 || lids[i] >= m->max_landmarks) return fail(MCORB_E_ARG, who, "landmark id outside the store");
    return MCORB_OK;
}

// the rounds of a batch: order[] lists the items round by round (batch order inside a round), first[r] is round r's first entry
// (first.size() - 1 rounds), nth[i] is how often lids[i] occurred before item i.  Leaves m->life.occ zero.
void cut_rounds(mcorb_lmap *m, const int32_t *lids, int n, std::vector<int> &order, std::vector<int> &first, std::vector<int> &nth)
{
    nth.resize((size_t)n);
    int rounds = 0;
    for (int i = 0; i < n; i++) {
        nth[i] = m->life.occ[lids[i]]++;
        rounds = std::max(rounds, nth[i] + 1);
    }
    for (int i = 0; i < n; i++) m->life.occ[lids[i]] = 0;
    first.assign((size_t)rounds + 1, 0);
    for (int i = 0; i < n; i++) first[nth[i] + 1]++;
    for (int r = 0; r < rounds; r++) first[r + 1] += first[r];
    std::vector<int> at(first.begin(), first.end() - (rounds ? 1 : 0));
    order.resize((size_t)n);
    for (int i = 0; i < n; i++) order[at[nth[i]]++] = i;
}

// of an id that occurs more than once only the last entry kept (keep[i] = -1 for the others), as mcorb_lmap_set does
void keep_last(mcorb_lmap *m, const int32_t *lids, int n, std::vector<int> &keep)
{
    keep.assign(lids, lids + n);
    for (int i = n - 1; i >= 0; i--)
        if (m->life.occ[lids[i]]++) keep[i] = -1;
    for (int i = 0; i < n; i++) m->life.occ[lids[i]] = 0;
}

}  // namespace

int mcorb::lmap_delete_checked(mcorb_lmap *m, const int32_t *lids, int n, int32_t *kfs, int32_t *feats)
{
    if (n == 0) return MCORB_OK;
    if (m->device >= 0) {
        TRY(use_device(m->device));
        hipStream_t st = m->st;
        TRY(m->life.d_rays.grow((size_t)n));
        Submission sub(st);   // (its wait also covers the pageable list)
        sub.copy(m->life.d_rays, lids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
        sub.run([&] { launch_lmap_put_rays(st, m->life.d_rays, nullptr, n, m->d_nrays); });
        TRY(sub.wait());
    }
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        std::vector<LmObs> &o = m->obs[lids[i]];
        for (const LmObs &x : o) { kfs[at] = x.kf_id; feats[at] = x.feat; at++; }
        std::vector<LmObs>().swap(o);
        m->flags[lids[i]] = 0;
        m->n_rays[lids[i]] = 0;
    }
    return MCORB_OK;
}

extern "C" {

int mcorb_lmap_set_rays(mcorb_lmap *m, const int32_t *lids, int n, const int32_t *n_rays)
{
    const char *who = "lmap set_rays";
    TRY(check_lmap(m, who));
    if (n < 0 || (n && (!lids || !n_rays))) return fail(MCORB_E_ARG, who, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    TRY(check_ids(m, lids, n, who));
    for (int i = 0; i < n; i++) {
        if (n_rays[i] < 0) return fail(MCORB_E_ARG, who, "a negative ray count");
        if ((m->flags[lids[i]] & kSet) != kSet) return fail(MCORB_E_STATE, who, "the slot was never set");
    }
    if (n == 0) return MCORB_OK;
    if (m->device >= 0) {
        std::vector<int> keep;
        keep_last(m, lids, n, keep);
        TRY(use_device(m->device));
        hipStream_t st = m->st;
        TRY(m->life.h_rays.grow(2 * (size_t)n, hipHostMallocDefault));
        TRY(m->life.d_rays.grow(2 * (size_t)n));
        int k = 0;
        for (int i = 0; i < n; i++)
            if (keep[i] >= 0) k++;
        int at = 0;
        for (int i = 0; i < n; i++)
            if (keep[i] >= 0) { m->life.h_rays[at] = lids[i]; m->life.h_rays[k + at] = n_rays[i]; at++; }
        Submission sub(st);
        sub.copy(m->life.d_rays, m->life.h_rays, 2 * (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice);
        sub.run([&] { launch_lmap_put_rays(st, m->life.d_rays, m->life.d_rays + k, k, m->d_nrays); });
        TRY(sub.wait());
    }
    for (int i = 0; i < n; i++) m->n_rays[lids[i]] = n_rays[i];
    return MCORB_OK;
}

int mcorb_lmap_get_observations(mcorb_lmap *m, int lid, int32_t *n_rays, int32_t *kfs, int32_t *feats, int cap, int *n)
{
    const char *who = "lmap get_observations";
    if (n) *n = 0;
    TRY(check_lmap(m, who));
    if (cap < 0 || (cap && (!kfs || !feats))) return fail(MCORB_E_ARG, who, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    if (lid < 0 || lid >= m->max_landmarks) return fail(MCORB_E_ARG, who, "landmark id outside the store");
    if ((m->flags[lid] & kSet) != kSet) return fail(MCORB_E_STATE, who, "the slot was never set");
    const std::vector<LmObs> &o = m->obs[lid];
    if (n_rays) *n_rays = m->n_rays[lid];
    if (n) *n = (int)o.size();
    if ((int)o.size() > cap) return fail(MCORB_E_CAP, who, "output too small");
    for (size_t i = 0; i < o.size(); i++) { kfs[i] = o[i].kf_id; feats[i] = o[i].feat; }
    return MCORB_OK;
}

int mcorb_lmap_observe(mcorb_lmap *m, const mcorb_obs_frame *frame, const int32_t *lids, const int32_t *feats, int n, int mode,
                       mcorb_kfdb *db, int entry, const uint8_t *mono, int32_t *n_rays_out)
{
    const char *who = "lmap observe";
    TRY(check_lmap(m, who));
    if (!frame || n < 0 || (n && (!lids || !feats)) || (mode != MCORB_OBS_UPDATE && mode != MCORB_OBS_RECORD) || entry < -1 ||
        (entry >= 0 && !db))
        return fail(MCORB_E_ARG, who, "bad argument");
    if (frame->kf_id < 0 || frame->nfeat < 0 || (frame->nfeat && !frame->match_index)) return fail(MCORB_E_ARG, who, "bad frame");
    const int C = frame->ncams;
    if (C < 1 || C > MCORB_MAX_CAMS) return fail(MCORB_E_ARG, who, "1 .. MCORB_MAX_CAMS cameras");
    std::lock_guard<std::mutex> lk(m->mu);
    std::unique_lock<std::mutex> lkdb;
    if (entry >= 0) lkdb = std::unique_lock<std::mutex>(db->mu);

    // ---- 1. everything that can be refused is refused before anything runs ----
    int ndesc = 0;
    if (entry >= 0) {
        if (db->device != m->device) return fail(MCORB_E_ARG, who, "the database lives on another device");
        if (entry >= db->n) return fail(MCORB_E_ARG, who, "no such entry");
        ndesc = m->device < 0 ? (int)(db->entries[entry].desc.size() / 32) : db->mirror[entry].ndesc;
    }
    TRY(check_ids(m, lids, n, who));
    std::vector<uint32_t> mask((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        if (feats[i] < 0 || feats[i] >= frame->nfeat) return fail(MCORB_E_ARG, who, "feature index outside the frame");
        const int32_t *row = frame->match_index + (size_t)feats[i] * C;
        for (int c = 0; c < C; c++)
            if (row[c] != -1) mask[i] |= 1u << c;
        if (!mask[i]) return fail(MCORB_E_ARG, who, "a feature without a view");
        if (entry >= 0 && feats[i] >= ndesc) return fail(MCORB_E_ARG, who, "feature index outside the entry");
    }
    for (int i = 0; i < n; i++)
        if (!(m->flags[lids[i]] & kHasPt)) return fail(MCORB_E_STATE, who, "a slot without a point");
    if (n == 0) return MCORB_OK;

    // ---- 2. the rounds; the first observation of a landmark is the constructor's (KFs.size() == 1 after the push) ----
    std::vector<int> order, first, nth;
    cut_rounds(m, lids, n, order, first, nth);
    const bool update = mode == MCORB_OBS_UPDATE;
    if (update)
        for (int i = 0; i < n; i++)
            if (m->obs[lids[i]].empty() && nth[i] == 0) mask[i] |= kLmFirst;
    LmCentres cen;
    memset(&cen, 0, sizeof(cen));
    memcpy(cen.c, frame->centre_w, (size_t)C * 3 * sizeof(double));

    // ---- 3. normals and ray counts, then the descriptors of the latest observation ----
    if (m->device < 0) {
        if (update)
            for (int i = 0; i < n; i++) {
                double *g = &m->geom[(size_t)lids[i] * 6];
                lm_observe(cen, C, mask[i], g, g + 3, m->n_rays[lids[i]]);
                if (n_rays_out) n_rays_out[i] = m->n_rays[lids[i]];
            }
        if (entry >= 0) {
            const uint8_t *src = db->entries[entry].desc.data();
            for (int i = 0; i < n; i++) memcpy(&m->desc[(size_t)lids[i] * 32], src + (size_t)feats[i] * 32, 32);
        }
    } else {
        TRY(use_device(m->device));
        hipStream_t st = m->st;
        std::vector<int> keep;
        if (update) {
            TRY(m->life.h_obsitems.grow((size_t)n, hipHostMallocDefault));
            TRY(m->life.d_obsitems.grow((size_t)n));
            for (int k = 0; k < n; k++) m->life.h_obsitems[k] = LmObsItem{lids[order[k]], mask[order[k]]};
        }
        if (entry >= 0) {
            TRY(m->batch.reserve((size_t)n, false, false, false, true));
            keep_last(m, lids, n, keep);
        }
        Submission sub(st);   // (no piece, no wait: update off and no entry; its wait also covers the pageable lists)
        if (update) {
            sub.copy(m->life.d_obsitems, m->life.h_obsitems, (size_t)n * sizeof(LmObsItem), hipMemcpyHostToDevice);
            sub.mark(m->life.observe, 0);
            for (size_t r = 0; r + 1 < first.size(); r++)
                sub.run([&] { launch_lmap_observe(st, cen, C, m->life.d_obsitems + first[r], first[r + 1] - first[r], m->d_geom, m->d_nrays); });
            sub.mark(m->life.observe, 1);
        }
        if (entry >= 0) {
            m->batch.upload(sub, m->batch.d_lids, keep.data(), (size_t)n);
            m->batch.upload(sub, m->batch.d_rows, feats, (size_t)n);
            const uint8_t *rows = place_of(db, entry, false).desc;
            sub.run([&] { launch_lmap_put(st, m->batch.d_lids, n, nullptr, nullptr, rows, m->batch.d_rows, m->d_geom, m->d_desc); });
        }
        TRY(sub.wait());
        if (update) {
            m->life.observe.read();
            // the host's copy of the ray counts: the integer part of lm_observe, in batch order
            for (int i = 0; i < n; i++) {
                int32_t &nr = m->n_rays[lids[i]];
                const int views = __builtin_popcount(mask[i] & ~kLmFirst);
                nr = (mask[i] & kLmFirst) ? views : nr + views;
                if (n_rays_out) n_rays_out[i] = nr;
            }
        }
    }
    for (int i = 0; i < n; i++) {
        uint8_t &f = m->flags[lids[i]];
        if (update) f |= kHasNormal;
        else if (n_rays_out) n_rays_out[i] = m->n_rays[lids[i]];
        if (entry >= 0) f |= kHasDesc;
        if (mono) f = (uint8_t)((f & ~kMono) | (mono[i] ? kMono : 0));
        m->obs[lids[i]].push_back(LmObs{frame->kf_id, feats[i]});
    }
    return MCORB_OK;
}

int mcorb_lmap_update_points(mcorb_lmap *m, const int32_t *lids, int n, const double *pt_new, double max_diff, uint8_t *updated,
                             double *diff_norm)
{
    const char *who = "lmap update_points";
    TRY(check_lmap(m, who));
    if (n < 0 || (n && (!lids || !pt_new))) return fail(MCORB_E_ARG, who, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    TRY(check_ids(m, lids, n, who));
    for (int i = 0; i < n; i++)
        if (!(m->flags[lids[i]] & kHasPt)) return fail(MCORB_E_STATE, who, "a slot without a point");
    if (n == 0) return MCORB_OK;
    if (m->device < 0) {
        for (int i = 0; i < n; i++) {
            double d = 0.0;
            const bool u = lm_update(&m->geom[(size_t)lids[i] * 6], pt_new + 3 * (size_t)i, max_diff, d);
            if (updated) updated[i] = u ? 1 : 0;
            if (diff_norm) diff_norm[i] = d;
        }
        return MCORB_OK;
    }
    std::vector<int> order, first, nth;
    cut_rounds(m, lids, n, order, first, nth);
    TRY(use_device(m->device));
    hipStream_t st = m->st;
    TRY(m->life.h_upditems.grow((size_t)n, hipHostMallocDefault));
    TRY(m->life.d_upditems.grow((size_t)n));
    TRY(m->life.h_updout.grow((size_t)n, hipHostMallocDefault));
    TRY(m->life.d_updout.grow((size_t)n));
    for (int k = 0; k < n; k++) {
        const int i = order[k];
        LmUpdItem &it = m->life.h_upditems[k];
        it.lid = lids[i];
        it.idx = i;
        memcpy(it.p, pt_new + 3 * (size_t)i, 3 * sizeof(double));
    }
    Submission sub(st);
    sub.copy(m->life.d_upditems, m->life.h_upditems, (size_t)n * sizeof(LmUpdItem), hipMemcpyHostToDevice);
    sub.mark(m->life.update, 0);
    for (size_t r = 0; r + 1 < first.size(); r++)
        sub.run([&] { launch_lmap_update(st, m->life.d_upditems + first[r], first[r + 1] - first[r], max_diff, m->d_geom, m->life.d_updout); });
    sub.mark(m->life.update, 1);
    sub.copy(m->life.h_updout, m->life.d_updout, (size_t)n * sizeof(LmUpdOut), hipMemcpyDeviceToHost);
    TRY(sub.wait());
    m->life.update.read();
    for (int i = 0; i < n; i++) {
        if (updated) updated[i] = m->life.h_updout[i].updated ? 1 : 0;
        if (diff_norm) diff_norm[i] = m->life.h_updout[i].diff_norm;
    }
    return MCORB_OK;
}

int mcorb_lmap_delete(mcorb_lmap *m, const int32_t *lids, int n, int32_t *kfs, int32_t *feats, int cap, int *n_out)
{
    const char *who = "lmap delete";
    if (n_out) *n_out = 0;
    TRY(check_lmap(m, who));
    if (n < 0 || (n && !lids) || cap < 0 || (cap && (!kfs || !feats))) return fail(MCORB_E_ARG, who, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    TRY(check_ids(m, lids, n, who));
    bool twice = false;
    for (int i = 0; i < n; i++)
        if (m->life.occ[lids[i]]++) twice = true;
    for (int i = 0; i < n; i++) m->life.occ[lids[i]] = 0;
    if (twice) return fail(MCORB_E_ARG, who, "a landmark id twice in the batch");
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if ((m->flags[lids[i]] & kSet) != kSet) return fail(MCORB_E_STATE, who, "the slot was never set");
        total += m->obs[lids[i]].size();
    }
    if (n_out) *n_out = (int)total;
    if (total > (size_t)cap) return fail(MCORB_E_CAP, who, "output too small");
    return lmap_delete_checked(m, lids, n, kfs, feats);
}

int mcorb_lmap_observers(mcorb_lmap *m, const int32_t *lids, int n, int32_t *kf_ids, int cap, int *n_out)
{
    const char *who = "lmap observers";
    if (n_out) *n_out = 0;
    TRY(check_lmap(m, who));
    if (n < 0 || (n && !lids) || cap < 0 || (cap && !kf_ids)) return fail(MCORB_E_ARG, who, "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    TRY(check_ids(m, lids, n, who));
    std::vector<int32_t> ids;
    for (int i = 0; i < n; i++) {
        if ((m->flags[lids[i]] & kSet) != kSet) return fail(MCORB_E_STATE, who, "the slot was never set");
        for (const LmObs &x : m->obs[lids[i]]) ids.push_back(x.kf_id);
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    if (n_out) *n_out = (int)ids.size();
    if ((int)ids.size() > cap) return fail(MCORB_E_CAP, who, "output too small");
    if (!ids.empty()) memcpy(kf_ids, ids.data(), ids.size() * sizeof(int32_t));
    return MCORB_OK;
}

int mcorb_lmap_last_landmark_timing(mcorb_lmap *m, float us[2])
{
    TRY(check_lmap_handle(m, "lmap last_landmark_timing"));
    if (!us) return fail(MCORB_E_ARG, "lmap last_landmark_timing", "bad argument");
    std::lock_guard<std::mutex> lk(m->mu);
    us[0] = m->life.observe.us[0];
    us[1] = m->life.update.us[0];
    return MCORB_OK;
}

}  // extern "C"
