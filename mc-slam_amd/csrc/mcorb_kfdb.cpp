// mcorb_kfdb.cpp -- the keyframe database: DBoW2's TemplatedDatabase add / query, TemplatedVocabulary::score and
// LoopCloser::featureMatchesBow (MCSlam/src/LoopCloser.cpp:59-241; Relocalization runs the same sequence), the consumer of a
// frame's lfBoW, lfFeatVec and LF descriptors.
//
// DBoW2 is an un-vendored dependency of the reference (the seventh unpinned third-party piece): the semantics restated
// here are the published TemplatedDatabase's (use_di = true, L1_NORM only) --
//   add      every (word, value) of the vector is stored as given, the FeatureVector is kept;
//   queryL1  for every entry e with max_id == -1 || (int)e < max_id that shares a word with the query, the sum over the shared
//            words, in ascending word id, of (|q - d| - |q|) - |d| in fp64 with one running accumulator; the list, built in
//            ascending entry id, goes through std::sort by raw value, is cut to max_results when that is > 0, and every score
//            becomes -s / 2.0;
//   score    the same sum over the shared words of two vectors.
//
// Two databases, deliberately of different structure so that they check each other:
//   device >= 0   entry-major fixed-stride arrays in HBM, scored by k_kfdb_score; featureMatchesBow's search by k_kfdb_best2;
//   device == -1  host only, written the way DBoW2 is: a word-major inverted file, a std::map<EntryId, double> per query filled
//                 with `+=` in query-word order, and the literal getMatches_distRatio loop over the descriptors.
// The final std::sort and the cut run on the host in both, on the same ascending-id input, so the order among equal scores is
// libstdc++'s in both (the dependence mcorb_sortmodel.h documents for selection).
//
// Probe slots hold a frame in the same layout without making it an entry: the current frame of FrontEnd::trackFrame
// (findInterMatchesBow -> InterMatchingBow, FrontEnd.cpp:3676-3788; findInterMatches, :3344-3499) and of Relocalization
// (relocalization.cpp:327-371).  They are queried, scored and matched against entries; nothing they do touches n, the inverted
// file or an entry.  In the descriptor allocation the probe slots lie behind the entries, all sets `fstride` rows apart, so
// that findInterMatches' knnMatch of an entry and a probe is one launch_knn2 on two sets of one base.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "mcorb_kfdb_store.h"

using namespace mcorb;

namespace {

constexpr int kMaxProbes = 128;

struct Result {   // DBoW2::Result: ordered by score alone
    uint32_t id;
    double score;
    bool operator<(const Result &r) const { return score < r.score; }
};

struct Vectors {   // a keyframe's vectors in mcorb_vocab_transform's layout
    const uint32_t *bow_ids; const double *bow_vals; int nbow;
    const uint32_t *fv_nodes; const int32_t *fv_offsets; int nfv;
    const int32_t *fv_feats;
    int nff;   // fv_offsets[nfv]
};

}  // namespace

// (entry: the vectors become a new entry, which needs room; a probe slot is overwritten)
static int check_vectors(const mcorb_kfdb *db, const Vectors &v, int ndesc, bool entry)
{
    if (v.nbow < 0 || v.nfv < 0 || ndesc < 0 || (v.nbow && (!v.bow_ids || !v.bow_vals)) || (v.nfv && (!v.fv_nodes || !v.fv_offsets))) {
        set_error("kfdb add: bad argument");
        return MCORB_E_ARG;
    }
    if (entry && db->n >= db->max_entries) { set_error("kfdb add: the database is full (max_entries)"); return MCORB_E_CAP; }
    if (v.nbow > db->max_words || v.nfv > db->max_feats || ndesc > db->max_feats) {
        set_error("kfdb add: a vector is longer than the database's caps (max_words / max_feats)");
        return MCORB_E_CAP;
    }
    for (int i = 1; i < v.nbow; i++)
        if (v.bow_ids[i] <= v.bow_ids[i - 1]) { set_error("kfdb add: BowVector word ids must ascend"); return MCORB_E_ARG; }
    for (int i = 0; i < v.nfv; i++)
        if ((i && v.fv_nodes[i] <= v.fv_nodes[i - 1]) || v.fv_offsets[i + 1] < v.fv_offsets[i] || v.fv_offsets[0] != 0) {
            set_error("kfdb add: FeatureVector node ids must ascend, its offsets start at 0 and not descend");
            return MCORB_E_ARG;
        }
    if (v.nff > db->max_feats) { set_error("kfdb add: the FeatureVector is longer than max_feats"); return MCORB_E_CAP; }
    if (v.nff && !v.fv_feats) { set_error("kfdb add: bad argument"); return MCORB_E_ARG; }
    for (int i = 0; i < v.nff; i++)
        if (v.fv_feats[i] < 0 || v.fv_feats[i] >= ndesc) { set_error("kfdb add: FeatureVector names a feature outside the descriptor set"); return MCORB_E_ARG; }
    return MCORB_OK;
}

// a frame's BowVector, FeatureVector and descriptor count to its place in the store, pieces of sub (the descriptors are the caller's)
static void store_vectors(Submission &sub, const Place &p, const Vectors &v, const int &ndesc)
{
    sub.copy(p.ids, v.bow_ids, (size_t)v.nbow * 4, hipMemcpyHostToDevice);
    sub.copy(p.vals, v.bow_vals, (size_t)v.nbow * 8, hipMemcpyHostToDevice);
    sub.copy(p.nbow, &v.nbow, sizeof(int), hipMemcpyHostToDevice);
    sub.copy(p.ndesc, &ndesc, sizeof(int), hipMemcpyHostToDevice);
    if (v.nfv) {
        sub.copy(p.nodes, v.fv_nodes, (size_t)v.nfv * 4, hipMemcpyHostToDevice);
        sub.copy(p.offs, v.fv_offsets, (size_t)(v.nfv + 1) * 4, hipMemcpyHostToDevice);
    }
    sub.copy(p.feats, v.fv_feats, (size_t)v.nff * 4, hipMemcpyHostToDevice);
}

static Mirror mirror_of(const Vectors &v, int ndesc)
{
    Mirror m;
    m.nbow = v.nbow; m.nfv = v.nfv; m.nff = v.nff; m.ndesc = ndesc;
    m.nodes.assign(v.fv_nodes, v.fv_nodes + v.nfv);
    if (v.nfv) m.offs.assign(v.fv_offsets, v.fv_offsets + v.nfv + 1);
    else m.offs.assign(1, 0);
    return m;
}

static HostEntry host_entry_of(const Vectors &v, const uint8_t *desc, int ndesc)
{
    HostEntry h;
    h.ids.assign(v.bow_ids, v.bow_ids + v.nbow);
    h.vals.assign(v.bow_vals, v.bow_vals + v.nbow);
    h.nodes.assign(v.fv_nodes, v.fv_nodes + v.nfv);
    if (v.nfv) h.offs.assign(v.fv_offsets, v.fv_offsets + v.nfv + 1);
    else h.offs.assign(1, 0);
    h.feats.assign(v.fv_feats, v.fv_feats + v.nff);
    h.desc.assign(desc, desc + (size_t)ndesc * 32);
    return h;
}

// What add, add_rig_frame, set_probe and set_probe_rig_frame share: a frame's vectors and descriptors become entry db->n
// (probe < 0) or overwrite probe slot `probe`.  The descriptors are host rows (desc), or, for a rig frame (s, o), rows of the
// slot's descriptor block in HBM (LfFrameOut::src) gathered device to device on the slot's stream; lfBoW and lfFeatVec are
// assembled on the host (lf_job_finish) and uploaded.  Nothing is stored when the vectors fail check_vectors.
static int put_frame(mcorb_kfdb *db, int probe, const Vectors &v, const uint8_t *desc, int ndesc, Slot *s, const LfFrameOut *o)
{
    TRY(check_vectors(db, v, ndesc, probe < 0));
    if (db->device < 0) {
        std::vector<uint8_t> rows;
        if (o) {
            rows.resize((size_t)ndesc * 32);
            for (int i = 0; i < ndesc; i++) memcpy(rows.data() + (size_t)i * 32, o->feats[i].desc, 32);
            desc = rows.data();
        }
        HostEntry h = host_entry_of(v, desc, ndesc);
        if (probe >= 0) {
            db->probes[probe] = std::move(h);
            db->probe_set[probe] = 1;
            return MCORB_OK;
        }
        const uint32_t e = (uint32_t)db->n;   // EntryId entry_id = m_nentries++
        for (int i = 0; i < v.nbow; i++) db->ifile[v.bow_ids[i]].emplace_back(e, v.bow_vals[i]);   // m_ifile[word_id].push_back(IFPair(entry_id, word_weight))
        db->entries.push_back(std::move(h));
        db->n++;
        return MCORB_OK;
    }
    TRY(use_device(db->device));
    hipStream_t st = s ? (hipStream_t)s->st : (hipStream_t)db->st;
    const Place p = place_of(db, probe < 0 ? db->n : probe, probe >= 0);
    if (ndesc && o) TRY(db->d_src.grow((size_t)db->max_feats));
    Submission sub(st);   // (its wait also covers the pageable vectors and the two counts)
    store_vectors(sub, p, v, ndesc);
    if (ndesc && o) {
        sub.copy(db->d_src, o->src.data(), (size_t)ndesc * sizeof(int), hipMemcpyHostToDevice);
        sub.run([&] { launch_kfdb_gather(st, s->d_desc, db->d_src, ndesc, p.desc); });
    } else {
        sub.copy(p.desc, desc, (size_t)ndesc * 32, hipMemcpyHostToDevice);
    }
    TRY(sub.wait());
    if (probe >= 0) {
        db->pmirror[probe] = mirror_of(v, ndesc);
        db->probe_set[probe] = 1;
    } else {
        db->mirror.push_back(mirror_of(v, ndesc));
        db->n++;
    }
    return MCORB_OK;
}

// the frame of a rig slot that add_rig_frame / set_probe_rig_frame name: MCORB_E_STATE unless the slot's last job ran the LF stage on it
static int rig_frame_of(const mcorb_kfdb *db, mcorb_rig *r, int slot, int frame, const char *who, Slot **s_out)
{
    if (!r || slot < 0 || slot >= (int)r->rig.slots.size()) { set_error(std::string(who) + ": bad argument"); return MCORB_E_ARG; }
    Slot *s = r->rig.slots[slot].get();
    {
        std::lock_guard<std::mutex> lk(s->m);
        if (s->busy) { set_error("slot busy"); return MCORB_E_STATE; }
    }
    if (frame < 0 || frame >= (int)s->lf_ok.size() || !s->lf_ok[frame]) {
        set_error(std::string(who) + ": frame not processed by the LF stage since the slot's last extraction");
        return MCORB_E_STATE;
    }
    if (db->device >= 0 && db->device != r->rig.device) { set_error(std::string(who) + ": the rig lives on another device"); return MCORB_E_ARG; }
    *s_out = s;
    return MCORB_OK;
}

static Vectors vectors_of(const LfFrameOut &o)
{
    const BowImageOut &b = o.bow;
    return Vectors{b.bow_ids.data(), b.bow_vals.data(), (int)b.bow_ids.size(), b.fv_nodes.data(), b.fv_offsets.data(), (int)b.fv_nodes.size(),
                   b.fv_feats.data(), (int)b.fv_feats.size()};
}

// TemplatedDatabase::queryL1 from the accumulation on: sort, cut, -s / 2
static int finish_query(std::vector<Result> &ret, int max_results, uint32_t *ids, double *scores, int cap, int *n_out)
{
    std::sort(ret.begin(), ret.end());
    if (max_results > 0 && (int)ret.size() > max_results) ret.resize(max_results);
    if (n_out) *n_out = (int)ret.size();
    if ((int)ret.size() > cap) { set_error("kfdb query: output too small"); return MCORB_E_CAP; }
    for (size_t i = 0; i < ret.size(); i++) {
        ids[i] = ret[i].id;
        scores[i] = -ret[i].score / 2.0;
    }
    return MCORB_OK;
}

static void query_host(const mcorb_kfdb *db, const uint32_t *qids, const double *qvals, int nq, int max_id, std::vector<Result> &ret)
{
    std::map<uint32_t, double> pairs;
    for (int i = 0; i < nq; i++) {
        const double qvalue = qvals[i];
        const auto row = db->ifile.find(qids[i]);
        if (row == db->ifile.end()) continue;
        for (const auto &d : row->second) {
            const uint32_t entry_id = d.first;
            const double dvalue = d.second;
            if ((int)entry_id < max_id || max_id == -1) {
                const double value = fabs(qvalue - dvalue) - fabs(qvalue) - fabs(dvalue);
                auto pit = pairs.lower_bound(entry_id);
                if (pit != pairs.end() && !(pairs.key_comp()(entry_id, pit->first))) pit->second += value;
                else pairs.insert(pit, std::map<uint32_t, double>::value_type(entry_id, value));
            }
        }
    }
    ret.clear();
    ret.reserve(pairs.size());
    for (const auto &p : pairs) ret.push_back(Result{p.first, p.second});
}

// entries [0, limit) of a query with this max_id
static int limit_of(int max_id, int n) { return max_id == -1 ? n : std::min(std::max(max_id, 0), n); }

// BowVectors as k_kfdb_score reads them (max_words apart): the entries, the probe slots, or the one-vector scratch of a host query
struct BowArrays { const uint32_t *ids; const double *vals; const int *n; };
static BowArrays entry_bows(const mcorb_kfdb *db) { return BowArrays{db->d_ids, db->d_vals, db->d_nbow}; }
static BowArrays probe_bows(const mcorb_kfdb *db) { return BowArrays{db->p_ids, db->p_vals, db->p_nbow}; }
static BowArrays scratch_bow(const mcorb_kfdb *db) { return BowArrays{db->d_qids, db->d_qvals, db->d_qn}; }

// k_kfdb_score for nq queries; sel[q]: the vector of `query` that is query q.  With against != nullptr query q is held against
// the single vector against[q] of `store` instead of the entries below its limit.  raw / shared of (q, x) land at h_raw /
// h_shared[q * stride_out + x].  before: what the caller queues in front (mcorb_kfdb_query's vector), behind the grows;
// NOT called when no query has an entry below its limit, where nothing is queued.
static int run_score(mcorb_kfdb *db, const BowArrays &store, const BowArrays &query, const int *sel, const int *limit, const int *against,
                     int nq, int *stride_out, const Pieces &before = nullptr)
{
    const int os = std::max(against ? 1 : db->n, 1);
    *stride_out = os;
    int max_limit = 0;
    for (int q = 0; q < nq; q++) max_limit = std::max(max_limit, limit[q]);
    if (max_limit < 1) return MCORB_OK;
    std::vector<int> ctl((size_t)nq * 2 + (against ? nq : 0));
    for (int q = 0; q < nq; q++) {
        ctl[q] = sel[q];
        ctl[nq + q] = limit[q];
        if (against) ctl[2 * (size_t)nq + q] = against[q];
    }
    const size_t nout = (size_t)nq * os;
    TRY(db->d_ctl.grow(ctl.size()));
    TRY(db->d_raw.grow(nout));
    TRY(db->d_shared.grow(nout));
    TRY(db->h_raw.grow(nout, hipHostMallocDefault));
    TRY(db->h_shared.grow(nout, hipHostMallocDefault));
    hipStream_t st = db->st;
    Submission sub(st);   // (its wait also covers the pageable control array)
    if (before) before(sub);
    sub.copy(db->d_ctl, ctl.data(), ctl.size() * sizeof(int), hipMemcpyHostToDevice);
    sub.run(db->score, 0, [&] {
        launch_kfdb_score(st, store.ids, store.vals, store.n, db->max_words, query.ids, query.vals, query.n, db->d_ctl, db->d_ctl + nq,
                          against ? db->d_ctl + 2 * (size_t)nq : nullptr, nq, max_limit, os, db->d_raw, db->d_shared);
    });
    sub.mark(db->score, 1);
    sub.copy(db->h_raw, db->d_raw, nout * sizeof(double), hipMemcpyDeviceToHost);
    sub.copy(db->h_shared, db->d_shared, nout * sizeof(int), hipMemcpyDeviceToHost);
    TRY(sub.wait());
    db->score.read();
    return MCORB_OK;
}

// the ascending-id list of query q from the launch's results: presence is "shares a word", not "score != 0"
static void list_of(const mcorb_kfdb *db, int q, int stride, int limit, std::vector<Result> &ret)
{
    ret.clear();
    for (int e = 0; e < limit; e++)
        if (db->h_shared[(size_t)q * stride + e] > 0) ret.push_back(Result{(uint32_t)e, db->h_raw[(size_t)q * stride + e]});
}

static int check_db(const mcorb_kfdb *db, const char *who)
{
    if (!db) { set_error(std::string(who) + ": bad argument"); return MCORB_E_ARG; }
    return MCORB_OK;
}

static int check_entry(const mcorb_kfdb *db, int e, const char *who)
{
    if (e < 0 || e >= db->n) { set_error(std::string(who) + ": no such entry"); return MCORB_E_ARG; }
    return MCORB_OK;
}

// L1Scoring::score: a merge walk over the two sorted vectors
static double score_host(const HostEntry &a, const HostEntry &b)
{
    double s = 0;
    size_t i = 0, j = 0;
    while (i < a.ids.size() && j < b.ids.size()) {
        if (a.ids[i] == b.ids[j]) {
            const double vi = a.vals[i], wi = b.vals[j];
            s += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++i; ++j;
        } else if (a.ids[i] < b.ids[j]) {
            i = std::lower_bound(a.ids.begin() + i, a.ids.end(), b.ids[j]) - a.ids.begin();
        } else {
            j = std::lower_bound(b.ids.begin() + j, b.ids.end(), a.ids[i]) - b.ids.begin();
        }
    }
    return -s / 2.0;
}

int Best2Search::create() { return launch.create(); }

void Best2Search::reset()
{
    items.clear(); recs.clear(); first_item.clear();
    first_rec.assign(1, 0);
}

void Best2Search::add_b(const std::vector<uint32_t> &a_nodes, const std::vector<int32_t> &a_offs, const Mirror &B, int set)
{
    size_t ia = 0, ib = 0;
    while (ia < a_nodes.size() && ib < B.nodes.size()) {
        if (a_nodes[ia] == B.nodes[ib]) {
            first_item.push_back((int)items.size());
            for (int a = a_offs[ia]; a < a_offs[ia + 1]; a++) items.push_back(int2{a, (int)recs.size()});
            recs.push_back(int4{set, B.offs[ib], B.offs[ib + 1] - B.offs[ib], 0});
            ++ia; ++ib;
        } else if (a_nodes[ia] < B.nodes[ib]) ++ia;
        else ++ib;
    }
    first_rec.push_back((int)recs.size());
}

int Best2Search::run(hipStream_t st, const uint8_t *desc_a, const int *feats_a, const uint8_t *desc_b, size_t desc_stride,
                     const int *feats_b, size_t feats_stride, double max_neighbor_ratio, std::vector<std::vector<uint32_t>> &i1,
                     std::vector<std::vector<uint32_t>> &i2, float *us, const Pieces &before)
{
    const size_t nb = first_rec.size() - 1;
    i1.assign(nb, {}); i2.assign(nb, {});
    if (items.empty()) return MCORB_OK;
    first_item.push_back((int)items.size());
    TRY(d_items.grow(items.size()));
    TRY(d_recs.grow(recs.size()));
    TRY(d_mtab.grow(items.size()));
    TRY(h_mtab.grow(items.size(), hipHostMallocDefault));
    Submission sub(st);   // (its wait also covers the pageable item and record lists)
    if (before) before(sub);
    sub.copy(d_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice);
    sub.copy(d_recs, recs.data(), recs.size() * sizeof(int4), hipMemcpyHostToDevice);
    sub.run(launch, 0, [&] {
        launch_kfdb_best2(st, desc_a, feats_a, desc_b, desc_stride, feats_b, feats_stride, d_items, (int)items.size(), d_recs, d_mtab);
    });
    sub.mark(launch, 1);
    sub.copy(h_mtab, d_mtab, items.size() * sizeof(int4), hipMemcpyDeviceToHost);
    TRY(sub.wait());
    launch.read();
    *us = launch.us[0];
    std::vector<uint32_t> mA, mB;
    std::vector<double> mD;
    for (size_t b = 0; b < nb; b++)
        for (int k = first_rec[b]; k < first_rec[b + 1]; k++) {
            mA.clear(); mB.clear(); mD.clear();
            for (int i = first_item[k]; i < first_item[k + 1]; i++) {
                const int4 t = h_mtab[i];   // {B feature of the best or -1, best, second, A feature}
                if (t.x < 0) continue;      // an empty B list: best_dist_1 stays 1e9
                accept((double)t.y, t.z == 0x7fffffff ? 1e9 : (double)t.z, (uint32_t)t.w, (uint32_t)t.x, max_neighbor_ratio, mA, mB, mD);
            }
            i1[b].insert(i1[b].end(), mA.begin(), mA.end());
            i2[b].insert(i2[b].end(), mB.begin(), mB.end());
        }
    return MCORB_OK;
}

extern "C" {

int mcorb_kfdb_create(const mcorb_vocab *v, int device, int max_entries, int max_words, int max_feats, mcorb_kfdb **out)
{
    if (out) *out = nullptr;
    if (!v || !out || device < -1 || max_entries < 1 || max_words < 1 || max_feats < 1) { set_error("kfdb create: bad argument"); return MCORB_E_ARG; }
    int scoring = 0, vdev = 0;
    vocab_props(v, scoring, vdev);
    if (scoring != 0) { set_error("kfdb create: only L1_NORM vocabularies (scoring 0) are supported"); return MCORB_E_ARG; }
    if (device >= 0 && vdev != device) { set_error("kfdb create: the vocabulary lives on another device"); return MCORB_E_ARG; }
    if (device >= 0 && max_words > MCORB_KFDB_MAX_WORDS) { set_error("kfdb create: max_words exceeds MCORB_KFDB_MAX_WORDS (a query is staged in LDS)"); return MCORB_E_ARG; }
    static_assert(MCORB_KFDB_MAX_WORDS == kKfdbMaxWords, "the header's limit is the kernel's");
    std::unique_ptr<mcorb_kfdb> db(new mcorb_kfdb);
    db->device = device; db->max_entries = max_entries; db->max_words = max_words; db->max_feats = max_feats;
    db->fstride = (max_feats + 63) / 64 * 64;   // (launch_knn2 walks whole 64-row tiles of a set)
    if (device >= 0) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { set_error("kfdb create: no such HIP device"); return MCORB_E_NODEVICE; }
        HIPCHK(hipSetDevice(device));
        const size_t E = (size_t)max_entries, W = (size_t)max_words, F = (size_t)max_feats;
        TRY(db->st.create(hipStreamNonBlocking));
        TRY(db->score.create());
        TRY(db->best2.create());
        TRY(db->d_ids.alloc(E * W));
        TRY(db->d_vals.alloc(E * W));
        TRY(db->d_nbow.alloc(E));
        TRY(db->d_nodes.alloc(E * F));
        TRY(db->d_offs.alloc(E * (F + 1)));
        TRY(db->d_feats.alloc(E * F));
        TRY(db->d_desc.alloc(E * db->fstride * 32));
        TRY(db->d_ndesc.alloc(E + kMaxProbes));
        TRY(db->d_qids.alloc(W));
        TRY(db->d_qvals.alloc(W));
        TRY(db->d_qn.alloc(1));
    }
    *out = db.release();
    return MCORB_OK;
}

void mcorb_kfdb_destroy(mcorb_kfdb *db)
{
    if (!db) return;
    if (db->device >= 0 && hipSetDevice(db->device) == hipSuccess && db->st.get()) (void)hipStreamSynchronize(db->st);
    delete db;
}

int mcorb_kfdb_size(const mcorb_kfdb *db) { return db ? db->n : MCORB_E_ARG; }

int mcorb_kfdb_add(mcorb_kfdb *db, const uint32_t *bow_ids, const double *bow_vals, int nbow, const uint32_t *fv_nodes,
                   const int32_t *fv_offsets, int nfv, const int32_t *fv_feats, const uint8_t *desc, int ndesc, int *entry_out)
{
    TRY(check_db(db, "kfdb add"));
    std::lock_guard<std::mutex> lk(db->mu);
    if (nfv < 0 || (nfv && !fv_offsets) || (ndesc > 0 && !desc)) { set_error("kfdb add: bad argument"); return MCORB_E_ARG; }
    const Vectors v{bow_ids, bow_vals, nbow, fv_nodes, fv_offsets, nfv, fv_feats, nfv ? fv_offsets[nfv] : 0};
    const int e = db->n;
    TRY(put_frame(db, -1, v, desc, ndesc, nullptr, nullptr));
    if (entry_out) *entry_out = e;
    return MCORB_OK;
}

int mcorb_kfdb_add_rig_frame(mcorb_kfdb *db, mcorb_rig *r, int slot, int frame, int *entry_out)
{
    TRY(check_db(db, "kfdb add_rig_frame"));
    Slot *s = nullptr;
    TRY(rig_frame_of(db, r, slot, frame, "kfdb add_rig_frame", &s));
    std::lock_guard<std::mutex> lk(db->mu);
    const LfFrameOut &o = s->lf[frame];
    const int e = db->n;
    TRY(put_frame(db, -1, vectors_of(o), nullptr, (int)o.feats.size(), s, &o));
    if (entry_out) *entry_out = e;
    return MCORB_OK;
}

// get_entry / get_probe: a stored frame as it is stored
static int get_frame(mcorb_kfdb *db, int idx, bool probe, const char *who, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow,
                     uint32_t *fv_nodes, int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap, uint8_t *desc,
                     int desc_cap, int *ndesc)
{
    int c_bow, c_fv, c_ff, c_desc;
    if (db->device < 0) {
        const HostEntry &h = probe ? db->probes[idx] : db->entries[idx];
        c_bow = (int)h.ids.size(); c_fv = (int)h.nodes.size(); c_ff = (int)h.feats.size(); c_desc = (int)(h.desc.size() / 32);
    } else {
        const Mirror &m = probe ? db->pmirror[idx] : db->mirror[idx];
        c_bow = m.nbow; c_fv = m.nfv; c_ff = m.nff; c_desc = m.ndesc;
    }
    if (nbow) *nbow = c_bow;
    if (nfv) *nfv = c_fv;
    if (ndesc) *ndesc = c_desc;
    if (c_bow > bow_cap || c_fv > fv_cap || c_ff > feat_cap || c_desc > desc_cap) { set_error(std::string(who) + ": output too small"); return MCORB_E_CAP; }
    if (!fv_offsets || (c_bow && (!bow_ids || !bow_vals)) || (c_fv && !fv_nodes) || (c_ff && !fv_feats) || (c_desc && !desc)) {
        set_error(std::string(who) + ": bad argument");
        return MCORB_E_ARG;
    }
    if (db->device < 0) {
        const HostEntry &h = probe ? db->probes[idx] : db->entries[idx];
        if (c_bow) { memcpy(bow_ids, h.ids.data(), (size_t)c_bow * 4); memcpy(bow_vals, h.vals.data(), (size_t)c_bow * 8); }
        if (c_fv) memcpy(fv_nodes, h.nodes.data(), (size_t)c_fv * 4);
        memcpy(fv_offsets, h.offs.data(), h.offs.size() * 4);
        if (c_ff) memcpy(fv_feats, h.feats.data(), (size_t)c_ff * 4);
        if (c_desc) memcpy(desc, h.desc.data(), (size_t)c_desc * 32);
        return MCORB_OK;
    }
    HIPCHK(hipSetDevice(db->device));
    const Place p = place_of(db, idx, probe);
    fv_offsets[0] = 0;
    if (c_bow) {
        HIPCHK(hipMemcpy(bow_ids, p.ids, (size_t)c_bow * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(bow_vals, p.vals, (size_t)c_bow * 8, hipMemcpyDeviceToHost));
    }
    if (c_fv) {
        HIPCHK(hipMemcpy(fv_nodes, p.nodes, (size_t)c_fv * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(fv_offsets, p.offs, (size_t)(c_fv + 1) * 4, hipMemcpyDeviceToHost));
    }
    if (c_ff) HIPCHK(hipMemcpy(fv_feats, p.feats, (size_t)c_ff * 4, hipMemcpyDeviceToHost));
    if (c_desc) HIPCHK(hipMemcpy(desc, p.desc, (size_t)c_desc * 32, hipMemcpyDeviceToHost));
    return MCORB_OK;
}

int mcorb_kfdb_get_entry(mcorb_kfdb *db, int entry, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow, uint32_t *fv_nodes,
                         int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap, uint8_t *desc, int desc_cap,
                         int *ndesc)
{
    TRY(check_db(db, "kfdb get_entry"));
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_entry(db, entry, "kfdb get_entry"));
    return get_frame(db, entry, false, "kfdb get_entry", bow_ids, bow_vals, bow_cap, nbow, fv_nodes, fv_offsets, fv_cap, nfv, fv_feats,
                     feat_cap, desc, desc_cap, ndesc);
}

int mcorb_kfdb_query(mcorb_kfdb *db, const uint32_t *bow_ids, const double *bow_vals, int nbow, int max_results, int max_id,
                     uint32_t *ids, double *scores, int cap, int *n_out)
{
    if (n_out) *n_out = 0;
    TRY(check_db(db, "kfdb query"));
    if (nbow < 0 || (nbow && (!bow_ids || !bow_vals)) || cap < 0 || (cap && (!ids || !scores))) { set_error("kfdb query: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    std::vector<Result> ret;
    if (db->device < 0) {
        query_host(db, bow_ids, bow_vals, nbow, max_id, ret);
        return finish_query(ret, max_results, ids, scores, cap, n_out);
    }
    if (nbow > db->max_words) { set_error("kfdb query: the vector is longer than max_words"); return MCORB_E_CAP; }
    for (int i = 1; i < nbow; i++)
        if (bow_ids[i] <= bow_ids[i - 1]) { set_error("kfdb query: BowVector word ids must ascend"); return MCORB_E_ARG; }
    const int limit = limit_of(max_id, db->n);
    if (nbow && limit) {
        TRY(use_device(db->device));
        const int sel = 0;
        int stride = 1;
        TRY(run_score(db, entry_bows(db), scratch_bow(db), &sel, &limit, nullptr, 1, &stride, [&](Submission &sub) {
            sub.copy(db->d_qids, bow_ids, (size_t)nbow * 4, hipMemcpyHostToDevice);
            sub.copy(db->d_qvals, bow_vals, (size_t)nbow * 8, hipMemcpyHostToDevice);
            sub.copy(db->d_qn, &nbow, sizeof(int), hipMemcpyHostToDevice);
        }));
        list_of(db, 0, stride, limit, ret);
    }
    return finish_query(ret, max_results, ids, scores, cap, n_out);
}

// query_entries / query_probes: nq stored vectors -- entries, or probe slots -- as the queries of one launch
static int query_stored(mcorb_kfdb *db, bool probe, const char *who, const int32_t *sel, const int32_t *max_ids, int nq, int max_results,
                        uint32_t *ids, double *scores, int cap, int *n_out)
{
    TRY(check_db(db, who));
    if (nq < 0 || (nq && (!sel || !max_ids || !n_out)) || cap < 0 || (cap && (!ids || !scores))) { set_error(std::string(who) + ": bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    for (int q = 0; q < nq; q++) {
        n_out[q] = 0;
        TRY(probe ? check_probe(db, sel[q], who) : check_entry(db, sel[q], who));
    }
    if (nq == 0) return MCORB_OK;
    std::vector<Result> ret;
    std::vector<int> limit(nq);
    int status = MCORB_OK, stride = 1;
    if (db->device >= 0) {
        TRY(use_device(db->device));
        for (int q = 0; q < nq; q++) limit[q] = limit_of(max_ids[q], db->n);
        TRY(run_score(db, entry_bows(db), probe ? probe_bows(db) : entry_bows(db), sel, limit.data(), nullptr, nq, &stride));
    }
    for (int q = 0; q < nq; q++) {
        if (db->device < 0) {
            const HostEntry &h = probe ? db->probes[sel[q]] : db->entries[sel[q]];
            query_host(db, h.ids.data(), h.vals.data(), (int)h.ids.size(), max_ids[q], ret);
        } else {
            list_of(db, q, stride, limit[q], ret);
        }
        const int st = finish_query(ret, max_results, ids + (size_t)q * cap, scores + (size_t)q * cap, cap, n_out + q);
        if (st != MCORB_OK && status == MCORB_OK) status = st;
    }
    return status;
}

int mcorb_kfdb_query_entries(mcorb_kfdb *db, const int32_t *entries, const int32_t *max_ids, int nq, int max_results, uint32_t *ids,
                             double *scores, int cap, int *n_out)
{
    return query_stored(db, false, "kfdb query_entries", entries, max_ids, nq, max_results, ids, scores, cap, n_out);
}

// score / score_probe: TemplatedVocabulary::score of an entry's vector and another entry's, or a probe's
static int score_stored(mcorb_kfdb *db, int entry, int b, bool probe, const char *who, double *score)
{
    TRY(check_db(db, who));
    if (!score) { set_error(std::string(who) + ": bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_entry(db, entry, who));
    TRY(probe ? check_probe(db, b, who) : check_entry(db, b, who));
    if (db->device < 0) {
        *score = score_host(db->entries[entry], probe ? db->probes[b] : db->entries[b]);
        return MCORB_OK;
    }
    // the entry is the query, b's store the one it is held against
    TRY(use_device(db->device));
    const int one = 1;
    int stride = 1;
    TRY(run_score(db, probe ? probe_bows(db) : entry_bows(db), entry_bows(db), &entry, &one, &b, 1, &stride));
    *score = db->h_shared[0] > 0 ? -db->h_raw[0] / 2.0 : 0.0;
    return MCORB_OK;
}

int mcorb_kfdb_score(mcorb_kfdb *db, int entry_a, int entry_b, double *score)
{
    return score_stored(db, entry_a, entry_b, false, "kfdb score", score);
}

int mcorb_kfdb_feature_matches(mcorb_kfdb *db, int best_entry, int curr_entry, double max_neighbor_ratio, uint32_t *indices_1,
                               uint32_t *indices_2, int cap, int *n_out)
{
    if (n_out) *n_out = 0;
    TRY(check_db(db, "kfdb feature_matches"));
    if (cap < 0 || (cap && (!indices_1 || !indices_2))) { set_error("kfdb feature_matches: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_entry(db, best_entry, "kfdb feature_matches"));
    TRY(check_entry(db, curr_entry, "kfdb feature_matches"));
    std::vector<std::vector<uint32_t>> i1(1), i2(1);
    if (db->device < 0) {
        matches_host(db->entries[best_entry], db->entries[curr_entry], max_neighbor_ratio, i1[0], i2[0]);
    } else {
        TRY(use_device(db->device));
        const Mirror &A = db->mirror[best_entry];
        const Place pa = place_of(db, best_entry, false), pb = place_of(db, curr_entry, false);
        db->best2.reset();
        db->best2.add_b(A.nodes, A.offs, db->mirror[curr_entry], 0);
        TRY(db->best2.run(db->st, pa.desc, pa.feats, pb.desc, 0, pb.feats, 0, max_neighbor_ratio, i1, i2, &db->us_best2));
    }
    if (n_out) *n_out = (int)i1[0].size();
    if ((int)i1[0].size() > cap) { set_error("kfdb feature_matches: output too small"); return MCORB_E_CAP; }
    if (!i1[0].empty()) { memcpy(indices_1, i1[0].data(), i1[0].size() * 4); memcpy(indices_2, i2[0].data(), i2[0].size() * 4); }
    return MCORB_OK;
}

int mcorb_kfdb_last_timing(mcorb_kfdb *db, float us[2])
{
    TRY(check_db(db, "kfdb last_timing"));
    if (!us) { set_error("kfdb last_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    us[0] = db->score.us[0];
    us[1] = db->us_best2;
    return MCORB_OK;
}

// ---------------------------------------------------------------------------
// probe slots
// ---------------------------------------------------------------------------
int mcorb_kfdb_reserve_probes(mcorb_kfdb *db, int nprobes)
{
    TRY(check_db(db, "kfdb reserve_probes"));
    if (nprobes < 1 || nprobes > kMaxProbes) { set_error("kfdb reserve_probes: 1 .. 128 probe slots"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->nprobes) { set_error("kfdb reserve_probes: the probe slots are reserved already"); return MCORB_E_STATE; }
    if (db->device < 0) {
        db->probes.resize(nprobes);
    } else {
        HIPCHK(hipSetDevice(db->device));
        const size_t P = (size_t)nprobes, E = (size_t)db->max_entries, W = (size_t)db->max_words, F = (size_t)db->max_feats;
        const size_t set = (size_t)db->fstride * 32;
        TRY(db->p_ids.alloc(P * W));
        TRY(db->p_vals.alloc(P * W));
        TRY(db->p_nbow.alloc(P));
        TRY(db->p_nodes.alloc(P * F));
        TRY(db->p_offs.alloc(P * (F + 1)));
        TRY(db->p_feats.alloc(P * F));
        // the probe slots go behind the entries in the descriptor allocation: a larger one, the entries copied over
        DevBuf<uint8_t> desc;
        TRY(desc.alloc((E + P) * set));
        HIPCHK(hipStreamSynchronize(db->st));
        if (db->n) HIPCHK(hipMemcpy(desc, db->d_desc, (size_t)db->n * set, hipMemcpyDeviceToDevice));
        HIPCHK(hipStreamSynchronize(nullptr));
        db->d_desc = std::move(desc);
        db->pmirror.resize(nprobes);
    }
    db->probe_set.assign(nprobes, 0);
    db->nprobes = nprobes;
    return MCORB_OK;
}

int mcorb_kfdb_set_probe(mcorb_kfdb *db, int probe, const uint32_t *bow_ids, const double *bow_vals, int nbow, const uint32_t *fv_nodes,
                         const int32_t *fv_offsets, int nfv, const int32_t *fv_feats, const uint8_t *desc, int ndesc)
{
    TRY(check_db(db, "kfdb set_probe"));
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_probe(db, probe, "kfdb set_probe", false));
    if (nfv < 0 || (nfv && !fv_offsets) || (ndesc > 0 && !desc)) { set_error("kfdb set_probe: bad argument"); return MCORB_E_ARG; }
    const Vectors v{bow_ids, bow_vals, nbow, fv_nodes, fv_offsets, nfv, fv_feats, nfv ? fv_offsets[nfv] : 0};
    return put_frame(db, probe, v, desc, ndesc, nullptr, nullptr);
}

int mcorb_kfdb_set_probe_rig_frame(mcorb_kfdb *db, int probe, mcorb_rig *r, int slot, int frame)
{
    TRY(check_db(db, "kfdb set_probe_rig_frame"));
    Slot *s = nullptr;
    TRY(rig_frame_of(db, r, slot, frame, "kfdb set_probe_rig_frame", &s));
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_probe(db, probe, "kfdb set_probe_rig_frame", false));
    const LfFrameOut &o = s->lf[frame];
    return put_frame(db, probe, vectors_of(o), nullptr, (int)o.feats.size(), s, &o);
}

int mcorb_kfdb_get_probe(mcorb_kfdb *db, int probe, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow, uint32_t *fv_nodes,
                         int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap, uint8_t *desc, int desc_cap,
                         int *ndesc)
{
    TRY(check_db(db, "kfdb get_probe"));
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_probe(db, probe, "kfdb get_probe"));
    return get_frame(db, probe, true, "kfdb get_probe", bow_ids, bow_vals, bow_cap, nbow, fv_nodes, fv_offsets, fv_cap, nfv, fv_feats, feat_cap,
                     desc, desc_cap, ndesc);
}

int mcorb_kfdb_query_probes(mcorb_kfdb *db, const int32_t *probes, const int32_t *max_ids, int nq, int max_results, uint32_t *ids,
                            double *scores, int cap, int *n_out)
{
    return query_stored(db, true, "kfdb query_probes", probes, max_ids, nq, max_results, ids, scores, cap, n_out);
}

int mcorb_kfdb_score_probe(mcorb_kfdb *db, int entry, int probe, double *score)
{
    return score_stored(db, entry, probe, true, "kfdb score_probe", score);
}

int mcorb_kfdb_probe_feature_matches(mcorb_kfdb *db, int entry, const int32_t *probes, int np, double max_neighbor_ratio,
                                     uint32_t *indices_1, uint32_t *indices_2, int cap, int *n_out)
{
    TRY(check_db(db, "kfdb probe_feature_matches"));
    if (np < 0 || (np && (!probes || !n_out)) || cap < 0 || (cap && (!indices_1 || !indices_2))) {
        set_error("kfdb probe_feature_matches: bad argument");
        return MCORB_E_ARG;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_entry(db, entry, "kfdb probe_feature_matches"));
    for (int p = 0; p < np; p++) {
        n_out[p] = 0;
        TRY(check_probe(db, probes[p], "kfdb probe_feature_matches"));
    }
    if (np == 0) return MCORB_OK;
    std::vector<std::vector<uint32_t>> i1(np), i2(np);
    if (db->device < 0) {
        for (int p = 0; p < np; p++) matches_host(db->entries[entry], db->probes[probes[p]], max_neighbor_ratio, i1[p], i2[p]);
    } else {
        // the probe store as the B sets, probe by probe: the order the kernel's lanes share B rows in
        TRY(use_device(db->device));
        const Mirror &A = db->mirror[entry];
        const Place pa = place_of(db, entry, false), p0 = place_of(db, 0, true);
        db->best2.reset();
        for (int p = 0; p < np; p++) db->best2.add_b(A.nodes, A.offs, db->pmirror[probes[p]], probes[p]);
        TRY(db->best2.run(db->st, pa.desc, pa.feats, p0.desc, (size_t)db->fstride * 32, p0.feats, (size_t)db->max_feats, max_neighbor_ratio,
                          i1, i2, &db->us_best2p));
    }
    int status = MCORB_OK;
    for (int p = 0; p < np; p++) {
        n_out[p] = (int)i1[p].size();
        if ((int)i1[p].size() > cap) { set_error("kfdb probe_feature_matches: output too small"); status = MCORB_E_CAP; continue; }
        if (!i1[p].empty()) {
            memcpy(indices_1 + (size_t)p * cap, i1[p].data(), i1[p].size() * 4);
            memcpy(indices_2 + (size_t)p * cap, i2[p].data(), i2[p].size() * 4);
        }
    }
    return status;
}

// knnMatch(descs_prev, descs_cur, 2) of an entry's and a probe's descriptors: per query {trainIdx0, dist0, trainIdx1, dist1}, -1
// for an absent neighbour; BFMatcher's order, the lowest train index first among equal distances
static int knn2_frames(mcorb_kfdb *db, int entry, int probe, int na, int nb, std::vector<int4> &rows)
{
    rows.assign((size_t)na, int4{-1, -1, -1, -1});
    if (na == 0 || nb == 0) return MCORB_OK;
    if (db->device < 0) {
        const uint8_t *A = db->entries[entry].desc.data(), *B = db->probes[probe].desc.data();
        for (int q = 0; q < na; q++) {
            int4 r = int4{-1, 0x7fffffff, -1, 0x7fffffff};
            for (int t = 0; t < nb; t++) {
                const int d = mcorb_hamming256(A + (size_t)q * 32, B + (size_t)t * 32);
                if (d < r.y) { r.z = r.x; r.w = r.y; r.x = t; r.y = d; }
                else if (d < r.w) { r.z = t; r.w = d; }
            }
            if (r.z < 0) r.w = -1;
            rows[q] = r;
        }
        return MCORB_OK;
    }
    const int kc = db->fstride;
    if (kc > 65535) { set_error("kfdb probe_inter_matches_bf: max_feats above 65535 (the k-NN table's 16-bit train index)"); return MCORB_E_SIZE; }
    TRY(use_device(db->device));
    if (!db->h_rows.size()) {
        TRY(db->d_exp.alloc((size_t)2 * kc * kKnnExpandBytes));
        TRY(db->d_lcounts.alloc(2));
        TRY(db->d_part.alloc(knn_part_entries(1, kc)));
        TRY(db->h_knnctl.alloc(4, hipHostMallocMapped));
        TRY(db->h_mlist.alloc(knn_mlist_stride(kc), hipHostMallocMapped));
        TRY(db->h_mcount.alloc((size_t)knn_qblocks(kc), hipHostMallocMapped));
        TRY(db->h_rows.alloc((size_t)kc, hipHostMallocMapped));
    }
    db->h_knnctl[0] = entry;                        // setmap: the two sets of d_desc that become local sets 0 and 1
    db->h_knnctl[1] = db->max_entries + probe;
    db->h_knnctl[2] = 0;                            // the pair (query, train)
    db->h_knnctl[3] = 1;
    Submission sub(db->st);
    sub.run([&] {
        launch_knn2(db->st, db->d_desc, db->d_ndesc, db->h_knnctl, 2, reinterpret_cast<const int2 *>(db->h_knnctl + 2), 1, kc, db->d_exp,
                    db->d_lcounts, db->d_part, 75.f, 0.85f, db->h_rows, db->h_mlist, db->h_mcount, nullptr, nullptr);   // (the accept flag is not read)
    });
    TRY(sub.wait());
    for (int q = 0; q < na; q++) {
        const KnnRow &k = db->h_rows[q];
        rows[q] = int4{knn_idx0(k), knn_d0(k), knn_idx1(k), knn_d1(k)};
    }
    return MCORB_OK;
}

int mcorb_kfdb_probe_inter_matches_bf(mcorb_kfdb *db, int entry, int probe, const int32_t *lids_prev, const uint8_t *mono_prev,
                                      const double *p3d_prev, const uint8_t *mono_cur, const double *p3d_cur, int32_t *query_idx,
                                      int32_t *train_idx, int32_t *dist, int cap, int *n_out)
{
    if (n_out) *n_out = 0;
    TRY(check_db(db, "kfdb probe_inter_matches_bf"));
    if (cap < 0 || (cap && (!query_idx || !train_idx || !dist))) { set_error("kfdb probe_inter_matches_bf: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_entry(db, entry, "kfdb probe_inter_matches_bf"));
    TRY(check_probe(db, probe, "kfdb probe_inter_matches_bf"));
    const int na = db->device < 0 ? (int)(db->entries[entry].desc.size() / 32) : db->mirror[entry].ndesc;
    const int nb = db->device < 0 ? (int)(db->probes[probe].desc.size() / 32) : db->pmirror[probe].ndesc;
    if ((na && (!lids_prev || !mono_prev || !p3d_prev)) || (nb && (!mono_cur || !p3d_cur))) {
        set_error("kfdb probe_inter_matches_bf: bad argument");
        return MCORB_E_ARG;
    }
    std::vector<int4> rows;
    TRY(knn2_frames(db, entry, probe, na, nb, rows));
    // `for (auto &m : matches)` of findInterMatches (FrontEnd.cpp:3392-3465)
    std::vector<int> inds1, inds2, dists;
    for (int q = 0; q < na; q++) {
        const int4 m = rows[q];   // {m[0].trainIdx, m[0].distance, m[1].trainIdx, m[1].distance}
        if (m.x < 0) continue;
        if (lids_prev[q] == -1) {
            if (m.z < 0) continue;   // (no second neighbour: the reference reads past m's end)
            if ((double)(float)m.y > 0.7 * (double)(float)m.w) continue;
        }
        const int t = m.x;
        if (!mono_prev[q] && !mono_cur[t]) {
            const double dx = p3d_prev[3 * (size_t)q] - p3d_cur[3 * (size_t)t], dy = p3d_prev[3 * (size_t)q + 1] - p3d_cur[3 * (size_t)t + 1],
                         dz = p3d_prev[3 * (size_t)q + 2] - p3d_cur[3 * (size_t)t + 2];
            const float distance = (float)sqrt(dx * dx + dy * dy + dz * dz);   // cv::norm of the 3x1 CV_64F difference
            if (!(distance <= 2.0)) continue;
        }
        const auto it = std::find(inds2.begin(), inds2.end(), t);
        if (it == inds2.end()) {
            inds2.push_back(t);
            inds1.push_back(q);
            dists.push_back(m.y);
        } else {
            const size_t k = it - inds2.begin();
            if (m.y < dists[k]) { inds1[k] = q; dists[k] = m.y; }
        }
    }
    if (n_out) *n_out = (int)inds1.size();
    if ((int)inds1.size() > cap) { set_error("kfdb probe_inter_matches_bf: output too small"); return MCORB_E_CAP; }
    for (size_t k = 0; k < inds1.size(); k++) { query_idx[k] = inds1[k]; train_idx[k] = inds2[k]; dist[k] = dists[k]; }
    return MCORB_OK;
}

int mcorb_kfdb_last_probe_timing(mcorb_kfdb *db, float *us)
{
    TRY(check_db(db, "kfdb last_probe_timing"));
    if (!us) { set_error("kfdb last_probe_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    *us = db->us_best2p;
    return MCORB_OK;
}

}  // extern "C"
