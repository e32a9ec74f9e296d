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
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "mcorb_engine.h"

using namespace mcorb;

namespace {

constexpr int TH_LOW = 75;   // ORBextractor.h:27

struct Result {   // DBoW2::Result: ordered by score alone
    uint32_t id;
    double score;
    bool operator<(const Result &r) const { return score < r.score; }
};

// one stored keyframe of the host-only database
struct HostEntry {
    std::vector<uint32_t> ids, nodes;
    std::vector<double> vals;
    std::vector<int32_t> offs, feats;
    std::vector<uint8_t> desc;
};

// what the host keeps of an entry of the device database: the counts, and the FeatureVector's node ids and offsets (short: the
// shared-node list of featureMatchesBow is built from them)
struct Mirror {
    int nbow = 0, nfv = 0, nff = 0, ndesc = 0;
    std::vector<uint32_t> nodes;
    std::vector<int32_t> offs;
};

struct Vectors {   // a keyframe's vectors in mcorb_vocab_transform's layout
    const uint32_t *bow_ids; const double *bow_vals; int nbow;
    const uint32_t *fv_nodes; const int32_t *fv_offsets; int nfv;
    const int32_t *fv_feats;
    int nff;   // fv_offsets[nfv]
};

}  // namespace

struct mcorb_kfdb {
    int device = -1, max_entries = 0, max_words = 0, max_feats = 0;
    int n = 0;
    std::mutex mu;   // one call at a time: the scratch below is the database's
    // host-only database
    std::vector<HostEntry> entries;
    std::map<uint32_t, std::vector<std::pair<uint32_t, double>>> ifile;   // word -> (entry, value), entries ascending
    // device database: the store, strided per entry
    Stream st;
    Event ev0, ev1;
    DevBuf<uint32_t> d_ids, d_nodes;     // [max_words], [max_feats]
    DevBuf<double> d_vals;               // [max_words]
    DevBuf<int> d_nbow;                  // one per entry
    DevBuf<int> d_offs, d_feats;         // [max_feats + 1], [max_feats]
    DevBuf<uint8_t> d_desc;              // [max_feats][32]
    std::vector<Mirror> mirror;
    // a host query vector's place on the device (one entry's stride), the control arrays and results of a launch (grow-only)
    DevBuf<uint32_t> d_qids;
    DevBuf<double> d_qvals;
    DevBuf<int> d_qn, d_ctl, d_shared, d_src;
    DevBuf<double> d_raw;
    HostBuf<double> h_raw;
    HostBuf<int> h_shared;
    DevBuf<int2> d_items, d_mnodes;
    DevBuf<int4> d_mtab;
    HostBuf<int4> h_mtab;
    float us_score = 0.f, us_best2 = 0.f;   // the last launch of each kernel, between HIP events
};

static int check_vectors(const mcorb_kfdb *db, const Vectors &v, int ndesc)
{
    if (v.nbow < 0 || v.nfv < 0 || ndesc < 0 || (v.nbow && (!v.bow_ids || !v.bow_vals)) || (v.nfv && (!v.fv_nodes || !v.fv_offsets))) {
        set_error("kfdb add: bad argument");
        return MCORB_E_ARG;
    }
    if (db->n >= db->max_entries) { set_error("kfdb add: the database is full (max_entries)"); return MCORB_E_CAP; }
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

// the entry's BowVector and FeatureVector to its place in the store, on `st` (the descriptors are the caller's)
static int store_vectors(mcorb_kfdb *db, int e, const Vectors &v, hipStream_t st)
{
    const size_t W = (size_t)db->max_words, F = (size_t)db->max_feats;
    if (v.nbow) {
        HIPCHK(hipMemcpyAsync(db->d_ids + e * W, v.bow_ids, (size_t)v.nbow * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(db->d_vals + e * W, v.bow_vals, (size_t)v.nbow * 8, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(db->d_nbow + e, &v.nbow, sizeof(int), hipMemcpyHostToDevice, st));
    if (v.nfv) {
        HIPCHK(hipMemcpyAsync(db->d_nodes + e * F, v.fv_nodes, (size_t)v.nfv * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(db->d_offs + e * (F + 1), v.fv_offsets, (size_t)(v.nfv + 1) * 4, hipMemcpyHostToDevice, st));
    }
    if (v.nff) HIPCHK(hipMemcpyAsync(db->d_feats + e * F, v.fv_feats, (size_t)v.nff * 4, hipMemcpyHostToDevice, st));
    return MCORB_OK;
}

static void commit_mirror(mcorb_kfdb *db, const Vectors &v, int ndesc)
{
    Mirror m;
    m.nbow = v.nbow; m.nfv = v.nfv; m.nff = v.nff; m.ndesc = ndesc;
    m.nodes.assign(v.fv_nodes, v.fv_nodes + v.nfv);
    if (v.nfv) m.offs.assign(v.fv_offsets, v.fv_offsets + v.nfv + 1);
    else m.offs.assign(1, 0);
    db->mirror.push_back(std::move(m));
    db->n++;
}

static void add_host(mcorb_kfdb *db, const Vectors &v, const uint8_t *desc, int ndesc)
{
    HostEntry h;
    h.ids.assign(v.bow_ids, v.bow_ids + v.nbow);
    h.vals.assign(v.bow_vals, v.bow_vals + v.nbow);
    h.nodes.assign(v.fv_nodes, v.fv_nodes + v.nfv);
    if (v.nfv) h.offs.assign(v.fv_offsets, v.fv_offsets + v.nfv + 1);
    else h.offs.assign(1, 0);
    h.feats.assign(v.fv_feats, v.fv_feats + v.nff);
    h.desc.assign(desc, desc + (size_t)ndesc * 32);
    const uint32_t e = (uint32_t)db->n;   // EntryId entry_id = m_nentries++
    for (int i = 0; i < v.nbow; i++) db->ifile[v.bow_ids[i]].emplace_back(e, v.bow_vals[i]);   // m_ifile[word_id].push_back(IFPair(entry_id, word_weight))
    db->entries.push_back(std::move(h));
    db->n++;
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

// k_kfdb_score for nq queries; sel[q]: the entry that is the query, or -1 for the vector uploaded to the scratch place.  With
// against != nullptr query q is held against the single entry against[q] instead of the entries below its limit.  raw / shared of
// (q, x) land at h_raw / h_shared[q * stride_out + x].
static int run_score(mcorb_kfdb *db, const int *sel, const int *limit, const int *against, int nq, int *stride_out)
{
    const int os = std::max(against ? 1 : db->n, 1);
    *stride_out = os;
    int max_limit = 0;
    for (int q = 0; q < nq; q++) max_limit = std::max(max_limit, limit[q]);
    if (max_limit < 1) return MCORB_OK;
    const bool scratch = sel[0] < 0;   // (a host query is one query per call)
    std::vector<int> ctl((size_t)nq * 2 + (against ? nq : 0));
    for (int q = 0; q < nq; q++) {
        ctl[q] = scratch ? 0 : sel[q];
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
    HIPCHK(hipMemcpyAsync(db->d_ctl, ctl.data(), ctl.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(db->ev0, st));
    launch_kfdb_score(st, db->d_ids, db->d_vals, db->d_nbow, db->max_words, scratch ? db->d_qids.get() : db->d_ids.get(),
                      scratch ? db->d_qvals.get() : db->d_vals.get(), scratch ? db->d_qn.get() : db->d_nbow.get(), db->d_ctl,
                      db->d_ctl + nq, against ? db->d_ctl + 2 * (size_t)nq : nullptr, nq, max_limit, os, db->d_raw, db->d_shared);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(db->ev1, st));
    HIPCHK(hipMemcpyAsync(db->h_raw, db->d_raw, nout * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(db->h_shared, db->d_shared, nout * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // (also covers the pageable control array)
    float ms = 0.f;
    ev_elapsed(&ms, db->ev0, db->ev1);
    db->us_score = ms * 1000.f;
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

// getMatches_distRatio's acceptance and one-to-one bookkeeping (ORBextractor.cpp:1264-1287) for one A feature of a call whose
// lists so far are mA / mB; mD: the best distance each holder was accepted with = DescriptorDistance(A[holder], B[idx_B])
static void accept(double best_dist_1, double best_dist_2, uint32_t idx_A, uint32_t idx_B, double max_neighbor_ratio,
                   std::vector<uint32_t> &mA, std::vector<uint32_t> &mB, std::vector<double> &mD)
{
    if (best_dist_1 <= TH_LOW) {
        if (best_dist_1 / best_dist_2 <= max_neighbor_ratio) {
            const auto bit = std::find(mB.begin(), mB.end(), idx_B);
            if (bit == mB.end()) {
                mB.push_back(idx_B);
                mA.push_back(idx_A);
                mD.push_back(best_dist_1);
            } else {
                const size_t k = bit - mB.begin();
                if (best_dist_1 < mD[k]) { mA[k] = idx_A; mD[k] = best_dist_1; }
            }
        }
    }
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
    if (device >= 0) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { set_error("kfdb create: no such HIP device"); return MCORB_E_NODEVICE; }
        HIPCHK(hipSetDevice(device));
        const size_t E = (size_t)max_entries, W = (size_t)max_words, F = (size_t)max_feats;
        TRY(db->st.create(hipStreamNonBlocking));
        TRY(db->ev0.create(hipEventDefault));
        TRY(db->ev1.create(hipEventDefault));
        TRY(db->d_ids.alloc(E * W));
        TRY(db->d_vals.alloc(E * W));
        TRY(db->d_nbow.alloc(E));
        TRY(db->d_nodes.alloc(E * F));
        TRY(db->d_offs.alloc(E * (F + 1)));
        TRY(db->d_feats.alloc(E * F));
        TRY(db->d_desc.alloc(E * F * 32));
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
    TRY(check_vectors(db, v, ndesc));
    const int e = db->n;
    if (db->device < 0) {
        add_host(db, v, desc, ndesc);
    } else {
        HIPCHK(hipSetDevice(db->device));
        TRY(store_vectors(db, e, v, db->st));
        if (ndesc) HIPCHK(hipMemcpyAsync(db->d_desc + (size_t)e * db->max_feats * 32, desc, (size_t)ndesc * 32, hipMemcpyHostToDevice, db->st));
        HIPCHK(hipStreamSynchronize(db->st));
        commit_mirror(db, v, ndesc);
    }
    if (entry_out) *entry_out = e;
    return MCORB_OK;
}

int mcorb_kfdb_add_rig_frame(mcorb_kfdb *db, mcorb_rig *r, int slot, int frame, int *entry_out)
{
    TRY(check_db(db, "kfdb add_rig_frame"));
    if (!r || slot < 0 || slot >= (int)r->rig.slots.size()) { set_error("kfdb add_rig_frame: bad argument"); return MCORB_E_ARG; }
    Rig &R = r->rig;
    Slot *s = R.slots[slot].get();
    {
        std::lock_guard<std::mutex> lk(s->m);
        if (s->busy) { set_error("slot busy"); return MCORB_E_STATE; }
    }
    if (frame < 0 || frame >= (int)s->lf_ok.size() || !s->lf_ok[frame]) {
        set_error("kfdb add_rig_frame: frame not processed by the LF stage since the slot's last extraction");
        return MCORB_E_STATE;
    }
    if (db->device >= 0 && db->device != R.device) { set_error("kfdb add_rig_frame: the rig lives on another device"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    const LfFrameOut &o = s->lf[frame];
    const BowImageOut &b = o.bow;
    const int ndesc = (int)o.feats.size(), nfv = (int)b.fv_nodes.size();
    const Vectors v{b.bow_ids.data(), b.bow_vals.data(), (int)b.bow_ids.size(), b.fv_nodes.data(), b.fv_offsets.data(), nfv,
                    b.fv_feats.data(), (int)b.fv_feats.size()};
    TRY(check_vectors(db, v, ndesc));
    const int e = db->n;
    if (db->device < 0) {
        std::vector<uint8_t> desc((size_t)ndesc * 32);
        for (int i = 0; i < ndesc; i++) memcpy(desc.data() + (size_t)i * 32, o.feats[i].desc, 32);
        add_host(db, v, desc.data(), ndesc);
    } else {
        // lfBoW and lfFeatVec are assembled on the host (lf_job_finish): they are uploaded.  The LF descriptors are rows of the
        // slot's descriptor block in HBM (LfFrameOut::src): gathered device to device, on the slot's stream.
        HIPCHK(hipSetDevice(db->device));
        TRY(store_vectors(db, e, v, s->st));
        if (ndesc) {
            TRY(db->d_src.grow((size_t)db->max_feats));
            HIPCHK(hipMemcpyAsync(db->d_src, o.src.data(), (size_t)ndesc * sizeof(int), hipMemcpyHostToDevice, s->st));
            launch_kfdb_gather(s->st, s->d_desc, db->d_src, ndesc, db->d_desc + (size_t)e * db->max_feats * 32);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(s->st));
        commit_mirror(db, v, ndesc);
    }
    if (entry_out) *entry_out = e;
    return MCORB_OK;
}

int mcorb_kfdb_get_entry(mcorb_kfdb *db, int entry, uint32_t *bow_ids, double *bow_vals, int bow_cap, int *nbow, uint32_t *fv_nodes,
                         int32_t *fv_offsets, int fv_cap, int *nfv, int32_t *fv_feats, int feat_cap, uint8_t *desc, int desc_cap,
                         int *ndesc)
{
    TRY(check_db(db, "kfdb get_entry"));
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_entry(db, entry, "kfdb get_entry"));
    int c_bow, c_fv, c_ff, c_desc;
    if (db->device < 0) {
        const HostEntry &h = db->entries[entry];
        c_bow = (int)h.ids.size(); c_fv = (int)h.nodes.size(); c_ff = (int)h.feats.size(); c_desc = (int)(h.desc.size() / 32);
    } else {
        const Mirror &m = db->mirror[entry];
        c_bow = m.nbow; c_fv = m.nfv; c_ff = m.nff; c_desc = m.ndesc;
    }
    if (nbow) *nbow = c_bow;
    if (nfv) *nfv = c_fv;
    if (ndesc) *ndesc = c_desc;
    if (c_bow > bow_cap || c_fv > fv_cap || c_ff > feat_cap || c_desc > desc_cap) { set_error("kfdb get_entry: output too small"); return MCORB_E_CAP; }
    if (!fv_offsets || (c_bow && (!bow_ids || !bow_vals)) || (c_fv && !fv_nodes) || (c_ff && !fv_feats) || (c_desc && !desc)) {
        set_error("kfdb get_entry: bad argument");
        return MCORB_E_ARG;
    }
    if (db->device < 0) {
        const HostEntry &h = db->entries[entry];
        if (c_bow) { memcpy(bow_ids, h.ids.data(), (size_t)c_bow * 4); memcpy(bow_vals, h.vals.data(), (size_t)c_bow * 8); }
        if (c_fv) memcpy(fv_nodes, h.nodes.data(), (size_t)c_fv * 4);
        memcpy(fv_offsets, h.offs.data(), h.offs.size() * 4);
        if (c_ff) memcpy(fv_feats, h.feats.data(), (size_t)c_ff * 4);
        if (c_desc) memcpy(desc, h.desc.data(), (size_t)c_desc * 32);
        return MCORB_OK;
    }
    HIPCHK(hipSetDevice(db->device));
    const size_t e = (size_t)entry, W = (size_t)db->max_words, F = (size_t)db->max_feats;
    fv_offsets[0] = 0;
    if (c_bow) {
        HIPCHK(hipMemcpy(bow_ids, db->d_ids + e * W, (size_t)c_bow * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(bow_vals, db->d_vals + e * W, (size_t)c_bow * 8, hipMemcpyDeviceToHost));
    }
    if (c_fv) {
        HIPCHK(hipMemcpy(fv_nodes, db->d_nodes + e * F, (size_t)c_fv * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(fv_offsets, db->d_offs + e * (F + 1), (size_t)(c_fv + 1) * 4, hipMemcpyDeviceToHost));
    }
    if (c_ff) HIPCHK(hipMemcpy(fv_feats, db->d_feats + e * F, (size_t)c_ff * 4, hipMemcpyDeviceToHost));
    if (c_desc) HIPCHK(hipMemcpy(desc, db->d_desc + e * F * 32, (size_t)c_desc * 32, hipMemcpyDeviceToHost));
    return MCORB_OK;
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
        HIPCHK(hipSetDevice(db->device));
        HIPCHK(hipMemcpyAsync(db->d_qids, bow_ids, (size_t)nbow * 4, hipMemcpyHostToDevice, db->st));
        HIPCHK(hipMemcpyAsync(db->d_qvals, bow_vals, (size_t)nbow * 8, hipMemcpyHostToDevice, db->st));
        HIPCHK(hipMemcpyAsync(db->d_qn, &nbow, sizeof(int), hipMemcpyHostToDevice, db->st));
        const int sel = -1;
        int stride = 1;
        TRY(run_score(db, &sel, &limit, nullptr, 1, &stride));
        list_of(db, 0, stride, limit, ret);
    }
    return finish_query(ret, max_results, ids, scores, cap, n_out);
}

int mcorb_kfdb_query_entries(mcorb_kfdb *db, const int32_t *entries, const int32_t *max_ids, int nq, int max_results, uint32_t *ids,
                             double *scores, int cap, int *n_out)
{
    TRY(check_db(db, "kfdb query_entries"));
    if (nq < 0 || (nq && (!entries || !max_ids || !n_out)) || cap < 0 || (cap && (!ids || !scores))) { set_error("kfdb query_entries: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    for (int q = 0; q < nq; q++) {
        n_out[q] = 0;
        TRY(check_entry(db, entries[q], "kfdb query_entries"));
    }
    if (nq == 0) return MCORB_OK;
    std::vector<Result> ret;
    int status = MCORB_OK;
    if (db->device < 0) {
        for (int q = 0; q < nq; q++) {
            const HostEntry &h = db->entries[entries[q]];
            query_host(db, h.ids.data(), h.vals.data(), (int)h.ids.size(), max_ids[q], ret);
            const int st = finish_query(ret, max_results, ids + (size_t)q * cap, scores + (size_t)q * cap, cap, n_out + q);
            if (st != MCORB_OK && status == MCORB_OK) status = st;
        }
        return status;
    }
    HIPCHK(hipSetDevice(db->device));
    std::vector<int> limit(nq);
    for (int q = 0; q < nq; q++) limit[q] = limit_of(max_ids[q], db->n);
    int stride = 1;
    TRY(run_score(db, entries, limit.data(), nullptr, nq, &stride));
    for (int q = 0; q < nq; q++) {
        list_of(db, q, stride, limit[q], ret);
        const int st = finish_query(ret, max_results, ids + (size_t)q * cap, scores + (size_t)q * cap, cap, n_out + q);
        if (st != MCORB_OK && status == MCORB_OK) status = st;
    }
    return status;
}

int mcorb_kfdb_score(mcorb_kfdb *db, int entry_a, int entry_b, double *score)
{
    TRY(check_db(db, "kfdb score"));
    if (!score) { set_error("kfdb score: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    TRY(check_entry(db, entry_a, "kfdb score"));
    TRY(check_entry(db, entry_b, "kfdb score"));
    if (db->device < 0) {
        // L1Scoring::score: a merge walk over the two sorted vectors
        const HostEntry &a = db->entries[entry_a], &b = db->entries[entry_b];
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
        *score = -s / 2.0;
        return MCORB_OK;
    }
    HIPCHK(hipSetDevice(db->device));
    const int one = 1;
    int stride = 1;
    TRY(run_score(db, &entry_a, &one, &entry_b, 1, &stride));
    *score = db->h_shared[0] > 0 ? -db->h_raw[0] / 2.0 : 0.0;
    return MCORB_OK;
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
    std::vector<uint32_t> i1, i2, mA, mB;
    std::vector<double> mD;
    if (db->device < 0) {
        // LoopCloser::featureMatchesBow (:217-240) calling the literal getMatches_distRatio (ORBextractor.cpp:1228-1290)
        const HostEntry &A = db->entries[best_entry], &B = db->entries[curr_entry];
        size_t ia = 0, ib = 0;
        while (ia < A.nodes.size() && ib < B.nodes.size()) {
            if (A.nodes[ia] == B.nodes[ib]) {
                mA.clear(); mB.clear(); mD.clear();
                for (int a = A.offs[ia]; a < A.offs[ia + 1]; a++) {
                    int best_j_now = -1;
                    double best_dist_1 = 1e9, best_dist_2 = 1e9;
                    for (int j = B.offs[ib]; j < B.offs[ib + 1]; j++) {
                        const double d = mcorb_hamming256(A.desc.data() + (size_t)A.feats[a] * 32, B.desc.data() + (size_t)B.feats[j] * 32);
                        if (d < best_dist_1) { best_j_now = j; best_dist_2 = best_dist_1; best_dist_1 = d; }
                        else if (d < best_dist_2) best_dist_2 = d;
                    }
                    if (best_dist_1 <= TH_LOW && best_dist_1 / best_dist_2 <= max_neighbor_ratio) {
                        const uint32_t idx_B = (uint32_t)B.feats[best_j_now];
                        const auto bit = std::find(mB.begin(), mB.end(), idx_B);
                        if (bit == mB.end()) {
                            mB.push_back(idx_B);
                            mA.push_back((uint32_t)A.feats[a]);
                        } else {
                            const uint32_t idx_A = mA[bit - mB.begin()];
                            const double d = mcorb_hamming256(A.desc.data() + (size_t)idx_A * 32, B.desc.data() + (size_t)idx_B * 32);
                            if (best_dist_1 < d) mA[bit - mB.begin()] = (uint32_t)A.feats[a];
                        }
                    }
                }
                i1.insert(i1.end(), mA.begin(), mA.end());
                i2.insert(i2.end(), mB.begin(), mB.end());
                ++ia; ++ib;
            } else if (A.nodes[ia] < B.nodes[ib]) {
                ia = std::lower_bound(A.nodes.begin() + ia, A.nodes.end(), B.nodes[ib]) - A.nodes.begin();
            } else {
                ib = std::lower_bound(B.nodes.begin() + ib, B.nodes.end(), A.nodes[ia]) - B.nodes.begin();
            }
        }
    } else {
        // the shared nodes in ascending id from the host's copy of the two node lists; one item per A feature of a shared node
        const Mirror &A = db->mirror[best_entry], &B = db->mirror[curr_entry];
        std::vector<int2> items, nodes;
        std::vector<int> first;   // per shared node: its first item
        size_t ia = 0, ib = 0;
        while (ia < A.nodes.size() && ib < B.nodes.size()) {
            if (A.nodes[ia] == B.nodes[ib]) {
                first.push_back((int)items.size());
                for (int a = A.offs[ia]; a < A.offs[ia + 1]; a++) items.push_back(int2{a, (int)nodes.size()});
                nodes.push_back(int2{B.offs[ib], B.offs[ib + 1] - B.offs[ib]});
                ++ia; ++ib;
            } else if (A.nodes[ia] < B.nodes[ib]) ++ia;
            else ++ib;
        }
        first.push_back((int)items.size());
        const int nitems = (int)items.size();
        if (nitems) {
            HIPCHK(hipSetDevice(db->device));
            TRY(db->d_items.grow(items.size()));
            TRY(db->d_mnodes.grow(nodes.size()));
            TRY(db->d_mtab.grow(items.size()));
            TRY(db->h_mtab.grow(items.size(), hipHostMallocDefault));
            hipStream_t st = db->st;
            const size_t F = (size_t)db->max_feats;
            HIPCHK(hipMemcpyAsync(db->d_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(db->d_mnodes, nodes.data(), nodes.size() * sizeof(int2), hipMemcpyHostToDevice, st));
            HIPCHK(hipEventRecord(db->ev0, st));
            launch_kfdb_best2(st, db->d_desc + best_entry * F * 32, db->d_feats + best_entry * F, db->d_desc + curr_entry * F * 32,
                              db->d_feats + curr_entry * F, db->d_items, nitems, db->d_mnodes, db->d_mtab);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(db->ev1, st));
            HIPCHK(hipMemcpyAsync(db->h_mtab, db->d_mtab, items.size() * sizeof(int4), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            float ms = 0.f;
            ev_elapsed(&ms, db->ev0, db->ev1);
            db->us_best2 = ms * 1000.f;
            for (size_t k = 0; k + 1 < first.size(); k++) {
                mA.clear(); mB.clear(); mD.clear();
                for (int i = first[k]; i < first[k + 1]; i++) {
                    const int4 t = db->h_mtab[i];   // {B feature of the best or -1, best, second, A feature}
                    if (t.x < 0) continue;          // an empty B list: best_dist_1 stays 1e9
                    accept((double)t.y, t.z == 0x7fffffff ? 1e9 : (double)t.z, (uint32_t)t.w, (uint32_t)t.x, max_neighbor_ratio, mA, mB, mD);
                }
                i1.insert(i1.end(), mA.begin(), mA.end());
                i2.insert(i2.end(), mB.begin(), mB.end());
            }
        }
    }
    if (n_out) *n_out = (int)i1.size();
    if ((int)i1.size() > cap) { set_error("kfdb feature_matches: output too small"); return MCORB_E_CAP; }
    if (!i1.empty()) { memcpy(indices_1, i1.data(), i1.size() * 4); memcpy(indices_2, i2.data(), i2.size() * 4); }
    return MCORB_OK;
}

int mcorb_kfdb_last_timing(mcorb_kfdb *db, float us[2])
{
    TRY(check_db(db, "kfdb last_timing"));
    if (!us) { set_error("kfdb last_timing: bad argument"); return MCORB_E_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    us[0] = db->us_score;
    us[1] = db->us_best2;
    return MCORB_OK;
}

}  // extern "C"
