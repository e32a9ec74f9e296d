// mcorb_kfdb_store.h -- the keyframe database object and the pieces of mcorb_kfdb.cpp that the local map (mcorb_lmap.cpp) also
// uses: a stored frame on the host (HostEntry) and on the device (Mirror, Place), the probe-slot check, and getMatches_distRatio --
// the literal loop of the host-only database (matches_host), and the device's: k_kfdb_best2 over the shared nodes and the
// acceptance that follows it (Best2Search, accept).
#pragma once
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "mcorb_engine.h"

namespace mcorb {

constexpr int TH_LOW = 75;   // ORBextractor.h:27

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

// getMatches_distRatio of frame A against one or more frames B over the nodes their FeatureVectors share, on the device: what
// mcorb_kfdb_feature_matches, mcorb_kfdb_probe_feature_matches and mcorb_lmap_search run.  reset(), add_b() per B, run().  The
// scratch is the owner's: one search at a time.
struct Best2Search {
    DevBuf<int2> d_items;
    DevBuf<int4> d_recs, d_mtab;   // (grow-only, like h_mtab)
    HostBuf<int4> h_mtab;
    Spans<1> launch;                           // around k_kfdb_best2
    std::vector<int2> items;                   // {position in A's feature list, record}, B by B and node by node
    std::vector<int4> recs;                    // a node A shares with a B: {B's set, first position, count, -} in B's feature list
    std::vector<int> first_item, first_rec;    // per record: its first item; per B: its first record

    int create();   // (the events; the device is current)
    void reset();
    // the nodes that A (ascending node ids, offsets into its feature list) shares with B, whose rows are set `set` of the B store
    void add_b(const std::vector<uint32_t> &a_nodes, const std::vector<int32_t> &a_offs, const Mirror &B, int set);
    // One upload, one k_kfdb_best2 launch on st (none without items), one copy back, one synchronisation; then the acceptance
    // record by record.  desc_a / feats_a: A's rows and feature list; desc_b / feats_b: set 0 of the B store, its sets desc_stride
    // bytes and feats_stride ints apart.  i1[b] / i2[b]: the matches of the b-th B; *us: the launch between the events, if any.
    // before: what the caller queues in front of the upload (mcorb_lmap_search's feature list), behind the grows; NOT called
    // without items, where nothing is queued.
    int run(hipStream_t st, const uint8_t *desc_a, const int *feats_a, const uint8_t *desc_b, size_t desc_stride, const int *feats_b,
            size_t feats_stride, double max_neighbor_ratio, std::vector<std::vector<uint32_t>> &i1,
            std::vector<std::vector<uint32_t>> &i2, float *us, const Pieces &before = nullptr);
};

}  // namespace mcorb

struct mcorb_kfdb {
    int device = -1, max_entries = 0, max_words = 0, max_feats = 0;
    int n = 0;
    int nprobes = 0;   // 0: mcorb_kfdb_reserve_probes has not run
    int fstride = 0;   // descriptor rows per set in d_desc: max_feats rounded up to launch_knn2's multiple of 64
    std::vector<char> probe_set;
    std::mutex mu;   // one call at a time: the scratch below is the database's
    // host-only database
    std::vector<mcorb::HostEntry> entries;
    std::map<uint32_t, std::vector<std::pair<uint32_t, double>>> ifile;   // word -> (entry, value), entries ascending
    std::vector<mcorb::HostEntry> probes;
    // device database: the store, strided per entry
    mcorb::Stream st;
    mcorb::Spans<1> score;                      // around the scoring kernel of a query
    mcorb::DevBuf<uint32_t> d_ids, d_nodes;     // [max_words], [max_feats]
    mcorb::DevBuf<double> d_vals;               // [max_words]
    mcorb::DevBuf<int> d_nbow;                  // one per entry
    mcorb::DevBuf<int> d_offs, d_feats;         // [max_feats + 1], [max_feats]
    mcorb::DevBuf<uint8_t> d_desc;              // [fstride][32]: the entries, then the probe slots
    mcorb::DevBuf<int> d_ndesc;                 // descriptors of each set of d_desc (launch_knn2's counts)
    std::vector<mcorb::Mirror> mirror;
    // the probe store: the entries' strides
    mcorb::DevBuf<uint32_t> p_ids, p_nodes;
    mcorb::DevBuf<double> p_vals;
    mcorb::DevBuf<int> p_nbow, p_offs, p_feats;
    std::vector<mcorb::Mirror> pmirror;
    // a host query vector's place on the device (one entry's stride), the control arrays and results of a launch (grow-only)
    mcorb::DevBuf<uint32_t> d_qids;
    mcorb::DevBuf<double> d_qvals;
    mcorb::DevBuf<int> d_qn, d_ctl, d_shared, d_src;
    mcorb::DevBuf<double> d_raw;
    mcorb::HostBuf<double> h_raw;
    mcorb::HostBuf<int> h_shared;
    mcorb::Best2Search best2;
    // launch_knn2's scratch for one (entry, probe) pair at capacity fstride; the control words and results are host-mapped
    mcorb::DevBuf<uint8_t> d_exp;
    mcorb::DevBuf<int> d_lcounts;
    mcorb::DevBuf<uint2> d_part;
    mcorb::HostBuf<int> h_knnctl, h_mcount;     // {setmap[2], pair}
    mcorb::HostBuf<mcorb::KnnRow> h_rows;
    mcorb::HostBuf<uint32_t> h_mlist;
    float us_best2 = 0.f, us_best2p = 0.f;      // the last k_kfdb_best2 launch of a feature-match call and of a probe call
};

namespace mcorb {

// a frame's rows in the device store: entry e, or probe slot e (whose descriptors lie behind the entries')
struct Place {
    uint32_t *ids; double *vals; int *nbow;
    uint32_t *nodes; int *offs, *feats;
    uint8_t *desc; int *ndesc;
};

inline Place place_of(const mcorb_kfdb *db, int e, bool probe)
{
    const size_t i = (size_t)e, W = (size_t)db->max_words, F = (size_t)db->max_feats;
    const size_t set = probe ? (size_t)db->max_entries + i : i;
    if (probe)
        return Place{db->p_ids + i * W, db->p_vals + i * W, db->p_nbow + i, db->p_nodes + i * F, db->p_offs + i * (F + 1), db->p_feats + i * F,
                     db->d_desc + set * db->fstride * 32, db->d_ndesc + set};
    return Place{db->d_ids + i * W, db->d_vals + i * W, db->d_nbow + i, db->d_nodes + i * F, db->d_offs + i * (F + 1), db->d_feats + i * F,
                 db->d_desc + set * db->fstride * 32, db->d_ndesc + set};
}

// (must_be_set = false: a slot about to be written)
inline int check_probe(const mcorb_kfdb *db, int p, const char *who, bool must_be_set = true)
{
    if (p < 0 || p >= db->nprobes) { set_error(std::string(who) + ": no such probe slot"); return MCORB_E_ARG; }
    if (must_be_set && !db->probe_set[p]) { set_error(std::string(who) + ": the probe slot was never set"); return MCORB_E_STATE; }
    return MCORB_OK;
}

// getMatches_distRatio's acceptance and one-to-one bookkeeping (ORBextractor.cpp:1264-1287) for one A feature of a call whose
// lists so far are mA / mB; mD: the best distance each holder was accepted with = DescriptorDistance(A[holder], B[idx_B])
inline void accept(double best_dist_1, double best_dist_2, uint32_t idx_A, uint32_t idx_B, double max_neighbor_ratio,
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

// LoopCloser::featureMatchesBow (:217-240) -- FrontEnd::InterMatchingBow and Relocalization::featureMatchesBow walk the same way --
// calling the literal getMatches_distRatio (ORBextractor.cpp:1228-1290); the matches are appended to i1 / i2
inline void matches_host(const HostEntry &A, const HostEntry &B, double max_neighbor_ratio, std::vector<uint32_t> &i1, std::vector<uint32_t> &i2)
{
    std::vector<uint32_t> mA, mB;
    size_t ia = 0, ib = 0;
    while (ia < A.nodes.size() && ib < B.nodes.size()) {
        if (A.nodes[ia] == B.nodes[ib]) {
            mA.clear(); mB.clear();
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
}

}  // namespace mcorb
