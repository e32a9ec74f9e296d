// mcorb_match.cpp -- the matcher's host half: the control block of a match, its launches, the accept lists and the track merge.
#include <cmath>

#include "mcorb_engine.h"
#include "mcorb_prof.h"

namespace mcorb {

// a descriptor count as the k-NN kernels clamp it
static inline int clamp_count(int n, int kcap) { return std::min(std::max(n, 0), kcap); }

// what both forms of an external match start with: is the block one the control block can hold, with its counts somewhere; the
// caller's host counts go into the control block, clamped (device-resident ones arrive with the job: finish_match)
static bool take_ext_block(Slot &s, const Job &j, int ext_cap, int kcap)
{
    if (!j.ext_desc || j.ext_total < 1 || j.ext_total > ext_cap || (!j.ext_counts && !j.ext_counts_dev)) return false;
    if (j.ext_counts)
        for (int i = 0; i < j.ext_total; i++) s.hc.extcounts[i] = clamp_count(j.ext_counts[i], kcap);
    return true;
}

// fills the host side of the control block for a match: per-(frame,cam) sets/counts and the pair list
int Rig::prepare_match(Slot &s, const Job &j)
{
    const bool ext = j.ext_desc != nullptr;
    if (j.ext_pairs) {
        // explicit (query set, train set) pairs of an external block: local set i = the i-th distinct set the list names
        if (j.ext_npairs < 1 || j.ext_npairs > max_pairs() || !take_ext_block(s, j, ext_cap, geom.kcap)) {
            set_error("match pairs: bad external block or pair count (at most " + std::to_string(max_pairs()) + " pairs per job)");
            return MCORB_E_ARG;
        }
        s.match_external = true;
        s.match_sets.clear();
        s.match_counts.clear();
        std::vector<int> local(j.ext_total, -1);
        for (int p = 0; p < j.ext_npairs; p++) {
            int lp[2];
            for (int k = 0; k < 2; k++) {
                const int set = j.ext_pairs[2 * p + k];
                if (set < 0 || set >= j.ext_total) { set_error("match pairs: set index out of range"); return MCORB_E_ARG; }
                if (local[set] < 0) {
                    if ((int)s.match_sets.size() >= max_images) { set_error("match pairs: more than " + std::to_string(max_images) + " distinct sets in one job"); return MCORB_E_ARG; }
                    local[set] = (int)s.match_sets.size();
                    s.hc.setmap[local[set]] = set;
                    s.match_sets.push_back(set);
                    s.match_counts.push_back(j.ext_counts ? s.hc.extcounts[set] : 0);
                }
                lp[k] = local[set];
            }
            s.hc.pairs[p] = int2{lp[0], lp[1]};
        }
        s.nsets_local = (int)s.match_sets.size();
        s.npairs_done = j.ext_npairs;
        s.nframes_done = 0;
        return MCORB_OK;
    }
    if (j.nframes < 1 || j.nframes > max_frames || (!ext && j.nframes * ncams > s.nimg_done)) {
        set_error("match: bad frame count or features not extracted");
        return MCORB_E_STATE;
    }
    const int C = ncams;
    s.match_external = ext;
    s.match_sets.resize((size_t)j.nframes * C);
    s.match_counts.resize((size_t)j.nframes * C);
    if (ext) {
        if (!j.ext_sets || !take_ext_block(s, j, ext_cap, geom.kcap)) {
            set_error("match: bad external block (at most " + std::to_string(ext_cap) + " sets = max(4096, 64 x images per slot))");
            return MCORB_E_ARG;
        }
        for (int i = 0; i < j.nframes * C; i++) {
            const int set = j.ext_sets[i];
            if (set < 0 || set >= j.ext_total) { set_error("match: set index out of range"); return MCORB_E_ARG; }
            s.match_sets[i] = set;
            s.match_counts[i] = j.ext_counts ? s.hc.extcounts[set] : 0;   // device-resident counts arrive with the job (finish_match)
        }
    } else {
        for (int i = 0; i < j.nframes * C; i++) { s.match_sets[i] = i; s.match_counts[i] = s.hc.nsel[i]; }
    }
    s.nframes_done = j.nframes;
    s.nsets_local = j.nframes * C;
    // the k-NN works on LOCAL set indices (frame * cameras + camera): k_expand gathers set setmap[i] into local slot i
    for (int i = 0; i < j.nframes * C; i++) s.hc.setmap[i] = s.match_sets[i];
    int p = 0;
    for (int f = 0; f < j.nframes; f++)
        for (int a = 0; a < C - 1; a++)
            for (int b = a + 1; b < C; b++) s.hc.pairs[p++] = int2{f * C + a, f * C + b};
    s.npairs_done = p;
    return MCORB_OK;
}

int Rig::enqueue_match(Slot &s, const Job &j, bool ctrl_on_device)
{
    if (!ctrl_on_device) {
        TRY(prepare_match(s, j));
        HIPCHK(hipMemcpyAsync(s.d_ctrl, s.h_ctrl, s.ctrl_pairs_end, hipMemcpyHostToDevice, s.st));
        s.set_ctl(false, false);
    }
    if (j.after_stream)   // the block is being produced on another stream (a collective): order this stream behind what the
        HIPCHK(hipStreamWaitEvent(s.st, s.ev_x, 0));   // caller had enqueued there at submit time (ev_x, recorded by the submit call)
    if (j.ext_counts_dev) {
        HIPCHK(hipMemcpyAsync(s.dc.extcounts, j.ext_counts_dev, (size_t)j.ext_total * sizeof(int), hipMemcpyDeviceToDevice, s.st));
        HIPCHK(hipMemcpyAsync(s.hc.extcounts, j.ext_counts_dev, (size_t)j.ext_total * sizeof(int), hipMemcpyDeviceToHost, s.st));
    }
    if (s.npairs_done == 0) return MCORB_OK;
    const bool ext = j.ext_desc != nullptr;
    const bool ev_on = s.ev_on();
    if (ev_on) HIPCHK(hipEventRecord(s.ev_knn0, s.st));
    launch_knn2(s.st, ext ? (const uint8_t *)j.ext_desc : s.d_desc, ext ? s.dc.extcounts : s.ctl.nsel, s.ctl.setmap, s.nsets_local, s.ctl.pairs,
                s.npairs_done, geom.kcap, s.d_exp, s.d_lcounts, s.d_part, j.dist_thresh, j.ratio, s.d_knn, s.h_mlist,
                s.h_mcount, ev_on ? s.ev_e : nullptr, ev_on ? s.ev_knn1 : nullptr);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_fin, s.st));
    HIPCHK(hipGetLastError());
    return MCORB_OK;
}

// The epipolar check of computeIntraMatches(matches, old=true) (MultiCameraFrame.cpp:1178-1207): line in
// image i = F^T * kp2, normalised, squared point-line distance against 3.84 * sigma2[octave].  The mixed
// float/double arithmetic follows the reference's declared types statement by statement.
static bool epipolar_ok(const double *F, const mcorb_keypoint &k1, const mcorb_keypoint &k2, const float *sigma2)
{
    float a = (float)((double)k2.x * F[0] + (double)k2.y * F[3] + F[6]);
    float b = (float)((double)k2.x * F[1] + (double)k2.y * F[4] + F[7]);
    float c = (float)((double)k2.x * F[2] + (double)k2.y * F[5] + F[8]);
    float den = a * a + b * b;
    den = den ? (float)(1. / (double)std::sqrt(den)) : (float)1.;
    a *= den; b *= den; c *= den;
    den = a * a + b * b;
    const float num = a * k1.x + b * k1.y + c;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    const float check_thresh = (float)(3.84 * (double)sigma2[k1.octave]);
    return dsqr < check_thresh;
}

// computeIntraMatches' track merge over the BruteForceMatch lists of one frame
// (MultiCameraFrame.cpp:1167-1268); gate != nullptr adds the old=true epipolar check.
void merge_pair_lists(int C, const int *counts, const uint32_t *const *idx1, const uint32_t *const *idx2, const int *np,
                             const EpipolarGate *gate, std::vector<int32_t> &tr, int &mergeable_out)
{
    tr.clear();
    int ntr = 0, mergeable = 0;
    // keypoint -> track, one flat table for all cameras (per thread: this runs once per rig frame, on pool threads)
    static thread_local std::vector<int> inv_flat;
    int *inv[MCORB_MAX_CAMS];
    {
        size_t total = 0, worst = 0;
        for (int c = 0; c < C; c++) total += (size_t)std::max(counts[c], 0);
        inv_flat.assign(total, -1);
        size_t o = 0;
        for (int c = 0; c < C; c++) { inv[c] = inv_flat.data() + o; o += (size_t)std::max(counts[c], 0); }
        for (int p = 0; p < C * (C - 1) / 2; p++) worst += (size_t)std::max(np[p], 0);
        tr.resize(worst * C);   // a track per accepted match at most; cut to the tracks made at the end
    }
    int32_t *T = tr.data();
    int pl = 0;
    for (int a = 0; a < C - 1; a++) {
        for (int b = a + 1; b < C; b++, pl++) {
            const uint32_t *i1 = idx1[pl], *i2 = idx2[pl];
            for (int k = 0; k < np[pl]; k++) {
                const int fa = (int)i1[k], fb = (int)i2[k];
                const int ma = inv[a][fa], mb = inv[b][fb];
                if (gate && !epipolar_ok(gate->F + 9 * pl, gate->kps[a][fa], gate->kps[b][fb], gate->sigma2)) continue;
                if (ma == -1 && mb == -1) {
                    int32_t *row = T + (size_t)ntr * C;
                    for (int c = 0; c < C; c++) row[c] = -1;
                    row[a] = fa;
                    row[b] = fb;
                    inv[a][fa] = ntr;
                    inv[b][fb] = ntr;
                    ntr++;
                } else {
                    if (ma == -1 && mb != -1) {
                        if (T[(size_t)mb * C + a] == -1) {
                            T[(size_t)mb * C + a] = fa;
                            inv[a][fa] = mb;
                        }
                    }
                    if (ma != -1 && mb != -1) {
                        if (ma != mb) mergeable++;
                    }
                    if (ma != -1 && mb == -1) {
                        T[(size_t)ma * C + b] = fb;
                        inv[b][fb] = ma;
                    }
                }
            }
        }
    }
    tr.resize((size_t)ntr * C);
    mergeable_out = mergeable;
}

void Rig::merge_tracks(Slot &s, int f, const EpipolarGate *gate, std::vector<int32_t> &tr, int &mergeable_out) const
{
    const int C = ncams;
    const uint32_t *i1[MCORB_MAX_CAMS * MCORB_MAX_CAMS], *i2[MCORB_MAX_CAMS * MCORB_MAX_CAMS];
    int np[MCORB_MAX_CAMS * MCORB_MAX_CAMS];
    for (int p = 0; p < npp; p++) {
        i1[p] = s.m_idx1[f * npp + p].data();
        i2[p] = s.m_idx2[f * npp + p].data();
        np[p] = (int)s.m_idx1[f * npp + p].size();
    }
    merge_pair_lists(C, &s.match_counts[(size_t)f * C], i1, i2, np, gate, tr, mergeable_out);
}

// BruteForceMatch's output lists (MultiCameraFrame.cpp:1060-1078) + the track merge, host side,
// after the k-NN tables landed.
int Rig::finish_match(Slot &s, const Job &j)
{
    HostProf::Scope prof(2);
    if (j.ext_counts_dev)   // the counts came over with the job's own stream; the k-NN kernels clamped them the same way
        for (size_t i = 0; i < s.match_sets.size(); i++)
            s.match_counts[i] = clamp_count(s.hc.extcounts[s.match_sets[i]], geom.kcap);
    const int nqb = knn_qblocks(geom.kcap);
    // k_knn2_finalize's output of pair pi (pair index within the job): accepted pairs per block of queries, and the pairs
    auto pair_lists = [&](int pi) {
        return std::pair<const int *, const uint32_t *>(s.h_mcount + (size_t)pi * nqb, s.h_mlist + (size_t)pi * knn_mlist_stride(geom.kcap));
    };
    auto filter_pair = [&](int pi, int) {   // BruteForceMatch's accept loop for one camera pair
        // k_knn2_finalize already compacted the accepted pairs in query order: unpack query << 16 | train
        std::vector<uint32_t> &i1 = s.m_idx1[pi], &i2 = s.m_idx2[pi];
        const auto [cnt, ml] = pair_lists(pi);
        int n = 0;
        for (int b = 0; b < nqb; b++) n += cnt[b];
        i1.resize(n); i2.resize(n);
        int k = 0;
        for (int b = 0; b < nqb; b++)
            for (int e = 0; e < cnt[b]; e++, k++) { i1[k] = ml[b * kKnnQueriesPerBlock + e] >> 16; i2[k] = ml[b * kKnnQueriesPerBlock + e] & 0xffffu; }
    };
    auto one_frame = [&](int f, int w) {
        // the accept lists were written by the GPU into pinned host memory: every line is a miss, and the lists are short runs
        // (one per 256 queries) that the hardware prefetcher does not get ahead of -- ask for all of a frame's lines at once
        for (int pi = f * npp; pi < (f + 1) * npp; pi++) {
            const auto [cnt, ml] = pair_lists(pi);
            for (int b = 0; b < nqb; b++) {
                const char *p0 = reinterpret_cast<const char *>(ml + (size_t)b * kKnnQueriesPerBlock);
                const int bytes = std::min(std::max(cnt[b], 0), kKnnQueriesPerBlock) * 4;
                for (int o = 0; o < bytes; o += 64) __builtin_prefetch(p0 + o, 0, 0);
            }
        }
        for (int pi = f * npp; pi < (f + 1) * npp; pi++) filter_pair(pi, w);
        LatProf::mark(9);
        merge_tracks(s, f, nullptr, s.tracks[f], s.mergeable[f]);
        LatProf::mark(10);
    };
    // frames are independent (own pair lists, own track table): one pool task each
    if (j.ext_pairs) pool->parallel_for(s.npairs_done, filter_pair, pool_threads + s.index);   // explicit pairs: lists only, the merge is the caller's
    else if (s.nframes_done > 1) pool->parallel_for(s.nframes_done, one_frame, pool_threads + s.index);
    else if (s.nframes_done == 1) one_frame(0, 0);   // (spreading one frame's pairs over the pool was slower: wake-ups)
    if (s.npairs_done > 0 && !s.graph_timing) {
        float m = 0;
        ev_elapsed(&m, s.ev_knn0, s.ev_fin); s.timing[T_MATCH] = m * 1000.f;
        ev_elapsed(&m, s.ev_e, s.ev_knn1); s.timing[T_KNN2] = m * 1000.f;   // k_knn2 (k_expand in front of it: T_MATCH - T_KNN2 - finalize)
    }
    return MCORB_OK;
}

}  // namespace mcorb
