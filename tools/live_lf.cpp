// live_lf: MC-SLAM's per-frame chain up to tracking through the C ABI alone (no Python), one rig frame at a time and in 32-frame
// batches: extraction, transform, the BoW-guided computeIntraMatches, obtainLfFeatures and the LF set's transform
// (FrontEnd.cpp:999-1024).
//   (a) bound:    mcorb_rig_set_vocabulary(MCORB_BOW_MATCH) + mcorb_rig_set_lf once; per batch upload + the extraction job + the
//                 LF getters of every frame
//   (b) separate: the bound BoW job (upload + extraction job + mcorb_rig_get_bow_tracks), then per frame mcorb_rig_obtain_lf_features
//                 on those tracks with words_ all 1 and mcorb_vocab_transform of the returned descriptors
// (b)'s first half is also reported alone (c_bow_job_alone).  4 cameras at 1280x720, 2000 features, the synthetic k = 10, L = 6
// vocabulary of live_frame.cpp, levelsup 4, cameras side by side (fx = 0.8 W, baseline 0.5: the synthetic rig's 24 px disparity
// sits at z = 21).  (a) and (b) alternate batch by batch; every batch's outputs are compared, doubles bit for bit.  Prints one
// JSON line: medians and p90 in ms.
//   live_lf [frames_one_at_a_time=300] [batches_of_32=20]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <random>
#include <vector>

#include "../include/mcorb.h"

#define CK(x)                                                                                   \
    do {                                                                                        \
        int e_ = (x);                                                                           \
        if (e_ != MCORB_OK) { fprintf(stderr, "%s: %d %s\n", #x, e_, mcorb_last_error()); exit(1); } \
    } while (0)

static const int C = 4, W = 1280, H = 720, N = 2000, LEVELSUP = 4, BATCH = 32, TOTAL = 3000;

struct Out {   // everything the user reads for one batch
    std::vector<uint8_t> feats;   // mcorb_lf_feature records, byte for byte
    std::vector<int32_t> sizes, offs, fvf;
    std::vector<uint32_t> ids, nodes, wfil;
    std::vector<double> vals;
    bool operator==(const Out &o) const
    {
        return feats == o.feats && sizes == o.sizes && offs == o.offs && fvf == o.fvf && ids == o.ids && nodes == o.nodes &&
               wfil == o.wfil && vals.size() == o.vals.size() && (vals.empty() || !memcmp(vals.data(), o.vals.data(), vals.size() * 8));
    }
};

struct Scratch {
    std::vector<mcorb_lf_feature> f = std::vector<mcorb_lf_feature>(8192);
    std::vector<uint32_t> w = std::vector<uint32_t>(8192), ids = std::vector<uint32_t>(8192), nodes = std::vector<uint32_t>(8192);
    std::vector<double> vals = std::vector<double>(8192);
    std::vector<int32_t> offs = std::vector<int32_t>(8193), fvf = std::vector<int32_t>(8192);
    std::vector<int32_t> tracks = std::vector<int32_t>((size_t)65536 * C), rays = std::vector<int32_t>(65536);
    std::vector<uint32_t> bw = std::vector<uint32_t>(65536), ones = std::vector<uint32_t>(65536, 1u);
    std::vector<uint8_t> descs = std::vector<uint8_t>((size_t)8192 * 32);
};

static void append(Out &o, const Scratch &s, int n, int ni, int nm, int nw, int nb, int nf)
{
    o.feats.insert(o.feats.end(), (const uint8_t *)s.f.data(), (const uint8_t *)(s.f.data() + n));
    o.sizes.push_back(ni); o.sizes.push_back(nm);
    o.wfil.insert(o.wfil.end(), s.w.begin(), s.w.begin() + nw);
    o.ids.insert(o.ids.end(), s.ids.begin(), s.ids.begin() + nb);
    o.vals.insert(o.vals.end(), s.vals.begin(), s.vals.begin() + nb);
    o.nodes.insert(o.nodes.end(), s.nodes.begin(), s.nodes.begin() + nf);
    o.offs.insert(o.offs.end(), s.offs.begin(), s.offs.begin() + nf + 1);
    o.fvf.insert(o.fvf.end(), s.fvf.begin(), s.fvf.begin() + s.offs[nf]);
}

static mcorb_vocab *full_vocabulary(int k, int L, uint64_t seed)
{
    int n = 0;
    for (int d = 1, p = k; d <= L; d++, p *= k) n += p;
    std::vector<int32_t> parent(n);
    std::vector<uint8_t> leaf(n, 0), desc((size_t)n * 32);
    std::vector<double> weight(n, 0.0);
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> uw(0.1, 9.0);
    int pos = 0, first = 1, prev0 = 0, prevn = 1;
    for (int d = 1; d <= L; d++) {
        const int cnt = prevn * k;
        for (int i = 0; i < cnt; i++) {
            parent[pos + i] = prev0 + i / k;
            leaf[pos + i] = d == L;
        }
        prev0 = first; prevn = cnt;
        first += cnt; pos += cnt;
    }
    for (size_t i = 0; i < desc.size(); i += 8) {
        const uint64_t x = rng();
        memcpy(&desc[i], &x, 8);
    }
    for (int i = 0; i < n; i++)
        if (leaf[i]) weight[i] = uw(rng);
    mcorb_vocab *v = nullptr;
    CK(mcorb_vocab_create(k, L, 0, 0, parent.data(), leaf.data(), desc.data(), weight.data(), n, 0, &v));
    return v;
}

static double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static void stats(const char *name, std::vector<double> v, double per, bool last)
{
    std::sort(v.begin(), v.end());
    const double med = v[v.size() / 2] / per, p90 = v[std::min(v.size() - 1, v.size() * 9 / 10)] / per;
    printf("\"%s\": {\"median_ms\": %.4f, \"p90_ms\": %.4f, \"n\": %zu}%s", name, med, p90, v.size(), last ? "" : ", ");
}

int main(int argc, char **argv)
{
    const int nsingle = argc > 1 ? atoi(argv[1]) : 300, nbatch = argc > 2 ? atoi(argv[2]) : 20;
    const int warm_single = 30, warm_batch = 3, distinct = 64;   // frames cycled through
    mcorb_params p;
    mcorb_default_params(&p);
    p.nfeatures = N;
    mcorb_vocab *voc = full_vocabulary(10, 6, 1);
    std::vector<std::vector<uint8_t>> img((size_t)distinct * C, std::vector<uint8_t>((size_t)W * H));
    for (int f = 0; f < distinct; f++)
        for (int c = 0; c < C; c++) CK(mcorb_synth_rig_frame(f, C, c, W, H, img[(size_t)f * C + c].data(), W));
    std::vector<mcorb_camera> cams(C);
    for (int c = 0; c < C; c++) {
        memset(&cams[c], 0, sizeof(cams[c]));
        const double K[9] = {0.8 * W, 0, W / 2.0, 0, 0.8 * W, H / 2.0, 0, 0, 1};
        memcpy(cams[c].K, K, sizeof(K));
        cams[c].Rt[0] = cams[c].Rt[5] = cams[c].Rt[10] = 1.0;
        cams[c].Rt[3] = -0.5 * c;
    }
    bool identical = true;
    long compared = 0, lf_features = 0, intramatch = 0, frames_seen = 0;
    Scratch S;
    printf("{\"rig\": \"4 x 1280x720, 2000 features\", \"vocabulary\": \"k=10 L=6 synthetic\", \"levelsup\": %d, \"total_feats\": %d, ", LEVELSUP, TOTAL);
    for (int nf : {1, BATCH}) {
        mcorb_rig *ra = nullptr, *rb = nullptr;
        CK(mcorb_rig_create(&p, C, W, H, nf, 1, &ra));
        CK(mcorb_rig_create(&p, C, W, H, nf, 1, &rb));
        CK(mcorb_rig_set_vocabulary(ra, voc, LEVELSUP, 0.85, MCORB_BOW_MATCH));
        CK(mcorb_rig_set_lf(ra, cams.data(), TOTAL));
        CK(mcorb_rig_set_vocabulary(rb, voc, LEVELSUP, 0.85, MCORB_BOW_MATCH));
        const int iters = nf == 1 ? nsingle : nbatch, warm = nf == 1 ? warm_single : warm_batch;
        std::vector<double> ta, tb, tc;
        std::vector<const uint8_t *> ptrs(nf * C);
        for (int it = 0; it < warm + iters; it++) {
            for (int m = 0; m < nf * C; m++) ptrs[m] = img[((size_t)it * nf * C + m) % img.size()].data();
            Out oa, ob;
            auto t0 = std::chrono::steady_clock::now();
            CK(mcorb_rig_upload_u8(ra, 0, ptrs.data(), nf * C, W));
            CK(mcorb_rig_extract(ra, 0, nf * C, 0, 0));
            for (int f = 0; f < nf; f++) {
                int n = 0, ni = 0, nm = 0, nw = 0, nb = 0, nfv = 0;
                CK(mcorb_rig_get_lf_features(ra, 0, f, S.f.data(), (int)S.f.size(), &n, &ni, &nm, S.w.data(), (int)S.w.size(), &nw));
                CK(mcorb_rig_get_lf_bow(ra, 0, f, S.ids.data(), S.vals.data(), (int)S.ids.size(), &nb, S.nodes.data(), S.offs.data(),
                                        (int)S.nodes.size(), &nfv, S.fvf.data(), (int)S.fvf.size()));
                append(oa, S, n, ni, nm, nw, nb, nfv);
                lf_features += n;
                intramatch += ni;
                frames_seen++;
            }
            const double a = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            CK(mcorb_rig_upload_u8(rb, 0, ptrs.data(), nf * C, W));
            CK(mcorb_rig_extract(rb, 0, nf * C, 0, 0));
            std::vector<std::vector<int32_t>> trs(nf);
            for (int f = 0; f < nf; f++) {
                int nt = 0, nw = 0;
                CK(mcorb_rig_get_bow_tracks(rb, 0, f, S.tracks.data(), S.rays.data(), 65536, &nt, S.bw.data(), 65536, &nw));
                trs[f].assign(S.tracks.begin(), S.tracks.begin() + (size_t)nt * C);
            }
            const double c = ms_since(t0);
            for (int f = 0; f < nf; f++) {
                const int nt = (int)trs[f].size() / C;
                int n = 0, ni = 0, nm = 0, nw = 0, nb = 0, nfv = 0;
                CK(mcorb_rig_obtain_lf_features(rb, 0, f, trs[f].data(), nt, S.ones.data(), cams.data(), nullptr, 0, nullptr, TOTAL, S.f.data(),
                                                (int)S.f.size(), &n, &ni, &nm, S.w.data(), (int)S.w.size(), &nw));
                for (int i = 0; i < n; i++) memcpy(S.descs.data() + (size_t)i * 32, S.f[i].desc, 32);
                CK(mcorb_vocab_transform(voc, S.descs.data(), n, LEVELSUP, S.ids.data(), S.vals.data(), (int)S.ids.size(), &nb, S.nodes.data(),
                                         S.offs.data(), (int)S.nodes.size(), &nfv, S.fvf.data(), (int)S.fvf.size()));
                append(ob, S, n, ni, nm, nw, nb, nfv);
            }
            const double b = ms_since(t0);
            if (it >= warm) { ta.push_back(a); tb.push_back(b); tc.push_back(c); }
            identical = identical && oa == ob && !oa.feats.empty();
            compared++;
        }
        printf("\"%s\": {", nf == 1 ? "one_frame" : "batch32_per_frame");
        stats("a_bound", ta, nf, false);
        stats("b_separate", tb, nf, false);
        stats("c_bow_job_alone", tc, nf, true);
        printf("}, ");
        mcorb_rig_destroy(ra);
        mcorb_rig_destroy(rb);
    }
    printf("\"batches_compared\": %ld, \"lf_features_per_frame\": %.1f, \"intramatch_per_frame\": %.1f, \"identical\": %s}\n", compared,
           (double)lf_features / std::max<long>(1, frames_seen), (double)intramatch / std::max<long>(1, frames_seen), identical ? "true" : "false");
    mcorb_vocab_destroy(voc);
    return identical ? 0 : 1;
}
