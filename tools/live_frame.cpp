// live_frame: MC-SLAM's per-frame BoW chain through the C ABI alone (no Python), one rig frame at a time and in 32-frame batches.
//   (a) bound:    mcorb_rig_set_vocabulary once; per batch upload + the extraction job (which also runs transform() and the
//                 BoW-guided computeIntraMatches on the device) + the getters for the tracks and every camera's BowVector
//   (b) separate: upload + mcorb_rig_extract + mcorb_rig_transform_images + mcorb_rig_match_bow_frames + the same getters
// 4 cameras at 1280x720, 2000 features, a synthetic k = 10, L = 6 vocabulary (the shape scripts/bow_rate.py's full_vocabulary
// builds: a full breadth-first tree, random node descriptors, leaf weights in [0.1, 9)), levelsup 4.  (a) and (b) alternate
// batch by batch; every batch's outputs of the two are compared for equality.  Prints one JSON line: medians and p90 in ms.
//   live_frame [frames_one_at_a_time=300] [batches_of_32=20]
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

static const int C = 4, W = 1280, H = 720, N = 2000, LEVELSUP = 4, BATCH = 32;

struct Out {   // everything the user reads for one batch
    std::vector<uint32_t> ids, nodes, words;
    std::vector<double> vals;
    std::vector<int32_t> offs, feats, tracks, rays;
    bool operator==(const Out &o) const
    {
        return ids == o.ids && nodes == o.nodes && words == o.words && offs == o.offs && feats == o.feats && tracks == o.tracks &&
               rays == o.rays && vals.size() == o.vals.size() && (vals.empty() || !memcmp(vals.data(), o.vals.data(), vals.size() * 8));
    }
};

static void read_results(mcorb_rig *r, int nframes, Out &o)
{
    const int kcap = mcorb_rig_kcap(r);
    o = Out();
    std::vector<uint32_t> ids(kcap), nodes(kcap), words((size_t)kcap * C);
    std::vector<double> vals(kcap);
    std::vector<int32_t> offs(kcap + 1), feats(kcap), tracks((size_t)kcap * C * C), rays((size_t)kcap * C);
    for (int f = 0; f < nframes; f++) {
        int nt = 0, nw = 0;
        CK(mcorb_rig_get_bow_tracks(r, 0, f, tracks.data(), rays.data(), kcap * C, &nt, words.data(), kcap * C, &nw));
        o.tracks.insert(o.tracks.end(), tracks.begin(), tracks.begin() + (size_t)nt * C);
        o.rays.insert(o.rays.end(), rays.begin(), rays.begin() + nt);
        o.words.insert(o.words.end(), words.begin(), words.begin() + nw);
        for (int c = 0; c < C; c++) {
            int nb = 0, nf = 0;
            CK(mcorb_rig_get_transform(r, 0, f * C + c, ids.data(), vals.data(), kcap, &nb, nodes.data(), offs.data(), kcap, &nf, feats.data(), kcap));
            o.ids.insert(o.ids.end(), ids.begin(), ids.begin() + nb);
            o.vals.insert(o.vals.end(), vals.begin(), vals.begin() + nb);
            o.nodes.insert(o.nodes.end(), nodes.begin(), nodes.begin() + nf);
            o.offs.insert(o.offs.end(), offs.begin(), offs.begin() + nf + 1);
            o.feats.insert(o.feats.end(), feats.begin(), feats.begin() + offs[nf]);
        }
    }
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
    bool identical = true;
    long compared = 0;
    printf("{\"rig\": \"4 x 1280x720, 2000 features\", \"vocabulary\": \"k=10 L=6 synthetic\", \"levelsup\": %d, ", LEVELSUP);
    for (int nf : {1, BATCH}) {
        mcorb_rig *ra = nullptr, *rb = nullptr;
        CK(mcorb_rig_create(&p, C, W, H, nf, 1, &ra));
        CK(mcorb_rig_create(&p, C, W, H, nf, 1, &rb));
        CK(mcorb_rig_set_vocabulary(ra, voc, LEVELSUP, 0.85, MCORB_BOW_MATCH));
        const int iters = nf == 1 ? nsingle : nbatch, warm = nf == 1 ? warm_single : warm_batch;
        std::vector<double> ta, tb;
        Out oa, ob;
        std::vector<const uint8_t *> ptrs(nf * C);
        for (int it = 0; it < warm + iters; it++) {
            for (int m = 0; m < nf * C; m++) ptrs[m] = img[((size_t)it * nf * C + m) % img.size()].data();
            auto t0 = std::chrono::steady_clock::now();
            CK(mcorb_rig_upload_u8(ra, 0, ptrs.data(), nf * C, W));
            CK(mcorb_rig_extract(ra, 0, nf * C, 0, 0));
            read_results(ra, nf, oa);
            const double a = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            CK(mcorb_rig_upload_u8(rb, 0, ptrs.data(), nf * C, W));
            CK(mcorb_rig_extract(rb, 0, nf * C, 0, 0));
            CK(mcorb_rig_transform_images(rb, 0, 0, nf * C, voc, LEVELSUP));
            CK(mcorb_rig_match_bow_frames(rb, 0, 0, nf, voc, LEVELSUP, 0.85, nullptr));
            read_results(rb, nf, ob);
            const double b = ms_since(t0);
            if (it >= warm) { ta.push_back(a); tb.push_back(b); }
            identical = identical && oa == ob && !oa.tracks.empty();
            compared++;
        }
        printf("\"%s\": {", nf == 1 ? "one_frame" : "batch32_per_frame");
        stats("a_bound", ta, nf, false);
        stats("b_separate", tb, nf, true);
        printf("}, ");
        mcorb_rig_destroy(ra);
        mcorb_rig_destroy(rb);
    }
    printf("\"batches_compared\": %ld, \"identical\": %s}\n", compared, identical ? "true" : "false");
    mcorb_vocab_destroy(voc);
    return identical ? 0 : 1;
}
