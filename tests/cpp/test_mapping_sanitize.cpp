// test_mapping_sanitize.cpp -- csrc/mcorb_mapping.h's host path (map_depth, then per neighbour the baseline gate over the median
// depth and the walk over its matches through map_item: what a host-only store runs for triangulate_neighbours) as a stand-alone
// program, built by tests/test_mapping_cpu.py with -fsanitize=address,undefined.  The block is packed by the code
// mcorb_mapping.cpp packs it with (MapCall, csrc/mcorb_map_host.h).  argv[1]: a problem written by the test -- int32 C, n_neigh,
// nlevels, next_lid, the current frame's nfeat; K (9 C doubles), inv_sigma2 (nlevels floats), Rcw (9 doubles), tcw (3); the
// current frame; per neighbour int32 nfeat, n_matches, then the frame, the points of its features that have a landmark (3
// doubles each, in the order of the features), its F table (9 C C doubles), match_query and match_train (n_matches int32 each).
// A frame is twc (3 doubles), match_index (nfeat C int32), proj (12 C doubles), centre_w (3 C doubles), nkps (C int32), per
// camera the keypoints' xy (2 floats each) and octaves (int32 each), then the features' landmark ids (nfeat int32).  argv[2]: the
// records written back, the neighbours' matches back to back -- verdict and new_lid (int32 each), dist2 and cos (double each),
// pt3d and normal (3 doubles each) -- and then one skip flag per neighbour (bytes).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mcorb_map_host.h"
#include "mcorb_mapping.h"

using namespace mcorb;

void mcorb::set_error(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); }

template <class T>
static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

// a frame of the problem file and the arrays its mcorb_map_frame points into
struct Frame {
    std::vector<int32_t> rows, nk, lids;
    std::vector<std::vector<mcorb_keypoint>> kps;
    std::vector<const mcorb_keypoint *> kp_ptr;
    mcorb_map_frame f;
    void read(FILE *in, int C, int nfeat)
    {
        memset(&f, 0, sizeof(f));
        const std::vector<double> twc = rd<double>(in, 3);
        rows = rd<int32_t>(in, (size_t)nfeat * C);
        const std::vector<double> proj = rd<double>(in, (size_t)C * 12), centre = rd<double>(in, (size_t)C * 3);
        nk = rd<int32_t>(in, (size_t)C);
        memcpy(f.twc, twc.data(), sizeof(f.twc));
        memcpy(f.proj, proj.data(), proj.size() * sizeof(double));
        memcpy(f.centre_w, centre.data(), centre.size() * sizeof(double));
        kps.resize((size_t)C);
        for (int c = 0; c < C; c++) {
            if (nk[c] < 0) exit(2);
            const std::vector<float> xy = rd<float>(in, (size_t)nk[c] * 2);
            const std::vector<int32_t> oct = rd<int32_t>(in, (size_t)nk[c]);
            for (int k = 0; k < nk[c]; k++) kps[c].push_back(mcorb_keypoint{xy[2 * k], xy[2 * k + 1], 0.f, 0.f, 0.f, oct[k], 0});
        }
        for (int c = 0; c < C; c++) kp_ptr.push_back(kps[c].data());
        lids = rd<int32_t>(in, (size_t)nfeat);
        f.nfeat = nfeat;
        f.ncams = C;
        f.match_index = rows.data();
        f.kps_undist = kp_ptr.data();
        f.nkps = nk.data();
    }
};

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    const std::vector<int32_t> h = rd<int32_t>(in, 5);
    const int C = h[0], n_neigh = h[1], nlevels = h[2], next_lid = h[3];
    if (C < 1 || C > MCORB_MAX_CAMS || n_neigh < 1 || n_neigh > 64 || nlevels < 1 || nlevels > MCORB_MAX_LEVELS || h[4] < 0) return 2;
    const std::vector<double> K = rd<double>(in, (size_t)C * 9);
    const std::vector<float> sig = rd<float>(in, (size_t)nlevels);
    const std::vector<double> Rcw = rd<double>(in, 9), tcw = rd<double>(in, 3);
    MapCall mc{"mapping sanitize", 0x7fffffff, C, nlevels};
    std::vector<Frame> frames((size_t)n_neigh + 1);
    frames[0].read(in, C, h[4]);
    if (mc.check_frame(frames[0].f) != MCORB_OK) return 2;
    mc.add(frames[0].f);
    std::vector<std::vector<double>> pts((size_t)n_neigh), F((size_t)n_neigh);
    std::vector<std::vector<int32_t>> mq((size_t)n_neigh), mt((size_t)n_neigh);
    std::vector<size_t> moff((size_t)n_neigh + 1, 0);
    size_t nz = 0;
    for (int s = 0; s < n_neigh; s++) {
        const std::vector<int32_t> hs = rd<int32_t>(in, 2);
        if (hs[0] < 0 || hs[1] < 0) return 2;
        Frame &d = frames[(size_t)s + 1];
        d.read(in, C, hs[0]);
        if (mc.check_frame(d.f) != MCORB_OK) return 2;
        mc.add(d.f);
        size_t have = 0;
        for (int32_t l : d.lids) have += l != -1;
        pts[s] = rd<double>(in, have * 3);
        F[s] = rd<double>(in, (size_t)C * C * 9);
        mq[s] = rd<int32_t>(in, (size_t)hs[1]);
        mt[s] = rd<int32_t>(in, (size_t)hs[1]);
        moff[s + 1] = moff[s] + (size_t)hs[1];
        nz += have;
    }
    fclose(in);
    const size_t total = moff[n_neigh];
    std::vector<uint8_t> nviews(total, 0);
    for (int s = 0; s < n_neigh; s++)
        for (size_t j = 0; j < mq[s].size(); j++) {
            uint8_t nv_cur;
            if (mc.count_views(frames[(size_t)s + 1].f, mq[s][j], mt[s][j], nviews[moff[s] + j], nv_cur) != MCORB_OK) return 2;
        }
    if (mc.fits() != MCORB_OK) return 2;
    const MapLayout L = mc.layout((size_t)n_neigh * C * C * 9, nz);
    std::vector<uint8_t> block(L.p.total);   // exactly the block's bytes
    mc.pack(block.data(), L, K.data(), sig.data());
    for (int s = 0; s < n_neigh; s++) memcpy(block.data() + L.F + (size_t)s * C * C * 9 * sizeof(double), F[s].data(), F[s].size() * sizeof(double));
    const MapArgs ha = L.args(block.data(), nullptr, C);

    std::vector<int32_t> lc = frames[0].lids, verdict(total, 0), new_lid(total, -1);
    std::vector<double> dist2(total, 0.0), cosp(total, 0.0), pt3d(3 * total, 0.0), normal(3 * total, 0.0);
    std::vector<uint8_t> skipped((size_t)n_neigh, 0);
    int ntri = 0;
    for (int s = 0; s < n_neigh; s++) {
        std::vector<int32_t> ln = frames[(size_t)s + 1].lids;
        const mcorb_map_frame &nf = frames[(size_t)s + 1].f;
        std::vector<double> zs;
        for (size_t i = 0; 3 * i < pts[s].size(); i++) zs.push_back(map_depth(Rcw.data(), tcw.data(), &pts[s][3 * i]));
        if (zs.empty()) skipped[s] = 2;
        else {
            std::sort(zs.begin(), zs.end());
            const double median = zs[(zs.size() - 1) / 2];
            double sq = 0.0;
            for (int k = 0; k < 3; k++) { const double d = frames[0].f.twc[k] - nf.twc[k]; sq += d * d; }
            if (sqrt(sq) / median < 0.01) skipped[s] = 1;
        }
        for (size_t j = 0; j < mq[s].size(); j++) {
            const size_t i = moff[s] + j;
            const int q = mq[s][j], t = mt[s][j];
            if (skipped[s]) { verdict[i] = kMapNeighbourSkipped; continue; }
            if (ln[q] != -1 || lc[t] != -1) { verdict[i] = kMapAssigned; continue; }
            MapOut o;
            MapArgs a = ha;
            a.out = &o;
            const MapItem it{q, t, 0};
            if (nviews[i] <= 4) map_item<false>(a, s, it); else map_item<true>(a, s, it);
            verdict[i] = o.verdict;
            dist2[i] = o.dist2;
            cosp[i] = o.cos;
            if (o.verdict != kMapLandmark) continue;
            ln[q] = lc[t] = new_lid[i] = next_lid + ntri++;
            memcpy(&pt3d[3 * i], o.X, sizeof(o.X));
            memcpy(&normal[3 * i], o.normal, sizeof(o.normal));
        }
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(verdict.data(), sizeof(int32_t), total, out);
    fwrite(new_lid.data(), sizeof(int32_t), total, out);
    fwrite(dist2.data(), sizeof(double), total, out);
    fwrite(cosp.data(), sizeof(double), total, out);
    fwrite(pt3d.data(), sizeof(double), pt3d.size(), out);
    fwrite(normal.data(), sizeof(double), normal.size(), out);
    fwrite(skipped.data(), 1, skipped.size(), out);
    fclose(out);
    printf("matches=%d landmarks=%d bad=0\n", (int)total, ntri);
    return 0;
}
