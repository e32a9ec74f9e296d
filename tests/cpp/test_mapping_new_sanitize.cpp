// The host path of mcorb_mapping_new.h in a plain g++ program (built with -fsanitize=address,undefined by
// tests/test_mapping_new_cpu.py): reads a scene the test wrote -- cameras, the two frames, the matches -- packs it with
// the code mcorb_lmap_triangulate_new packs it with (MapCall, csrc/mcorb_map_host.h), runs every match through map_new_item and prints one line per match: the verdict, the solves
// and the bytes of X, normal, dist, both costs and cos.  The test compares them with the library's answer on the same scene.
//   test_mapping_new_sanitize scene.txt
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mcorb_map_host.h"
#include "mcorb_mapping_new.h"

using namespace mcorb;

void mcorb::set_error(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); }

// a frame of the scene file and the arrays its mcorb_map_frame points into
struct Frame {
    std::vector<int32_t> rows, nk;
    std::vector<std::vector<mcorb_keypoint>> kps;
    std::vector<const mcorb_keypoint *> kp_ptr;
    mcorb_map_frame f;
};

static FILE *f;
static double rd() { double v; if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "short file\n"); exit(2); } return v; }
static int ri() { int v; if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "short file\n"); exit(2); } return v; }

static void hex(const void *p, size_t n)
{
    for (size_t i = 0; i < n; i++) printf("%02x", ((const uint8_t *)p)[i]);
    printf(" ");
}

int main(int argc, char **argv)
{
    if (argc != 2 || !(f = fopen(argv[1], "r"))) { fprintf(stderr, "usage: test_mapping_new_sanitize scene.txt\n"); return 2; }
    const int C = ri(), nlevels = ri();
    std::vector<double> K((size_t)C * 9);
    for (double &v : K) v = rd();
    std::vector<float> sig((size_t)nlevels);
    for (float &v : sig) v = (float)rd();
    MapCall mc{"mapping_new sanitize", 0x7fffffff, C, nlevels};
    Frame frames[2];
    for (int fr = 0; fr < 2; fr++) {                 // the current frame, then the previous keyframe
        Frame &d = frames[fr];
        memset(&d.f, 0, sizeof(d.f));
        for (int k = 0; k < 3; k++) d.f.twc[k] = rd();
        for (int c = 0; c < C; c++) {
            for (int k = 0; k < 12; k++) d.f.proj[c][k] = rd();
            for (int k = 0; k < 3; k++) d.f.centre_w[c][k] = rd();
        }
        d.kps.resize((size_t)C);
        for (int c = 0; c < C; c++) {
            d.nk.push_back(ri());
            for (int k = 0; k < d.nk[c]; k++) {
                mcorb_keypoint p;
                memset(&p, 0, sizeof(p));
                p.x = (float)rd(); p.y = (float)rd(); p.octave = ri();
                d.kps[c].push_back(p);
            }
            d.kp_ptr.push_back(d.kps[c].data());
        }
        d.f.nfeat = ri();
        d.f.ncams = C;
        for (int i = 0; i < d.f.nfeat * C; i++) d.rows.push_back(ri());
        d.f.match_index = d.rows.data();
        d.f.kps_undist = d.kp_ptr.data();
        d.f.nkps = d.nk.data();
        if (mc.check_frame(d.f) != MCORB_OK) return 2;
        mc.add(d.f);
    }
    const int nm = ri();
    std::vector<MapItem> items((size_t)nm);
    std::vector<uint8_t> nviews((size_t)nm);
    for (int j = 0; j < nm; j++) {
        items[j].q = ri(); items[j].t = ri(); items[j].rec = j;
        uint8_t nv_cur;
        if (mc.count_views(frames[1].f, items[j].q, items[j].t, nviews[j], nv_cur) != MCORB_OK) return 2;
    }
    fclose(f);
    if (mc.fits() != MCORB_OK) return 2;
    const MapLayout L = mc.layout(0, 0);
    std::vector<uint8_t> block(L.p.total);   // exactly the block's bytes
    mc.pack(block.data(), L, K.data(), sig.data());
    std::vector<MapOut> out((size_t)nm);
    std::vector<MapNewExtra> ext((size_t)nm);
    MapNewArgs n;
    n.a = L.args(block.data(), out.data(), C);
    n.extra = ext.data();
    for (int k = 0; k < 3; k++) { n.twc_cur[k] = frames[0].f.twc[k]; n.twc_prev[k] = frames[1].f.twc[k]; }
    for (int j = 0; j < nm; j++) {
        if (nviews[j] <= 4) map_new_item<false>(n, items[j]); else map_new_item<true>(n, items[j]);
        printf("%d %d %d ", out[j].verdict, out[j].n_rays, ext[j].solves);
        hex(out[j].X, 24); hex(out[j].normal, 24); hex(&out[j].dist2, 8); hex(&ext[j].cost_initial, 8); hex(&ext[j].cost_final, 8);
        hex(&ext[j].cos, 4);
        printf("\n");
    }
    return 0;
}
