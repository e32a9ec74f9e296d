// The host path of mcorb_mapping_new.h in a plain g++ program (built with -fsanitize=address,undefined by
// tests/test_mapping_new_cpu.py): reads a scene the test wrote -- cameras, the two frames, the matches -- packs it as
// mcorb_lmap_triangulate_new does, runs every match through map_new_item and prints one line per match: the verdict, the solves
// and the bytes of X, normal, dist, both costs and cos.  The test compares them with the library's answer on the same scene.
//   test_mapping_new_sanitize scene.txt
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mcorb_mapping_new.h"

using namespace mcorb;

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
    std::vector<MapFrameDev> frames(2);
    std::vector<int32_t> mi;
    std::vector<MapKp> kp;
    MapNewArgs n;
    for (int fr = 0; fr < 2; fr++) {                 // the current frame, then the previous keyframe
        MapFrameDev &d = frames[fr];
        memset(&d, 0, sizeof(d));
        double *twc = fr == 0 ? n.twc_cur : n.twc_prev;
        for (int k = 0; k < 3; k++) twc[k] = rd();
        for (int c = 0; c < C; c++) {
            for (int k = 0; k < 12; k++) d.proj[c][k] = rd();
            for (int k = 0; k < 3; k++) d.centre[c][k] = rd();
        }
        for (int c = 0; c < MCORB_MAX_CAMS; c++) {
            d.kp_off[c] = (int32_t)kp.size();
            if (c >= C) continue;
            const int nk = ri();
            for (int k = 0; k < nk; k++) {
                MapKp p;
                p.x = (float)rd(); p.y = (float)rd(); p.octave = ri();
                kp.push_back(p);
            }
        }
        const int nfeat = ri();
        d.mi_off = (int32_t)mi.size();
        for (int i = 0; i < nfeat * C; i++) mi.push_back(ri());
    }
    const int nm = ri();
    std::vector<MapItem> items((size_t)nm);
    for (int j = 0; j < nm; j++) { items[j].q = ri(); items[j].t = ri(); items[j].rec = j; }
    fclose(f);
    std::vector<MapOut> out((size_t)nm);
    std::vector<MapNewExtra> ext((size_t)nm);
    n.a.frames = frames.data(); n.a.mi = mi.data(); n.a.kp = kp.data(); n.a.F = nullptr; n.a.K = K.data();
    n.a.inv_sigma2 = sig.data(); n.a.blocks = nullptr; n.a.items = items.data(); n.a.out = out.data(); n.a.ncams = C;
    n.extra = ext.data();
    for (int j = 0; j < nm; j++) {
        int nv = 0;
        for (int c = 0; c < C; c++)
            nv += (mi[frames[1].mi_off + (size_t)items[j].q * C + c] != -1) + (mi[frames[0].mi_off + (size_t)items[j].t * C + c] != -1);
        if (nv <= 4) map_new_item<false>(n, items[j]); else map_new_item<true>(n, items[j]);
        printf("%d %d %d ", out[j].verdict, out[j].n_rays, ext[j].solves);
        hex(out[j].X, 24); hex(out[j].normal, 24); hex(&out[j].dist2, 8); hex(&ext[j].cost_initial, 8); hex(&ext[j].cost_final, 8);
        hex(&ext[j].cos, 4);
        printf("\n");
    }
    return 0;
}
