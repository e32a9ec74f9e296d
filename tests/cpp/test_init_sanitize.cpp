// test_init_sanitize.cpp -- init_run_serial (csrc/mcorb_init.h), the host-only store's path of mcorb_lmap_initialize, as a plain
// g++ program under -fsanitize=address,undefined (tests/test_init_cpu.py builds and runs it).  argv[1]: the scene as
// test_init_cpu.py writes it; argv[2]: the records of all matches, then the call's record, which the test compares with the
// library's.  The block is packed by the code mcorb_init.cpp packs it with (MapCall, csrc/mcorb_map_host.h): the current frame
// first, its centres cam_centre_body, then the flags and the matches.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mcorb_map_host.h"
#include "mcorb_init.h"

using namespace mcorb;

void mcorb::set_error(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); }

// a frame of the scene file and the arrays its mcorb_map_frame points into
struct Frame {
    std::vector<int32_t> rows, nk;
    std::vector<std::vector<mcorb_keypoint>> kps;
    std::vector<const mcorb_keypoint *> kp_ptr;
    mcorb_map_frame f;
};

template <class T>
static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> h = rd<int32_t>(f, 6);
    const int C = h[0], n = h[1], nlevels = h[2], next_lid = h[3], nfeat[2] = {h[5], h[4]};   // [0] cur, [1] prev
    const std::vector<double> R = rd<double>(f, 9), t = rd<double>(f, 3), body = rd<double>(f, (size_t)C * 3), K = rd<double>(f, (size_t)C * 9);
    const std::vector<float> sig = rd<float>(f, (size_t)nlevels);
    const std::vector<int32_t> m = rd<int32_t>(f, (size_t)n * 2);
    const std::vector<uint8_t> flags = rd<uint8_t>(f, (size_t)n);
    MapCall mc{"init sanitize", 0x7fffffff, C, nlevels};
    Frame frames[2];
    for (int fr = 0; fr < 2; fr++) {
        Frame &d = frames[fr];
        memset(&d.f, 0, sizeof(d.f));
        d.rows = rd<int32_t>(f, (size_t)nfeat[fr] * C);
        const std::vector<double> proj = rd<double>(f, (size_t)C * 12), centre = rd<double>(f, (size_t)C * 3);
        d.nk = rd<int32_t>(f, (size_t)C);
        memcpy(d.f.proj, proj.data(), proj.size() * sizeof(double));
        memcpy(d.f.centre_w, centre.data(), centre.size() * sizeof(double));
        d.kps.resize((size_t)C);
        for (int c = 0; c < C; c++) {
            const std::vector<float> xy = rd<float>(f, (size_t)d.nk[c] * 2);
            const std::vector<int32_t> oct = rd<int32_t>(f, (size_t)d.nk[c]);
            for (int k = 0; k < d.nk[c]; k++) d.kps[c].push_back(mcorb_keypoint{xy[2 * k], xy[2 * k + 1], 0.f, 0.f, 0.f, oct[k], 0});
            d.kp_ptr.push_back(d.kps[c].data());
        }
        d.f.nfeat = nfeat[fr];
        d.f.ncams = C;
        d.f.match_index = d.rows.data();
        d.f.kps_undist = d.kp_ptr.data();
        d.f.nkps = d.nk.data();
        if (mc.check_frame(d.f) != MCORB_OK) return 2;
        mc.add(d.f);
    }
    fclose(f);
    std::vector<int32_t> q((size_t)n), tr((size_t)n);
    InitJob job;
    memset(&job, 0, sizeof(job));
    memcpy(job.R, R.data(), sizeof(job.R));
    memcpy(job.t, t.data(), sizeof(job.t));
    job.n = n;
    job.ncams = C;
    job.next_lid = next_lid;
    for (int i = 0; i < n; i++) { q[i] = m[2 * i]; tr[i] = m[2 * i + 1]; job.n_initial += flags[i] ? 1 : 0; }
    for (int i = 0; i < n; i++) {
        uint8_t nv, nv_cur;
        if (mc.count_views(frames[1].f, q[i], tr[i], nv, nv_cur) != MCORB_OK) return 2;
    }
    if (mc.fits() != MCORB_OK) return 2;
    const InitLayout L((size_t)C, (size_t)nlevels, mc.nmi, mc.nkp, 0, 0, (size_t)n);
    std::vector<uint8_t> block(L.m.p.total);   // exactly the block's bytes
    mc.pack(block.data(), L.m, K.data(), sig.data());
    mc.pack_init(block.data(), L, body.data(), flags.data(), q.data(), tr.data(), (size_t)n);
    const MapArgs a = L.m.args(block.data(), nullptr, C);
    // exactly the slots the call may write: a store of next_lid + n_initial landmarks
    std::vector<double> geom((size_t)(next_lid + job.n_initial) * 6);
    std::vector<int32_t> n_rays((size_t)(next_lid + job.n_initial));
    std::vector<MapOut> recs((size_t)n);
    InitCall call;
    memset(&call, 0, sizeof(call));
    init_run_serial(job, a, q.data(), tr.data(), flags.data(), recs.data(), call, geom.data(), n_rays.data());
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(recs.data(), sizeof(MapOut), recs.size(), o);
    fwrite(&call, sizeof(call), 1, o);
    fclose(o);
    return 0;
}
