// test_init_sanitize.cpp -- init_run_serial (csrc/mcorb_init.h), the host-only store's path of mcorb_lmap_initialize, as a plain
// g++ program under -fsanitize=address,undefined (tests/test_init_cpu.py builds and runs it).  argv[1]: the scene as
// test_init_cpu.py writes it; argv[2]: the records of all matches, then the call's record, which the test compares with the
// library's.  The frames are packed here the way mcorb_init.cpp packs them: the current frame first, its centres cam_centre_body.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mcorb_init.h"

using namespace mcorb;

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
    std::vector<MapFrameDev> frames(2);
    std::vector<int32_t> mi;
    std::vector<MapKp> kp;
    for (int fr = 0; fr < 2; fr++) {
        MapFrameDev &d = frames[fr];
        memset(&d, 0, sizeof(d));
        const std::vector<int32_t> rows = rd<int32_t>(f, (size_t)nfeat[fr] * C);
        const std::vector<double> proj = rd<double>(f, (size_t)C * 12), centre = rd<double>(f, (size_t)C * 3);
        const std::vector<int32_t> nk = rd<int32_t>(f, (size_t)C);
        d.mi_off = (int32_t)mi.size();
        mi.insert(mi.end(), rows.begin(), rows.end());
        memcpy(d.proj, proj.data(), proj.size() * sizeof(double));
        memcpy(d.centre, fr == 0 ? body.data() : centre.data(), (size_t)C * 3 * sizeof(double));
        for (int c = 0; c < C; c++) {
            d.kp_off[c] = (int32_t)kp.size();
            const std::vector<float> xy = rd<float>(f, (size_t)nk[c] * 2);
            const std::vector<int32_t> oct = rd<int32_t>(f, (size_t)nk[c]);
            for (int k = 0; k < nk[c]; k++) kp.push_back(MapKp{xy[2 * k], xy[2 * k + 1], oct[k]});
        }
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
    MapArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = frames.data();
    a.mi = mi.data();
    a.kp = kp.data();
    a.K = K.data();
    a.inv_sigma2 = sig.data();
    a.ncams = C;
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
