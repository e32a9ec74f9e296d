// test_ess_sanitize.cpp -- the host path of the essential-matrix pose (csrc/mcorb_ess.h, ess_run_serial) as a stand-alone program,
// built by tests/test_ess_cpu.py with -fsanitize=address,undefined.  Input file: n, H (int32), fx, fy, s, u0, v0, threshold_px,
// distance_thresh (double), seed (uint64), then n matches of four floats.  Output file: the EssOut record, the n flags, the 10 H
// counts, the 5 H sample members and the 10 H EssModel records.  Prints "bad=0" when it ran to the end.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mcorb.h"
#include "mcorb_ess.h"

using namespace mcorb;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[2];
    double par[7];
    uint64_t seed;
    int bad = 0;
    bad += fread(head, sizeof(head), 1, f) != 1;
    bad += fread(par, sizeof(par), 1, f) != 1;
    bad += fread(&seed, sizeof(seed), 1, f) != 1;
    const int n = head[0], H = head[1];
    std::vector<EssObs> obs((size_t)n);
    bad += fread(obs.data(), sizeof(EssObs), (size_t)n, f) != (size_t)n;
    fclose(f);
    if (bad) return 2;

    EssJob job;
    memset(&job, 0, sizeof(job));
    job.fx = par[0], job.fy = par[1], job.s = par[2], job.u0 = par[3], job.v0 = par[4];
    const double thr = par[5] / ((job.fx + job.fy) / 2.0);
    job.threshold2 = thr * thr;
    job.distance = par[6];
    job.seed = seed;
    job.S = n;
    job.H = H;

    std::vector<EssModel> models((size_t)H * kEssRoots);
    std::vector<int32_t> samples((size_t)H * kEssSample), count((size_t)H * kEssRoots);
    std::vector<EssPt> pts((size_t)n);
    std::vector<uint8_t> flags((size_t)n);
    EssOut out;
    memset(&out, 0, sizeof(out));
    ess_run_serial(job, obs.data(), models.data(), samples.data(), count.data(), pts.data(), out, flags.data());

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    bad += fwrite(&out, sizeof(out), 1, f) != 1;
    bad += fwrite(flags.data(), 1, flags.size(), f) != flags.size();
    bad += fwrite(count.data(), sizeof(int32_t), count.size(), f) != count.size();
    bad += fwrite(samples.data(), sizeof(int32_t), samples.size(), f) != samples.size();
    bad += fwrite(models.data(), sizeof(EssModel), models.size(), f) != models.size();
    fclose(f);
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
