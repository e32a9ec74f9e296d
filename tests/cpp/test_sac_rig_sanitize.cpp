// test_sac_rig_sanitize.cpp -- csrc/mcorb_sac.h's host path with the rig solver (sac_run_serial with MCORB_SAC_SOLVER_RIG: what a
// host-only store runs) as a stand-alone program, built by tests/test_sac_rig_cpu.py with -fsanitize=address,undefined.  argv[1]: a
// problem written by the test -- int32 ncams, n, S, H; double threshold; uint64 seed; ncams cameras (17 doubles each); n
// observations (u, v as floats, cam, octave as int32); n points (3 doubles each); cons (S) as int32 (the rig solver's sample reads
// no per-camera lists: none are given).  argv[2]: the records written back -- the SacOut, n flag bytes, H counts (int32) and H
// models.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mcorb_sac.h"

using namespace mcorb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    SacJob job = SacJob();
    if (!get(f, head, 4) || !get(f, &job.threshold, 1) || !get(f, &job.seed, 1)) return 3;
    job.ncams = head[0], job.n = head[1], job.S = head[2], job.H = head[3];
    job.solver = MCORB_SAC_SOLVER_RIG;
    if (job.ncams < 1 || job.ncams > MCORB_MAX_CAMS || job.n < 1 || job.S < 1 || job.S > job.n || job.H < 1) return 3;
    std::vector<PoseObs> obs((size_t)job.n);
    std::vector<double> X((size_t)job.n * 3), bearings((size_t)job.S * 3);
    std::vector<int32_t> cons((size_t)job.S), count((size_t)job.H);
    if (!get(f, job.cams, (size_t)job.ncams) || !get(f, obs.data(), obs.size()) || !get(f, X.data(), X.size()) || !get(f, cons.data(), cons.size()))
        return 3;
    fclose(f);
    std::vector<SacModel> models((size_t)job.H);
    std::vector<uint8_t> flags((size_t)job.n);
    SacOut out = SacOut();
    sac_run_serial(job, obs.data(), X.data(), cons.data(), nullptr, nullptr, models.data(), count.data(), bearings.data(), out, flags.data());
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&out, sizeof(out), 1, f);
    fwrite(flags.data(), 1, flags.size(), f);
    fwrite(count.data(), sizeof(int32_t), count.size(), f);
    fwrite(models.data(), sizeof(SacModel), models.size(), f);
    fclose(f);
    printf("best=%d n_inliers=%d n_models=%d bad=0\n", out.best, out.n_inliers, out.n_models);
    return 0;
}
