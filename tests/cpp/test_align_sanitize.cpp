// test_align_sanitize.cpp -- csrc/mcorb_align.h's host path (align_run_serial: what a host-only store runs) as a stand-alone
// program, built by tests/test_align_cpu.py with -fsanitize=address,undefined.  argv[1]: a problem written by the test -- int32 n,
// H, mode, refit; double threshold, inlier_dist; uint64 seed; n points of frame 1, then n of frame 2 (3 doubles each).  argv[2]:
// the records written back -- the AlignOut, n flag bytes, H counts (int32) and H models.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mcorb_align.h"

using namespace mcorb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    AlignJob job = AlignJob();
    if (!get(f, head, 4) || !get(f, &job.threshold, 1) || !get(f, &job.inlier_dist, 1) || !get(f, &job.seed, 1)) return 3;
    job.n = head[0], job.H = head[1], job.mode = head[2], job.refit = head[3];
    const bool sac = job.mode == MCORB_ALIGN_MODE_SAC;
    if (job.n < 1 || (!sac && job.mode != MCORB_ALIGN_MODE_ALL) || (sac && (job.H < 1 || job.H > MCORB_ALIGN_MAX_ITERATIONS))) return 3;
    if (!sac) job.H = 0;
    std::vector<double> p1((size_t)job.n * 3), p2((size_t)job.n * 3);
    if (!get(f, p1.data(), p1.size()) || !get(f, p2.data(), p2.size())) return 3;
    fclose(f);
    std::vector<AlignModel> models((size_t)job.H);
    std::vector<int32_t> count((size_t)job.H);
    std::vector<uint8_t> member((size_t)job.n), flags((size_t)job.n);
    AlignOut out = AlignOut();
    align_run_serial(job, p1.data(), p2.data(), models.data(), count.data(), member.data(), out, flags.data());
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&out, sizeof(out), 1, f);
    fwrite(flags.data(), 1, flags.size(), f);
    if (job.H) {   // (mode 0 has neither)
        fwrite(count.data(), sizeof(int32_t), count.size(), f);
        fwrite(models.data(), sizeof(AlignModel), models.size(), f);
    }
    fclose(f);
    printf("status=%d best=%d n_inliers=%d n_models=%d bad=0\n", out.status, out.best, out.n_inliers, out.n_models);
    return 0;
}
