// test_rel_polish_sanitize.cpp -- csrc/mcorb_rel.h's host path of the polished relative pose (rel_run_serial + rel_polish_serial:
// what a host-only store runs) as a stand-alone program, built by tests/test_rel_polish_cpu.py with -fsanitize=address,undefined.
// argv[1]: a problem written by the test -- int32 ncams, S, H, rounds; double threshold; uint64 seed; int32 max_iterations, 0; ncams
// cameras (17 doubles each); S matches (u1, v1, u2, v2 as floats, cam1, cam2 as int32).  argv[2]: the records written back -- the
// RelOut with the accepted pose and count, the mcorb_rel_polish, S flag bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mcorb_rel.h"

using namespace mcorb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4], tail[2];
    RelJob job = RelJob();
    if (!get(f, head, 4) || !get(f, &job.threshold, 1) || !get(f, &job.seed, 1) || !get(f, tail, 2)) return 3;
    job.ncams = head[0], job.S = head[1], job.H = head[2];
    const int rounds = head[3], max_iterations = tail[0];
    if (job.ncams < 1 || job.ncams > MCORB_MAX_CAMS || job.S < 1 || job.H < 1 || job.H > MCORB_REL_MAX_ITERATIONS) return 3;
    if (rounds < 1 || rounds > kRelFitRounds || max_iterations < 1 || max_iterations > kRelFitMaxIterations) return 3;
    std::vector<RelObs> obs((size_t)job.S);
    if (!get(f, job.cams, (size_t)job.ncams) || !get(f, obs.data(), obs.size())) return 3;
    fclose(f);
    for (const RelObs &o : obs)
        if (o.cam1 < 0 || o.cam1 >= job.ncams || o.cam2 < 0 || o.cam2 >= job.ncams) return 3;
    std::vector<RelModel> models((size_t)job.H);
    std::vector<int32_t> count((size_t)job.H);
    std::vector<RelRays> rays((size_t)job.S);
    std::vector<uint8_t> flags((size_t)job.S);
    RelOut out = RelOut();
    rel_run_serial(job, obs.data(), models.data(), count.data(), rays.data(), out, flags.data());
    RelPolish rec;
    PoseState P;
    memcpy(P.R, out.R, sizeof(P.R));
    memcpy(P.t, out.t, sizeof(P.t));
    if (out.best >= 0) {
        std::vector<uint8_t> member(flags), scratch((size_t)job.S);
        std::vector<double> lanes((size_t)MCORB_POSE_LANES * kPoseSums);
        rel_polish_serial(rays.data(), job.S, job.threshold, rounds, max_iterations, P, out.n_inliers, flags.data(), member.data(),
                          scratch.data(), reinterpret_cast<double (*)[kPoseSums]>(lanes.data()), rec);
        memcpy(out.R, P.R, sizeof(P.R));
        memcpy(out.t, P.t, sizeof(P.t));
    } else {
        rel_polish_begin(rec, P, out.n_inliers);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&out, sizeof(out), 1, f);
    fwrite(&rec, sizeof(rec), 1, f);
    fwrite(flags.data(), 1, flags.size(), f);
    fclose(f);
    printf("best=%d n_inliers=%d rounds_run=%d bad=0\n", out.best, out.n_inliers, rec.rounds_run);
    return 0;
}
