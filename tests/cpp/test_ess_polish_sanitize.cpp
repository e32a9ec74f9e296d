// test_ess_polish_sanitize.cpp -- the host path of the polished essential pose (csrc/mcorb_ess.h's ess_run_serial + csrc/
// mcorb_ess_polish.h's ess_polish_serial: what a host-only store runs) as a stand-alone program, built by tests/
// test_ess_polish_cpu.py with -fsanitize=address,undefined.
// argv[1]: a problem written by the test -- int32 S, H, rounds, max_iterations; double fx, fy, s, u0, v0, threshold_px, distance;
// uint64 seed; S matches (u1, v1, u2, v2 as floats).  argv[2]: the records written back -- the EssOut with the accepted pose, E and
// counts, the mcorb_ess_polish, S flag bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mcorb_ess_polish.h"

using namespace mcorb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    double cal[7];
    EssJob job = EssJob();
    if (!get(f, head, 4) || !get(f, cal, 7) || !get(f, &job.seed, 1)) return 3;
    job.S = head[0], job.H = head[1];
    const int rounds = head[2], max_iterations = head[3];
    if (job.S < 1 || job.H < 1 || job.H > MCORB_ESS_MAX_ITERATIONS) return 3;
    if (rounds < 1 || rounds > kEssFitRounds || max_iterations < 1 || max_iterations > kEssFitMaxIterations) return 3;
    job.fx = cal[0], job.fy = cal[1], job.s = cal[2], job.u0 = cal[3], job.v0 = cal[4];
    const double thr = cal[5] / ((job.fx + job.fy) / 2.0);
    job.threshold2 = thr * thr;
    job.distance = cal[6];
    std::vector<EssObs> obs((size_t)job.S);
    if (!get(f, obs.data(), obs.size())) return 3;
    fclose(f);
    const size_t slots = (size_t)job.H * kEssRoots;
    std::vector<EssModel> models(slots);
    std::vector<int32_t> samples((size_t)job.H * kEssSample), count(slots);
    std::vector<EssPt> pts((size_t)job.S);
    std::vector<uint8_t> flags((size_t)job.S);
    EssOut out = EssOut();
    ess_run_serial(job, obs.data(), models.data(), samples.data(), count.data(), pts.data(), out, flags.data());
    EssPolish rec;
    PoseState P;
    memcpy(P.R, out.R, sizeof(P.R));
    memcpy(P.t, out.t, sizeof(P.t));
    if (out.status == MCORB_ESS_OK) {
        std::vector<uint8_t> member(flags), scratch((size_t)job.S);
        std::vector<double> lanes((size_t)MCORB_POSE_LANES * kEssFitSums);
        ess_polish_serial(pts.data(), job.S, job.threshold2, job.distance, ess_fit_scale(cal[5], job.fx, job.fy), rounds, max_iterations, P, out.E,
                          out.n_ransac_inliers, out.n_inliers, flags.data(), member.data(), scratch.data(),
                          reinterpret_cast<double (*)[kEssFitSums]>(lanes.data()), rec);
        memcpy(out.R, P.R, sizeof(P.R));
        memcpy(out.t, P.t, sizeof(P.t));
    } else {
        ess_polish_begin(rec, P, out.E, out.n_ransac_inliers, out.n_inliers);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&out, sizeof(out), 1, f);
    fwrite(&rec, sizeof(rec), 1, f);
    fwrite(flags.data(), 1, flags.size(), f);
    fclose(f);
    printf("status=%d n_inliers=%d rounds_run=%d bad=0\n", out.status, out.n_inliers, rec.rounds_run);
    return 0;
}
