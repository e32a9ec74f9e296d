// test_pose_sanitize.cpp -- csrc/mcorb_pose.h's host path (the two rounds of pose_round over a serial pass whose lanes fold as the
// workgroup's do: what a host-only store runs for refine_pose) as a stand-alone program, built by tests/test_pose_cpu.py with
// -fsanitize=address,undefined.  argv[1]: a problem written by the test -- int32 ncams, n, nlevels, max_iterations; nlevels
// inv_sigma2 (double); ncams cameras (17 doubles each); the initial R (9 doubles) and t (3); cam (n int32), uv (2 floats each),
// octave (n int32), the points (3 n doubles).  argv[2]: the records written back -- the mcorb_pose_result, then n flag bytes.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mcorb_pose.h"

using namespace mcorb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

// lane l adds observations l, l + MCORB_POSE_LANES, ..; the lanes fold as the workgroup does
struct Pass {
    const PoseJob &job;
    const PoseObs *obs;
    const double *pts;
    const uint8_t *alive;
    int n;
    std::vector<double> s;
    void operator()(const PoseState &P, double S[kPoseSums])
    {
        double(*lanes)[kPoseSums] = (double(*)[kPoseSums])s.data();
        for (int l = 0; l < MCORB_POSE_LANES; l++) {
            for (int k = 0; k < kPoseSums; k++) lanes[l][k] = 0.0;
            for (int i = l; i < n; i += MCORB_POSE_LANES)
                if (alive[i]) pose_add(job.cams[obs[i].cam], P, pts + 3 * (size_t)i, obs[i].u, obs[i].v, job.huber_k, lanes[l]);
        }
        pose_fold(lanes, S);
    }
};

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    if (!get(f, head, 4)) return 3;
    const int ncams = head[0], n = head[1], nlevels = head[2];
    if (ncams < 1 || ncams > MCORB_MAX_CAMS || n < 1 || nlevels < 1 || nlevels > MCORB_MAX_LEVELS || head[3] < 1 || head[3] > 100) return 3;
    std::vector<PoseJob> jobs(1);
    PoseJob &job = jobs[0];
    memset(&job, 0, sizeof(job));
    std::vector<int32_t> cam((size_t)n), octave((size_t)n);
    std::vector<float> uv(2 * (size_t)n);
    std::vector<double> pts(3 * (size_t)n);
    if (!get(f, job.inv_sigma2, (size_t)nlevels) || !get(f, job.cams, (size_t)ncams) || !get(f, job.init.R, 9) || !get(f, job.init.t, 3) ||
        !get(f, cam.data(), cam.size()) || !get(f, uv.data(), uv.size()) || !get(f, octave.data(), octave.size()) || !get(f, pts.data(), pts.size()))
        return 3;
    fclose(f);
    job.ncams = ncams, job.nlevels = nlevels, job.max_iterations = head[3], job.n = n;
    job.huber_k = sqrt(5.991);
    std::vector<PoseObs> obs((size_t)n);
    for (int i = 0; i < n; i++) {
        if (cam[i] < 0 || cam[i] >= ncams || octave[i] < 0 || octave[i] >= nlevels) return 3;
        obs[i] = PoseObs{uv[2 * i], uv[2 * i + 1], cam[i], octave[i]};
    }
    std::vector<uint8_t> alive((size_t)n, 1);
    mcorb_pose_result res;
    memset(&res, 0, sizeof(res));
    res.n_obs = n;
    Pass pass{job, obs.data(), pts.data(), alive.data(), n, std::vector<double>((size_t)MCORB_POSE_LANES * kPoseSums)};
    PoseState pose = job.init;
    for (int round = 0; round < 2; round++) {
        double c0, c1;
        pose_round(pass, job.init, job.max_iterations, pose, res.iterations[round], res.status, c0, c1);
        if (round == 0) res.cost_initial = pose_default_nan(c0);
        res.cost_final = pose_default_nan(c1);
        for (int i = 0; i < n; i++)
            if (alive[i] && pose_is_outlier(job.cams[obs[i].cam], pose, &pts[3 * (size_t)i], obs[i].u, obs[i].v, job.inv_sigma2[obs[i].octave]))
                alive[i] = 0;
    }
    memcpy(res.R, pose.R, sizeof(res.R));
    memcpy(res.t, pose.t, sizeof(res.t));
    for (int i = 0; i < n; i++) res.n_inliers += alive[i];
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&res, sizeof(res), 1, f);
    fwrite(alive.data(), 1, alive.size(), f);
    fclose(f);
    printf("status=%d iterations=%d,%d n_inliers=%d bad=0\n", res.status, res.iterations[0], res.iterations[1], res.n_inliers);
    return 0;
}
