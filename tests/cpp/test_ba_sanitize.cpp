// test_ba_sanitize.cpp -- csrc/mcorb_ba.h's host path (ba_plan and ba_run_serial: what a host-only store runs) as a stand-alone
// program, built by tests/test_ba_cpu.py with -fsanitize=address,undefined.  argv[1]: a problem written by the test -- int32 nkf,
// ncams, nlm, nobs, nlevels, max_iterations; nlevels sigmas (double); ncams cameras (17 doubles each); the keyframes' R (9 nkf
// doubles), t (3 nkf) and fixed flags (nkf bytes); the points (3 nlm doubles); obs_kf, obs_cam, obs_lm (int32 each), uv (2 floats
// each), octave (int32).  argv[2]: the records written back -- the mcorb_ba_result, R, t, the points, nobs flag bytes.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mcorb_ba.h"

using namespace mcorb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[6];
    if (!get(f, head, 6)) return 3;
    BaJob job = BaJob();
    job.nkf = head[0], job.ncams = head[1], job.nlm = head[2], job.nobs = head[3], job.max_iterations = head[5];
    const int nlevels = head[4];
    if (job.nkf < 1 || job.nkf > MCORB_BA_MAX_KF || job.ncams < 1 || job.ncams > MCORB_MAX_CAMS || job.nlm < 1 || job.nobs < 1 || nlevels < 1 ||
        nlevels > MCORB_MAX_LEVELS)
        return 3;
    double sigma[MCORB_MAX_LEVELS];
    const size_t nkf = job.nkf, nlm = job.nlm, nobs = job.nobs;
    std::vector<double> R(9 * nkf), t(3 * nkf), pts(3 * nlm);
    std::vector<uint8_t> fixed(nkf), flags(nobs);
    std::vector<int32_t> obs_kf(nobs), obs_cam(nobs), obs_lm(nobs), octave(nobs);
    std::vector<float> uv(2 * nobs);
    if (!get(f, sigma, (size_t)nlevels) || !get(f, job.cams, (size_t)job.ncams) || !get(f, R.data(), R.size()) || !get(f, t.data(), t.size()) ||
        !get(f, fixed.data(), nkf) || !get(f, pts.data(), pts.size()) || !get(f, obs_kf.data(), nobs) || !get(f, obs_cam.data(), nobs) ||
        !get(f, obs_lm.data(), nobs) || !get(f, uv.data(), uv.size()) || !get(f, octave.data(), nobs))
        return 3;
    fclose(f);
    for (size_t i = 0; i < nobs; i++)
        if (obs_kf[i] < 0 || obs_kf[i] >= job.nkf || obs_cam[i] < 0 || obs_cam[i] >= job.ncams || obs_lm[i] < 0 || obs_lm[i] >= job.nlm ||
            octave[i] < 0 || octave[i] >= nlevels)
            return 3;
    for (int l = 0; l < nlevels; l++) job.inv_s[l] = 1.0 / sigma[l];
    job.huber_k = sqrt(5.991);
    std::vector<PoseState> poses(nkf);
    for (size_t k = 0; k < nkf; k++) {
        for (int i = 0; i < 9; i++) poses[k].R[i] = R[9 * k + i];
        for (int i = 0; i < 3; i++) poses[k].t[i] = t[3 * k + i];
    }
    BaPlan plan;
    ba_plan(job, fixed.data(), obs_kf.data(), obs_cam.data(), obs_lm.data(), uv.data(), octave.data(), plan);
    mcorb_ba_result res = mcorb_ba_result();
    ba_run_serial(job, plan, poses.data(), pts.data(), res, flags.data());
    for (size_t k = 0; k < nkf; k++) {
        for (int i = 0; i < 9; i++) R[9 * k + i] = poses[k].R[i];
        for (int i = 0; i < 3; i++) t[3 * k + i] = poses[k].t[i];
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&res, sizeof(res), 1, f);
    fwrite(R.data(), sizeof(double), R.size(), f);
    fwrite(t.data(), sizeof(double), t.size(), f);
    fwrite(pts.data(), sizeof(double), pts.size(), f);
    fwrite(flags.data(), 1, flags.size(), f);
    fclose(f);
    printf("status=%d iterations=%d n_inliers=%d views=%d bad=0\n", res.status, res.iterations, res.n_inliers, job.nviews);
    return 0;
}
