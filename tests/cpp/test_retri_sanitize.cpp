// test_retri_sanitize.cpp -- csrc/mcorb_retri.h's host path (retri_plan and retri_run_serial: what a host-only store runs) as a
// stand-alone program, built by tests/test_retri_cpu.py with -fsanitize=address,undefined.  argv[1]: a problem written by the
// test -- int32 nkf, ncams, nlm, nobs; rank_tol, the far and outlier thresholds, max_diff (double); ncams cameras (17 doubles
// each); the keyframes' R (9 nkf doubles), t (3 nkf) and moved flags (nkf bytes); the landmarks' points (3 nlm doubles); obs_kf,
// obs_cam, obs_lm (int32 each), uv (2 floats each).  The run is in apply mode on a store of its own whose slot j holds landmark
// j.  argv[2]: the records written back -- per landmark X, diff_norm, n_views, verdict -- and then the store's points.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mcorb_retri.h"

using namespace mcorb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    double par[4];
    if (!get(f, head, 4) || !get(f, par, 4)) return 3;
    RetriJob job = RetriJob();
    const int nkf = head[0], ncams = head[1], nlm = head[2], nobs = head[3];
    if (nkf < 1 || nkf > MCORB_RETRI_MAX_KF || ncams < 1 || ncams > MCORB_MAX_CAMS || nlm < 1 || nobs < 1) return 3;
    std::vector<double> R(9 * (size_t)nkf), t(3 * (size_t)nkf), pts(3 * (size_t)nlm);
    std::vector<uint8_t> moved((size_t)nkf);
    std::vector<int32_t> obs_kf((size_t)nobs), obs_cam((size_t)nobs), obs_lm((size_t)nobs);
    std::vector<float> uv(2 * (size_t)nobs);
    if (!get(f, job.cams, (size_t)ncams) || !get(f, R.data(), R.size()) || !get(f, t.data(), t.size()) || !get(f, moved.data(), moved.size()) ||
        !get(f, pts.data(), pts.size()) || !get(f, obs_kf.data(), obs_kf.size()) || !get(f, obs_cam.data(), obs_cam.size()) ||
        !get(f, obs_lm.data(), obs_lm.size()) || !get(f, uv.data(), uv.size()))
        return 3;
    fclose(f);
    for (int i = 0; i < nobs; i++)
        if (obs_kf[i] < 0 || obs_kf[i] >= nkf || obs_cam[i] < 0 || obs_cam[i] >= ncams || obs_lm[i] < 0 || obs_lm[i] >= nlm) return 3;
    RetriPlan plan;
    retri_plan(nkf, ncams, nlm, nobs, obs_lm.data(), obs_kf.data(), obs_cam.data(), uv.data(), plan);
    const int nslots = (int)plan.kf_of_slot.size();
    std::vector<PoseState> poses((size_t)nslots);
    std::vector<uint8_t> slot_moved((size_t)nslots);
    for (int s = 0; s < nslots; s++) {
        const size_t k = (size_t)plan.kf_of_slot[s];
        pose_load(poses[s], &R[9 * k], &t[3 * k]);
        slot_moved[s] = moved[k];
    }
    job.rank_tol = par[0], job.far_threshold = par[1], job.outlier_threshold = par[2], job.max_diff = par[3];
    job.ncams = ncams, job.nslots = nslots, job.nlm = nlm, job.nobs = nobs, job.apply = 1;
    std::vector<double> geom(6 * (size_t)nlm, 0.0);
    std::vector<int32_t> lids((size_t)nlm);
    for (int j = 0; j < nlm; j++) {
        lids[j] = j;
        for (int c = 0; c < 3; c++) geom[6 * (size_t)j + c] = pts[3 * (size_t)j + c];
    }
    std::vector<RetriOut> out((size_t)nlm);
    retri_run_serial(job, plan, poses.data(), slot_moved.data(), lids.data(), geom.data(), out.data());
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    int valid = 0;
    for (int j = 0; j < nlm; j++) {
        fwrite(out[j].X, sizeof(double), 3, f);
        fwrite(&out[j].diff_norm, sizeof(double), 1, f);
        fwrite(&out[j].n_views, sizeof(int32_t), 1, f);
        fwrite(&out[j].verdict, sizeof(int32_t), 1, f);
        valid += out[j].verdict == MCORB_RETRI_VALID_UPDATED;
    }
    for (int j = 0; j < nlm; j++) fwrite(&geom[6 * (size_t)j], sizeof(double), 3, f);
    fclose(f);
    printf("slots=%d updated=%d bad=0\n", nslots, valid);
    return 0;
}
