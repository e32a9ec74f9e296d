// mcorb_lf_gpu.hip -- k_lf_tracks: the per-track half of FrontEnd::obtainLfFeatures (MCSlam/src/FrontEnd.cpp:280-349) on gfx950,
// for every track of every frame of an extraction job in one launch (mcorb_rig_set_lf).  One lane per track: gather the views,
// normalise the raw keypoints ((x - cx) / fx, :291-293), triangulate (cv::sfm::triangulatePoints, mcorb_triangulate.h), gate on
// 0.5 < z < 40 (:309), project K_0 X to the reference camera (:339-341) and pick computeRepresentativeDesc's view from the
// descriptors in HBM (:349).  The host (lf_job_finish) orders the tracks by view count, so a wave runs one compile-time shape of
// the null-vector solver; the records go straight to host-mapped memory.  What stays on the host is order-dependent: the
// keypoint mask, the mono pool and argsorte's std::sort.
//
// Registers and scratch: the solver's LU and permutation arrays are indexed by run-time pivots, and the run-time-shaped solver
// (five views or more) holds up to a 48 x 20 design, so the kernel keeps its arrays in scratch.  At one lane per track and a
// few thousand tracks per rig frame the launch is latency-bound (tools/live_lf.cpp).
#include <hip/hip_runtime.h>

#include "mcorb_common.h"
#include "mcorb_kernels.h"
#include "mcorb_triangulate.h"

namespace mcorb {

constexpr int kLfBlock = 64;   // one wave per workgroup: the tracks of one shape bin fill whole waves

template <bool kAnyViews>
__global__ __launch_bounds__(kLfBlock) void k_lf_tracks(const int4 *__restrict__ trk, const LfView *__restrict__ views, int ntr,
                                                        const LfCam *__restrict__ cams, const uint8_t *__restrict__ desc, int kcap,
                                                        int ncams, LfTrackOut *__restrict__ out)
{
    const int t = blockIdx.x * kLfBlock + threadIdx.x;
    if (t >= ntr) return;
    const int4 r = trk[t];   // {first view, view count, frame, output record}
    const int nv = r.y;
    double xx[2 * MCORB_MAX_CAMS];
    const double *PJs[MCORB_MAX_CAMS];
    const uint8_t *rows[MCORB_MAX_CAMS];
    for (int ii = 0; ii < nv; ii++) {
        const LfView v = views[r.x + ii];
        const LfCam &c = cams[v.cam];
        PJs[ii] = c.Rt;
        xx[2 * ii] = ((double)v.x - c.K[2]) / c.K[0];          // (pt.x - cx) / fx
        xx[2 * ii + 1] = ((double)v.y - c.K[5]) / c.K[4];
        rows[ii] = desc + ((size_t)(r.z * ncams + v.cam) * kcap + v.kp) * 32;
    }
    LfTrackOut o;
    triangulate<kAnyViews>(xx, PJs, nv, o.X);
    o.accept = o.X[2] < 40 && o.X[2] > 0.5;
    o.uv[0] = o.uv[1] = 0.f;
    o.rep = 0;
    if (o.accept) {
        const double *K0 = cams[0].K, *X = o.X;
        const double px = K0[0] * X[0] + K0[1] * X[1] + K0[2] * X[2], py = K0[3] * X[0] + K0[4] * X[1] + K0[5] * X[2],
                     pz = K0[6] * X[0] + K0[7] * X[1] + K0[8] * X[2];
        o.uv[0] = (float)(px / pz);
        o.uv[1] = (float)(py / pz);
        o.rep = representative_desc(rows, nv);
    }
    out[r.w] = o;
}

void launch_lf_tracks(hipStream_t st, const int4 *trk, const LfView *views, int ntr, const LfCam *cams, const uint8_t *desc, int kcap,
                      int ncams, LfTrackOut *out)
{
    if (ntr <= 0) return;
    // (a rig of up to four cameras has tracks of up to four views: the instance without the run-time-shaped solver)
    if (ncams <= 4)
        hipLaunchKernelGGL(k_lf_tracks<false>, dim3((ntr + kLfBlock - 1) / kLfBlock), dim3(kLfBlock), 0, st, trk, views, ntr, cams, desc,
                           kcap, ncams, out);
    else
        hipLaunchKernelGGL(k_lf_tracks<true>, dim3((ntr + kLfBlock - 1) / kLfBlock), dim3(kLfBlock), 0, st, trk, views, ntr, cams, desc,
                           kcap, ncams, out);
}

// mcorb_dev_triangulate_selftest: problem i has nv[i] views starting at view voff[i] (x: 2 doubles per view, P: 12 per view)
__global__ __launch_bounds__(kLfBlock) void k_tri_selftest(const double *__restrict__ x, const double *__restrict__ P,
                                                           const int *__restrict__ nv, const int *__restrict__ voff, int n,
                                                           double *__restrict__ X, int *__restrict__ branch)
{
    const int i = blockIdx.x * kLfBlock + threadIdx.x;
    if (i >= n) return;
    const int v0 = voff[i], k = nv[i];
    const double *PJs[MCORB_MAX_CAMS];
    for (int ii = 0; ii < k; ii++) PJs[ii] = P + (size_t)12 * (v0 + ii);
    double Xi[3];
    branch[i] = triangulate(x + (size_t)2 * v0, PJs, k, Xi);
    for (int j = 0; j < 3; j++) X[(size_t)3 * i + j] = Xi[j];
}

void launch_tri_selftest(hipStream_t st, const double *x, const double *P, const int *nv, const int *voff, int n, double *X, int *branch)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_tri_selftest, dim3((n + kLfBlock - 1) / kLfBlock), dim3(kLfBlock), 0, st, x, P, nv, voff, n, X, branch);
}

}  // namespace mcorb
