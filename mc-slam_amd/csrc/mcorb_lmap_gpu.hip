// mcorb_lmap_gpu.hip -- the local map's kernels (mcorb_lmap.cpp): k_lmap_cull (the frustum test of FrontEnd::searchLocalMap2,
// FrontEnd.cpp:5000-5027, for every candidate landmark and camera) and k_lmap_put (a batch of points, normals and descriptors
// into their slots).  The descent and the best / second-best search of a search are k_bow_descend and k_kfdb_best2.  No
// extraction job runs them and no benchmark leg times them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcorb.h"
#include "mcorb_common.h"
#include "mcorb_kernels.h"

namespace mcorb {

// One lane per candidate, the cameras looped inside: the view is uniform, so its 24 doubles per camera come through the scalar
// cache; a lane's own traffic is its 48 bytes of point and normal, gathered by landmark id, and the 4-byte mask.  All arithmetic
// is fp64 with separate multiplies and adds (the file is built with -ffp-contract=off) in cv::Mat's order: an element of a small
// matrix product is the sum over k ascending, from 0.0, of a[k] * b[k], and the addend of `A * b + c` comes last.  sqrt and
// 1.0 / z are the correctly rounded IEEE operations, as on the host.  The comparisons keep the reference's form, so that a NaN
// (tmp_z == 0 with a zero numerator) fails none of them and the camera is kept.
// No LDS, no atomics, no lane talks to another: the host compacts the masks in candidate order.
__global__ __launch_bounds__(kLmapCullT) void k_lmap_cull(const mcorb_lmap_view *__restrict__ view, const double *__restrict__ geom,
                                                          const int *__restrict__ cand, int n, uint32_t *__restrict__ masks)
{
    const int i = blockIdx.x * kLmapCullT + threadIdx.x;
    if (i >= n) return;
    const double *g = geom + (size_t)cand[i] * 6;
    const double pt[3] = {g[0], g[1], g[2]}, nrm[3] = {g[3], g[4], g[5]};
    double body[3];
    for (int r = 0; r < 3; r++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s += view->Rcw[3 * r + k] * pt[k];
        body[r] = s + view->tcw[r];
    }
    const int ncams = view->ncams;
    const double xmax = (double)(view->width - 30), ymax = (double)(view->height - 30);
    uint32_t mask = 0;
    for (int c = 0; c < ncams; c++) {
        const mcorb_lmap_cam &cam = view->cams[c];
        double pc[3];
        for (int r = 0; r < 3; r++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += cam.R[3 * r + k] * body[k];
            pc[r] = s + cam.t[r];
        }
        if (pc[2] < 0) continue;
        double dot = 0.0, sq = 0.0;
        for (int k = 0; k < 3; k++) {
            const double d = pt[k] - cam.centre_w[k];
            dot += nrm[k] * d;
            sq += d * d;
        }
        if (dot < 0.5 * sqrt(sq)) continue;
        double tmp[3];
        for (int r = 0; r < 3; r++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += cam.K[3 * r + k] * pc[k];
            tmp[r] = s;
        }
        const double inv = 1.0 / tmp[2];
        const double x = tmp[0] * inv, y = tmp[1] * inv;
        if (x < 30 || x > xmax) continue;
        if (y < 30 || y > ymax) continue;
        mask |= 1u << c;
    }
    masks[i] = mask;
}

void launch_lmap_cull(hipStream_t st, const mcorb_lmap_view *view, const double *geom, const int *cand, int n, uint32_t *masks)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_lmap_cull, dim3((n + kLmapCullT - 1) / kLmapCullT), dim3(kLmapCullT), 0, st, view, geom, cand, n, masks);
}

// the host lists every slot at most once per batch (a repeated id keeps its last entry, the others become -1), so no two lanes
// write one slot
__global__ __launch_bounds__(256) void k_lmap_put(const int *__restrict__ lids, int n, const double *__restrict__ pt,
                                                  const double *__restrict__ normal, const uint8_t *__restrict__ src_desc,
                                                  const int *__restrict__ rows, double *__restrict__ geom, uint8_t *__restrict__ desc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int slot = lids[i];
    if (slot < 0) return;
    if (pt)
        for (int k = 0; k < 3; k++) geom[(size_t)slot * 6 + k] = pt[3 * (size_t)i + k];
    if (normal)
        for (int k = 0; k < 3; k++) geom[(size_t)slot * 6 + 3 + k] = normal[3 * (size_t)i + k];
    if (src_desc) {
        const size_t row = rows ? (size_t)rows[i] : (size_t)i;
        *reinterpret_cast<ulonglong4 *>(desc + (size_t)slot * 32) = *reinterpret_cast<const ulonglong4 *>(src_desc + row * 32);
    }
}

void launch_lmap_put(hipStream_t st, const int *lids, int n, const double *pt, const double *normal, const uint8_t *src_desc,
                     const int *rows, double *geom, uint8_t *desc)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_lmap_put, dim3((n + 255) / 256), dim3(256), 0, st, lids, n, pt, normal, src_desc, rows, geom, desc);
}

}  // namespace mcorb
