// mcorb_landmark_gpu.hip -- the kernels that keep a device store's landmarks up to date (mcorb_landmark.cpp): k_lmap_observe
// (Landmark::updateNormal(frame, featInd), GlobalMap.cpp:37-74, for a batch of addLfFrame calls of one keyframe), k_lmap_update
// (GlobalMap::updateLandmark, :162-185) and k_lmap_put_rays (ray counts into their slots).  The arithmetic is mcorb_landmark.h,
// the code the host-only store runs.  No extraction job runs them and no benchmark leg times them.
//
// One lane per item.  The keyframe's camera centres (MCORB_MAX_CAMS x 3 doubles) and max_diff are kernel arguments, uniform for
// the launch: scalar registers, as k_map_depth's pose.  A lane's own traffic is its 8-byte (32-byte) item, the slot's point and
// normal gathered by id and the plain stores of what changed: normal and ray count, or the point and the 16-byte result.  No LDS,
// no atomics, no lane talks to another.  A landmark that a batch names more than once depends on its own earlier result; the host
// launches such a batch in rounds (round r holds every landmark's r-th occurrence) on one stream, so no two lanes of a launch
// touch one slot and the launch shape cannot change a result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_kernels.h"
#include "mcorb_landmark.h"

namespace mcorb {

__global__ __launch_bounds__(256) void k_lmap_observe(LmCentres cen, int ncams, const LmObsItem *__restrict__ items, int n,
                                                      double *__restrict__ geom, int32_t *__restrict__ nrays)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const LmObsItem it = items[i];
    double *g = geom + (size_t)it.lid * 6;
    const double pt[3] = {g[0], g[1], g[2]};
    double normal[3] = {g[3], g[4], g[5]};
    int32_t nr = nrays[it.lid];
    lm_observe(cen, ncams, it.mask, pt, normal, nr);
    for (int k = 0; k < 3; k++) g[3 + k] = normal[k];
    nrays[it.lid] = nr;
}

void launch_lmap_observe(hipStream_t st, const LmCentres &cen, int ncams, const LmObsItem *items, int n, double *geom, int32_t *nrays)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_lmap_observe, dim3((n + 255) / 256), dim3(256), 0, st, cen, ncams, items, n, geom, nrays);
}

__global__ __launch_bounds__(256) void k_lmap_update(const LmUpdItem *__restrict__ items, int n, double max_diff,
                                                     double *__restrict__ geom, LmUpdOut *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const LmUpdItem it = items[i];
    double *g = geom + (size_t)it.lid * 6;
    double pt[3] = {g[0], g[1], g[2]};
    LmUpdOut o;
    o.updated = lm_update(pt, it.p, max_diff, o.diff_norm) ? 1 : 0;
    o.pad = 0;
    if (o.updated)
        for (int k = 0; k < 3; k++) g[k] = pt[k];
    out[it.idx] = o;
}

void launch_lmap_update(hipStream_t st, const LmUpdItem *items, int n, double max_diff, double *geom, LmUpdOut *out)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_lmap_update, dim3((n + 255) / 256), dim3(256), 0, st, items, n, max_diff, geom, out);
}

__global__ __launch_bounds__(256) void k_lmap_put_rays(const int32_t *__restrict__ lids, const int32_t *__restrict__ vals, int n,
                                                       int32_t *__restrict__ nrays)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    nrays[lids[i]] = vals ? vals[i] : 0;
}

void launch_lmap_put_rays(hipStream_t st, const int32_t *lids, const int32_t *vals, int n, int32_t *nrays)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_lmap_put_rays, dim3((n + 255) / 256), dim3(256), 0, st, lids, vals, n, nrays);
}

}  // namespace mcorb
