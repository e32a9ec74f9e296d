// mcorb_mapping_gpu.hip -- the kernels of mcorb_lmap_triangulate_neighbours (mcorb_mapping.cpp): k_map_triangulate (one inter-frame
// match of FrontEnd::triangulateMatches, FrontEnd.cpp:5826-5933, per lane: the views, the epipolar gate, the N-view DLT, the
// reprojection and parallax gates and the new landmark's normal, mcorb_mapping.h), k_map_depth (getSceneDepthStats' z, :4846-4847),
// k_map_put (accepted points, normals and ray counts from the result records into the local map's slots) and the gates' self-test.  No
// extraction job runs them and no benchmark leg times them.
//
// k_map_triangulate: one wave per workgroup, and a wave's matches belong to ONE neighbour (the host cuts every neighbour's matches
// into blocks of up to 64 and orders them by view count), so the block record, the frame tables' bases and the F table's base are
// uniform and come through the scalar cache; what a lane indexes by its own camera (a projection matrix, a centre, K, one F) and
// its keypoints are vector loads that hit L1 / L2 -- a call's whole input is one block of a few hundred KiB.  A lane writes its
// 80-byte record with plain stores.  No LDS, no atomics, no workgroup waits on another; a record depends on the match alone, so
// the launch shape cannot change it.  Two instances, as k_lf_tracks has: matches of at most 4 views in total (2 views is almost
// every match of a non-overlapping rig) without the run-time-shaped solver, and the general one, whose 48 x 20 design lives in
// scratch.  The solver's arrays are indexed by run-time pivots, so both keep them in scratch (DESIGN.md section 9d has the figures).
//
// k_map_refine_new (mcorb_lmap_triangulate_new): one match of FrontEnd::TriangulateNewLandmarks (:6465-6700) per lane, the same block
// record, tables and two instances; after the DLT a lane runs its own 3-unknown Levenberg-Marquardt (mcorb_mapping_new.h) with X, H,
// g, the trial, lambda and the costs in registers, and every pass walks the lane's views again from MapViews.  Lanes of a wave leave
// the loop after different numbers of solves and the wave runs until its slowest lane ends; 50 solves bound it (section 9h).
#include <hip/hip_runtime.h>

#include "mcorb_common.h"
#include "mcorb_kernels.h"
#include "mcorb_mapping_new.h"

namespace mcorb {

template <bool kAnyViews>
__global__ __launch_bounds__(kMapBlock) void k_map_triangulate(MapArgs a, int block0)
{
    MapBlock b;
    if (map_lane(a, block0, b)) map_item<kAnyViews>(a, b.seg, a.items[b.first + threadIdx.x]);
}

void launch_map_triangulate(hipStream_t st, const MapArgs &a, int nblocks_small, int nblocks_any)
{
    if (nblocks_small > 0) hipLaunchKernelGGL(k_map_triangulate<false>, dim3(nblocks_small), dim3(kMapBlock), 0, st, a, 0);
    if (nblocks_any > 0) hipLaunchKernelGGL(k_map_triangulate<true>, dim3(nblocks_any), dim3(kMapBlock), 0, st, a, nblocks_small);
}

template <bool kAnyViews>
__global__ __launch_bounds__(kMapBlock) void k_map_refine_new(MapNewArgs n, int block0)
{
    MapBlock b;
    if (map_lane(n.a, block0, b)) map_new_item<kAnyViews>(n, n.a.items[b.first + threadIdx.x]);
}

void launch_map_refine_new(hipStream_t st, const MapNewArgs &n, int nblocks_small, int nblocks_any)
{
    if (nblocks_small > 0) hipLaunchKernelGGL(k_map_refine_new<false>, dim3(nblocks_small), dim3(kMapBlock), 0, st, n, 0);
    if (nblocks_any > 0) hipLaunchKernelGGL(k_map_refine_new<true>, dim3(nblocks_any), dim3(kMapBlock), 0, st, n, nblocks_small);
}

// the pose (12 doubles) is a kernel argument: scalar registers
struct MapPose { double Rcw[9], tcw[3]; };

__global__ __launch_bounds__(256) void k_map_depth(MapPose pose, const double *__restrict__ geom, const int *__restrict__ lids, int n,
                                                   double *__restrict__ z)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *g = geom + (size_t)lids[i] * 6;
    const double pt[3] = {g[0], g[1], g[2]};
    z[i] = map_depth(pose.Rcw, pose.tcw, pt);
}

void launch_map_depth(hipStream_t st, const double Rcw[9], const double tcw[3], const double *geom, const int *lids, int n, double *z)
{
    if (n < 1) return;
    MapPose p;
    for (int k = 0; k < 9; k++) p.Rcw[k] = Rcw[k];
    for (int k = 0; k < 3; k++) p.tcw[k] = tcw[k];
    hipLaunchKernelGGL(k_map_depth, dim3((n + 255) / 256), dim3(256), 0, st, p, geom, lids, n, z);
}

// k_lmap_put's sibling: the source is the result records, put[i] = {record, slot}; the walk gives every new landmark an id of its
// own, so no two lanes write one slot
__global__ __launch_bounds__(256) void k_map_put(const MapOut *__restrict__ rec, const int2 *__restrict__ put, int n,
                                                 double *__restrict__ geom, int32_t *__restrict__ nrays)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int2 p = put[i];
    const MapOut &o = rec[p.x];
    double *g = geom + (size_t)p.y * 6;
    for (int k = 0; k < 3; k++) { g[k] = o.X[k]; g[3 + k] = o.normal[k]; }
    nrays[p.y] = o.n_rays;
}

void launch_map_put(hipStream_t st, const MapOut *rec, const int2 *put, int n, double *geom, int32_t *nrays)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_map_put, dim3((n + 255) / 256), dim3(256), 0, st, rec, put, n, geom, nrays);
}

// mcorb_dev_map_gates_selftest: case i has nv[i] views (the first nv1[i] the neighbour's) starting at view voff[i]
__global__ __launch_bounds__(kMapBlock) void k_map_gates(MapGateCases c, int n, MapOut *__restrict__ out)
{
    const int i = blockIdx.x * kMapBlock + threadIdx.x;
    if (i >= n) return;
    MapOut o;
    map_gate_case(c, i, o);
    out[i] = o;
}

void launch_map_gates(hipStream_t st, const MapGateCases &c, int n, MapOut *out)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_map_gates, dim3((n + kMapBlock - 1) / kMapBlock), dim3(kMapBlock), 0, st, c, n, out);
}

// mcorb_dev_map_refine_selftest: case i has nv[i] views (the first nv1[i] the previous keyframe's) starting at view voff[i]
__global__ __launch_bounds__(kMapBlock) void k_map_refine_cases(MapRefineCases c, int n, MapOut *__restrict__ out,
                                                                MapNewExtra *__restrict__ extra)
{
    const int i = blockIdx.x * kMapBlock + threadIdx.x;
    if (i >= n) return;
    MapOut o;
    MapNewExtra e;
    map_refine_case(c, i, o, e);
    out[i] = o;
    extra[i] = e;
}

void launch_map_refine_cases(hipStream_t st, const MapRefineCases &c, int n, MapOut *out, MapNewExtra *extra)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_map_refine_cases, dim3((n + kMapBlock - 1) / kMapBlock), dim3(kMapBlock), 0, st, c, n, out, extra);
}

}  // namespace mcorb
