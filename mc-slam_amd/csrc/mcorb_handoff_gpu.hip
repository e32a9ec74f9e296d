// mcorb_handoff_gpu.hip -- the kernels at the two ends of an extraction job that no benchmark leg times: frames coming in
// (k_stage_f32: the reference's CV_32F hand-off, k_remap_u8: cv::undistort of a rectified rig's raw planes), results going out
// (k_undistort: UndistortKeyPoints of the selected keypoints, k_copy_to_host: device -> pinned host as a small grid).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcorb_common.h"
#include "mcorb_device.h"
#include "mcorb_kernels.h"
#include "mcorb_undistort.h"
#include "mcorb_undistort_image.h"

namespace mcorb {

// ---------------------------------------------------------------------------
// Frame hand-off: CV_32F [0,1] (1 or 3 channels, BGR) -> u8 gray level-0 plane.
// multiply(img,255) -> convertTo(CV_8U) -> cvtColor(BGR2GRAY)
// (MCSlam/src/MultiCameraFrame.cpp:108-116).
// ---------------------------------------------------------------------------
// What an int cannot hold (NaN, +-Inf, a product outside [-2^31, 2^31)) is 0: x86's cvtss2si / cvtps2dq answer 0x80000000, which
// the saturating packs clamp to 0 (docs/design/02_oracle.md).  The conversion alone would saturate +Inf to INT_MAX, i.e. 255.
__device__ __forceinline__ int sat_u8_rne(float v)
{
    if (!(v >= -2147483648.f && v < 2147483648.f)) return 0;
    int r = __float2int_rn(v);   // cvRound: round-half-even
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// one output pixel of row S (x < w)
__device__ __forceinline__ int stage_f32_px(const float *__restrict__ S, int x, int channels)
{
    if (channels == 1) return sat_u8_rne(__fmul_rn(S[x], 255.f));
    int b = sat_u8_rne(__fmul_rn(S[3 * x + 0], 255.f));
    int gg = sat_u8_rne(__fmul_rn(S[3 * x + 1], 255.f));
    int r = sat_u8_rne(__fmul_rn(S[3 * x + 2], 255.f));
    return (b * 1868 + gg * 9617 + r * 4899 + 8192) >> 14;
}

// dst: image m at m * dst_img_stride, row y at y * dst_pitch -- level 0 of the pyramid blocks, or the raw planes of a rig with
// image undistortion set (k_remap_u8 follows)
__global__ __launch_bounds__(256) void k_stage_f32(const float *__restrict__ src, int w, int src_pitch_f, int channels,
                                                   size_t src_img_stride_f, uint8_t *__restrict__ dst, int dst_pitch,
                                                   size_t dst_img_stride)
{
    const int img = blockIdx.z;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= w) return;
    const float *S = src + (size_t)img * src_img_stride_f + (size_t)y * src_pitch_f;
    dst[(size_t)img * dst_img_stride + (size_t)y * dst_pitch + x] = (uint8_t)stage_f32_px(S, x, channels);
}

void launch_stage_f32(hipStream_t st, const float *src, int w, int h, int pitch_f, int channels, size_t img_stride_f,
                      uint8_t *pyr, const Geom &g, int nimg)
{
    hipLaunchKernelGGL(k_stage_f32, dim3((w + 255) / 256, h, nimg), dim3(256), 0, st, src, w, pitch_f, channels, img_stride_f,
                       pyr + g.lv[0].off, g.lv[0].pitch, (size_t)g.imgBytes);
}

void launch_stage_f32_raw(hipStream_t st, const float *src, int w, int h, int pitch_f, int channels, size_t img_stride_f,
                          uint8_t *raw, int nimg)
{
    hipLaunchKernelGGL(k_stage_f32, dim3((w + 255) / 256, h, nimg), dim3(256), 0, st, src, w, pitch_f, channels, img_stride_f,
                       raw, w, (size_t)w * h);
}

// ---------------------------------------------------------------------------
// Frame hand-off of a rectified rig (RECTIFY, MultiCameraFrame.cpp:123-136): cv::undistort of every raw plane into level 0.
// The map of a camera (mcorb_undistort_image.h, built on the host when the calibration is set) is the same for every frame, and
// it is 6 of the 8 bytes an output pixel moves.  So a workgroup owns 1024 consecutive output pixels of ONE camera: each lane
// loads the map entries of its 4 pixels once (16 + 8 bytes), turns them into tap offsets and weights in registers, and then
// walks the batch's frames of that camera -- per frame 16 byte gathers (two short row segments per pixel, shared with the
// neighbouring lanes: they hit in TCP / L2) and one dword store.  Cameras that are not set (mode 0) are copied through.
// Every tap offset lies inside the plane by construction (remap_taps: a tap outside gets offset 0, weight 0).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_remap_u8(const uint8_t *__restrict__ raw, uint8_t *__restrict__ pyr,
                                                  const RemapCam *__restrict__ cams, int ncams, int nimg, int w, int h, int wq,
                                                  uint32_t imgBytes, uint32_t off0, int pitch0)
{
    const int cam = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;   // quad of 4 output pixels; wq quads per row
    if (q >= wq * h) return;
    const int y = q / wq, x = (q - y * wq) * 4;
    const int nv = min(4, w - x);
    const size_t plane = (size_t)w * h;
    const RemapCam C = cams[cam];
    uint8_t *dst = pyr + off0 + (size_t)y * pitch0 + x;
    if (C.mode == 0) {
        const size_t so = (size_t)y * w + x;
        for (int m = cam; m < nimg; m += ncams) {
            const uint8_t *s = raw + (size_t)m * plane + so;
            uint8_t *d = dst + (size_t)m * imgBytes;
            if (nv == 4 && (w & 3) == 0) *reinterpret_cast<uint32_t *>(d) = *reinterpret_cast<const uint32_t *>(s);
            else for (int i = 0; i < nv; i++) d[i] = s[i];
        }
        return;
    }
    // the device maps are padded to wq * 4 entries per row (zeros): both loads are aligned whatever w is
    const size_t mo = ((size_t)y * wq) * 4 + x;
    const uint4 a = *reinterpret_cast<const uint4 *>(C.map1 + mo * 2);
    const uint2 b = *reinterpret_cast<const uint2 *>(C.map2 + mo);
    const uint32_t a4[4] = {a.x, a.y, a.z, a.w};
    const uint32_t b4[4] = {b.x & 0xffffu, b.x >> 16, b.y & 0xffffu, b.y >> 16};
    RemapTaps t[4];
#pragma unroll
    for (int i = 0; i < 4; i++) remap_taps((int)(int16_t)(a4[i] & 0xffffu), (int)(int16_t)(a4[i] >> 16), b4[i], w, h, w, t[i]);
#pragma unroll 2
    for (int m = cam; m < nimg; m += ncams) {
        const uint8_t *s = raw + (size_t)m * plane;
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) v |= (uint32_t)remap_pixel(s, t[i]) << (8 * i);
        uint8_t *d = dst + (size_t)m * imgBytes;
        if (nv == 4) *reinterpret_cast<uint32_t *>(d) = v;
        else for (int i = 0; i < nv; i++) d[i] = (uint8_t)(v >> (8 * i));
    }
}

void launch_remap_u8(hipStream_t st, const uint8_t *raw, uint8_t *pyr, const Geom &g, const RemapCam *cams, int ncams, int nimg)
{
    const int w = g.lv[0].w, h = g.lv[0].h, wq = remap_map_pitch(w) / 4;
    dim3 grid((wq * h + 255) / 256, ncams < nimg ? ncams : nimg);
    hipLaunchKernelGGL(k_remap_u8, grid, dim3(256), 0, st, raw, pyr, cams, ncams, nimg, w, h, wq, g.imgBytes, g.lv[0].off, g.lv[0].pitch);
}

// ---------------------------------------------------------------------------
// MultiCameraFrame::UndistortKeyPoints (MultiCameraFrame.cpp:300-347): cv::undistortPoints of every selected keypoint, one lane
// per keypoint (mcorb_undistort.h).  pt is rebuilt from the packed selection exactly as the host's keypoint records are
// ((float)x, times the float scale factor above level 0); image m belongs to camera m % ncams.  fp64 throughout, no contraction
// (-ffp-contract=off): bit-equal to the host restatement.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_undistort(const uint32_t *__restrict__ sel, const int *__restrict__ nsel, int kcap, int ncams,
                                                   const UndistCam *__restrict__ cams, UndistScales sc, float2 *__restrict__ out)
{
    const int m = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int n = min(nsel[m], kcap);
    if (k >= n) return;
    const float2 p = sel_point(sel[(size_t)m * kcap + k], sc);
    float ox, oy;
    undistort_point(cams[m % ncams], p.x, p.y, ox, oy);
    out[(size_t)m * kcap + k] = make_float2(ox, oy);
}

void launch_undistort(hipStream_t st, const uint32_t *sel, const int *nsel, int kcap, int nimg, int ncams, const UndistCam *cams,
                      const float *scale, int nlevels, float2 *out)
{
    hipLaunchKernelGGL(k_undistort, dim3((kcap + 255) / 256, nimg), dim3(256), 0, st, sel, nsel, kcap, ncams, cams,
                       UndistScales(scale, nlevels), out);
}

// ---------------------------------------------------------------------------
// Device -> pinned host copy as a SMALL kernel.  hipMemcpyAsync to pinned memory runs as a blit kernel on this stack
// (__amd_rocclr_copyBuffer; HSA_ENABLE_SDMA changes nothing), and the kernel of the job that runs beside it is stretched
// to the copy's length (k_expand: 12 us alone, 150 us beside the descriptor read-back).  The link moves ~50 GB/s whatever
// feeds it; kCopyWG workgroups looping over the buffer with 16-byte accesses, four loads in flight per lane, feed it as
// well and leave the neighbour alone (k_expand 23 us).  Used for single-slot rigs only: with six slots in flight the
// runtime's copy still gives 4-6 % more frames/s (profiles/r03_copy_kernel_ab.txt; the smaller the grid the closer: 1024
// workgroups 30.7 k, 128: 30.9 k, 24: 32.3 k, 4: 33.5 k, runtime 34.0 k frames/s).
// ---------------------------------------------------------------------------
constexpr int kCopyWG = 24;
__global__ __launch_bounds__(256) void k_copy_to_host(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16)
{
    const v4i *s = reinterpret_cast<const v4i *>(src);
    v4i *d = reinterpret_cast<v4i *>(dst);
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {   // four 16-byte loads in flight per lane
        const v4i a = __builtin_nontemporal_load(s + i), b = __builtin_nontemporal_load(s + i + stride);
        const v4i c = __builtin_nontemporal_load(s + i + 2 * stride), e = __builtin_nontemporal_load(s + i + 3 * stride);
        __builtin_nontemporal_store(a, d + i);
        __builtin_nontemporal_store(b, d + i + stride);
        __builtin_nontemporal_store(c, d + i + 2 * stride);
        __builtin_nontemporal_store(e, d + i + 3 * stride);
    }
    for (; i < n16; i += stride) {
        const v4i v = __builtin_nontemporal_load(s + i);
        __builtin_nontemporal_store(v, d + i);
    }
}

void launch_copy_to_host(hipStream_t st, const void *src_dev, void *dst_host_mapped, size_t bytes)
{
    const size_t n16 = (bytes + 15) / 16;   // both buffers are allocated in multiples of 16 bytes
    if (!n16) return;
    const size_t wgs = (n16 + 255) / 256 < (size_t)kCopyWG ? (n16 + 255) / 256 : (size_t)kCopyWG;
    hipLaunchKernelGGL(k_copy_to_host, dim3((unsigned)wgs), dim3(256), 0, st, reinterpret_cast<const uint4 *>(src_dev),
                       reinterpret_cast<uint4 *>(dst_host_mapped), n16);
}

}  // namespace mcorb
