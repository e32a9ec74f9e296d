// mcorb_upload.cpp -- the three upload forms: caller memory into level 0 of a slot's pyramid planes.
#include <string.h>

#include "mcorb_engine.h"

namespace mcorb {

// An upload into a slot whose job is still running would overwrite the staging buffer and level 0 between the job's
// GPU phases (the slot's stream is idle while the host selects): refuse it like every other call on a busy slot.
static bool slot_busy(Slot &s)
{
    std::lock_guard<std::mutex> lk(s.m);
    if (s.busy) set_error("slot busy: wait for the submitted job before uploading into its slot");
    return s.busy;
}

// Frame staging: caller memory -> pinned buffer -> hipMemcpy2DAsync into the
// level-0 planes (replaces the clone/convert chain of MultiCameraFrame::setData).
int Rig::upload_u8(int slot, const uint8_t *const *images, int nimg, int stride)
{
    if (slot < 0 || slot >= (int)slots.size() || nimg < 1 || nimg > max_images || !images || stride < W) {
        set_error("upload_u8: bad argument");
        return MCORB_E_ARG;
    }
    Slot &s = *slots[slot];
    if (slot_busy(s)) return MCORB_E_STATE;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(s.st));   // staging buffer free again
    for (int m = 0; m < nimg; m++)
        if (!images[m]) { set_error("upload_u8: empty image"); return MCORB_E_EMPTY; }
    // pageable caller memory -> pinned staging buffer: one pool task per image (the calling thread takes its share)
    auto copy_one = [&](int m, int) {
        uint8_t *dst = s.h_stage + (size_t)m * W * H;
        if (stride == W) memcpy(dst, images[m], (size_t)W * H);
        else for (int y = 0; y < H; y++) memcpy(dst + (size_t)y * W, images[m] + (size_t)y * stride, W);
    };
    if (nimg > 1 && nimg <= kSmallBatch && upload_pipelined) {
        // one rig frame at a time: the staging copy and the DMA overlap -- the planes are copied a quarter at a time, image by image,
        // and whoever finishes an image's last quarter puts its DMA on the stream while the others go on with the next image
        constexpr int Q = 4;
        const bool raw = imgud_on;   // image undistortion set: into the raw planes, k_remap_u8 behind the last copy
        std::atomic<int> left[kSmallBatch];
        for (int m = 0; m < nimg; m++) left[m].store(Q);
        std::atomic<int> err{(int)hipSuccess};
        const size_t plane = (size_t)W * H;
        auto quarter = [&](int t, int) {
            const int m = t / Q, q = t % Q, y0 = H * q / Q, y1 = H * (q + 1) / Q;
            uint8_t *dst = s.h_stage + (size_t)m * plane;
            if (stride == W) memcpy(dst + (size_t)y0 * W, images[m] + (size_t)y0 * W, (size_t)(y1 - y0) * W);
            else for (int y = y0; y < y1; y++) memcpy(dst + (size_t)y * W, images[m] + (size_t)y * stride, W);
            if (left[m].fetch_sub(1, std::memory_order_acq_rel) != 1) return;
            hipError_t e = hipSetDevice(device);   // (pool threads make no other HIP call)
            if (e == hipSuccess)
                e = raw ? hipMemcpyAsync(s.d_raw + (size_t)m * plane, dst, plane, hipMemcpyHostToDevice, s.st)
                        : hipMemcpy2DAsync(s.d_pyr + (size_t)m * geom.imgBytes + geom.lv[0].off, geom.lv[0].pitch, dst, W, W, H, hipMemcpyHostToDevice, s.st);
            if (e != hipSuccess) err.store((int)e);
        };
        pool->parallel_for(nimg * Q, quarter, pool_threads + s.index);
        HIPCHK((hipError_t)err.load());
        return raw ? enqueue_remap(s, nimg) : MCORB_OK;
    }
    if (nimg > 1) pool->parallel_for(nimg, copy_one, pool_threads + s.index);
    else copy_one(0, 0);
    return upload_staged(slot, nimg);
}

// DMA of the slot's pinned staging buffer (image m at m*W*H, row stride W) into level 0 of the pyramid planes.
int Rig::upload_staged(int slot, int nimg)
{
    if (slot < 0 || slot >= (int)slots.size() || nimg < 1 || nimg > max_images) { set_error("upload_staged: bad argument"); return MCORB_E_ARG; }
    Slot &s = *slots[slot];
    if (slot_busy(s)) return MCORB_E_STATE;
    HIPCHK(hipSetDevice(device));
    const size_t plane = (size_t)W * H;
    if (imgud_on) {   // the raw planes are the staging buffer's layout: one copy, then cv::undistort into level 0
        HIPCHK(hipMemcpyAsync(s.d_raw, s.h_stage, plane * nimg, hipMemcpyHostToDevice, s.st));
        return enqueue_remap(s, nimg);
    }
    if (geom.lv[0].pitch == W) {
        // level-0 rows are contiguous: the whole batch is one strided copy (one row = one image)
        HIPCHK(hipMemcpy2DAsync(s.d_pyr + geom.lv[0].off, geom.imgBytes, s.h_stage, plane, plane, nimg, hipMemcpyHostToDevice, s.st));
    } else {
        for (int m = 0; m < nimg; m++)
            HIPCHK(hipMemcpy2DAsync(s.d_pyr + (size_t)m * geom.imgBytes + geom.lv[0].off, geom.lv[0].pitch, s.h_stage + m * plane, W, W, H,
                                    hipMemcpyHostToDevice, s.st));
    }
    return MCORB_OK;
}

int Rig::upload_f32(int slot, const float *const *images, int nimg, int stride_bytes, int channels)
{
    if (slot < 0 || slot >= (int)slots.size() || nimg < 1 || nimg > max_images || !images ||
        (channels != 1 && channels != 3) || stride_bytes < W * channels * 4 || (stride_bytes & 3)) {
        set_error("upload_f32: bad argument");
        return MCORB_E_ARG;
    }
    Slot &s = *slots[slot];
    if (slot_busy(s)) return MCORB_E_STATE;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(s.st));
    const size_t row_f = (size_t)W * channels, img_f = row_f * H;
    TRY(s.d_f32.grow(img_f * (size_t)max_images));
    for (int m = 0; m < nimg; m++) {
        if (!images[m]) { set_error("upload_f32: empty image"); return MCORB_E_EMPTY; }
        HIPCHK(hipMemcpy2DAsync(s.d_f32 + (size_t)m * img_f, row_f * 4, images[m], stride_bytes, row_f * 4, H,
                                hipMemcpyHostToDevice, s.st));
    }
    if (imgud_on) {
        launch_stage_f32_raw(s.st, s.d_f32, W, H, (int)row_f, channels, img_f, s.d_raw, nimg);
        HIPCHK(hipGetLastError());
        TRY(enqueue_remap(s, nimg));
    } else {
        launch_stage_f32(s.st, s.d_f32, W, H, (int)row_f, channels, img_f, s.d_pyr, geom, nimg);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s.st));   // caller memory may be pageable: copies above were staged by the runtime
    return MCORB_OK;
}

}  // namespace mcorb
