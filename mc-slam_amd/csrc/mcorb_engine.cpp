// mcorb_engine.cpp -- host orchestration: a rig's buffers and slots, the slot drivers, the stages of an extraction job.
//
// Data flow of one batch (nimg equally sized images, all resident in HBM):
//   phase A (GPU)  pyramid L1..L7 -> FAST score + cell NMS -> candidate compaction
//                  (bucket tables to the host by DMA; whole-level blur only in the IC-angle mode)
//   selection      host worker pool, one task per image                 [mcorb_select.cpp]
//   phase B (GPU)  blur around the selected keypoints + BRIEF descriptors (one kernel) -> D2H
//   match (GPU)    all-pairs Hamming k-NN (k=2) + ratio/threshold flags -> host-mapped
//   merge          per-frame IntraMatch track merge on the host
// Each slot owns a stream, a complete buffer set and a driver thread, so several
// batches can be in flight and the host stage of one overlaps the GPU phases of others.
#include <stdlib.h>
#include <string.h>
#include <sys/prctl.h>
#include <time.h>

#include "mcorb_engine.h"
#include "mcorb_prof.h"

namespace mcorb {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
const char *get_error() { return g_err.c_str(); }
hipError_t Rig::wait_event(hipEvent_t ev) const
{
    if (wait_mode != 2) return hipEventSynchronize(ev);   // spins, or sleeps on the interrupt (event flag)
    for (int i = 0;; i++) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (i < 4) { std::this_thread::yield(); continue; }   // a wait that is almost over
        timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
    }
}

// the buffers Rig::init allocates on the host: device-mapped, zero-filled
template <typename T>
static int host_alloc(HostBuf<T> &b, size_t n)
{
    TRY(b.alloc(n, kHostMapped));
    memset(b, 0, n * sizeof(T));
    return MCORB_OK;
}

int Rig::init(const mcorb_params &p, int ncams_, int W_, int H_, int max_frames_, int nslots)
{
    if (ncams_ < 1 || ncams_ > MCORB_MAX_CAMS || max_frames_ < 1 || nslots < 1 || W_ < 1 || H_ < 1) {
        set_error("bad rig arguments");
        return MCORB_E_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || p.device_id < 0 || p.device_id >= ndev) {
        set_error("no usable HIP device (libmcorb has no CPU path)");
        return MCORB_E_NODEVICE;
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, p.device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("device is ") + prop.gcnArchName + ", libmcorb is built for gfx950 only");
        return MCORB_E_NODEVICE;
    }
    params = p;
    ncams = ncams_; W = W_; H = H_; max_frames = max_frames_;
    max_images = ncams * max_frames;
    undist_cams.assign(ncams, UndistCam{});
    undist_set.assign(ncams, 0);
    imgud_cams.assign(ncams, UndistImageCam{});
    imgud_set.assign(ncams, 0);
    imgud_map1.assign(ncams, {});
    imgud_map2.assign(ncams, {});
    d_imgud_map1.resize(ncams);
    d_imgud_map2.resize(ncams);
    npp = ncams * (ncams - 1) / 2;
    device = p.device_id;
    HIPCHK(hipSetDevice(device));
    TRY(compute_tables(p, tab));
    std::vector<ResizeTap> taps;
    std::vector<uint16_t> lut;
    TRY(build_geometry(p, tab, W, H, geom, taps, &lut));
    for (int l = 0; l < geom.nlevels; l++)
        selp[l] = make_select_params(kMinBorder, geom.lv[l].maxBorderX, kMinBorder, geom.lv[l].maxBorderY, tab.quota[l],
                                     geom.lv[l].wCell, geom.lv[l].hCell);
    if (taps.empty()) taps.push_back(ResizeTap{0, 0, 0, 0});
    TRY(resize_windows(geom, taps, resize_win));
    TRY(d_taps.alloc(taps.size()));
    HIPCHK(hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(ResizeTap), hipMemcpyHostToDevice));
    TRY(d_lut.alloc(lut.size() + 8));
    HIPCHK(hipMemcpy(d_lut, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    {
        std::vector<uint32_t> ft;
        fast_cell_off = fast_cell_table(geom, ft);   // (16-byte aligned: the records are read 16 bytes at a time)
        TRY(d_fasttab.alloc(ft.size()));
        HIPCHK(hipMemcpy(d_fasttab, ft.data(), ft.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    HIPCHK(upload_umax(tab.umax));

    // Host threads: the selection workers, one driver per slot (spinning on its events unless the rig sleeps, below) and
    // the submitting thread all draw on the cores this process may use -- the scheduler affinity AND the cgroup CPU quota
    // (a GPU box gives 16 cores per GPU: with 16 workers + 6 spinning drivers the quota ran out in 10 of 40 periods and the
    // whole process was stalled for 5-15 ms each time, 15 % of the throughput).  Default: what is left after the drivers
    // and the caller, at most one worker per image of a batch and at most 16.
    const int cores = usable_cores();
    // How the slot drivers wait for the GPU.  hipEventSynchronize spins: one core per slot, ~60 % of it spent doing
    // nothing at six slots -- cores the selection needs (at 31 k frames/s the selection alone keeps 8.7 cores busy and
    // the GPU box grants 16).  HIP's interrupt-driven wait (hipEventBlockingSync) measured no cheaper in CPU time.
    // Default with several slots: poll hipEventQuery with 20 us sleeps in between (a few % of a core; the added latency
    // is hidden behind the other slots).  One slot = latency mode: spin.  MCORB_SYNC=spin|block|poll overrides.
    const char *sync_env = getenv("MCORB_SYNC");
    wait_mode = nslots > 1 ? 2 : 0;
    if (sync_env) wait_mode = !strcmp(sync_env, "block") ? 1 : (!strcmp(sync_env, "poll") ? 2 : 0);
    const bool blocking = wait_mode == 1;   // the events a thread waits on are created with hipEventBlockingSync
    int nthreads = p.host_threads > 0 ? p.host_threads : (wait_mode == 0 ? cores - nslots - 2 : cores - 4);
    if (p.host_threads <= 0) nthreads = std::max(2, std::min(nthreads, std::min(max_images, 16)));
    if (getenv("MCORB_HOST_THREADS")) nthreads = atoi(getenv("MCORB_HOST_THREADS"));
    nthreads = std::max(1, std::min(nthreads, 64));
    blur_planes = p.orientation != 0 || getenv("MCORB_BLUR_PLANES") != nullptr;
    // Device -> host copies of the tables and the descriptors: the runtime's hipMemcpyAsync (a blit kernel on this stack) or
    // k_copy_to_host (a 24-workgroup kernel of ours).  Measured (profiles/r03_copy_kernel_ab.txt): with six slots in flight the
    // runtime's copy gives 4-6 % more frames/s although k_expand / k_knn2 run stretched beside it; with one slot (latency mode)
    // ours keeps k_expand at 12 us instead of 150 and the frame a few % shorter.  MCORB_COPY_KERNEL=0|1 overrides.
    copy_kernel = getenv("MCORB_COPY_KERNEL") ? atoi(getenv("MCORB_COPY_KERNEL")) != 0 : nslots == 1;
    {   // where DistributeOctTree's list discipline runs (include/mcorb.h, MCORB_SELECT_*)
        const char *e = getenv("MCORB_SELECT");
        int mode = p.selection;
        if (mode == MCORB_SELECT_AUTO && e) mode = !strcmp(e, "host") ? MCORB_SELECT_HOST : (!strcmp(e, "gpu") ? MCORB_SELECT_GPU : MCORB_SELECT_AUTO);
        if (mode != MCORB_SELECT_AUTO && mode != MCORB_SELECT_HOST && mode != MCORB_SELECT_GPU) { set_error("mcorb_params.selection: unknown mode"); return MCORB_E_ARG; }
        gpu_select = mode != MCORB_SELECT_HOST && select_fits(geom);
        if (gpu_select) HIPCHK(configure_select(geom));
        // (test knobs, read once here -- never from the slot drivers' threads: a getenv per launch raced with a profiler's setenv)
        if (getenv("MCORB_SELECT_DEEP_CAP")) select_deep_cap = std::max(1, atoi(getenv("MCORB_SELECT_DEEP_CAP")));
        compact_one_copy = getenv("MCORB_COMPACT_ONE_COPY") != nullptr;
        select_prof = getenv("MCORB_SELECT_PROF") != nullptr;
        // HIP graphs: a single-slot rig (one job at a time, how MC-SLAM calls) replays its job from a captured graph -- 0.35 -> 0.29 ms
        // per rig frame; with several jobs in flight the replay measured 3 - 5 % SLOWER than launch by launch (profiles/r04_overlap.txt)
        gpu_job_limit = getenv("MCORB_GPU_JOBS") ? atoi(getenv("MCORB_GPU_JOBS")) : p.gpu_jobs;
        if (gpu_job_limit < 0 || gpu_job_limit >= nslots) gpu_job_limit = 0;
        upload_pipelined = !(getenv("MCORB_UPLOAD_PIPE") && atoi(getenv("MCORB_UPLOAD_PIPE")) == 0);   // (A/B knob)
        graph_every = !gpu_select ? 0 : getenv("MCORB_GRAPH") ? std::max(0, atoi(getenv("MCORB_GRAPH"))) : (nslots == 1 ? 1 : 0);   // (mcorb_rig_select_mode reports what the rig really runs)
    }
    pool.reset(new WorkerPool(nthreads));
    pool_threads = nthreads;
    for (int i = 0; i < nthreads + nslots; i++) scratch.emplace_back(new SelectScratch);   // workers, then one per slot's submitting thread

    const int npairs_max = std::max(1, npp * max_frames);
    // an external block usually holds the sets of all slots of a rank (all-to-all) or of all ranks (all-gather)
    ext_cap = (int)align_up(std::max((size_t)4096, (size_t)64 * max_images), 64);
    for (int si = 0; si < nslots; si++) {
        slots.emplace_back(new Slot);
        Slot *s = slots.back().get();
        s->rig = this;
        s->index = si;
        for (Stream *st : {&s->st, &s->st_copy, &s->st_dma}) TRY(st->create(hipStreamNonBlocking));
        // the events a driver thread waits on (tables, compute stream, DMA stream).  HIP spins by default, which
        // measured 2-4 % faster than interrupt-driven waits at 6 slots; with many slots the spinning drivers would take
        // the cores the selection workers need, so those rigs sleep instead.  MCORB_SYNC=block|spin overrides.
        TRY(s->ev_x.create(hipEventDisableTiming));
        for (Event *e : {&s->ev_c, &s->ev_e, &s->ev_start, &s->ev_pyr, &s->ev_fast, &s->ev_blur, &s->ev_desc0, &s->ev_desc1, &s->ev_knn0, &s->ev_knn1, &s->ev_fin})
            TRY(e->create(hipEventDefault));
        for (Event *e : {&s->ev_tables, &s->ev_done, &s->ev_side}) TRY(e->create(blocking ? hipEventBlockingSync : hipEventDefault));
        const size_t M = (size_t)max_images;
        TRY(s->d_pyr.alloc(M * geom.imgBytes));
        HIPCHK(hipMemset(s->d_pyr, 0, M * geom.imgBytes));
        if (blur_planes) {   // whole blurred planes: only the plane-based descriptor paths write them with every job;
            TRY(s->d_blur.alloc(M * geom.imgBytes));   // mcorb_rig_get_blurred allocates on first use otherwise
            HIPCHK(hipMemset(s->d_blur, 0, M * geom.imgBytes));
        }
        TRY(s->d_cellkp.alloc(M * geom.cells * geom.cellCap));
        TRY(s->d_cellcnt.alloc(M * geom.cells));
        TRY(s->d_sorted.alloc(M * geom.candCap));
        s->tbl_ints_per_image = tbl_ints(geom.bucketTotal);
        TRY(s->d_tbl.alloc(M * s->tbl_ints_per_image));
        TRY(host_alloc(s->h_tbl, M * s->tbl_ints_per_image));
        TRY(s->d_desc.alloc(M * geom.kcap * 32));
        HIPCHK(hipMemset(s->d_desc, 0, M * geom.kcap * 32));
        TRY(s->d_angles.alloc(M * geom.kcap));
        TRY(s->d_part.alloc(knn_part_entries(npairs_max, geom.kcap)));
        TRY(s->d_exp.alloc(M * geom.kcap * (size_t)kKnnExpandBytes));
        TRY(s->d_lcounts.alloc(M));
        TRY(host_alloc(s->h_cand, M * geom.hostCandCap));
        TRY(host_alloc(s->h_overflow, 16));
        TRY(s->d_knn.alloc((size_t)npairs_max * geom.kcap));
        TRY(host_alloc(s->h_mlist, (size_t)npairs_max * knn_mlist_stride(geom.kcap)));
        TRY(host_alloc(s->h_mcount, (size_t)npairs_max * knn_qblocks(geom.kcap)));
        {
            const size_t o_nsel = (size_t)ext_cap * sizeof(int);
            const size_t o_setmap = align_up(o_nsel + M * sizeof(int), 64);
            const size_t o_pairs = align_up(o_setmap + M * sizeof(int), 64);
            const size_t o_sel = align_up(o_pairs + (size_t)npairs_max * sizeof(int2), 64);
            s->ctrl_pairs_end = o_sel;
            s->ctrl_nsel_off = o_nsel;
            s->ctrl_bytes = o_sel + M * geom.kcap * sizeof(uint32_t);
            TRY(host_alloc(s->h_ctrl, s->ctrl_bytes));
            TRY(s->d_ctrl.alloc(s->ctrl_bytes));
            HIPCHK(hipMemset(s->d_ctrl, 0, s->ctrl_bytes));
            auto view = [&](uint8_t *base) {
                return Slot::CtrlView{(int *)base, (int *)(base + o_nsel), (int *)(base + o_setmap), (int2 *)(base + o_pairs), (uint32_t *)(base + o_sel)};
            };
            s->hc = view(s->h_ctrl);
            s->dc = view(s->d_ctrl);
        }
        if (gpu_select) {
            TRY(s->d_selval.alloc(M * geom.nlevels * (size_t)select_cap(geom)));
            TRY(s->d_selcnt.alloc(M * geom.nlevels));
            s->res_mono_off = 16 * sizeof(int);
            s->res_resp_off = align_up(s->res_mono_off + M * sizeof(int), 64);
            s->res_bytes = align_up(s->res_resp_off + M * geom.kcap, 64);
            TRY(s->d_res.alloc(s->res_bytes));
            TRY(host_alloc(s->h_res, s->res_bytes));
            HIPCHK(hipMemset(s->d_res, 0, s->res_bytes));
            TRY(host_alloc(s->h_sig, M));
            TRY(s->ev_s.create(hipEventDefault));
            TRY(s->ev_g.create(hipEventDefault));
        }
        TRY(host_alloc(s->h_stage, M * (size_t)W * H));
        TRY(host_alloc(s->h_desc, M * geom.kcap * 32));
        TRY(host_alloc(s->h_angles, M * geom.kcap));
        s->kps.resize(M);
        s->mono.assign(M, 0);
        s->sel_val.resize(M * geom.nlevels);
        s->m_idx1.resize(npairs_max);
        s->m_idx2.resize(npairs_max);
        s->tracks.resize(max_frames);
        s->mergeable.assign(max_frames, 0);
        s->th = std::thread([this, s] { driver(s); });
    }
    // The hipMemset calls above run on the null stream and return before the fill kernels have executed; the slots'
    // streams are non-blocking, i.e. NOT ordered against the null stream, so without this an early upload could be
    // zeroed again by a fill that was still queued (seen as an occasional empty first frame).
    HIPCHK(hipDeviceSynchronize());
    return MCORB_OK;
}

// What is order-dependent: a slot's driver thread stops before its streams drain, and the graph exec goes before the buffers
// and events it names.  Everything else is released by the members' destructors (order: the comment at the top of Slot).
Rig::~Rig()
{
    HostProf::report();
    (void)hipSetDevice(device);
    for (auto &s : slots) {
        if (s->th.joinable()) {
            {
                std::lock_guard<std::mutex> lk(s->m);
                s->quit = true;
            }
            s->cv.notify_all();
            s->th.join();
        }
        for (hipStream_t st : {(hipStream_t)s->st, (hipStream_t)s->st_copy, (hipStream_t)s->st_dma})
            if (st) (void)hipStreamSynchronize(st);
        if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    }
}

static const char *const kCandOverflowMsg = "candidate list of a sparse level does not fit the host buffer (raise mcorb_params.cand_cap)";

int Rig::submit(int slot, const Job &job)
{
    if (slot < 0 || slot >= (int)slots.size()) { set_error("bad slot"); return MCORB_E_ARG; }
    Slot &s = *slots[slot];
    TRY(check_job_shape(job));
    std::unique_lock<std::mutex> lk(s.m);
    if (s.busy) { set_error("slot busy"); return MCORB_E_STATE; }
    s.job = job;
    s.busy = true;
    s.submitted = true;
    s.status = MCORB_OK;
    lk.unlock();
    s.cv.notify_all();
    return MCORB_OK;
}

int Rig::wait(int slot)
{
    if (slot < 0 || slot >= (int)slots.size()) { set_error("bad slot"); return MCORB_E_ARG; }
    Slot &s = *slots[slot];
    std::unique_lock<std::mutex> lk(s.m);
    s.cv.wait(lk, [&s] { return !s.busy; });
    s.submitted = false;
    if (s.status != MCORB_OK) set_error(s.err);
    return s.status;
}

int Rig::execute(Slot &s, const Job &j)
{
    // A stale error of this thread is not this job's: e.g. an elapsed-time query (mcorb_rig_last_timing, the fallback path's own
    // accounting) on events that a captured graph holds as nodes and no stream ever recorded leaves "invalid resource handle" behind,
    // and the next hipGetLastError() check -- possibly another rig's job on the same thread -- would trip over it.
    (void)hipGetLastError();
    int st = MCORB_OK;
    switch (j.kind) {
    case Job::EXTRACT:
        if (gpu_select) st = run_gpu_selected(s, j, false);
        else {
            st = run_extract_phaseA(s, j);
            if (st == MCORB_OK) st = run_select_and_describe(s, j, false);
        }
        if (st == MCORB_OK && s.bow_job) st = bow_job_finish(*this, s, j.nimg);
        break;
    case Job::PROCESS:
        LatProf::mark(0);
        if (gpu_select) {
            st = run_gpu_selected(s, j, true);   // (marks 1 .. 5 inside: enqueue | - | - | - | wait GPU | post)
        } else {
            st = run_extract_phaseA(s, j);
            LatProf::mark(1);
            if (st == MCORB_OK) st = run_select_and_describe(s, j, true);
        }
        LatProf::mark(6);
        if (st == MCORB_OK && s.bow_job) st = bow_job_finish(*this, s, j.nimg);
        if (st == MCORB_OK) st = finish_match(s, j);
        LatProf::mark(7);
        LatProf::flush();
        break;
    case Job::MATCH:
        st = enqueue_match(s, j, false);
        if (st == MCORB_OK) {
            hipError_t e = hipEventRecord(s.ev_done, s.st);
            if (e == hipSuccess) e = wait_event(s.ev_done);
            if (e != hipSuccess) { set_error(hipGetErrorString(e)); st = MCORB_E_HIP; }
        }
        if (st == MCORB_OK) st = finish_match(s, j);
        break;
    default: break;
    }
    return st;
}

// Synchronous entry points run the job on the calling thread: no hand-off to the slot's driver thread and back
// (two futex wake-ups, ~50-100 us of a 0.6 ms single-frame call).
int Rig::run_sync(int slot, const Job &job)
{
    if (slot < 0 || slot >= (int)slots.size()) { set_error("bad slot"); return MCORB_E_ARG; }
    Slot &s = *slots[slot];
    TRY(check_job_shape(job));
    {
        std::lock_guard<std::mutex> lk(s.m);
        if (s.busy) { set_error("slot busy"); return MCORB_E_STATE; }
        s.busy = true;
        s.inline_job = true;   // the driver thread must not pick this one up
        s.status = MCORB_OK;
    }
    (void)hipSetDevice(device);
    const int st = execute(s, job);
    {
        std::lock_guard<std::mutex> lk(s.m);
        s.status = st;
        if (st != MCORB_OK) s.err = get_error();
        s.busy = false;
        s.inline_job = false;
    }
    s.cv.notify_all();
    return st;
}

void Rig::driver(Slot *sp)
{
    Slot &s = *sp;
    (void)hipSetDevice(device);
    // the polling wait sleeps 20 us at a time: without this the kernel's default 50 us timer slack triples that
    if (wait_mode == 2) (void)prctl(PR_SET_TIMERSLACK, 2000UL, 0, 0, 0);
    for (;;) {
        Job j;
        {
            std::unique_lock<std::mutex> lk(s.m);
            s.cv.wait(lk, [&s] { return s.quit || (s.busy && !s.inline_job); });
            if (s.quit) return;
            j = s.job;
        }
        const int st = execute(s, j);
        {
            std::lock_guard<std::mutex> lk(s.m);
            s.status = st;
            if (st != MCORB_OK) s.err = get_error();
            s.busy = false;
        }
        s.cv.notify_all();
    }
}

// What every extraction job does before its first launch.  A single rig frame (how MC-SLAM calls, mc_slam_app.cpp:564-572) is launch-
// and hand-off-bound: ~25 runtime calls and three small copies around 250 us of kernels.  For such small batches the copies go:
// the results travel through host-mapped memory.  Selected on the host, k_compact writes its tables straight into h_tbl and the
// describe / k-NN kernels read the control block from h_ctrl; selected on the GPU, k_assemble writes the host's sel / responses /
// counts itself and signals them per image, and the matcher reads its pair list from h_ctrl; either way k_describe_fused writes
// the host's descriptor copy itself (a few hundred KB over PCIe in all).
int Rig::begin_extract(Slot &s, const Job &j)
{
    if (j.nimg < 1 || j.nimg > max_images) { set_error("extract: bad image count"); return MCORB_E_ARG; }
    s.invalidate_bow();   // tracks / BoW vectors of the previous batch index keypoints that are about to disappear
    // the bindings the job runs with: all fixed while a job is in flight
    s.bow_job = bow_bind.flags;
    s.lf_job = lf_on && (bow_bind.flags & MCORB_BOW_MATCH);   // (the LF stage reads the job's BoW-guided tracks)
    s.undist_job = undist_on;
    s.undist_gen = undist_gen;
    std::fill(s.kps_undist_ok.begin(), s.kps_undist_ok.end(), (uint8_t)0);
    s.h_overflow[0] = 0;
    s.host_results = j.nimg <= kSmallBatch && params.orientation == 0 && !blur_planes &&
                     (!gpu_select || (!j.ext_desc && geom.kcap <= kSelSignalMaxCount));   // (the signal word carries the count)
    s.set_ctl(s.host_results, s.host_results && !gpu_select);   // (k_assemble's sel / nsel are the device's in a small batch too)
    // Reference mode blurs inside the descriptor kernel, only around the kept keypoints (k_describe_fused).  Whole
    // blurred planes are made when the rotated taps of the orientation mode need them, when MCORB_BLUR_PLANES asks for
    // the plane-based path (A/B comparison), or later, on demand, for mcorb_rig_get_blurred.
    s.blur_valid = blur_planes;
    return MCORB_OK;
}

int Rig::enqueue_front(Slot &s, int nimg, int *tbl)
{
    const bool ev_on = s.ev_on();
    if (ev_on) HIPCHK(hipEventRecord(s.ev_start, s.st));
    launch_pyramid(s.st, s.d_pyr, geom, d_taps, resize_win, nimg);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_pyr, s.st));
    launch_fast(s.st, s.d_pyr, geom, params.ini_th_fast, params.min_th_fast, d_fasttab + fast_cell_off, s.d_cellkp, s.d_cellcnt, nimg);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_fast, s.st));
    // compaction fills the per-image table blocks (a short kernel: it runs on the compute stream, ahead of whatever comes next)
    launch_compact(s.st, s.d_cellkp, s.d_cellcnt, geom, d_lut, s.d_sorted, s.h_cand, tbl, s.h_overflow, nimg, compact_one_copy);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_c, s.st));
    return MCORB_OK;
}

int Rig::enqueue_tables_to_host(Slot &s, int nimg, bool by_kernel)
{
    const size_t bytes = (size_t)nimg * s.tbl_ints_per_image * sizeof(int);
    if (!by_kernel) HIPCHK(hipMemcpyAsync(s.h_tbl, s.d_tbl, bytes, hipMemcpyDeviceToHost, s.st_copy));
    else launch_copy_to_host(s.st_copy, s.d_tbl, s.h_tbl, bytes);
    HIPCHK(hipEventRecord(s.ev_tables, s.st_copy));
    return MCORB_OK;
}

int Rig::run_extract_phaseA(Slot &s, const Job &j)
{
    TRY(begin_extract(s, j));
    TRY(enqueue_front(s, j.nimg, s.host_results ? s.h_tbl : s.d_tbl));
    if (s.host_results) {
        HIPCHK(hipEventRecord(s.ev_tables, s.st));   // the tables are in host memory when k_compact is done
    } else {   // the DMA that takes the blocks to the host runs on the side stream
        HIPCHK(hipStreamWaitEvent(s.st_copy, s.ev_c, 0));
        TRY(enqueue_tables_to_host(s, j.nimg, copy_kernel));
        if (blur_planes) launch_blur(s.st, s.d_pyr, s.d_blur, geom, j.nimg);
    }
    HIPCHK(hipEventRecord(s.ev_blur, s.st));
    HIPCHK(hipGetLastError());
    return MCORB_OK;
}

// the keypoint record (ORBextractor.cpp:1103-1170's fields) of a retained candidate at (xl, yl) of its level's plane
mcorb_keypoint Rig::make_keypoint(int level, int xl, int yl, float response, float angle) const
{
    mcorb_keypoint kp;
    kp.x = (float)xl; kp.y = (float)yl;
    kp.size = (float)tab.scaled_patch[level];
    kp.angle = angle;
    kp.response = response;
    kp.octave = level;
    kp.class_id = -1;
    if (level != 0) { kp.x *= tab.scale[level]; kp.y *= tab.scale[level]; }
    return kp;
}

// per-kernel times (us) of a job that ran launch by launch, from its events
void Rig::read_timing(Slot &s, hipEvent_t blur0)
{
    float a = 0, b = 0, c = 0, t = 0;
    ev_elapsed(&a, s.ev_start, s.ev_fast);
    if (blur0) ev_elapsed(&b, blur0, s.ev_blur);
    ev_elapsed(&c, s.ev_desc0, s.ev_desc1);
    s.timing[T_FRONT] = a * 1000.f;
    s.timing[T_DESC] = (b + c) * 1000.f;
    s.timing[T_BLUR] = b * 1000.f;   // k_blur
    s.timing[T_DESCRIBE] = c * 1000.f;   // k_describe
    ev_elapsed(&t, s.ev_start, s.ev_pyr); s.timing[T_PYR] = t * 1000.f;   // pyramid launches
    ev_elapsed(&t, s.ev_pyr, s.ev_fast); s.timing[T_FAST] = t * 1000.f;   // k_fast_cells
    ev_elapsed(&t, s.ev_fast, s.ev_c); s.timing[T_COMPACT] = t * 1000.f;   // k_compact (the table DMA behind it is not included)
}

int Rig::run_select_and_describe(Slot &s, const Job &j, bool then_match)
{
    HIPCHK(wait_event(s.ev_tables));
    LatProf::mark(2);
    if (s.h_overflow[0]) {
        set_error(kCandOverflowMsg);
        (void)hipStreamSynchronize(s.st);
        return MCORB_E_OVERFLOW;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const int L = geom.nlevels, nimg = j.nimg;
    std::atomic<int> bad{0};
    // selection of one level of one image (worker w's scratch)
    auto select_level = [&](int m, int level, int w) {
        const int *tb = s.tbl(m);
        const int *lo = tb + kTblLvlOff, *shp = tb + kTblShipped;
        const int *bst = tb + kTblHead;
        const BucketWin *win = reinterpret_cast<const BucketWin *>(tb + tbl_win_off(geom.bucketTotal));
        const int n = lo[level + 1] - lo[level];
        std::vector<uint32_t> &out = s.sel_val[(size_t)m * L + level];
        out.resize((size_t)tab.quota[level] + 64);
        std::vector<int> &idx = scratch[w]->idx;
        idx.resize(out.size());
        int r = 0;
        if (n > 0)
            r = select_octree(shp[level] ? s.h_cand + (size_t)m * geom.hostCandCap + lo[level] : nullptr,
                              bst + geom.lv[level].bucket0, win + geom.lv[level].bucket0, n, selp[level],
                              idx.data(), out.data(), *scratch[w]);
        if (r == -3) { bad.store(3); r = 0; }
        if (r < 0) { bad.store(1); r = 0; }
        out.resize(r);
    };
    // selection + assembly: one task per image.  (One task per (image, level) for single rig frames was measured slower twice:
    // in round 2 the extra tasks waited for sleeping workers; in round 3, with the workers woken ahead of time and spinning, the
    // selection still went from 83 to 106 us: the per-image task streams its tables into the cache once, 32 small tasks miss
    // them one by one.  Waking the workers ahead of time by itself was worth 9 us of 92 for twelve spinning cores: not kept.
    // Two tasks per image (levels {0, 3, 4, 7} and {1, 2, 5, 6}; the one that finishes second assembles) with workers that
    // spin for 1 ms between jobs: 88 - 92 against 76 - 87 us: not kept either.)
    pool->parallel_for(nimg, [&](int m, int w) {
        HostProf::Scope prof_task(0);
        const int *tb = s.tbl(m);
        const int *lo = tb + kTblLvlOff, *shp = tb + kTblShipped;
        const int *bst = tb + kTblHead;
        const BucketWin *win = reinterpret_cast<const BucketWin *>(tb + tbl_win_off(geom.bucketTotal));
        {
            // the DMA engine wrote these over PCIe, so they sit in DRAM, not in this core's caches: stream them in with one
            // demand load per cache line instead of taking the misses one by one below (software prefetches were
            // measured slower, most get dropped)
            uint32_t touch = 0;
            const uint32_t *c = s.h_cand + (size_t)m * geom.hostCandCap;
            const uint32_t *b1 = reinterpret_cast<const uint32_t *>(bst);
            const uint32_t *b2 = reinterpret_cast<const uint32_t *>(win);
            for (int l = 0; l < L; l++) {
                if (shp[l])
                    for (int i = lo[l], e = lo[l + 1]; i < e; i += 16) touch += c[i];
                const int b0 = geom.lv[l].bucket0, nb = geom.lv[l].nBuckets + 1;
                for (int i = b0; i < b0 + nb; i += 16) touch += b1[i];
                for (int i = 2 * b0; i < 2 * (b0 + nb); i += 16) touch += b2[i];
            }
            s.touch_sink[m & 15] = touch;   // keeps the loads alive
        }
        {
            HostProf::Scope prof_sel(1);
            for (int level = 0; level < L; level++) select_level(m, level, w);
        }
        // assembly (ORBextractor.cpp:1103-1170): final order, lapping partition, coordinate scaling
        int total = 0;
        for (int l = 0; l < L; l++) total += (int)s.sel_val[(size_t)m * L + l].size();
        if (total > geom.kcap) { bad.store(2); total = 0; }
        std::vector<mcorb_keypoint> &K = s.kps[m];
        K.assign(total, mcorb_keypoint{});
        uint32_t *sel = s.hc.sel + (size_t)m * geom.kcap;
        int monoIndex = 0, stereoIndex = total - 1;
        if (total) {
            for (int l = 0; l < L; l++) {
                for (const uint32_t c : s.sel_val[(size_t)m * L + l]) {
                    const int xl = cand_x(c) + kMinBorder, yl = cand_y(c) + kMinBorder;
                    const mcorb_keypoint kp = make_keypoint(l, xl, yl, (float)cand_resp(c), 0.f);
                    int pos;
                    if (kp.x >= (float)j.lap0 && kp.x <= (float)j.lap1) pos = stereoIndex--;
                    else pos = monoIndex++;
                    K[pos] = kp;
                    sel[pos] = pack_sel(l, xl, yl);
                }
            }
        }
        s.mono[m] = monoIndex;
        s.hc.nsel[m] = total;
    }, pool_threads + s.index);
    if (bad.load() == 3) { set_error("internal: quad-tree went below the bucketing without the candidate list"); (void)hipStreamSynchronize(s.st); return MCORB_E_STATE; }
    if (bad.load() == 1) { set_error("selection failed: level too tall"); (void)hipStreamSynchronize(s.st); return MCORB_E_SIZE; }
    if (bad.load()) { set_error("keypoint capacity exceeded"); (void)hipStreamSynchronize(s.st); return MCORB_E_CAP; }
    const auto t1 = std::chrono::steady_clock::now();
    s.timing[T_SELECT] = std::chrono::duration<float, std::micro>(t1 - t0).count();
    LatProf::mark(3);

    s.nimg_done = nimg;
    if (then_match) TRY(prepare_match(s, j));
    TRY(enqueue_back(s, j, then_match, false));
    HIPCHK(hipEventRecord(s.ev_done, s.st));
    LatProf::mark(4);
    HIPCHK(wait_event(s.ev_done));   // (events, not stream synchronisation: wait_event waits the way the rig's wait_mode says)
    if (!s.host_results) HIPCHK(wait_event(s.ev_side));
    LatProf::mark(5);
    if (params.orientation)
        for (int m = 0; m < nimg; m++)
            for (size_t k = 0; k < s.kps[m].size(); k++) s.kps[m][k].angle = s.h_angles[(size_t)m * geom.kcap + k];
    read_timing(s, s.host_results ? nullptr : s.ev_c);
    return MCORB_OK;
}

// From ev_desc0 to the last operation the job enqueues: descriptors, then -- a small batch -- k_undistort forked onto the side stream
// beside them and the matcher, joined in front of the BoW stages, no copies; or -- a large batch -- the result copies on the side
// stream while the BoW stages and the matcher run.  ev_side closes the side stream's work (a GPU-selected small batch's: the compute
// stream's; the host-selected small batch has none and records nothing).
int Rig::enqueue_back(Slot &s, const Job &j, bool then_match, bool gpu_sel)
{
    const int nimg = j.nimg;
    const bool small = s.host_results, ev_on = s.ev_on();
    // selected on the host: one H2D copy of the control block -- counts, pair list, packed selected keypoints
    if (!gpu_sel && !small) HIPCHK(hipMemcpyAsync(s.d_ctrl, s.h_ctrl, s.ctrl_bytes, hipMemcpyHostToDevice, s.st));
    if (ev_on) HIPCHK(hipEventRecord(s.ev_desc0, s.st));
    if (small && undist_on) {   // fork: into host-mapped memory (ev_u0, not ev_desc0: a captured job records no ev_desc0)
        HIPCHK(hipEventRecord(s.ubuf.ev_u0, s.st));
        HIPCHK(hipStreamWaitEvent(s.st_dma, s.ubuf.ev_u0, 0));
        TRY(enqueue_undistort(s, nimg));
    }
    launch_describe(s.st, s.d_pyr, blur_planes ? s.d_blur : nullptr, geom, s.ctl.sel, s.ctl.nsel, params.orientation, s.d_desc, s.d_angles, nimg,
                    small ? s.h_desc : nullptr);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_desc1, s.st));
    if (small) {
        if (then_match) TRY(enqueue_match(s, j, true));
        HIPCHK(hipGetLastError());
        if (undist_on) HIPCHK(hipStreamWaitEvent(s.st, s.ubuf.ev_u1, 0));   // join
        if (s.bow_job) TRY(enqueue_bow(s, nimg));
        if (gpu_sel && ev_on) HIPCHK(hipEventRecord(s.ev_side, s.st));
        return MCORB_OK;
    }
    // results to the host on the side stream (DMA) while the matcher already runs: descriptors; of a GPU-selected job also the
    // control block from nsel on (nsel, the set map and pair list as uploaded, sel) and responses + monoIndex + flags.
    // (The descriptor copy starts beside k_expand.  Whatever kernel of the job ENDS while the copy's host writes are in flight is
    // held until they have drained -- k_expand 12 -> 148 us beside the copy, k_knn2 154 -> 276 us when the copy starts behind
    // k_expand, with the runtime's blit and with k_copy_to_host alike (profiles/r03_copy_kernel_ab.txt) -- so the copy stays beside
    // k_expand, whose result nobody needs before k_knn2 anyway: 13.3 k vs 13.0 k frames/s at one slot.)
    const size_t nk = (size_t)nimg * geom.kcap;
    HIPCHK(hipStreamWaitEvent(s.st_dma, s.ev_desc1, 0));
    if (!copy_kernel) HIPCHK(hipMemcpyAsync(s.h_desc, s.d_desc, nk * 32, hipMemcpyDeviceToHost, s.st_dma));
    else launch_copy_to_host(s.st_dma, s.d_desc, s.h_desc, nk * 32);
    if (gpu_sel) {
        HIPCHK(hipMemcpyAsync(s.h_ctrl + s.ctrl_nsel_off, s.d_ctrl + s.ctrl_nsel_off, s.ctrl_pairs_end - s.ctrl_nsel_off + nk * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, s.st_dma));
        HIPCHK(hipMemcpyAsync(s.h_res, s.d_res, s.res_resp_off + nk, hipMemcpyDeviceToHost, s.st_dma));
    }
    if (params.orientation) HIPCHK(hipMemcpyAsync(s.h_angles, s.d_angles, nk * sizeof(float), hipMemcpyDeviceToHost, s.st_dma));
    if (undist_on) TRY(enqueue_undistort(s, nimg));   // behind the result copies: the side stream's last work
    if (s.bow_job) TRY(enqueue_bow(s, nimg));
    if (then_match) TRY(enqueue_match(s, j, true));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s.ev_side, s.st_dma));
    return MCORB_OK;
}

// everything a GPU-selected job puts on the slot's streams, from the control block's head to the result copies
int Rig::enqueue_gpu_job(Slot &s, const Job &j, bool then_match)
{
    const int nimg = j.nimg;
    (void)hipGetLastError();   // (a stale error of this thread -- e.g. an elapsed-time query on an event a replayed graph never recorded -- is not this job's)
    const bool small = s.host_results, ev_on = s.ev_on();
    if (then_match && !small)   // pair list / set map first: k_assemble overwrites the control block's nsel and sel afterwards, in stream order
        HIPCHK(hipMemcpyAsync(s.d_ctrl, s.h_ctrl, s.ctrl_pairs_end, hipMemcpyHostToDevice, s.st));
    int *d_flags = reinterpret_cast<int *>(s.d_res.get());
    if (!small) HIPCHK(hipMemsetAsync(d_flags, 0, 16 * sizeof(int), s.st));   // (a small batch's flags travel with its per-image signals)
    TRY(enqueue_front(s, nimg, s.d_tbl));
    HIPCHK(launch_select(s.st, s.d_tbl, s.d_sorted, geom, s.d_selval, s.d_selcnt, d_flags, nimg, select_deep_cap, select_prof));
    launch_assemble(s.st, s.d_selval, s.d_selcnt, geom, tab.scale, j.lap0, j.lap1, s.dc.sel, s.d_res + s.res_resp_off, s.dc.nsel,
                    reinterpret_cast<int *>(s.d_res + s.res_mono_off), d_flags, nimg, small ? s.hc.sel : nullptr,
                    small ? s.h_res + s.res_resp_off : nullptr, small ? s.h_sig : nullptr);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_s, s.st));
    if (ev_on) HIPCHK(hipEventRecord(s.ev_tables, s.st));
    if (blur_planes) launch_blur(s.st, s.d_pyr, s.d_blur, geom, nimg);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_blur, s.st));
    return enqueue_back(s, j, then_match, true);
}

void Rig::gpu_job_begin()
{
    if (!gpu_job_limit) return;
    std::unique_lock<std::mutex> lk(gpu_jobs_m);
    gpu_jobs_cv.wait(lk, [this] { return gpu_jobs_running < gpu_job_limit; });
    gpu_jobs_running++;
}
void Rig::gpu_job_end()
{
    if (!gpu_job_limit) return;
    {
        std::lock_guard<std::mutex> lk(gpu_jobs_m);
        gpu_jobs_running--;
    }
    gpu_jobs_cv.notify_one();
}

// MCORB_SELECT_GPU: the whole job -- pyramid, FAST, compaction, selection, assembly, descriptors, matching -- is enqueued in one go;
// the host comes back when the results have landed (descriptors, the control block's sel / nsel, responses, monoIndex, flags) and
// only builds its keypoint records from them.  A batch with a level whose tree goes below the bucketing depth (flag) is redone
// through the host stage: run_select_and_describe on the tables, exactly the MCORB_SELECT_HOST path.
int Rig::run_gpu_selected(Slot &s, const Job &j, bool then_match)
{
    TRY(begin_extract(s, j));
    const int nimg = j.nimg;
    s.nimg_done = nimg;
    if (then_match) TRY(prepare_match(s, j));
    if (s.host_results)
        for (int m = 0; m < nimg; m++) static_cast<volatile unsigned long long *>(s.h_sig)[m] = 0;
    // The job is the same ~20 launches and copies every time: captured once per (slot, shape of the job) into a HIP graph and
    // replayed with one call -- the CPU side of a job drops from ~20 runtime calls to one, the gaps between its kernels shrink.
    // (Per-kernel HIP events do not exist inside a replayed graph: mcorb_rig_last_timing reports the job as a whole then.)
    // graph_every: 0 = never, 1 = every job, K > 1 = all but every K-th job of a slot, which runs launch by launch with its
    // per-kernel events (a sample of the same pipeline for mcorb_rig_last_timing)
    // keypoint records of one image from what k_assemble left
    auto records = [&](int m) {
        const int n = s.hc.nsel[m];
        std::vector<mcorb_keypoint> &K = s.kps[m];
        K.resize((size_t)n);
        const uint32_t *sel = s.hc.sel + (size_t)m * geom.kcap;
        const uint8_t *rs = s.h_res + s.res_resp_off + (size_t)m * geom.kcap;
        const float *ang = params.orientation ? s.h_angles + (size_t)m * geom.kcap : nullptr;
        for (int k = 0; k < n; k++) {
            int level, x, y;
            unpack_sel(sel[k], level, x, y);
            K[k] = make_keypoint(level, x, y, (float)rs[k], ang ? ang[k] : 0.f);
        }
        s.mono[m] = reinterpret_cast<const int *>(s.h_res + s.res_mono_off)[m];
    };
    // a small batch: count, monoIndex and flags of an image travel in its signal word (sel_signal()); returns the count
    int small_flags = 0;
    auto decode_signal = [&](int m, unsigned long long w) {
        small_flags |= sel_signal_bad(w);
        const int n = std::min(sel_signal_count(w), geom.kcap);   // (k_assemble never signals more than kcap; the clamp is for the reads that follow)
        s.hc.nsel[m] = n;
        reinterpret_cast<int *>(s.h_res + s.res_mono_off)[m] = sel_signal_mono(w);
        return n;
    };
    // a small batch: the records are built here, image by image as k_assemble signals them, while the descriptor and matching
    // kernels still run; returns the number of images done (all of them unless the job ended without signalling: an error), -1 on
    // a HIP error
    int records_done = 0, early_stale = 0;
    auto records_early = [&](hipEvent_t end) {
        const volatile unsigned long long *sig = s.h_sig;
        for (int m = 0; m < nimg; m++) {
            unsigned spins = 0;
            while (!sig[m]) {
                if ((++spins & (wait_mode == 2 ? 0u : 1023u)) == 0) {
                    const hipError_t e = hipEventQuery(end);
                    if (e == hipSuccess) { if (!sig[m]) return; break; }   // the job is over: nothing more will be signalled
                    if (e != hipErrorNotReady) { set_error(std::string("event query: ") + hipGetErrorString(e)); records_done = -1; return; }
                }
                if (wait_mode == 2) { timespec ts = {0, 20000}; nanosleep(&ts, nullptr); }   // (slot drivers that poll: no core per slot)
                else __builtin_ia32_pause();
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            const unsigned long long w = sig[m];
            const int n = decode_signal(m, w);
            // the word also carries a checksum of the sel / response values k_assemble sent: values the word does not vouch for have
            // not all landed yet (never seen with the atomic signal; cheap to be sure) -- this image and the ones behind it are expanded
            // after the job's end event instead
            uint32_t x = 0;
            const uint32_t *sel = s.hc.sel + (size_t)m * geom.kcap;
            const uint8_t *rs = s.h_res + s.res_resp_off + (size_t)m * geom.kcap;
            for (int k = 0; k < n; k++) x ^= sel_check(sel[k], rs[k], k);
            if (x != sel_signal_check(w)) { early_stale++; return; }
            records(m);
            records_done = m + 1;
        }
    };
    const int ge = graph_every.load(std::memory_order_relaxed);
    const bool graphed = ge > 0 && !j.ext_desc && (ge == 1 || (++s.job_counter % ge) != 0);
    struct GpuTurn {   // this slot's turn on the GPU: from the first launch until the results have landed
        Rig &r; bool held = true;
        explicit GpuTurn(Rig &rig) : r(rig) { r.gpu_job_begin(); }
        void done() { if (held) { held = false; r.gpu_job_end(); } }
        ~GpuTurn() { done(); }
    } turn(*this);
    if (graphed) {
        const Slot::GraphKey key{nimg, then_match ? 1 : 0, j.nframes, j.lap0, j.lap1, j.dist_thresh, j.ratio, undist_on ? 1 : 0,
                                 bow_bind.flags, bow_bind.flags ? bow_bind.levelsup : 0, bow_gen, lf_on ? 1 : 0, lf_gen};
        if (!s.graph_exec || memcmp(&key, &s.graph_key, sizeof(key)) != 0) {
            if (s.graph_exec) { (void)hipGraphExecDestroy(s.graph_exec); s.graph_exec = nullptr; }
            hipGraph_t graph = nullptr;
            HIPCHK(hipStreamBeginCapture(s.st, hipStreamCaptureModeThreadLocal));
            s.capturing = true;
            int st = enqueue_gpu_job(s, j, then_match);
            s.capturing = false;
            hipError_t e = s.host_results ? hipSuccess : hipStreamWaitEvent(s.st, s.ev_side, 0);   // the side stream joins again
            const hipError_t e2 = hipStreamEndCapture(s.st, &graph);
            if (st != MCORB_OK) { if (graph) (void)hipGraphDestroy(graph); return st; }
            if (e == hipSuccess) e = e2;
            if (e == hipSuccess) e = hipGraphInstantiate(&s.graph_exec, graph, nullptr, nullptr, 0);
            if (graph) (void)hipGraphDestroy(graph);
            if (e != hipSuccess) { s.graph_exec = nullptr; set_error(std::string("graph capture: ") + hipGetErrorString(e)); return MCORB_E_HIP; }
            s.graph_key = key;
        }
        HIPCHK(hipEventRecord(s.ev_g, s.st));
        HIPCHK(hipGraphLaunch(s.graph_exec, s.st));
    } else {
        TRY(enqueue_gpu_job(s, j, then_match));
    }
    HIPCHK(hipEventRecord(s.ev_done, s.st));
    LatProf::mark(1); LatProf::mark(2); LatProf::mark(3);
    if (s.host_results) records_early(s.ev_done);
    LatProf::mark(4);
    HIPCHK(wait_event(s.ev_done));
    if (!graphed) HIPCHK(wait_event(s.ev_side));   // (the replayed graph joins the side stream itself)
    LatProf::mark(5);
    turn.done();
    if (s.h_overflow[0]) { set_error(kCandOverflowMsg); return MCORB_E_OVERFLOW; }
    if (records_done < 0) return MCORB_E_HIP;
    if (s.host_results && records_done < nimg) {
        // the job is over: every signal word and everything behind it has landed
        for (int m = records_done; m < nimg; m++) {
            const unsigned long long w = static_cast<const volatile unsigned long long *>(s.h_sig)[m];
            if (!sel_signal_done(w)) { set_error("extract: the job ended without its results"); return MCORB_E_HIP; }
            decode_signal(m, w);
        }
        s.stale_reads.fetch_add(early_stale, std::memory_order_relaxed);
    }
    const int flags = s.host_results ? small_flags : reinterpret_cast<const int *>(s.h_res.get())[0];
    if (flags) {
        // the host stage on the same tables (bit 0: a tree below the bucketing depth; bit 1: more than kcap keypoints -- the host
        // stage reports that error itself)
        s.fallbacks.fetch_add(1, std::memory_order_relaxed);
        s.graph_timing = false;
        s.host_results = false;   // (the host stage uploads the whole control block and copies its results back)
        s.set_ctl(false, false);
        TRY(enqueue_tables_to_host(s, nimg, false));   // (the runtime's copy, whatever copy_kernel says for the first pass)
        return run_select_and_describe(s, j, then_match);
    }
    if (records_done < nimg) pool->parallel_for(nimg, [&](int m, int) { records(m); }, pool_threads + s.index);
    if (then_match && !j.ext_desc)
        for (size_t i = 0; i < s.match_counts.size(); i++) s.match_counts[i] = s.hc.nsel[s.match_sets[i]];
    s.graph_timing = graphed;
    if (graphed) {   // one interval: the whole job
        float a = 0;
        for (float &v : s.timing) v = 0.f;
        ev_elapsed(&a, s.ev_g, s.ev_done);
        s.timing[T_FRONT] = a * 1000.f;
        return MCORB_OK;
    }
    read_timing(s, s.ev_tables);
    float t = 0;
    ev_elapsed(&t, s.ev_c, s.ev_s); s.timing[T_SELECT] = t * 1000.f;   // k_select + k_assemble
    return MCORB_OK;
}

}  // namespace mcorb
