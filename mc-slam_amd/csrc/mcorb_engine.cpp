// mcorb_engine.cpp -- host orchestration: tables, geometry, buffers, slot drivers.
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
#include "mcorb_engine.h"

#include <alloca.h>
#include <math.h>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>

#include <sched.h>
#include <sys/prctl.h>
#include <algorithm>
#include <new>
#include <cmath>
#include <chrono>

namespace mcorb {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
const char *get_error() { return g_err.c_str(); }

static inline int cv_round_f(float v) { return (int)lrintf(v); }
static inline int cv_round_d(double v) { return (int)lrint(v); }
static inline int cv_floor_f(float v) { int i = (int)v; return i - (i > v); }
static inline int cv_ceil_f(float v) { int i = (int)v; return i + (i < v); }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---------------------------------------------------------------------------
// ORBextractor::ORBextractor (ORBextractor.cpp:408-468).  scaleFactor is a
// double member initialised from a float argument (ORBextractor.h:103).
// ---------------------------------------------------------------------------
int compute_tables(const mcorb_params &p, Tables &t)
{
    if (p.nlevels < 1 || p.nlevels > kMaxLevels || p.nfeatures < 1 || !(p.scale_factor > 1.0f)) {
        set_error("bad extractor parameters");
        return MCORB_E_ARG;
    }
    const int L = p.nlevels;
    const double sf = (double)p.scale_factor;
    t.nlevels = L;
    t.scale[0] = 1.0f;
    t.sigma2[0] = 1.0f;
    for (int i = 1; i < L; i++) {
        t.scale[i] = (float)((double)t.scale[i - 1] * sf);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    for (int i = 0; i < L; i++) {
        t.inv_scale[i] = 1.0f / t.scale[i];
        t.inv_sigma2[i] = 1.0f / t.sigma2[i];
        t.scaled_patch[i] = (int)(31 * t.scale[i]);   // PATCH_SIZE*mvScaleFactor[level] (:879)
    }
    const float factor = (float)(1.0 / sf);
    float desired = (float)p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
        t.quota[l] = cv_round_f(desired);
        sum += t.quota[l];
        desired *= factor;
    }
    t.quota[L - 1] = std::max(p.nfeatures - sum, 0);
    // umax (:450-467)
    const int HP = 15;
    int v, v0;
    const int vmax = cv_floor_f(HP * sqrtf(2.f) / 2 + 1);
    const int vmin = cv_ceil_f(HP * sqrtf(2.f) / 2);
    const double hp2 = HP * HP;
    for (v = 0; v < 16; v++) t.umax[v] = 0;
    for (v = 0; v <= vmax; ++v) t.umax[v] = cv_round_d(sqrt(hp2 - v * v));
    for (v = HP, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    return MCORB_OK;
}

// cv::resize's table loop for one axis: x clamps (sx, fx), y keeps
// the fraction and clips the row indices at use.
void build_resize_axis(int ssize, int dsize, bool is_x, std::vector<ResizeTap> &out, int pad_to)
{
    const double scale = (double)ssize / dsize;
    const size_t first = out.size();
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = cv_floor_f(f);
        f -= s;
        if (is_x) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= ssize - 1) { f = 0; s = ssize - 1; }
        }
        int c0 = cv_round_f((1.f - f) * 2048.f), c1 = cv_round_f(f * 2048.f);
        c0 = std::min(std::max(c0, -32768), 32767);
        c1 = std::min(std::max(c1, -32768), 32767);
        int s0 = std::min(std::max(s, 0), ssize - 1);
        int s1 = std::min(std::max(s + 1, 0), ssize - 1);
        if (is_x && s + 1 >= ssize) { c0 = 2048; c1 = 0; }   // HResizeLinear tail: S[sx]*ONE
        ResizeTap t;
        t.s0 = (uint16_t)s0; t.s1 = (uint16_t)s1; t.c0 = (int16_t)c0; t.c1 = (int16_t)c1;
        out.push_back(t);
    }
    // padding: copies of the last tap, so that a kernel reading whole groups of `pad_to` never sees an out-of-range column
    const ResizeTap last = out.size() > first ? out.back() : ResizeTap{0, 0, 0, 0};
    while ((out.size() - first) % pad_to) out.push_back(last);
}

int build_geometry(const mcorb_params &p, const Tables &t, int W, int H, Geom &g, std::vector<ResizeTap> &taps,
                   std::vector<uint16_t> *lut)
{
    memset(&g, 0, sizeof(g));
    taps.clear();
    if (lut) lut->clear();
    g.nlevels = t.nlevels;
    size_t off = 0;
    int cells = 0, tiles = 0, cellCap = 4, buckets = 0;
    for (int l = 0; l < t.nlevels; l++) {
        LevelGeom &L = g.lv[l];
        const float sc = t.inv_scale[l];
        L.w = cv_round_f((float)W * sc);   // ORBextractor.cpp:1177-1178
        L.h = cv_round_f((float)H * sc);
        L.maxBorderX = L.w - kEdge + 3;
        L.maxBorderY = L.h - kEdge + 3;
        const float width = (float)(L.maxBorderX - kMinBorder);
        const float height = (float)(L.maxBorderY - kMinBorder);
        L.nCols = (int)(width / (float)kCellW);
        L.nRows = (int)(height / (float)kCellW);
        if (L.nCols < 1 || L.nRows < 1) {
            set_error("image too small for the reference's 35-px cell grid at level " + std::to_string(l));
            return MCORB_E_SIZE;
        }
        L.wCell = (int)ceilf(width / L.nCols);
        L.hCell = (int)ceilf(height / L.nRows);
        const SelectParams sp = make_select_params(kMinBorder, L.maxBorderX, kMinBorder, L.maxBorderY, t.quota[l], 1, 1);
        if (sp.nIni < 1) {
            set_error("image too tall: DistributeOctTree would have no root node");
            return MCORB_E_SIZE;
        }
        if (sp.nIni > 16) { set_error("image too wide (more than 16 root nodes)"); return MCORB_E_SIZE; }
        L.nIni = sp.nIni;
        L.hX = sp.hX;
        L.depth = sp.depth;
        L.nBuckets = sp.nIni << (2 * sp.depth);
        L.bucket0 = buckets;
        L.quota = t.quota[l];
        buckets += L.nBuckets + 1;
        if (lut) {   // path-code tables of this level (k_compact): code(x, y) = lut[L.lutx + x] | lut[L.luty + y]
            const int W0 = L.maxBorderX - kMinBorder, H0 = L.maxBorderY - kMinBorder;
            L.lutx = (uint32_t)lut->size();
            L.luty = L.lutx + (uint32_t)W0;
            lut->resize(lut->size() + (size_t)W0 + H0);
            path_code_tables(W0, H0, L.nIni, L.hX, L.depth, lut->data() + L.lutx, lut->data() + L.luty);
            while (lut->size() & 7) lut->push_back(0);
        }
        if (L.w > 4096 || L.h > 4096) { set_error("image larger than 4096 px"); return MCORB_E_SIZE; }
        L.pitch = (int)align_up((size_t)L.w, 64);
        L.off = (uint32_t)off;
        off += align_up((size_t)L.pitch * align_up((size_t)L.h, kBlurTileRows), 256);   // whole 16x8 tiles (blurred planes)
        L.cell0 = cells;
        cells += L.nCols * L.nRows;
        L.tilesX = (L.w + kBlurTW - 1) / kBlurTW;
        L.tilesY = (L.h + kBlurTH - 1) / kBlurTH;
        L.tile0 = tiles;
        tiles += L.tilesX * L.tilesY;
        cellCap = std::max(cellCap, ((L.wCell + 1) / 2) * ((L.hCell + 1) / 2));
        if (l > 0) {
            L.xtab = (uint32_t)taps.size();
            build_resize_axis(g.lv[l - 1].w, L.w, true, taps, 4);
            L.ytab = (uint32_t)taps.size();
            build_resize_axis(g.lv[l - 1].h, L.h, false, taps, 4);
        }
    }
    g.cells = cells;
    g.tiles = tiles;
    g.bucketTotal = buckets;
    g.cellCap = (int)align_up((size_t)cellCap, 4);
    g.imgBytes = (uint32_t)(off + 256);
    g.kcap = (int)align_up((size_t)p.nfeatures + 4 * t.nlevels + 48, 64);
    if (g.kcap > 65535) { set_error("nfeatures too large (k-NN index is 16 bits)"); return MCORB_E_ARG; }
    // default: one candidate slot per 4 level-0 pixels (measured: ~1 per 28 px on the synthetic rig frames)
    // device list: worst case (every cell full: one corner per 2x2 px survives the 3x3 NMS at most), so FAST itself can
    // never overflow; host copy: one slot per 4 level-0 pixels by default (~1 per 28 px measured on the synthetic rig
    // frames) -- it is only written when the quad-tree may go below the bucketing, i.e. for sparse levels
    g.candCap = (int)align_up((size_t)g.cells * g.cellCap, 4096);
    g.hostCandCap = p.cand_cap > 0 ? p.cand_cap : (int)align_up(std::max((size_t)65536, (size_t)W * H / 4), 4096);
    if (g.hostCandCap > g.candCap) g.hostCandCap = g.candCap;
    if (g.lv[0].nCols * g.lv[0].nRows * g.cellCap > kPickOrderMask) { set_error("image too large (pick order is 23 bits)"); return MCORB_E_SIZE; }
    return MCORB_OK;
}

// ---------------------------------------------------------------------------
// optional host-side profile (MCORB_HOST_PROF=1): wall and thread-CPU time of the selection tasks
// ---------------------------------------------------------------------------
namespace HostProf {
static const bool on = getenv("MCORB_HOST_PROF") != nullptr;
static std::atomic<long long> wall[4], cpu[4], cnt[4];
static inline long long now(clockid_t c) { timespec t; clock_gettime(c, &t); return t.tv_sec * 1000000000LL + t.tv_nsec; }
struct Scope {
    int k; long long w0 = 0, c0 = 0;
    explicit Scope(int k_) : k(k_) { if (on) { w0 = now(CLOCK_MONOTONIC); c0 = now(CLOCK_THREAD_CPUTIME_ID); } }
    ~Scope() { if (on) { wall[k] += now(CLOCK_MONOTONIC) - w0; cpu[k] += now(CLOCK_THREAD_CPUTIME_ID) - c0; cnt[k]++; } }
};
static void report()
{
    if (!on) return;
    const char *names[4] = {"select task (per image)", "  select_octree x levels", "finish_match (per job)", "prepare_match (per job)"};
    for (int k = 0; k < 4; k++)
        if (cnt[k].load())
            fprintf(stderr, "[mcorb host prof] %-26s n=%lld wall %.1f us cpu %.1f us\n", names[k], cnt[k].load(),
                    wall[k].load() / 1e3 / cnt[k].load(), cpu[k].load() / 1e3 / cnt[k].load());
}
}  // namespace HostProf

// ---------------------------------------------------------------------------
// worker pool
// ---------------------------------------------------------------------------
WorkerPool::WorkerPool(int nthreads)
{
    for (int i = 0; i < nthreads; i++) threads_.emplace_back([this, i] { run(i); });
}
WorkerPool::~WorkerPool()
{
    {
        std::lock_guard<std::mutex> lk(m_);
        stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : threads_) t.join();
}
void WorkerPool::run(int widx)
{
    for (;;) {
        Batch *b = nullptr;
        {
            std::unique_lock<std::mutex> lk(m_);
            // spin briefly before sleeping: batches arrive every few hundred microseconds when the
            // pipeline is busy, and a futex wake-up costs more than the selection of one image
            if (queue_.empty() && !stop_) {
                lk.unlock();
                const auto t0 = std::chrono::steady_clock::now();
                while (pending_.load(std::memory_order_acquire) == 0 &&
                       std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(150)) {
                    __builtin_ia32_pause();
                }
                lk.lock();
            }
            cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
            if (stop_ && queue_.empty()) return;
            b = queue_.front();
            if (b->next.load() >= b->n) {   // exhausted: drop it from the queue
                queue_.erase(queue_.begin());
                pending_.fetch_sub(1, std::memory_order_acq_rel);
                continue;
            }
            b->refs.fetch_add(1, std::memory_order_acq_rel);   // the batch lives on its submitter's stack
        }
        for (;;) {
            const int t = b->next.fetch_add(1);
            if (t >= b->n) break;
            (*b->fn)(t, widx);
            if (b->done.fetch_add(1) + 1 == b->n) {
                std::lock_guard<std::mutex> lk(b->m);
                b->cv.notify_all();
            }
        }
        b->refs.fetch_sub(1, std::memory_order_acq_rel);
    }
}
void WorkerPool::parallel_for(int n, const std::function<void(int, int)> &fn, int caller_widx)
{
    if (n <= 0) return;
    Batch b;
    b.fn = &fn;
    b.n = n;
    {
        std::lock_guard<std::mutex> lk(m_);
        queue_.push_back(&b);
        pending_.fetch_add(1, std::memory_order_acq_rel);
    }
    cv_.notify_all();
    // the submitting thread works on its own batch too (with its own scratch index): a one-frame batch does not
    // have to wait for a sleeping worker to wake up
    if (caller_widx >= 0) {
        for (;;) {
            const int t = b.next.fetch_add(1);
            if (t >= b.n) break;
            fn(t, caller_widx);
            b.done.fetch_add(1);
        }
    }
    {
        std::unique_lock<std::mutex> lk(b.m);
        b.cv.wait(lk, [&b] { return b.done.load() >= b.n; });
    }
    {
        std::lock_guard<std::mutex> lk(m_);   // after this no new worker can pick the batch up
        auto it = std::find(queue_.begin(), queue_.end(), &b);
        if (it != queue_.end()) {
            queue_.erase(it);
            pending_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    while (b.refs.load(std::memory_order_acquire) != 0) std::this_thread::yield();   // workers still leaving the task loop
}

// ---------------------------------------------------------------------------
// Rig
// ---------------------------------------------------------------------------
// Elapsed milliseconds between two events of a finished job; 0 when either was not recorded on a stream (a job that ran from its
// captured graph holds them as graph nodes).  A failed query must not stay behind as the thread's "last error".
static inline void ev_elapsed(float *ms, hipEvent_t a, hipEvent_t b)
{
    if (hipEventElapsedTime(ms, a, b) != hipSuccess) { *ms = 0.f; (void)hipGetLastError(); }
}

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

// Cores this process can actually use: hardware threads, cut down to the scheduler affinity mask and to the cgroup CPU
// quota (v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us), whichever is smallest.
static int usable_cores()
{
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(n, std::max(1, CPU_COUNT(&set)));
    long long quota = -1, period = 0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
        fclose(f);
    } else {
        FILE *fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"), *fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
        if (fq && fp && fscanf(fq, "%lld", &quota) == 1 && fscanf(fp, "%lld", &period) == 1) {}
        else quota = -1;
        if (fq) fclose(fq);
        if (fp) fclose(fp);
    }
    if (quota > 0 && period > 0) n = std::min(n, (int)std::max(1LL, quota / period));
    // one process per GPU on a multi-GPU node: the ranks of the node share those cores (torch.distributed.run exports
    // LOCAL_WORLD_SIZE; MCORB_LOCAL_RANKS says the same for other launchers)
    const char *lr = getenv("MCORB_LOCAL_RANKS") ? getenv("MCORB_LOCAL_RANKS") : getenv("LOCAL_WORLD_SIZE");
    const int ranks = lr ? atoi(lr) : 1;
    if (ranks > 1) n = std::max(2, n / ranks);
    return n;
}

constexpr unsigned kHostMapped = hipHostMallocMapped | hipHostMallocPortable;
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
    // LDS source window of one resize workgroup (256 x kResizeTileH outputs): widest column span / tallest row span per level
    for (int l = 1; l < geom.nlevels; l++) {
        const LevelGeom &D = geom.lv[l];
        int maxc = 16, maxr = 2;
        for (int bx0 = 0; bx0 < D.w; bx0 += 256) {
            const int bx1 = std::min(bx0 + 255, D.w - 1);
            const int a = taps[D.xtab + bx0].s0 & ~15, b = taps[D.xtab + bx1].s1;
            maxc = std::max(maxc, ((b - a) / 16 + 1) * 16);
        }
        for (int by0 = 0; by0 < D.h; by0 += kResizeTileH) {
            const int by1 = std::min(by0 + kResizeTileH - 1, D.h - 1);
            maxr = std::max(maxr, (int)taps[D.ytab + by1].s1 - (int)taps[D.ytab + by0].s0 + 1);
        }
        resize_win[2 * l] = maxc;
        resize_win[2 * l + 1] = maxr;
        if ((size_t)maxc * maxr > 60000) { set_error("scale factor too large for the resize window"); return MCORB_E_ARG; }
    }
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
    const char *sync_env0 = getenv("MCORB_SYNC");
    wait_mode = nslots > 1 ? 2 : 0;
    if (sync_env0) wait_mode = !strcmp(sync_env0, "block") ? 1 : (!strcmp(sync_env0, "poll") ? 2 : 0);
    const bool crowded = wait_mode == 1;   // events created with hipEventBlockingSync
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
        // events a driver thread waits on (3 compaction, 10 compute stream, 11 DMA stream).  HIP spins by default, which
        // measured 2-4 % faster than interrupt-driven waits at 6 slots; with many slots the spinning drivers would take
        // the cores the selection workers need, so those rigs sleep instead.  MCORB_SYNC=block|spin overrides.
        const char *sync_env = getenv("MCORB_SYNC");
        const bool blocking = sync_env ? !strcmp(sync_env, "block") : crowded;
        TRY(s->ev_x.create(hipEventDisableTiming));
        TRY(s->ev_c.create(hipEventDefault));
        TRY(s->ev_e.create(hipEventDefault));
        for (int e = 0; e < 12; e++) {
            const bool waited = e == 3 || e == 10 || e == 11;
            TRY(s->ev[e].create(waited && blocking ? hipEventBlockingSync : hipEventDefault));
        }
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
            s->h_extcounts = (int *)s->h_ctrl.get();        s->d_extcounts = (int *)s->d_ctrl.get();
            s->h_nsel = (int *)(s->h_ctrl + o_nsel);      s->d_nsel = (int *)(s->d_ctrl + o_nsel);
            s->h_setmap = (int *)(s->h_ctrl + o_setmap);  s->d_setmap = (int *)(s->d_ctrl + o_setmap);
            s->h_pairs = (int2 *)(s->h_ctrl + o_pairs);   s->d_pairs = (int2 *)(s->d_ctrl + o_pairs);
            s->h_sel = (uint32_t *)(s->h_ctrl + o_sel);   s->d_sel = (uint32_t *)(s->d_ctrl + o_sel);
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

// An upload into a slot whose job is still running would overwrite the staging buffer and level 0 between the job's
// GPU phases (the slot's stream is idle while the host selects): refuse it like every other call on a busy slot.
constexpr int kSmallBatch = 8;   // images: at most two 4-camera rig frames
static const char *const kCandOverflowMsg = "candidate list of a sparse level does not fit the host buffer (raise mcorb_params.cand_cap)";

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

// MCORB_LAT_PROF=1: where a synchronous PROCESS job spends its wall time (host clock), printed every 50 jobs
namespace LatProf {
static const bool on = getenv("MCORB_LAT_PROF") != nullptr;
static thread_local double t[12];
static thread_local double acc[12];
static thread_local int n = 0;
static inline void mark(int i) { if (on) t[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void flush()
{
    if (!on) return;
    for (int i = 1; i < 9; i++) acc[i] += t[i] - t[i - 1];
    acc[9] += t[9] - t[6]; acc[10] += t[10] - t[9];   // inside finish_match: accept lists unpacked | tracks merged
    if (++n % 50 == 0) {
        fprintf(stderr, "[mcorb lat prof] per job: enqueue A %.0f us, wait tables %.0f, select %.0f, prepare+enqueue B %.0f, wait GPU %.0f, post %.0f, merge %.0f (lists %.0f, tracks %.0f), total %.0f\n",
                acc[1] / 50, acc[2] / 50, acc[3] / 50, acc[4] / 50, acc[5] / 50, acc[6] / 50, acc[7] / 50, acc[9] / 50, acc[10] / 50, (acc[1] + acc[2] + acc[3] + acc[4] + acc[5] + acc[6] + acc[7]) / 50);
        for (int i = 0; i < 12; i++) acc[i] = 0;
    }
}
}  // namespace LatProf

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
            hipError_t e = hipEventRecord(s.ev[10], s.st);
            if (e == hipSuccess) e = wait_event(s.ev[10]);
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
    if (ev_on) HIPCHK(hipEventRecord(s.ev[0], s.st));
    launch_pyramid(s.st, s.d_pyr, geom, d_taps, resize_win, nimg);
    if (ev_on) HIPCHK(hipEventRecord(s.ev[1], s.st));
    launch_fast(s.st, s.d_pyr, geom, params.ini_th_fast, params.min_th_fast, d_fasttab + fast_cell_off, s.d_cellkp, s.d_cellcnt, nimg);
    if (ev_on) HIPCHK(hipEventRecord(s.ev[2], s.st));
    // compaction fills the per-image table blocks (a short kernel: it runs on the compute stream, ahead of whatever comes next)
    launch_compact(s.st, s.d_cellkp, s.d_cellcnt, geom, d_lut, s.d_sorted, s.h_cand, tbl, s.h_overflow, nimg, compact_one_copy);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_c, s.st));
    return MCORB_OK;
}

int Rig::run_extract_phaseA(Slot &s, const Job &j)
{
    TRY(begin_extract(s, j));
    TRY(enqueue_front(s, j.nimg, s.host_results ? s.h_tbl : s.d_tbl));
    if (s.host_results) {
        HIPCHK(hipEventRecord(s.ev[3], s.st));   // the tables are in host memory when k_compact is done
    } else {   // the DMA that takes the blocks to the host runs on the side stream
        HIPCHK(hipStreamWaitEvent(s.st_copy, s.ev_c, 0));
        if (!copy_kernel) HIPCHK(hipMemcpyAsync(s.h_tbl, s.d_tbl, (size_t)j.nimg * s.tbl_ints_per_image * sizeof(int), hipMemcpyDeviceToHost, s.st_copy));
        else launch_copy_to_host(s.st_copy, s.d_tbl, s.h_tbl, (size_t)j.nimg * s.tbl_ints_per_image * sizeof(int));
        HIPCHK(hipEventRecord(s.ev[3], s.st_copy));
        if (blur_planes) launch_blur(s.st, s.d_pyr, s.d_blur, geom, j.nimg);
    }
    HIPCHK(hipEventRecord(s.ev[4], s.st));
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
    ev_elapsed(&a, s.ev[0], s.ev[2]);
    if (blur0) ev_elapsed(&b, blur0, s.ev[4]);
    ev_elapsed(&c, s.ev[5], s.ev[6]);
    s.timing[0] = a * 1000.f;
    s.timing[2] = (b + c) * 1000.f;
    s.timing[8] = b * 1000.f;   // k_blur
    s.timing[9] = c * 1000.f;   // k_describe
    ev_elapsed(&t, s.ev[0], s.ev[1]); s.timing[4] = t * 1000.f;   // pyramid launches
    ev_elapsed(&t, s.ev[1], s.ev[2]); s.timing[5] = t * 1000.f;   // k_fast_cells
    ev_elapsed(&t, s.ev[2], s.ev_c); s.timing[6] = t * 1000.f;   // k_compact (the table DMA behind it is not included)
}

int Rig::run_select_and_describe(Slot &s, const Job &j, bool then_match)
{
    HIPCHK(wait_event(s.ev[3]));
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
        uint32_t *sel = s.h_sel + (size_t)m * geom.kcap;
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
        s.h_nsel[m] = total;
    }, pool_threads + s.index);
    if (bad.load() == 3) { set_error("internal: quad-tree went below the bucketing without the candidate list"); (void)hipStreamSynchronize(s.st); return MCORB_E_STATE; }
    if (bad.load() == 1) { set_error("selection failed: level too tall"); (void)hipStreamSynchronize(s.st); return MCORB_E_SIZE; }
    if (bad.load()) { set_error("keypoint capacity exceeded"); (void)hipStreamSynchronize(s.st); return MCORB_E_CAP; }
    const auto t1 = std::chrono::steady_clock::now();
    s.timing[1] = std::chrono::duration<float, std::micro>(t1 - t0).count();
    LatProf::mark(3);

    s.nimg_done = nimg;
    if (then_match) TRY(prepare_match(s, j));
    TRY(enqueue_back(s, j, then_match, false));
    HIPCHK(hipEventRecord(s.ev[10], s.st));
    LatProf::mark(4);
    HIPCHK(wait_event(s.ev[10]));   // (events, not stream synchronisation: wait_event waits the way the rig's wait_mode says)
    if (!s.host_results) HIPCHK(wait_event(s.ev[11]));
    LatProf::mark(5);
    if (params.orientation)
        for (int m = 0; m < nimg; m++)
            for (size_t k = 0; k < s.kps[m].size(); k++) s.kps[m][k].angle = s.h_angles[(size_t)m * geom.kcap + k];
    read_timing(s, s.host_results ? nullptr : s.ev_c);
    return MCORB_OK;
}

// From ev[5] to the last operation the job enqueues: descriptors, then -- a small batch -- k_undistort forked onto the side stream
// beside them and the matcher, joined in front of the BoW stages, no copies; or -- a large batch -- the result copies on the side
// stream while the BoW stages and the matcher run.  ev[11] closes the side stream's work (a GPU-selected small batch's: the compute
// stream's; the host-selected small batch has none and records nothing).
int Rig::enqueue_back(Slot &s, const Job &j, bool then_match, bool gpu_sel)
{
    const int nimg = j.nimg;
    const bool small = s.host_results, ev_on = s.ev_on();
    // selected on the host: one H2D copy of the control block -- counts, pair list, packed selected keypoints
    if (!gpu_sel && !small) HIPCHK(hipMemcpyAsync(s.d_ctrl, s.h_ctrl, s.ctrl_bytes, hipMemcpyHostToDevice, s.st));
    if (ev_on) HIPCHK(hipEventRecord(s.ev[5], s.st));
    if (small && undist_on) {   // fork: into host-mapped memory (ev_u0, not ev[5]: a captured job records no ev[5])
        HIPCHK(hipEventRecord(s.ubuf.ev_u0, s.st));
        HIPCHK(hipStreamWaitEvent(s.st_dma, s.ubuf.ev_u0, 0));
        TRY(enqueue_undistort(s, nimg));
    }
    launch_describe(s.st, s.d_pyr, blur_planes ? s.d_blur : nullptr, geom, s.ctl.sel, s.ctl.nsel, params.orientation, s.d_desc, s.d_angles, nimg,
                    small ? s.h_desc : nullptr);
    if (ev_on) HIPCHK(hipEventRecord(s.ev[6], s.st));
    if (small) {
        if (then_match) TRY(enqueue_match(s, j, true));
        HIPCHK(hipGetLastError());
        if (undist_on) HIPCHK(hipStreamWaitEvent(s.st, s.ubuf.ev_u1, 0));   // join
        if (s.bow_job) TRY(enqueue_bow(s, nimg));
        if (gpu_sel && ev_on) HIPCHK(hipEventRecord(s.ev[11], s.st));
        return MCORB_OK;
    }
    // results to the host on the side stream (DMA) while the matcher already runs: descriptors; of a GPU-selected job also the
    // control block from nsel on (nsel, the set map and pair list as uploaded, sel) and responses + monoIndex + flags.
    // (The descriptor copy starts beside k_expand.  Whatever kernel of the job ENDS while the copy's host writes are in flight is
    // held until they have drained -- k_expand 12 -> 148 us beside the copy, k_knn2 154 -> 276 us when the copy starts behind
    // k_expand, with the runtime's blit and with k_copy_to_host alike (profiles/r03_copy_kernel_ab.txt) -- so the copy stays beside
    // k_expand, whose result nobody needs before k_knn2 anyway: 13.3 k vs 13.0 k frames/s at one slot.)
    const size_t nk = (size_t)nimg * geom.kcap;
    HIPCHK(hipStreamWaitEvent(s.st_dma, s.ev[6], 0));
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
    HIPCHK(hipEventRecord(s.ev[11], s.st_dma));
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
    launch_assemble(s.st, s.d_selval, s.d_selcnt, geom, tab.scale, j.lap0, j.lap1, s.d_sel, s.d_res + s.res_resp_off, s.d_nsel,
                    reinterpret_cast<int *>(s.d_res + s.res_mono_off), d_flags, nimg, small ? s.h_sel : nullptr,
                    small ? s.h_res + s.res_resp_off : nullptr, small ? s.h_sig : nullptr);
    if (ev_on) HIPCHK(hipEventRecord(s.ev_s, s.st));
    if (ev_on) HIPCHK(hipEventRecord(s.ev[3], s.st));
    if (blur_planes) launch_blur(s.st, s.d_pyr, s.d_blur, geom, nimg);
    if (ev_on) HIPCHK(hipEventRecord(s.ev[4], s.st));
    return enqueue_back(s, j, then_match, true);
}


// ---------------------------------------------------------------------------
// UndistortKeyPoints (MultiCameraFrame.cpp:300-347) inside the job.  Nothing of this runs, is allocated or is captured while no
// camera has undistortion set (undist_on): such a job is exactly the job without the feature.
// ---------------------------------------------------------------------------
// on the side stream, behind whatever the caller ordered it after; small batches write the host-mapped points directly and record
// ev_u1 for the caller's join, the others copy them back behind the kernel
int Rig::enqueue_undistort(Slot &s, int nimg)
{
    const bool host_out = s.host_results;
    launch_undistort(s.st_dma, s.ctl.sel, s.ctl.nsel, geom.kcap, nimg, ncams, d_undist_cams, tab.scale, tab.nlevels, host_out ? s.ubuf.h_undist : s.ubuf.d_undist);
    if (host_out || s.bow_job) HIPCHK(hipEventRecord(s.ubuf.ev_u1, s.st_dma));   // (a bound job's BoW tables read the points: enqueue_bow)
    if (!host_out) HIPCHK(hipMemcpyAsync(s.ubuf.h_undist, s.ubuf.d_undist, (size_t)nimg * geom.kcap * sizeof(float2), hipMemcpyDeviceToHost, s.st_dma));
    return MCORB_OK;
}

int Rig::lock_idle_slots(const char *who, std::vector<std::unique_lock<std::mutex>> &locks)
{
    for (auto &sp : slots) {
        locks.emplace_back(sp->m);
        if (sp->busy || sp->submitted) { set_error(std::string(who) + ": a submitted job has not been waited for"); return MCORB_E_STATE; }
    }
    return MCORB_OK;
}

int UndistBufs::alloc(size_t npoints)
{
    TRY(d_undist.alloc(npoints));
    TRY(h_undist.alloc(npoints, kHostMapped));
    TRY(ev_u0.create(hipEventDisableTiming));
    TRY(ev_u1.create(hipEventDisableTiming));
    bound = true;
    return MCORB_OK;
}

int Rig::set_undistortion(int cam, const double *K, const double *dist, int ncoeffs)
{
    if (cam < 0 || cam >= ncams) { set_error("set_undistortion: camera out of range"); return MCORB_E_ARG; }
    const bool clear = !dist || ncoeffs == 0;
    UndistCam c = {};
    if (!clear) {
        if (!K) { set_error("set_undistortion: no camera matrix"); return MCORB_E_ARG; }
        if (undist_prepare(K, dist, ncoeffs, c) != 0) { set_error("set_undistortion: 4, 5, 8 or 12 coefficients (the tilt model is not supported)"); return MCORB_E_ARG; }
        for (double f : {K[0], K[4], c.K[0], c.K[4]})
            if (!std::isfinite(f) || f == 0.) { set_error("set_undistortion: fx / fy must be finite and non-zero"); return MCORB_E_ARG; }
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    TRY(lock_idle_slots("set_undistortion", locks));
    if (imgud_on) {   // RECTIFY: image_kps_undist is the raw keypoint set (MultiCameraFrame.cpp:241-242)
        set_error("set_undistortion: image undistortion is set (mcorb_rig_set_image_undistortion); a rig is rectified or it is not");
        return MCORB_E_STATE;
    }
    HIPCHK(hipSetDevice(device));
    if (!clear && !slots[0]->ubuf.bound) {   // first set call: the device table and every slot's buffers and events
        DevBuf<UndistCam> cams;
        std::vector<UndistBufs> fresh(slots.size());
        TRY(cams.alloc((size_t)ncams));
        for (UndistBufs &b : fresh) TRY(b.alloc((size_t)max_images * geom.kcap));
        d_undist_cams = std::move(cams);   // all there: commit (nothing below fails before every slot has its bundle)
        for (size_t i = 0; i < slots.size(); i++) {
            slots[i]->ubuf = std::move(fresh[i]);
            slots[i]->kps_undist.assign(max_images, {});
            slots[i]->kps_undist_ok.assign(max_images, 0);
        }
    }
    undist_cams[cam] = c;
    undist_set[cam] = clear ? 0 : 1;
    undist_on = std::any_of(undist_set.begin(), undist_set.end(), [](uint8_t v) { return v != 0; });
    if (d_undist_cams) HIPCHK(hipMemcpy(d_undist_cams, undist_cams.data(), (size_t)ncams * sizeof(UndistCam), hipMemcpyHostToDevice));
    undist_gen++;
    return MCORB_OK;
}

// ---------------------------------------------------------------------------
// cv::undistort at the hand-off (the RECTIFY branch of setData, MultiCameraFrame.cpp:123-136).  It belongs to the upload, as it
// belongs to setData: a job, its captured graph and a re-run on resident inputs read level 0 and never know.  Nothing of this
// runs or is allocated while no camera has it set (imgud_on): an upload is then exactly the upload without the feature.
// ---------------------------------------------------------------------------
int Rig::enqueue_remap(Slot &s, int nimg)
{
    launch_remap_u8(s.st, s.d_raw, s.d_pyr, geom, d_remap_cams, ncams, nimg);
    HIPCHK(hipGetLastError());
    return MCORB_OK;
}

int Rig::set_image_undistortion(int cam, const double *K, const double *dist, int ncoeffs)
{
    if (cam < 0 || cam >= ncams) { set_error("set_image_undistortion: camera out of range"); return MCORB_E_ARG; }
    const bool clear = !dist || ncoeffs == 0;
    UndistImageCam c = {};
    if (!clear) {
        if (!K) { set_error("set_image_undistortion: no camera matrix"); return MCORB_E_ARG; }
        if (undist_image_prepare(K, dist, ncoeffs, c) != 0) { set_error("set_image_undistortion: 4, 5, 8 or 12 coefficients (the tilt model is not supported)"); return MCORB_E_ARG; }
        for (double v : c.K) if (!std::isfinite(v)) { set_error("set_image_undistortion: non-finite camera matrix"); return MCORB_E_ARG; }
        for (double v : c.k) if (!std::isfinite(v)) { set_error("set_image_undistortion: non-finite coefficient"); return MCORB_E_ARG; }
        if (c.K[0] == 0. || c.K[4] == 0.) { set_error("set_image_undistortion: fx / fy must be non-zero"); return MCORB_E_ARG; }
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    TRY(lock_idle_slots("set_image_undistortion", locks));
    if (undist_on) {   // the reference's RECTIFY is rig-wide and excludes UndistortKeyPoints (MultiCameraFrame.cpp:241-242)
        set_error("set_image_undistortion: keypoint undistortion is set (mcorb_rig_set_undistortion); a rig is rectified or it is not");
        return MCORB_E_STATE;
    }
    HIPCHK(hipSetDevice(device));
    for (auto &sp : slots) HIPCHK(hipStreamSynchronize(sp->st));   // an earlier upload's k_remap_u8 reads the tables changed below
    const size_t plane = (size_t)W * H, mp = remap_map_pitch(W);
    if (!clear) {
        if (!d_remap_cams) {   // first set call: the camera table and every slot's raw planes
            DevBuf<RemapCam> cams;
            std::vector<DevBuf<uint8_t>> fresh(slots.size());
            TRY(cams.alloc((size_t)ncams));
            for (auto &b : fresh) {
                TRY(b.alloc((size_t)max_images * plane));
                HIPCHK(hipMemset(b, 0, (size_t)max_images * plane));
            }
            d_remap_cams = std::move(cams);
            for (size_t i = 0; i < slots.size(); i++) slots[i]->d_raw = std::move(fresh[i]);
        }
        // the camera's maps: built here, once (the row loop is a serial sum), padded for the device
        std::vector<int16_t> m1(plane * 2);
        std::vector<uint16_t> m2(plane);
        undist_image_map(c, W, H, m1.data(), m2.data());
        std::vector<int16_t> p1((size_t)H * mp * 2, 0);
        std::vector<uint16_t> p2((size_t)H * mp, 0);
        for (int y = 0; y < H; y++) {
            memcpy(p1.data() + (size_t)y * mp * 2, m1.data() + (size_t)y * W * 2, (size_t)W * 4);
            memcpy(p2.data() + (size_t)y * mp, m2.data() + (size_t)y * W, (size_t)W * 2);
        }
        DevBuf<int16_t> d1;
        DevBuf<uint16_t> d2;
        TRY(d1.alloc(p1.size()));
        TRY(d2.alloc(p2.size()));
        HIPCHK(hipMemcpy(d1, p1.data(), p1.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d2, p2.data(), p2.size() * 2, hipMemcpyHostToDevice));
        d_imgud_map1[cam] = std::move(d1);   // all there: commit
        d_imgud_map2[cam] = std::move(d2);
        imgud_map1[cam] = std::move(m1);
        imgud_map2[cam] = std::move(m2);
    } else {
        d_imgud_map1[cam].reset();
        d_imgud_map2[cam].reset();
        imgud_map1[cam] = {};
        imgud_map2[cam] = {};
    }
    imgud_cams[cam] = c;
    imgud_set[cam] = clear ? 0 : 1;
    imgud_on = std::any_of(imgud_set.begin(), imgud_set.end(), [](uint8_t v) { return v != 0; });
    if (d_remap_cams) {
        std::vector<RemapCam> t((size_t)ncams);
        for (int i = 0; i < ncams; i++) t[i] = RemapCam{d_imgud_map1[i].get(), d_imgud_map2[i].get(), imgud_set[i] ? 1 : 0, 0};
        HIPCHK(hipMemcpy(d_remap_cams, t.data(), t.size() * sizeof(RemapCam), hipMemcpyHostToDevice));
    }
    return MCORB_OK;
}

// ---------------------------------------------------------------------------
// transform() (MultiCameraFrame.cpp:257) and computeIntraMatches(matches, words_) (:586-943) inside the job.  Nothing of this runs,
// is allocated or is captured while no vocabulary is bound (bow_bind.flags == 0): such a job is exactly the job without the feature.
// ---------------------------------------------------------------------------
int Rig::check_job_shape(const Job &j) const
{
    if ((j.kind == Job::EXTRACT || j.kind == Job::PROCESS) && (bow_bind.flags & MCORB_BOW_MATCH) && j.nimg % ncams != 0) {
        set_error("extract: a vocabulary bound with MCORB_BOW_MATCH needs whole rig frames (nimg a multiple of the camera count)");
        return MCORB_E_ARG;
    }
    return MCORB_OK;
}

int Rig::enqueue_bow(Slot &s, int nimg)
{
    const BowBinding &b = bow_bind;
    const uint32_t *sel = s.ctl.sel;
    const int *nsel = s.ctl.nsel;
    const bool host_out = s.host_results;
    const int kcap = geom.kcap, nframes = nimg / ncams;
    const bool match = (s.bow_job & MCORB_BOW_MATCH) && npp > 0 && nframes > 0;
    launch_bow_descend(s.st, s.d_desc, nimg * kcap, b.child_start, b.child_count, b.child_desc, b.child_id, b.word_id, b.weight,
                       b.L - b.levelsup, s.bbuf.d_bowres);
    launch_bow_fold(s.st, s.bbuf.d_bowres, nsel, kcap, nimg, b.weighting, b.scoring, s.bbuf.d_bowrec, host_out ? s.bbuf.h_bowrec : nullptr);
    if (match) {
        // the rows of the |dy| < 50 gate: the job's own undistorted points when undistortion is set (k_undistort on the side stream)
        if (undist_on && !host_out) HIPCHK(hipStreamWaitEvent(s.st, s.ubuf.ev_u1, 0));   // (small batches joined it already)
        launch_bow_tables(s.st, s.bbuf.d_bowrec, kcap, ncams, nframes, nsel, sel, tab.scale, tab.nlevels,
                          undist_on ? (host_out ? s.ubuf.h_undist : s.ubuf.d_undist) : nullptr, s.bbuf.d_bslot, s.bbuf.d_bnfeats, s.bbuf.d_bnfeat, s.bbuf.d_brgbase,
                          s.bbuf.d_byv, s.bbuf.d_brange);
        launch_bow_best2(s.st, s.d_desc, 0, kcap, ncams, nframes, s.bbuf.d_byv, s.bbuf.d_bslot, s.bbuf.d_brange, s.bbuf.d_brgbase, s.bbuf.d_bnfeats, s.bbuf.d_bnfeat,
                         host_out ? s.bbuf.h_btab : s.bbuf.d_btab);
    }
    HIPCHK(hipGetLastError());
    if (host_out) return MCORB_OK;
    HIPCHK(hipEventRecord(s.bbuf.ev_b, s.st));
    HIPCHK(hipStreamWaitEvent(s.st_dma, s.bbuf.ev_b, 0));
    HIPCHK(hipMemcpyAsync(s.bbuf.h_bowrec, s.bbuf.d_bowrec, (size_t)nimg * bow_rec_ints(kcap) * sizeof(int), hipMemcpyDeviceToHost, s.st_dma));
    if (match)
        HIPCHK(hipMemcpyAsync(s.bbuf.h_btab, s.bbuf.d_btab, (size_t)nframes * npp * kcap * sizeof(int4), hipMemcpyDeviceToHost, s.st_dma));
    return MCORB_OK;
}

int BowBufs::alloc(const Rig &R)
{
    const size_t M = (size_t)R.max_images, kc = (size_t)R.geom.kcap, F = (size_t)R.max_frames;
    const size_t tab_n = std::max<size_t>((size_t)std::max(R.npp, 1) * F * kc, 1);
    TRY(d_bowres.alloc(M * kc));
    TRY(d_bowrec.alloc(M * bow_rec_ints(R.geom.kcap)));
    TRY(h_bowrec.alloc(M * bow_rec_ints(R.geom.kcap), kHostMapped));
    TRY(d_bslot.alloc(M * kc));
    TRY(d_bnfeats.alloc(M * kc));
    TRY(d_bnfeat.alloc(M));
    TRY(d_brgbase.alloc(F + 1));
    TRY(d_byv.alloc(M * kc));
    TRY(d_brange.alloc(M * kc * (size_t)R.ncams));
    TRY(d_btab.alloc(tab_n));
    TRY(h_btab.alloc(tab_n, kHostMapped));
    TRY(ev_b.create(hipEventDisableTiming));
    bound = true;
    return MCORB_OK;
}

int Rig::set_vocabulary(const BowBinding &b)
{
    if (b.flags && geom.kcap > kBowFoldMaxKcap) {
        set_error("set_vocabulary: the rig's keypoint capacity (kcap " + std::to_string(geom.kcap) + ") exceeds MCORB_BOW_MAX_KCAP (" +
                  std::to_string(kBowFoldMaxKcap) + ")");
        return MCORB_E_ARG;
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    TRY(lock_idle_slots("set_vocabulary", locks));
    HIPCHK(hipSetDevice(device));
    if (b.flags && !slots.empty() && !slots[0]->bbuf.bound) {   // first bind: every slot's buffers
        std::vector<BowBufs> fresh(slots.size());
        for (BowBufs &f : fresh) TRY(f.alloc(*this));
        for (size_t i = 0; i < slots.size(); i++) slots[i]->bbuf = std::move(fresh[i]);   // all there: commit
    }
    bow_bind = b.flags ? b : BowBinding{};
    bow_gen++;
    return MCORB_OK;
}

int LfBufs::alloc(size_t n)
{
    TRY(h_lftrk.alloc(n, hipHostMallocDefault));
    TRY(d_lftrk.alloc(n));
    TRY(h_lfview.alloc(n, hipHostMallocDefault));
    TRY(d_lfview.alloc(n));
    TRY(h_lfout.alloc(n, kHostMapped));
    TRY(h_lfres.alloc(n, hipHostMallocDefault));
    TRY(ev_lf.create(hipEventDisableTiming));
    bound = true;
    return MCORB_OK;
}

// obtainLfFeatures inside the job (lf_job_finish).  Nothing of it runs, is allocated or is captured while no cameras are bound.
int Rig::set_lf(const mcorb_camera *cams, int total_feats)
{
    if (cams && total_feats < 0) { set_error("set_lf: total_feats must be >= 0"); return MCORB_E_ARG; }
    std::vector<std::unique_lock<std::mutex>> locks;
    TRY(lock_idle_slots("set_lf", locks));
    HIPCHK(hipSetDevice(device));
    if (cams && !slots[0]->lbuf.bound) {   // first bind: the camera table and every slot's buffers, sized for one track per keypoint
        DevBuf<LfCam> table;
        std::vector<LfBufs> fresh(slots.size());
        TRY(table.alloc(MCORB_MAX_CAMS));
        for (LfBufs &f : fresh) TRY(f.alloc((size_t)max_images * geom.kcap));
        d_lfcams = std::move(table);   // all there: commit
        for (size_t i = 0; i < slots.size(); i++) slots[i]->lbuf = std::move(fresh[i]);
    }
    if (cams) {
        std::vector<LfCam> dc((size_t)ncams);
        for (int c = 0; c < ncams; c++) {
            memcpy(dc[c].K, cams[c].K, sizeof(dc[c].K));
            memcpy(dc[c].Rt, cams[c].Rt, sizeof(dc[c].Rt));
        }
        HIPCHK(hipMemcpy(d_lfcams, dc.data(), dc.size() * sizeof(LfCam), hipMemcpyHostToDevice));
        lf_cams.assign(cams, cams + ncams);
        lf_total_feats = total_feats;
    } else {
        lf_cams.clear();
    }
    lf_on = cams != nullptr;
    lf_gen++;
    return MCORB_OK;
}

int Rig::undist_records(Slot &s, int m0, int n, std::vector<const mcorb_keypoint *> &out)
{
    if (m0 < 0 || n < 0 || m0 + n > s.nimg_done) { set_error("undistorted keypoints: image index out of range"); return MCORB_E_ARG; }
    if (s.undist_gen != undist_gen) { set_error("undistorted keypoints: image not extracted since the last mcorb_rig_set_undistortion"); return MCORB_E_STATE; }
    std::lock_guard<std::mutex> lk(s.undist_m);
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const int m = m0 + i;
        if (!s.undist_job) { out[i] = s.kps[m].data(); continue; }
        if (!s.kps_undist_ok[m]) {   // the keypoint records with pt replaced (:336-344)
            std::vector<mcorb_keypoint> &U = s.kps_undist[m];
            U = s.kps[m];
            const float2 *p = s.ubuf.h_undist + (size_t)m * geom.kcap;
            for (size_t k = 0; k < U.size(); k++) { U[k].x = p[k].x; U[k].y = p[k].y; }
            s.kps_undist_ok[m] = 1;
        }
        out[i] = s.kps_undist[m].data();
    }
    return MCORB_OK;
}

int Rig::undist_default(Slot &s, int m0, int n, std::vector<const mcorb_keypoint *> &out)
{
    if (!undist_on) return 0;
    const int st = undist_records(s, m0, n, out);
    return st == MCORB_OK ? 1 : st;
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
        const int n = s.h_nsel[m];
        std::vector<mcorb_keypoint> &K = s.kps[m];
        K.resize((size_t)n);
        const uint32_t *sel = s.h_sel + (size_t)m * geom.kcap;
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
        s.h_nsel[m] = n;
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
            const uint32_t *sel = s.h_sel + (size_t)m * geom.kcap;
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
            hipError_t e = s.host_results ? hipSuccess : hipStreamWaitEvent(s.st, s.ev[11], 0);   // the side stream joins again
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
    HIPCHK(hipEventRecord(s.ev[10], s.st));
    LatProf::mark(1); LatProf::mark(2); LatProf::mark(3);
    if (s.host_results) records_early(s.ev[10]);
    LatProf::mark(4);
    HIPCHK(wait_event(s.ev[10]));
    if (!graphed) HIPCHK(wait_event(s.ev[11]));   // (the replayed graph joins the side stream itself)
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
        s.stale_reads += early_stale;
    }
    const int flags = s.host_results ? small_flags : reinterpret_cast<const int *>(s.h_res.get())[0];
    if (flags) {
        // the host stage on the same tables (bit 0: a tree below the bucketing depth; bit 1: more than kcap keypoints -- the host
        // stage reports that error itself)
        s.fallbacks++;
        s.graph_timing = false;
        s.host_results = false;   // (the host stage uploads the whole control block and copies its results back)
        s.set_ctl(false, false);
        HIPCHK(hipMemcpyAsync(s.h_tbl, s.d_tbl, (size_t)nimg * s.tbl_ints_per_image * sizeof(int), hipMemcpyDeviceToHost, s.st_copy));
        HIPCHK(hipEventRecord(s.ev[3], s.st_copy));
        return run_select_and_describe(s, j, then_match);
    }
    if (records_done < nimg) pool->parallel_for(nimg, [&](int m, int) { records(m); }, pool_threads + s.index);
    if (then_match && !j.ext_desc)
        for (size_t i = 0; i < s.match_counts.size(); i++) s.match_counts[i] = s.h_nsel[s.match_sets[i]];
    s.graph_timing = graphed;
    if (graphed) {   // one interval: the whole job
        float a = 0;
        for (float &v : s.timing) v = 0.f;
        ev_elapsed(&a, s.ev_g, s.ev[10]);
        s.timing[0] = a * 1000.f;
        return MCORB_OK;
    }
    read_timing(s, s.ev[3]);
    float t = 0;
    ev_elapsed(&t, s.ev_c, s.ev_s); s.timing[1] = t * 1000.f;   // k_select + k_assemble
    return MCORB_OK;
}

// fills the host side of the control block for a match: per-(frame,cam) sets/counts and the pair list
int Rig::prepare_match(Slot &s, const Job &j)
{
    const bool ext = j.ext_desc != nullptr;
    if (j.ext_pairs) {
        // explicit (query set, train set) pairs of an external block: local set i = the i-th distinct set the list names
        if (!ext || j.ext_npairs < 1 || j.ext_npairs > max_pairs() || j.ext_total < 1 || j.ext_total > ext_cap || (!j.ext_counts && !j.ext_counts_dev)) {
            set_error("match pairs: bad external block or pair count (at most " + std::to_string(max_pairs()) + " pairs per job)");
            return MCORB_E_ARG;
        }
        s.match_external = true;
        s.match_sets.clear();
        s.match_counts.clear();
        std::vector<int> local(j.ext_total, -1);
        if (j.ext_counts)
            for (int i = 0; i < j.ext_total; i++) s.h_extcounts[i] = std::min(std::max(j.ext_counts[i], 0), geom.kcap);
        for (int p = 0; p < j.ext_npairs; p++) {
            int lp[2];
            for (int k = 0; k < 2; k++) {
                const int set = j.ext_pairs[2 * p + k];
                if (set < 0 || set >= j.ext_total) { set_error("match pairs: set index out of range"); return MCORB_E_ARG; }
                if (local[set] < 0) {
                    if ((int)s.match_sets.size() >= max_images) { set_error("match pairs: more than " + std::to_string(max_images) + " distinct sets in one job"); return MCORB_E_ARG; }
                    local[set] = (int)s.match_sets.size();
                    s.h_setmap[local[set]] = set;
                    s.match_sets.push_back(set);
                    s.match_counts.push_back(j.ext_counts ? s.h_extcounts[set] : 0);
                }
                lp[k] = local[set];
            }
            s.h_pairs[p] = int2{lp[0], lp[1]};
        }
        s.nsets_local = (int)s.match_sets.size();
        s.npairs_done = j.ext_npairs;
        s.nframes_done = 0;
        return MCORB_OK;
    }
    if (j.nframes < 1 || j.nframes > max_frames || (!ext && j.nframes * ncams > s.nimg_done)) {
        set_error("match: bad frame count or features not extracted");
        return MCORB_E_STATE;
    }
    const int C = ncams;
    s.match_external = ext;
    s.match_sets.resize((size_t)j.nframes * C);
    s.match_counts.resize((size_t)j.nframes * C);
    if (ext) {
        if (j.ext_total < 1 || j.ext_total > ext_cap || (!j.ext_counts && !j.ext_counts_dev) || !j.ext_sets) {
            set_error("match: bad external block (at most " + std::to_string(ext_cap) + " sets = max(4096, 64 x images per slot))");
            return MCORB_E_ARG;
        }
        if (j.ext_counts)
            for (int i = 0; i < j.ext_total; i++) s.h_extcounts[i] = std::min(std::max(j.ext_counts[i], 0), geom.kcap);
        for (int i = 0; i < j.nframes * C; i++) {
            const int set = j.ext_sets[i];
            if (set < 0 || set >= j.ext_total) { set_error("match: set index out of range"); return MCORB_E_ARG; }
            s.match_sets[i] = set;
            s.match_counts[i] = j.ext_counts ? s.h_extcounts[set] : 0;   // device-resident counts arrive with the job (finish_match)
        }
    } else {
        for (int i = 0; i < j.nframes * C; i++) { s.match_sets[i] = i; s.match_counts[i] = s.h_nsel[i]; }
    }
    s.nframes_done = j.nframes;
    s.nsets_local = j.nframes * C;
    // the k-NN works on LOCAL set indices (frame * cameras + camera): k_expand gathers set setmap[i] into local slot i
    for (int i = 0; i < j.nframes * C; i++) s.h_setmap[i] = s.match_sets[i];
    int p = 0;
    for (int f = 0; f < j.nframes; f++)
        for (int a = 0; a < C - 1; a++)
            for (int b = a + 1; b < C; b++) s.h_pairs[p++] = int2{f * C + a, f * C + b};
    s.npairs_done = p;
    return MCORB_OK;
}

int Rig::enqueue_match(Slot &s, const Job &j, bool ctrl_on_device)
{
    if (!ctrl_on_device) {
        TRY(prepare_match(s, j));
        HIPCHK(hipMemcpyAsync(s.d_ctrl, s.h_ctrl, s.ctrl_pairs_end, hipMemcpyHostToDevice, s.st));
        s.set_ctl(false, false);
    }
    if (j.after_stream)   // the block is being produced on another stream (a collective): order this stream behind what the
        HIPCHK(hipStreamWaitEvent(s.st, s.ev_x, 0));   // caller had enqueued there at submit time (ev_x, recorded by the submit call)
    if (j.ext_counts_dev) {
        HIPCHK(hipMemcpyAsync(s.d_extcounts, j.ext_counts_dev, (size_t)j.ext_total * sizeof(int), hipMemcpyDeviceToDevice, s.st));
        HIPCHK(hipMemcpyAsync(s.h_extcounts, j.ext_counts_dev, (size_t)j.ext_total * sizeof(int), hipMemcpyDeviceToHost, s.st));
    }
    if (s.npairs_done == 0) return MCORB_OK;
    const bool ext = j.ext_desc != nullptr;
    const bool ev_on = s.ev_on();
    if (ev_on) HIPCHK(hipEventRecord(s.ev[7], s.st));
    launch_knn2(s.st, ext ? (const uint8_t *)j.ext_desc : s.d_desc, ext ? s.d_extcounts : s.ctl.nsel, s.ctl.setmap, s.nsets_local, s.ctl.pairs,
                s.npairs_done, geom.kcap, s.d_exp, s.d_lcounts, s.d_part, j.dist_thresh, j.ratio, s.d_knn, s.h_mlist,
                s.h_mcount, ev_on ? s.ev_e : nullptr, ev_on ? s.ev[8] : nullptr);
    if (ev_on) HIPCHK(hipEventRecord(s.ev[9], s.st));
    HIPCHK(hipGetLastError());
    return MCORB_OK;
}

// The epipolar check of computeIntraMatches(matches, old=true) (MultiCameraFrame.cpp:1178-1207): line in
// image i = F^T * kp2, normalised, squared point-line distance against 3.84 * sigma2[octave].  The mixed
// float/double arithmetic follows the reference's declared types statement by statement.
static bool epipolar_ok(const double *F, const mcorb_keypoint &k1, const mcorb_keypoint &k2, const float *sigma2)
{
    float a = (float)((double)k2.x * F[0] + (double)k2.y * F[3] + F[6]);
    float b = (float)((double)k2.x * F[1] + (double)k2.y * F[4] + F[7]);
    float c = (float)((double)k2.x * F[2] + (double)k2.y * F[5] + F[8]);
    float den = a * a + b * b;
    den = den ? (float)(1. / (double)std::sqrt(den)) : (float)1.;
    a *= den; b *= den; c *= den;
    den = a * a + b * b;
    const float num = a * k1.x + b * k1.y + c;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    const float check_thresh = (float)(3.84 * (double)sigma2[k1.octave]);
    return dsqr < check_thresh;
}

// computeIntraMatches' track merge over the BruteForceMatch lists of one frame
// (MultiCameraFrame.cpp:1167-1268); gate != nullptr adds the old=true epipolar check.
void merge_pair_lists(int C, const int *counts, const uint32_t *const *idx1, const uint32_t *const *idx2, const int *np,
                             const EpipolarGate *gate, std::vector<int32_t> &tr, int &mergeable_out)
{
    tr.clear();
    int ntr = 0, mergeable = 0;
    // keypoint -> track, one flat table for all cameras (per thread: this runs once per rig frame, on pool threads)
    static thread_local std::vector<int> inv_flat;
    int *inv[MCORB_MAX_CAMS];
    {
        size_t total = 0, worst = 0;
        for (int c = 0; c < C; c++) total += (size_t)std::max(counts[c], 0);
        inv_flat.assign(total, -1);
        size_t o = 0;
        for (int c = 0; c < C; c++) { inv[c] = inv_flat.data() + o; o += (size_t)std::max(counts[c], 0); }
        for (int p = 0; p < C * (C - 1) / 2; p++) worst += (size_t)std::max(np[p], 0);
        tr.resize(worst * C);   // a track per accepted match at most; cut to the tracks made at the end
    }
    int32_t *T = tr.data();
    int pl = 0;
    for (int a = 0; a < C - 1; a++) {
        for (int b = a + 1; b < C; b++, pl++) {
            const uint32_t *i1 = idx1[pl], *i2 = idx2[pl];
            for (int k = 0; k < np[pl]; k++) {
                const int fa = (int)i1[k], fb = (int)i2[k];
                const int ma = inv[a][fa], mb = inv[b][fb];
                if (gate && !epipolar_ok(gate->F + 9 * pl, gate->kps[a][fa], gate->kps[b][fb], gate->sigma2)) continue;
                if (ma == -1 && mb == -1) {
                    int32_t *row = T + (size_t)ntr * C;
                    for (int c = 0; c < C; c++) row[c] = -1;
                    row[a] = fa;
                    row[b] = fb;
                    inv[a][fa] = ntr;
                    inv[b][fb] = ntr;
                    ntr++;
                } else {
                    if (ma == -1 && mb != -1) {
                        if (T[(size_t)mb * C + a] == -1) {
                            T[(size_t)mb * C + a] = fa;
                            inv[a][fa] = mb;
                        }
                    }
                    if (ma != -1 && mb != -1) {
                        if (ma != mb) mergeable++;
                    }
                    if (ma != -1 && mb == -1) {
                        T[(size_t)ma * C + b] = fb;
                        inv[b][fb] = ma;
                    }
                }
            }
        }
    }
    tr.resize((size_t)ntr * C);
    mergeable_out = mergeable;
}

void Rig::merge_tracks(Slot &s, int f, const EpipolarGate *gate, std::vector<int32_t> &tr, int &mergeable_out) const
{
    const int C = ncams;
    const uint32_t *i1[MCORB_MAX_CAMS * MCORB_MAX_CAMS], *i2[MCORB_MAX_CAMS * MCORB_MAX_CAMS];
    int np[MCORB_MAX_CAMS * MCORB_MAX_CAMS];
    for (int p = 0; p < npp; p++) {
        i1[p] = s.m_idx1[f * npp + p].data();
        i2[p] = s.m_idx2[f * npp + p].data();
        np[p] = (int)s.m_idx1[f * npp + p].size();
    }
    merge_pair_lists(C, &s.match_counts[(size_t)f * C], i1, i2, np, gate, tr, mergeable_out);
}

// BruteForceMatch's output lists (MultiCameraFrame.cpp:1060-1078) + the track merge, host side,
// after the k-NN tables landed.
int Rig::finish_match(Slot &s, const Job &j)
{
    HostProf::Scope prof(2);
    if (j.ext_counts_dev)   // the counts came over with the job's own stream; the k-NN kernels clamped them the same way
        for (size_t i = 0; i < s.match_sets.size(); i++)
            s.match_counts[i] = std::min(std::max(s.h_extcounts[s.match_sets[i]], 0), geom.kcap);
    (void)ncams;
    auto filter_pair = [&](int pi, int) {   // BruteForceMatch's accept loop for one camera pair (pair index within the job)
        // k_knn2_finalize already compacted the accepted pairs in query order: unpack query << 16 | train
        std::vector<uint32_t> &i1 = s.m_idx1[pi], &i2 = s.m_idx2[pi];
        const int nqb = knn_qblocks(geom.kcap);
        const int *cnt = s.h_mcount + (size_t)pi * nqb;
        const uint32_t *ml = s.h_mlist + (size_t)pi * knn_mlist_stride(geom.kcap);
        int n = 0;
        for (int b = 0; b < nqb; b++) n += cnt[b];
        i1.resize(n); i2.resize(n);
        int k = 0;
        for (int b = 0; b < nqb; b++)
            for (int e = 0; e < cnt[b]; e++, k++) { i1[k] = ml[b * kKnnQueriesPerBlock + e] >> 16; i2[k] = ml[b * kKnnQueriesPerBlock + e] & 0xffffu; }
    };
    auto one_frame = [&](int f, int w) {
        // the accept lists were written by the GPU into pinned host memory: every line is a miss, and the lists are short runs
        // (one per 256 queries) that the hardware prefetcher does not get ahead of -- ask for all of a frame's lines at once
        {
            const int nqb = knn_qblocks(geom.kcap);
            for (int pi = f * npp; pi < (f + 1) * npp; pi++) {
                const int *cnt = s.h_mcount + (size_t)pi * nqb;
                const uint32_t *ml = s.h_mlist + (size_t)pi * knn_mlist_stride(geom.kcap);
                for (int b = 0; b < nqb; b++) {
                    const char *p0 = reinterpret_cast<const char *>(ml + (size_t)b * kKnnQueriesPerBlock);
                    const int bytes = std::min(std::max(cnt[b], 0), kKnnQueriesPerBlock) * 4;
                    for (int o = 0; o < bytes; o += 64) __builtin_prefetch(p0 + o, 0, 0);
                }
            }
        }
        for (int pi = f * npp; pi < (f + 1) * npp; pi++) filter_pair(pi, w);
        LatProf::mark(9);
        merge_tracks(s, f, nullptr, s.tracks[f], s.mergeable[f]);
        LatProf::mark(10);
    };
    // frames are independent (own pair lists, own track table): one pool task each
    if (j.ext_pairs) pool->parallel_for(s.npairs_done, filter_pair, pool_threads + s.index);   // explicit pairs: lists only, the merge is the caller's
    else if (s.nframes_done > 1) pool->parallel_for(s.nframes_done, one_frame, pool_threads + s.index);
    else if (s.nframes_done == 1) one_frame(0, 0);   // (spreading one frame's pairs over the pool was slower: wake-ups)
    if (s.npairs_done > 0 && !s.graph_timing) {
        float m = 0;
        ev_elapsed(&m, s.ev[7], s.ev[9]); s.timing[3] = m * 1000.f;
        ev_elapsed(&m, s.ev_e, s.ev[8]); s.timing[7] = m * 1000.f;   // k_knn2 (k_expand in front of it: timing[3] - [7] - finalize)
    }
    return MCORB_OK;
}

}  // namespace mcorb
