// mcorb_engine.h -- host orchestration of the gfx950 ORB front-end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mcorb.h"
#include "mcorb_common.h"
#include "mcorb_hip.h"
#include "mcorb_kernels.h"
#include "mcorb_select.h"

namespace mcorb {

const char *get_error();

// ORBextractor constructor tables (ORBextractor.cpp:408-468)
struct Tables {
    int nlevels = 0;
    float scale[kMaxLevels], inv_scale[kMaxLevels], sigma2[kMaxLevels], inv_sigma2[kMaxLevels];
    int quota[kMaxLevels];
    int scaled_patch[kMaxLevels];
    int umax[16];
};
int compute_tables(const mcorb_params &p, Tables &t);

// cv::resize's per-axis tables, folded into ResizeTap entries
void build_resize_axis(int ssize, int dsize, bool is_x, std::vector<ResizeTap> &out, int pad_to);

// level / cell / tile geometry for W x H; returns MCORB_OK or MCORB_E_SIZE
// lut (optional): receives the path-code tables of all levels (LevelGeom::lutx / luty index into it)
int build_geometry(const mcorb_params &p, const Tables &t, int W, int H, Geom &g, std::vector<ResizeTap> &taps,
                   std::vector<uint16_t> *lut = nullptr);
// LDS source window of one resize workgroup (256 x kResizeTileH outputs): per level, win[2 * l] = the widest column span (pitch) and
// win[2 * l + 1] = the tallest row span of its taps; MCORB_E_ARG where a window does not fit the LDS
int resize_windows(const Geom &g, const std::vector<ResizeTap> &taps, int win[2 * kMaxLevels]);

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
constexpr unsigned kHostMapped = hipHostMallocMapped | hipHostMallocPortable;   // pinned memory that kernels access
constexpr int kSmallBatch = 8;   // images: at most two 4-camera rig frames
int usable_cores();   // cores this process can use: affinity mask, cgroup quota, ranks per node (mcorb_pool.cpp)

class WorkerPool {
public:
    explicit WorkerPool(int nthreads);
    ~WorkerPool();
    // runs fn(task, worker_index) for task in [0, n); returns when all are done
    // caller_widx >= 0: the calling thread takes tasks as well, using that worker index
    void parallel_for(int n, const std::function<void(int, int)> &fn, int caller_widx = -1);
    int size() const { return (int)threads_.size(); }

private:
    struct Batch {
        const std::function<void(int, int)> *fn;
        std::atomic<int> next{0};
        int n = 0;
        std::atomic<int> done{0};
        std::atomic<int> refs{0};
        std::mutex m;
        std::condition_variable cv;
    };
    void run(int widx);
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<Batch *> queue_;
    std::atomic<int> pending_{0};   // batches in queue_ (lets idle workers spin without the lock)
    bool stop_ = false;
};

struct Job {
    enum Kind { NONE, EXTRACT, MATCH, PROCESS } kind = NONE;
    int nimg = 0, nframes = 0, lap0 = 0, lap1 = 0;
    float dist_thresh = 75.f, ratio = 0.85f;
    // external descriptor block (RCCL path): ext_total sets of [kcap][32] bytes on the device,
    // ext_counts[set] descriptors each; ext_sets[f*ncams + c] = set holding camera c of frame f
    const void *ext_desc = nullptr;
    const int32_t *ext_counts = nullptr;
    int ext_total = 0;
    const int32_t *ext_sets = nullptr;
    // device-resident form (no host synchronisation between the collective and the match): the counts live in device
    // memory, and the slot's stream first waits for everything enqueued so far on `after_stream` (the collective)
    const int32_t *ext_counts_dev = nullptr;
    hipStream_t after_stream = nullptr;
    // explicit pair list instead of "all camera pairs of nframes frames" (the pair-partitioned multi-GPU path: pair (i, j) of a
    // frame is matched on one rank): ext_npairs pairs of (query set, train set) indices into the external block; no
    // track merge on this rank (nframes = 0), the per-pair lists are read with mcorb_rig_get_pairlist
    const int32_t *ext_pairs = nullptr;
    int ext_npairs = 0;
};

class Rig;

// mcorb_rig_last_timing's ten floats (us), in the public order of include/mcorb.h: pyramid + FAST + compaction (a graphed job: the
// whole job) | selection | blur + describe | k-NN + finalize | pyramid | k_fast_cells | k_compact | k_knn2 | k_blur | k_describe
enum Timing { T_FRONT, T_SELECT, T_DESC, T_MATCH, T_PYR, T_FAST, T_COMPACT, T_KNN2, T_BLUR, T_DESCRIBE, T_COUNT };

// computeIntraMatches' track merge (MultiCameraFrame.cpp:1167-1268) over the BruteForceMatch lists of one frame's camera pairs
// in (0,1), (0,2), .., (1,2), .. order: counts[c] keypoints per camera, idx1[p] / idx2[p] the accepted (query, train) indices of
// pair p (np[p] of them).  gate != nullptr adds the old=true epipolar check.  Shared by the engine and mcorb_host_merge_tracks.
struct EpipolarGate;
void merge_pair_lists(int ncams, const int *counts, const uint32_t *const *idx1, const uint32_t *const *idx2, const int *np,
                      const EpipolarGate *gate, std::vector<int32_t> &tr, int &mergeable_out);

// computeIntraMatches(matches, words_) of one frame (mcorb_rig_match_bow_frames): tracks (ncams ints each), their n_rays, words_
struct BowFrameOut {
    std::vector<int32_t> tracks, n_rays;
    std::vector<uint32_t> words;
};

// transform() of one image (mcorb_rig_transform_images): BowVector as sorted (word id, value) lists, FeatureVector as
// node ids + offsets into the feature list
struct BowImageOut {
    std::vector<uint32_t> bow_ids, fv_nodes;
    std::vector<double> bow_vals;
    std::vector<int32_t> fv_offsets, fv_feats;
};

// obtainLfFeatures of one frame (mcorb_rig_obtain_lf_features, and the job's stage of mcorb_rig_set_lf): the features in output
// order, words_fil, intramatch_size / mono_size; src: per feature, the slot-local keypoint its descriptor is (image * kcap + k);
// bow: the LF set's transform() (FrontEnd.cpp:525), filled by the job's stage only
struct LfFrameOut {
    std::vector<mcorb_lf_feature> feats;
    std::vector<uint32_t> words_fil;
    std::vector<int32_t> src;
    int intramatch_size = 0, mono_size = 0;
    BowImageOut bow;
};

// UndistortKeyPoints (mcorb_rig_set_undistortion): k_undistort's points of the images in the slot, [image][kcap] (d_ device, h_
// host-mapped pinned); a fork / join pair of events for small batches, whose kernel runs beside the descriptors and the matcher on
// the side stream.  Like the two bundles below: allocated whole for every slot at the rig's first set call and only then moved
// into the slots (`bound`), never while the feature is unused.
struct UndistBufs {
    Event ev_u0, ev_u1;
    DevBuf<float2> d_undist;
    HostBuf<float2> h_undist;
    bool bound = false;
    int alloc(size_t npoints);
};

// transform() / computeIntraMatches(matches, words_) inside the job (mcorb_rig_set_vocabulary): descent results, k_bow_fold's
// per-image records (d_ device, h_ host-mapped pinned), k_bow_best2's index tables and its best / second-best table (d_ device, h_
// host-mapped pinned); ev_b: the BoW kernels are done (the copies of a large batch follow it on st_dma)
struct BowBufs {
    Event ev_b;
    DevBuf<BowRes> d_bowres;
    DevBuf<int> d_bowrec, d_bslot, d_bnfeats, d_bnfeat, d_brgbase;
    HostBuf<int> h_bowrec;
    DevBuf<float> d_byv;
    DevBuf<int2> d_brange;
    DevBuf<int4> d_btab;
    HostBuf<int4> h_btab;
    bool bound = false;
    int alloc(const Rig &R);
};

// obtainLfFeatures inside the job (mcorb_rig_set_lf): k_lf_tracks' tracks and views (h_ pinned, staged for one H2D copy; d_
// device), its per-track records (host-mapped pinned, written by the kernel), the job's descent results (pinned copy of d_bowres:
// the LF set's transform reads them); tracks and views are grown by a job that needs more (lf_job_finish); ev_lf: the stage's
// kernel and copies are done
struct LfBufs {
    Event ev_lf;
    HostBuf<int4> h_lftrk;
    DevBuf<int4> d_lftrk;
    HostBuf<LfView> h_lfview;
    DevBuf<LfView> d_lfview;
    HostBuf<LfTrackOut> h_lfout;
    HostBuf<BowRes> h_lfres;
    bool bound = false;
    int alloc(size_t n);
};

// Members are destroyed in reverse order of declaration: the three bundles and the buffers go first, then the events, the streams
// last.  Rig::~Rig has joined the driver thread, synchronised the streams and destroyed the graph exec before that.
struct Slot {
    Rig *rig = nullptr;
    int index = 0;
    bool blur_valid = false;   // d_blur holds the blurred planes of the images in d_pyr
    Stream st, st_copy, st_dma;   // compute; PCIe-bound compaction kernel; D2H copies only
    Event ev_x;   // cross-stream hand-offs with the caller's streams (export / external match)
    Event ev_c;   // k_compact finished (the table DMA follows it on the side stream)
    Event ev_e;   // k_expand finished (k_knn2 follows)
    // what has finished when each is reached, in job order: nothing yet | pyramid | FAST | the tables are with whoever selects (and
    // the selection itself, on the GPU) | blur | control block in place, describe starts | describe | k-NN starts | k_knn2 | finalize |
    // the compute stream's last operation | the side stream's.  A thread waits on ev_tables, ev_done and ev_side only.
    Event ev_start, ev_pyr, ev_fast, ev_tables, ev_blur, ev_desc0, ev_desc1, ev_knn0, ev_knn1, ev_fin, ev_done, ev_side;
    Event ev_s;   // k_select + k_assemble finished
    Event ev_g;   // in front of a replayed job graph
    // device
    DevBuf<uint8_t> d_pyr, d_blur, d_desc;
    DevBuf<uint32_t> d_cellkp, d_sorted;
    DevBuf<int> d_cellcnt;
    DevBuf<float> d_angles, d_f32;   // (d_f32: upload_f32's staging, grown on first use)
    DevBuf<uint2> d_part;
    DevBuf<uint8_t> d_exp;           // descriptors of the sets being matched, expanded to +-64 int8 in MFMA fragment order (k_expand)
    DevBuf<int> d_lcounts;           // their clamped counts, local set order
    DevBuf<uint8_t> d_raw;           // raw planes of a rig with image undistortion set (image m at m * W * H); empty otherwise
    // host, device-mapped (kernels write/read these directly over PCIe)
    HostBuf<uint32_t> h_cand;
    HostBuf<int> h_overflow;
    // k_compact's per-image table blocks (level offsets, shipped flags, bucket starts, bucket winners; layout in
    // mcorb_common.h): written to d_tbl by the kernel, brought to the pinned h_tbl by one DMA per batch
    DevBuf<int> d_tbl;
    HostBuf<int> h_tbl;
    int tbl_ints_per_image = 0;
    const int *tbl(int img) const { return h_tbl + (size_t)img * tbl_ints_per_image; }
    volatile uint32_t touch_sink[16] = {};
    DevBuf<KnnRow> d_knn;            // k-NN rows per pair (device; read back only by mcorb_rig_get_pair_knn2)
    HostBuf<uint32_t> h_mlist;       // per pair: accepted (query << 16 | train), query order (k_knn2_finalize)
    HostBuf<int> h_mcount;
    // control block: one pinned host buffer + one device mirror, copied with a single
    // hipMemcpyAsync: [extcounts ext_cap ints][nsel][setmap][pairs][sel]; hc / dc: the host and the device side of that layout
    HostBuf<uint8_t> h_ctrl;
    DevBuf<uint8_t> d_ctrl;
    size_t ctrl_pairs_end = 0, ctrl_bytes = 0;
    struct CtrlView {
        int *extcounts, *nsel, *setmap;
        int2 *pairs;
        uint32_t *sel;
    } hc = {}, dc = {};
    // GPU selection (MCORB_SELECT_GPU): k_select's per-(image, level) lists, and the result block k_assemble fills for the host
    // ([16 ints of flags][mono M ints][responses M x kcap bytes]; sel / nsel are written into the control block)
    DevBuf<uint32_t> d_selval;
    DevBuf<int> d_selcnt;
    DevBuf<uint8_t> d_res;
    HostBuf<uint8_t> h_res;
    size_t res_bytes = 0, res_mono_off = 0, res_resp_off = 0, ctrl_nsel_off = 0;
    HostBuf<unsigned long long> h_sig;        // small GPU-selected jobs: per image, set by k_assemble behind its host-mapped results
    bool capturing = false;    // enqueue_gpu_job is being captured into the slot's graph
    std::atomic<int> stale_reads{0};   // small batches: images whose early read did not match the signal word's checksum (redone after the end event)
    std::atomic<int> fallbacks{0};     // jobs of this slot the host stage had to redo (a tree below the bucketing depth)
    // (lf / lf_gen: mcorb_rig_set_lf's binding and set calls -- the LF stage runs after the graph, the key keeps it in view;
    // bow_*: the vocabulary binding the job was captured with -- its tables and levelsup are kernel arguments; bow_gen counts
    // mcorb_rig_set_vocabulary calls, so a freed vocabulary whose address comes back never replays a stale graph.  4-byte fields
    // only: the key is compared with memcmp)
    struct GraphKey { int nimg, match, nframes, lap0, lap1; float dist_thresh, ratio; int undist, bow_flags, bow_levelsup; unsigned bow_gen; int lf; unsigned lf_gen; };
    hipGraphExec_t graph_exec = nullptr;   // the captured job (run_gpu_selected), valid for graph_key
    GraphKey graph_key = {};
    unsigned job_counter = 0;
    bool graph_timing = false;             // the last job ran as a graph: timing[] holds the whole job only
    // host, pinned
    HostBuf<uint8_t> h_stage, h_desc;
    HostBuf<float> h_angles;
    // results
    std::vector<std::vector<mcorb_keypoint>> kps;   // per image
    std::vector<int> mono;
    std::vector<std::vector<uint32_t>> sel_val;     // per (image, level): retained candidates (packed), result order
    int npairs_done = 0, nframes_done = 0, nimg_done = 0;
    int nsets_local = 0;   // descriptor sets the last match expanded (frames x cameras, or the distinct sets of an explicit pair list)
    std::vector<std::vector<uint32_t>> m_idx1, m_idx2;   // per pair
    std::vector<std::vector<int32_t>> tracks;            // per frame, ncams ints per track
    std::vector<int> mergeable;
    // cached BoW results of the images the slot holds NOW: a new extraction clears the flags (begin_extract), the
    // getters refuse frames / images that were not matched / transformed since
    std::vector<BowFrameOut> bow;   // per frame
    std::vector<uint8_t> bow_ok;    // per frame: bow[f] belongs to the current extraction
    std::vector<BowImageOut> bowvec;   // per image
    std::vector<uint8_t> bowvec_ok;
    void invalidate_bow()
    {
        std::fill(bow_ok.begin(), bow_ok.end(), (uint8_t)0);
        std::fill(bowvec_ok.begin(), bowvec_ok.end(), (uint8_t)0);
        std::fill(lf_ok.begin(), lf_ok.end(), (uint8_t)0);
    }
    std::vector<LfFrameOut> lf;     // per frame: the job's obtainLfFeatures + LF transform (mcorb_rig_set_lf)
    std::vector<uint8_t> lf_ok;
    float timing[T_COUNT] = {};
    bool undist_job = false;      // the images in the slot were extracted with k_undistort (some camera had undistortion set)
    unsigned undist_gen = 0;      // Rig::undist_gen when they were extracted
    bool submitted = false;       // a job was submitted and not yet waited for (mcorb_rig_set_undistortion refuses then)
    int bow_job = 0;              // MCORB_BOW_* flags the images in the slot were extracted with (0: no BoW stage ran)
    bool lf_job = false;          // the job ran the LF stage (LF bound and the vocabulary bound with MCORB_BOW_MATCH)
    // image_kps_undist of the images, built on first read from kps and h_undist (Rig::undist_records)
    std::vector<std::vector<mcorb_keypoint>> kps_undist;
    std::vector<uint8_t> kps_undist_ok;
    std::mutex undist_m;
    std::vector<int> match_sets, match_counts;   // per (frame, cam) of the last match: set index, descriptor count
    bool match_external = false;
    // the running job is a small batch: its results (and, selected on the host, its tables and control block) go through host-mapped
    // memory, no copies; cleared when the host stage redoes a GPU-selected job.  Implies orientation == 0 and no blurred planes.
    bool host_results = false;
    // (a small batch replayed from its graph: kernels only -- event-record nodes between them split the graph into separately
    // submitted pieces, and nothing reads these events after a replay)
    bool ev_on() const { return !(host_results && capturing); }
    // the control block as the job's kernels read it, chosen once per job (begin_extract; the fallback redo and a MATCH job read
    // the device mirror): the host-mapped side where no upload is made -- set map and pair list / the host's sel and nsel
    struct Ctrl {
        const int *nsel, *setmap;
        const int2 *pairs;
        const uint32_t *sel;
    } ctl = {};
    void set_ctl(bool host_lists, bool host_sel)
    {
        const CtrlView &sel = host_sel ? hc : dc, &lists = host_lists ? hc : dc;
        ctl = {sel.nsel, lists.setmap, lists.pairs, sel.sel};
    }
    // driver thread
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    Job job;
    bool busy = false, quit = false, inline_job = false;
    int status = MCORB_OK;
    std::string err;
    // the lazily bound bundles (last: released first)
    UndistBufs ubuf;
    BowBufs bbuf;
    LfBufs lbuf;
};

// inputs of the old=true epipolar check: F per camera pair (i<j, row-major 3x3, x_j^T F x_i = 0), the
// per-camera keypoints the reference reads (image_kps_undist) and the extractor's sigma2 table
struct EpipolarGate {
    const double *F;
    const mcorb_keypoint *const *kps;
    const float *sigma2;
};

class Rig {
public:
    Rig() = default;
    ~Rig();
    int init(const mcorb_params &p, int ncams, int W, int H, int max_frames, int nslots);

    int upload_u8(int slot, const uint8_t *const *images, int nimg, int stride);
    int upload_staged(int slot, int nimg);
    int upload_f32(int slot, const float *const *images, int nimg, int stride_bytes, int channels);
    int submit(int slot, const Job &job);
    int run_sync(int slot, const Job &job);   // submit + wait on the calling thread
    int wait(int slot);

    mcorb_params params;
    Tables tab;
    Geom geom;
    int ncams = 0, W = 0, H = 0, max_frames = 0, max_images = 0, npp = 0 /* pairs per frame */;
    int ext_cap = 0;   // descriptor sets an external block may hold (mcorb_rig_match_external*)
    int device = 0;
    DevBuf<ResizeTap> d_taps;
    DevBuf<uint16_t> d_lut;                // path-code tables of all levels (k_compact)
    DevBuf<uint32_t> d_fasttab;            // k_fast_cells' per-cell records (fast_cell_table)
    int fast_cell_off = 0;                  // dword offset of the records inside d_fasttab
    SelectParams selp[kMaxLevels];         // per-level DistributeOctTree constants + bucketing depth
    int resize_win[2 * kMaxLevels] = {};   // per level: LDS window pitch, rows (see launch_pyramid)
    std::vector<std::unique_ptr<Slot>> slots;
    std::unique_ptr<WorkerPool> pool;
    int pool_threads = 0;
    // admission to the GPU (mcorb_params.gpu_jobs): with more slots than jobs the GPU runs well side by side, the extra slots are
    // the ones whose results the host is post-processing -- the GPU does not wait for the host, and is not oversubscribed either
    int gpu_job_limit = 0;     // 0 = none
    int gpu_jobs_running = 0;
    std::mutex gpu_jobs_m;
    std::condition_variable gpu_jobs_cv;
    void gpu_job_begin();
    void gpu_job_end();
    bool upload_pipelined = true;   // upload_u8 of a small batch: staging copy and DMA overlapped image by image
    std::atomic<int> graph_every{0};   // GPU-selected jobs replayed from a captured HIP graph: 0 never, 1 always, K all but every K-th (mcorb_rig_set_graph)
    int select_deep_cap = 4096; // k_select: largest bucket it scans node by node below the bucketing depth (MCORB_SELECT_DEEP_CAP at rig creation)
    bool compact_one_copy = false;   // k_compact with one table copy in LDS even where four fit (MCORB_COMPACT_ONE_COPY at rig creation: test knob)
    bool select_prof = false;        // k_select's phase stamps on stderr (MCORB_SELECT_PROF at rig creation)
    bool gpu_select = false;   // DistributeOctTree's list discipline runs in k_select (MCORB_SELECT_GPU); else on the worker pool
    int wait_mode = 0;         // how a thread waits for a HIP event: 0 spin (hipEventSynchronize), 1 interrupt-driven, 2 poll + short sleeps
    hipError_t wait_event(hipEvent_t ev) const;
    std::vector<std::unique_ptr<SelectScratch>> scratch;   // one per worker

    void merge_tracks(Slot &s, int f, const EpipolarGate *gate, std::vector<int32_t> &tr, int &mergeable_out) const;

    // UndistortKeyPoints (MultiCameraFrame.cpp:300-347) on the device, inside the job: per camera the host's table (mode 0 for
    // cameras not set), its device copy k_undistort reads (graph replays included), and which cameras are set at all
    std::vector<UndistCam> undist_cams;
    std::vector<uint8_t> undist_set;
    DevBuf<UndistCam> d_undist_cams;   // (allocated with the slots' UndistBufs)
    bool undist_on = false;     // some camera is set: jobs run k_undistort; otherwise a job is exactly what it is without the feature
    unsigned undist_gen = 0;    // set calls so far (images extracted before the last one have no undistorted set)
    int set_undistortion(int cam, const double *K, const double *dist, int ncoeffs);
    // the slot's image_kps_undist of images [m0, m0 + n): MCORB_E_STATE for images not extracted since the last set call; the
    // records are the raw ones when the job ran with nothing set
    int undist_records(Slot &s, int m0, int n, std::vector<const mcorb_keypoint *> &out);
    // the set a consumer reads when the caller passes none: 0 = nothing set (the raw keypoints, as before), 1 = `out` holds the
    // rig's own set, < 0 = error (images extracted before the last set call)
    int undist_default(Slot &s, int m0, int n, std::vector<const mcorb_keypoint *> &out);
    int max_pairs() const { return std::max(1, npp * max_frames); }

    // The RECTIFY branch of setData (MultiCameraFrame.cpp:123-136): cv::undistort of every camera image at the hand-off.  Per
    // camera the calibration and the maps built from it on the host (mcorb_undistort_image.h) with their device copies, allocated
    // when the camera is set; d_remap_cams: what k_remap_u8 reads (mode 0 for cameras not set).  While imgud_on, every upload
    // form lands its planes in the slot's d_raw and enqueues k_remap_u8 behind the copies; a job never sees the difference.
    // Nothing of this is allocated or runs on a rig that never sets it.
    std::vector<UndistImageCam> imgud_cams;
    std::vector<uint8_t> imgud_set;
    std::vector<std::vector<int16_t>> imgud_map1;    // [cam][H * W * 2], unpadded rows (mcorb_rig_get_undistort_map)
    std::vector<std::vector<uint16_t>> imgud_map2;   // [cam][H * W]
    std::vector<DevBuf<int16_t>> d_imgud_map1;       // [cam][H * remap_map_pitch(W) * 2]
    std::vector<DevBuf<uint16_t>> d_imgud_map2;
    DevBuf<RemapCam> d_remap_cams;
    bool imgud_on = false;
    int set_image_undistortion(int cam, const double *K, const double *dist, int ncoeffs);
    int enqueue_remap(Slot &s, int nimg);   // k_remap_u8 on the slot's stream, behind the upload's copies

    // the vocabulary bound to the rig (mcorb_rig_set_vocabulary): flags = 0 unbound; otherwise the vocabulary's device tables,
    // levelsup and weighting / scoring, which every extraction job's BoW stages read; bow_gen counts the set calls
    struct BowBinding {
        int flags = 0, levelsup = 0, L = 0, weighting = 0, scoring = 0;
        double ratio = 0.85;
        const int *child_start = nullptr, *child_count = nullptr, *child_id = nullptr, *word_id = nullptr;
        const void *child_desc = nullptr;
        const double *weight = nullptr;
    };
    BowBinding bow_bind;
    unsigned bow_gen = 0;
    // obtainLfFeatures inside the job (mcorb_rig_set_lf): the cameras (host copy and the device copy k_lf_tracks reads) and
    // total_feats; lf_gen counts the set calls
    bool lf_on = false;
    int lf_total_feats = 3000;
    std::vector<mcorb_camera> lf_cams;
    DevBuf<LfCam> d_lfcams;            // (allocated with the slots' LfBufs)
    unsigned lf_gen = 0;
    int set_lf(const mcorb_camera *cams, int total_feats);
    int set_vocabulary(const BowBinding &b);
    int check_job_shape(const Job &j) const;   // a bound MCORB_BOW_MATCH needs whole frames
    // what the three set_* calls start with: no job of any slot may be in flight, or be waiting to be waited for -- every slot is
    // locked (the caller keeps `locks` until its tables are in place), MCORB_E_STATE with `who` in the message otherwise
    int lock_idle_slots(const char *who, std::vector<std::unique_lock<std::mutex>> &locks);

private:
    bool copy_kernel = false;  // D2H of tables / descriptors by k_copy_to_host instead of hipMemcpyAsync (see Rig::init)
    bool blur_planes = false;  // k_blur runs with every job (orientation mode / MCORB_BLUR_PLANES); otherwise blur is fused into k_describe_fused
    void driver(Slot *s);
    int execute(Slot &s, const Job &j);
    // The stages every extraction job is assembled from.  begin_extract: what a job does before its first launch (argument check,
    // the bindings' snapshot, small batch or not, the control block view).  enqueue_front: ev_start . pyramid . ev_pyr . FAST . ev_fast .
    // k_compact . ev_c on the compute stream, the tables into tbl.  enqueue_back: from ev_desc0 to the job's last enqueued operation;
    // gpu_sel: k_assemble left sel / nsel on the device (else the host filled the control block).
    int begin_extract(Slot &s, const Job &j);
    int enqueue_front(Slot &s, int nimg, int *tbl);
    // the slot's table blocks to the pinned h_tbl on st_copy and ev_tables behind them; by_kernel: k_copy_to_host, not the runtime's copy
    int enqueue_tables_to_host(Slot &s, int nimg, bool by_kernel);
    int enqueue_back(Slot &s, const Job &j, bool then_match, bool gpu_sel);
    void read_timing(Slot &s, hipEvent_t blur0);   // per-kernel times of an ungraphed job; blur0: k_blur's start event (null: none ran)
    mcorb_keypoint make_keypoint(int level, int xl, int yl, float response, float angle) const;
    int run_extract_phaseA(Slot &s, const Job &j);
    int run_select_and_describe(Slot &s, const Job &j, bool then_match);
    int run_gpu_selected(Slot &s, const Job &j, bool then_match);   // the whole job as one submission (gpu_select)
    int enqueue_gpu_job(Slot &s, const Job &j, bool then_match);
    // k_undistort of the job's images on the side stream st_dma; a small batch writes the host-mapped points, the others copy them
    // back behind the kernel
    int enqueue_undistort(Slot &s, int nimg);
    // the BoW stages of the job's nimg images on the compute stream, behind the descriptors (and k_undistort when it gives the rows):
    // a small batch's results go to host-mapped memory; otherwise they are copied on st_dma behind the job's other result copies
    int enqueue_bow(Slot &s, int nimg);
    int prepare_match(Slot &s, const Job &j);
    int enqueue_match(Slot &s, const Job &j, bool ctrl_on_device);
    int finish_match(Slot &s, const Job &j);
};

// k-NN rows as the API hands them out: (idx0, idx1) and (d0, d1) per query
inline void decode_rows(const KnnRow *rows, int nq, int32_t *idx, int32_t *dist)
{
    for (int q = 0; q < nq; q++) {
        const KnnRow &k = rows[q];
        idx[2 * q] = knn_idx0(k);
        dist[2 * q] = knn_d0(k);
        idx[2 * q + 1] = knn_idx1(k);
        dist[2 * q + 1] = knn_d1(k);
    }
}
// the host half of a job's BoW stages (mcorb_bow.cpp): the BowImageOut of every image from k_bow_fold's records and, with
// MCORB_BOW_MATCH, the reference's serial track bookkeeping of every frame on the worker pool
int bow_job_finish(Rig &R, Slot &s, int nimg);
// the job's obtainLfFeatures stage (mcorb_lf.cpp), called by bow_job_finish once the frames' tracks are replayed: k_lf_tracks on
// every track of every frame in one launch, then the order-dependent bookkeeping and the LF transform per frame on the worker pool
int lf_job_finish(Rig &R, Slot &s, int nframes);
// transform()'s BowVector / FeatureVector (mcorb_bow.cpp's assemble) of n descent results, for the given weighting / scoring
void bow_assemble(int weighting, int scoring, const BowRes *res, int n, BowImageOut &o);
// scoring type (DBoW2's enum) and device (-1: a host-only vocabulary) of a vocabulary (mcorb_bow.cpp), for the keyframe database
void vocab_props(const ::mcorb_vocab *v, int &scoring, int &device);
// transform(desc, levelsup)'s descent and assembly for the local map (mcorb_lmap.cpp): desc is n rows in device memory, descended by
// k_bow_descend on st -- or, for a host-only vocabulary, n host rows descended by the same walk on the host.  before: what the
// caller queues in front of the descent (the gather that fills desc), behind the scratch's grows; NOT called for a host-only
// vocabulary or n == 0, where nothing is queued
int vocab_feature_vector(::mcorb_vocab *v, const uint8_t *desc, int n, int levelsup, hipStream_t st, BowImageOut &o, const Pieces &before = nullptr);

}  // namespace mcorb

// the C handle of include/mcorb.h
struct mcorb_rig {
    mcorb::Rig rig;
};
