// mcorb_hip.h -- the one place where HIP buffers, events and streams are acquired and released: the error macros, four
// move-only owners and the events around the pieces of a submission (Spans).  No shared ownership, no allocator policy: an owner
// holds one handle and its destructor releases it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <functional>
#include <string>
#include <utility>

#include "../../include/mcorb.h"

namespace mcorb {
void set_error(const std::string &msg);
}

#define HIPCHK(x)                                                                      \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            mcorb::set_error(std::string(#x) + ": " + hipGetErrorString(e_));          \
            return MCORB_E_HIP;                                                        \
        }                                                                              \
    } while (0)
#define TRY(x)                         \
    do {                               \
        int r_ = (x);                  \
        if (r_ != MCORB_OK) return r_; \
    } while (0)

namespace mcorb {

// how a call begins on its device: a stale error of this thread is not this call's
static inline int use_device(int device)
{
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    return MCORB_OK;
}

// what the four owners share: handle H (null = empty), released with Release(H); n_ is the element count of a buffer
template <typename H, auto Release>
class Owner {
public:
    Owner() = default;
    Owner(Owner &&o) noexcept { swap(o); }
    Owner &operator=(Owner &&o) noexcept { swap(o); return *this; }   // (o's destructor releases what this held)
    Owner(const Owner &) = delete;
    Owner &operator=(const Owner &) = delete;
    ~Owner() { reset(); }
    void reset()
    {
        if (h_) (void)Release(h_);
        h_ = nullptr;
        n_ = 0;
    }
    operator H() const { return h_; }   // call sites pass the owner where they passed the raw handle
    H get() const { return h_; }        // (where a cast to another pointer type follows)

protected:
    void swap(Owner &o) { std::swap(h_, o.h_); std::swap(n_, o.n_); }
    H h_ = nullptr;
    size_t n_ = 0;
};

// alloc / create: release what is held, then acquire; MCORB_E_HIP through set_error (and an empty owner) on failure.
// grow, for grow-only scratch: nothing when n elements fit already, otherwise alloc -- size() is 0 after a failed one, so the next
// call allocates again.
template <typename T>
class DevBuf : public Owner<T *, hipFree> {
public:
    size_t size() const { return this->n_; }   // elements allocated
    int alloc(size_t n)
    {
        this->reset();
        void *p = nullptr;
        HIPCHK(hipMalloc(&p, n * sizeof(T)));
        this->h_ = (T *)p;
        this->n_ = n;
        return MCORB_OK;
    }
    int grow(size_t n) { return n <= size() ? MCORB_OK : alloc(n); }
};

// pinned host memory; flags: hipHostMallocDefault, or hipHostMallocMapped [| hipHostMallocPortable] where kernels access it
template <typename T>
class HostBuf : public Owner<T *, hipHostFree> {
public:
    size_t size() const { return this->n_; }
    int alloc(size_t n, unsigned flags)
    {
        this->reset();
        void *p = nullptr;
        HIPCHK(hipHostMalloc(&p, n * sizeof(T), flags));
        this->h_ = (T *)p;
        this->n_ = n;
        return MCORB_OK;
    }
    int grow(size_t n, unsigned flags) { return n <= size() ? MCORB_OK : alloc(n, flags); }
};

class Event : public Owner<hipEvent_t, hipEventDestroy> {
public:
    int create(unsigned flags)
    {
        reset();
        HIPCHK(hipEventCreateWithFlags(&h_, flags));
        return MCORB_OK;
    }
};

// Elapsed milliseconds between two events of a finished job; 0 when either was not recorded on a stream (a job that ran from its
// captured graph holds them as graph nodes).  A failed query must not stay behind as the thread's "last error".
static inline void ev_elapsed(float *ms, hipEvent_t a, hipEvent_t b)
{
    if (hipEventElapsedTime(ms, a, b) != hipSuccess) { *ms = 0.f; (void)hipGetLastError(); }
}

// N + 1 events around N consecutive pieces of a submission: Submission::mark(spans, i) records event i, so piece i runs between
// marks i and i + 1.  read(), after the synchronisation: us[i] = the microseconds of piece i by ev_elapsed's rule; the pieces below `from`
// did not run in this submission (their first events were not marked) and read 0
template <int N>
struct Spans {
    Event ev[N + 1];
    float us[N] = {};
    int create()
    {
        for (Event &e : ev) TRY(e.create(hipEventDefault));
        return MCORB_OK;
    }
    void read(int from = 0)
    {
        for (int i = 0; i < N; i++) {
            float ms = 0.f;
            if (i >= from) ev_elapsed(&ms, ev[i], ev[i + 1]);
            us[i] = ms * 1000.f;
        }
    }
};

// A chain of pieces on one stream with one wait.  A piece is a launch (run), a copy, a fill or a mark: run(spans, i, launch)
// marks event i of spans, then launches; run(launch) is a launch between no marks; mark(spans, i) the event behind the last
// piece; copy / fill of 0 bytes queue nothing.  From the first piece on nothing returns before the wait, and after the first
// piece that fails nothing more is queued: later pieces do nothing and their launch is not called, so no kernel runs behind a
// failed upload of its input.  wait() synchronises once if a piece was attempted and reports a failed synchronisation first,
// otherwise the first failed piece by its kind -- so nothing of the chain still reads the call's input (pinned or pageable) or
// writes its host-mapped records when the caller has its error.  failed() reads the state without waiting (the tracking pair
// waits elsewhere when nothing failed).  A Submission without a piece does not synchronise: mcorb_lmap_observe with nothing to
// do, knn2_frames with an empty side and a search without candidates rely on it.  A stale error of the thread is the caller's
// to discard first; buffers are grown before the first piece.
class Submission {
public:
    explicit Submission(hipStream_t stream) : st(stream) {}
    bool failed() const { return err != hipSuccess; }
    template <int N>
    void mark(Spans<N> &spans, int i)
    {
        if (!failed()) note("mark", hipEventRecord(spans.ev[i], st));
    }
    template <class Launch>
    void run(Launch &&launch)
    {
        if (failed()) return;
        launch();
        note("launch", hipGetLastError());
    }
    template <int N, class Launch>
    void run(Spans<N> &spans, int i, Launch &&launch)
    {
        mark(spans, i);
        run(launch);
    }
    void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
    {
        if (bytes && !failed()) note("copy", hipMemcpyAsync(dst, src, bytes, kind, st));
    }
    void fill(void *dst, int value, size_t bytes)
    {
        if (bytes && !failed()) note("fill", hipMemsetAsync(dst, value, bytes, st));
    }
    int wait()
    {
        if (attempted) {
            attempted = false;
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return fail("synchronisation", e);
        }
        return failed() ? fail(piece, err) : MCORB_OK;
    }

private:
    void note(const char *kind, hipError_t e)
    {
        attempted = true;
        if (e == hipSuccess) return;
        err = e;
        piece = kind;
        (void)hipGetLastError();   // (this piece's error is not the next call's)
    }
    static int fail(const char *kind, hipError_t e)
    {
        set_error(std::string("submission: ") + kind + " failed: " + hipGetErrorString(e));
        return MCORB_E_HIP;
    }
    hipStream_t st;
    bool attempted = false;
    hipError_t err = hipSuccess;
    const char *piece = "";
};
// what a caller hands a function that opens the Submission itself, to be queued first: behind the function's grows, in front of
// its own pieces.  It is called only if the function queues anything: each function that takes one says when it does not
using Pieces = std::function<void(Submission &)>;

class Stream : public Owner<hipStream_t, hipStreamDestroy> {
public:
    int create(unsigned flags)
    {
        reset();
        HIPCHK(hipStreamCreateWithFlags(&h_, flags));
        return MCORB_OK;
    }
};

}  // namespace mcorb
