// mcorb_hip.h -- the one place where HIP buffers, events and streams are acquired and released: the error macros, four
// move-only owners and the events around the pieces of a submission (Spans).  No shared ownership, no allocator policy: an owner
// holds one handle and its destructor releases it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

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

// N + 1 events around N consecutive pieces of a submission: mark(st, i) records event i, so piece i runs between marks i and
// i + 1.  read(), after the synchronisation: us[i] = the microseconds of piece i by ev_elapsed's rule; the pieces below `from`
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
    int mark(hipStream_t st, int i) { HIPCHK(hipEventRecord(ev[i], st)); return MCORB_OK; }
    void read(int from = 0)
    {
        for (int i = 0; i < N; i++) {
            float ms = 0.f;
            if (i >= from) ev_elapsed(&ms, ev[i], ev[i + 1]);
            us[i] = ms * 1000.f;
        }
    }
};

// A chain of kernels on one stream with one wait.  run(spans, i, launch): mark event i of spans, then launch; run(launch): a
// piece between no marks; mark(spans, i): the event behind the last piece.  From the first piece on nothing returns before the
// wait: the first failed launch (hipGetLastError after each) and the first failed mark are kept, and wait() reports, in this
// order, a failed synchronisation, the launch, the mark -- so no kernel of the chain still reads the call's pinned input or
// writes its host-mapped records when the caller has its error.  A stale error of the thread is the caller's to discard first.
class Submission {
public:
    explicit Submission(hipStream_t stream) : st(stream) {}
    template <int N>
    void mark(Spans<N> &spans, int i)
    {
        if (marked != MCORB_OK) return;
        marked = spans.mark(st, i);
        if (marked != MCORB_OK) (void)hipGetLastError();   // (the event's error is not the next launch's)
    }
    template <class Launch>
    void run(Launch &&launch)
    {
        launch();
        if (launched == hipSuccess) launched = hipGetLastError();
    }
    template <int N, class Launch>
    void run(Spans<N> &spans, int i, Launch &&launch)
    {
        mark(spans, i);
        run(launch);
    }
    int wait()
    {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(launched);
        return marked;
    }

private:
    hipStream_t st;
    hipError_t launched = hipSuccess;
    int marked = MCORB_OK;
};

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
