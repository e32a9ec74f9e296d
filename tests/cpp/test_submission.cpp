// Submission (mc-slam_amd/csrc/mcorb_hip.h) against a scripted HIP runtime: every runtime call a Submission makes is appended to a
// log, and one chosen call answers a chosen error.  No GPU and no HIP library: the declarations are tests/cpp/hipmock's, the
// definitions are below.  Prints "bad=<failed checks>"; tests/test_submission_cpu.py builds and runs it under the sanitizers.
#include <stdio.h>

#include <string>
#include <vector>

#include "mcorb_hip.h"

// ---- the scripted runtime ----
static std::vector<std::string> g_log;   // "mark", "launch", "copy", "fill", "sync", in call order
static int g_fail_at = -1;               // the log position whose call fails (-1: none) ...
static hipError_t g_fail_with = hipSuccess;
static bool g_sync_fails = false;        // ... and the synchronisation, whatever its position
static hipError_t g_last = hipSuccess;   // the thread's "last error"
static std::string g_error;              // what set_error was last handed

void mcorb::set_error(const std::string &msg) { g_error = msg; }

static hipError_t logged(const char *what)
{
    const bool fails = (int)g_log.size() == g_fail_at;
    g_log.push_back(what);
    if (fails) g_last = g_fail_with;
    return fails ? g_fail_with : hipSuccess;
}
// a kernel launch returns nothing: its error is the thread's last error
static void stub_launch() { (void)logged("launch"); }

const char *hipGetErrorString(hipError_t e)
{
    return e == hipSuccess ? "no error" : e == hipErrorInvalidValue ? "invalid argument" : e == hipErrorOutOfMemory ? "out of memory" : "unspecified launch failure";
}
hipError_t hipGetLastError(void) { const hipError_t e = g_last; g_last = hipSuccess; return e; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMalloc(void **, size_t) { return hipErrorOutOfMemory; }
hipError_t hipFree(void *) { return hipSuccess; }
hipError_t hipHostMalloc(void **, size_t, unsigned) { return hipErrorOutOfMemory; }
hipError_t hipHostFree(void *) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *, unsigned) { return hipErrorOutOfMemory; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return logged("mark"); }
hipError_t hipEventElapsedTime(float *, hipEvent_t, hipEvent_t) { return hipErrorInvalidValue; }
hipError_t hipStreamCreateWithFlags(hipStream_t *, unsigned) { return hipErrorOutOfMemory; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t)
{
    g_log.push_back("sync");
    return g_sync_fails ? hipErrorLaunchFailure : hipSuccess;
}
hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t) { return logged("copy"); }
hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return logged("fill"); }

// ---- the checks ----
static int bad = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) { bad++; printf("line %d: %s (%s)\n", __LINE__, #x, ctx.c_str()); } \
    } while (0)

static void script(int fail_at, hipError_t with, bool sync_fails)
{
    g_log.clear();
    g_error.clear();
    g_last = hipSuccess;
    g_fail_at = fail_at;
    g_fail_with = with;
    g_sync_fails = sync_fails;
}

static const char *name_of(char kind) { return kind == 'm' ? "mark" : kind == 'r' ? "launch" : kind == 'c' ? "copy" : "fill"; }

// piece `kind` of a chain: m mark, r run, c copy, f fill
static void piece(mcorb::Submission &sub, mcorb::Spans<1> &spans, char kind, int &launches)
{
    char buf[8];
    if (kind == 'm') sub.mark(spans, 0);
    if (kind == 'r') sub.run([&] { launches++; stub_launch(); });
    if (kind == 'c') sub.copy(buf, buf, sizeof(buf), hipMemcpyHostToDevice);
    if (kind == 'f') sub.fill(buf, 0, sizeof(buf));
}

// a chain of five pieces whose piece k fails (k < 0: none); sync_fails: and so does the synchronisation
static void chain(const std::string &kinds, int k, bool sync_fails)
{
    const std::string ctx = kinds + " k=" + std::to_string(k) + (sync_fails ? " sync fails" : "");
    const hipError_t with = k >= 0 && kinds[k] == 'r' ? hipErrorLaunchFailure : hipErrorInvalidValue;
    script(k, with, sync_fails);
    mcorb::Spans<1> spans;
    mcorb::Submission sub(nullptr);
    int launches = 0, want_launches = 0;
    std::vector<std::string> want;
    for (int i = 0; i < (int)kinds.size(); i++) {
        CHECK(sub.failed() == (k >= 0 && i > k));
        piece(sub, spans, kinds[i], launches);
        if (k < 0 || i <= k) {   // (piece k is attempted; nothing behind it is)
            want.push_back(name_of(kinds[i]));
            if (kinds[i] == 'r') want_launches++;
        }
    }
    CHECK(sub.failed() == (k >= 0));
    CHECK(g_log == want);   // (no synchronisation before the wait)
    CHECK(launches == want_launches);
    const int r = sub.wait();
    want.push_back("sync");
    CHECK(g_log == want);   // (exactly one synchronisation, behind everything)
    CHECK(g_last == hipSuccess);   // (the failed piece's error is not the next call's)
    if (sync_fails) {
        CHECK(r == MCORB_E_HIP && g_error.find("synchronisation") != std::string::npos);
        CHECK(g_error.find(hipGetErrorString(hipErrorLaunchFailure)) != std::string::npos);
    } else if (k >= 0) {
        CHECK(r == MCORB_E_HIP && g_error.find(name_of(kinds[k])) != std::string::npos);
        CHECK(g_error.find(hipGetErrorString(with)) != std::string::npos);
    } else {
        CHECK(r == MCORB_OK && g_error.empty());
    }
    // a second wait has nothing left to wait for and still knows the failure
    g_sync_fails = false;
    CHECK(sub.wait() == (k >= 0 ? MCORB_E_HIP : MCORB_OK));
    CHECK(g_log == want);
}

int main()
{
    // every rotation of mark, run, copy, fill, run: each kind of piece stands at each position once
    std::string kinds = "mrcfr";
    for (int rot = 0; rot < 5; rot++) {
        chain(kinds, -1, false);
        chain(kinds, -1, true);
        for (int k = 0; k < 5; k++) {
            chain(kinds, k, false);
            chain(kinds, k, true);   // (the failed synchronisation comes before the recorded piece)
        }
        kinds = kinds.substr(1) + kinds[0];
    }
    const std::string ctx = "edges";
    {   // run(spans, i, launch) is a mark and a launch: behind a failed mark the launch is not called
        script(0, hipErrorInvalidValue, false);
        mcorb::Spans<1> spans;
        mcorb::Submission sub(nullptr);
        int launches = 0;
        sub.run(spans, 0, [&] { launches++; stub_launch(); });
        CHECK(sub.failed() && launches == 0);
        CHECK(sub.wait() == MCORB_E_HIP && g_error.find("mark") != std::string::npos);
        CHECK((g_log == std::vector<std::string>{"mark", "sync"}));
    }
    {   // pieces of 0 bytes queue nothing, and a Submission without a piece does not synchronise
        script(-1, hipSuccess, false);
        char buf[1];
        mcorb::Submission sub(nullptr);
        sub.copy(buf, buf, 0, hipMemcpyHostToDevice);
        sub.fill(buf, 0, 0);
        CHECK(!sub.failed() && g_log.empty());
        CHECK(sub.wait() == MCORB_OK && g_log.empty() && g_error.empty());
        mcorb::Submission none(nullptr);
        CHECK(none.wait() == MCORB_OK && g_log.empty());
    }
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
