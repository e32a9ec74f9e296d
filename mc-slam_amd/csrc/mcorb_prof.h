// mcorb_prof.h -- the engine's two optional host-side profiles (MCORB_HOST_PROF, MCORB_LAT_PROF); their state is defined here, once.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include <atomic>
#include <chrono>

namespace mcorb {

// MCORB_HOST_PROF=1: wall and thread-CPU time of the selection tasks
namespace HostProf {
inline const bool on = getenv("MCORB_HOST_PROF") != nullptr;
inline std::atomic<long long> wall[4], cpu[4], cnt[4];
inline long long now(clockid_t c) { timespec t; clock_gettime(c, &t); return t.tv_sec * 1000000000LL + t.tv_nsec; }
struct Scope {
    int k; long long w0 = 0, c0 = 0;
    explicit Scope(int k_) : k(k_) { if (on) { w0 = now(CLOCK_MONOTONIC); c0 = now(CLOCK_THREAD_CPUTIME_ID); } }
    ~Scope() { if (on) { wall[k] += now(CLOCK_MONOTONIC) - w0; cpu[k] += now(CLOCK_THREAD_CPUTIME_ID) - c0; cnt[k]++; } }
};
inline void report()
{
    if (!on) return;
    const char *names[4] = {"select task (per image)", "  select_octree x levels", "finish_match (per job)", "prepare_match (per job)"};
    for (int k = 0; k < 4; k++)
        if (cnt[k].load())
            fprintf(stderr, "[mcorb host prof] %-26s n=%lld wall %.1f us cpu %.1f us\n", names[k], cnt[k].load(),
                    wall[k].load() / 1e3 / cnt[k].load(), cpu[k].load() / 1e3 / cnt[k].load());
}
}  // namespace HostProf

// MCORB_LAT_PROF=1: where a synchronous PROCESS job spends its wall time (host clock), printed every 50 jobs
namespace LatProf {
inline const bool on = getenv("MCORB_LAT_PROF") != nullptr;
inline thread_local double t[12];
inline thread_local double acc[12];
inline thread_local int n = 0;
inline void mark(int i) { if (on) t[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline void flush()
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

}  // namespace mcorb
