// mcorb_pool.cpp -- the host worker pool and the count of cores it may draw on.
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>

#include "mcorb_engine.h"

namespace mcorb {

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

// Cores this process can actually use: hardware threads, cut down to the scheduler affinity mask and to the cgroup CPU
// quota (v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us), whichever is smallest.
int usable_cores()
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

}  // namespace mcorb
