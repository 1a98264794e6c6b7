// host_threads.h — the library's host thread helpers: no HIP in here, so the file also builds with a
// plain host compiler and runs under ThreadSanitizer / ASan in tests/host/host_threads_main.cpp.
#pragma once
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

// Pin a thread to `cpus` (empty: leave it wherever the OS puts it).
inline void pin_thread(pthread_t th, const std::vector<int>& cpus) {
    if (cpus.empty()) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    for (int c : cpus) CPU_SET(c, &set);
    (void)pthread_setaffinity_np(th, sizeof(set), &set);
}

// Threads that are joined when the scope ends, however it ends (a throw while a later one starts
// included: a joinable std::thread's destructor would call std::terminate).
struct JoinedThreads {
    std::vector<std::thread> ts;
    void join() {
        for (auto& t : ts)
            if (t.joinable()) t.join();
    }
    ~JoinedThreads() { join(); }
};

// Fixed pool of copy threads: copy() splits one memcpy into page-aligned parts, the calling
// thread takes part 0 and blocks until every part is done.
class CopyPool {
  public:
    // cpus: where the workers run (worker i on cpus[i % size]); empty = wherever the OS puts them.
    // A throw while a worker starts stops and joins the ones already running, then goes on up.
    CopyPool(int nthreads, const std::vector<int>& cpus) {
        try {
            for (int i = 0; i < nthreads; ++i) {
                th_.ts.emplace_back([this, i] { worker(i); });
                if (!cpus.empty()) pin_thread(th_.ts.back().native_handle(), {cpus[i % cpus.size()]});
            }
        } catch (...) {
            shutdown();
            throw;
        }
    }
    ~CopyPool() { shutdown(); }
    void copy(void* dst, const void* src, size_t n) {
        const int parts = (int)th_.ts.size() + 1;
        if (n < (size_t(4) << 20) || parts == 1) {
            memcpy(dst, src, n);
            return;
        }
        {
            std::lock_guard<std::mutex> g(mu_);
            dst_ = (char*)dst;
            src_ = (const char*)src;
            n_ = n;
            parts_ = parts;
            pending_ = parts - 1;
            ++gen_;
        }
        cv_.notify_all();
        run_part(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
    }

  private:
    void shutdown() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    void run_part(int p) {
        const size_t per = ((n_ + parts_ - 1) / parts_ + 4095) & ~size_t(4095);
        const size_t a = std::min(n_, per * p), b = std::min(n_, a + per);
        if (b > a) memcpy(dst_ + a, src_ + a, b - a);
    }
    void worker(int i) {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
            }
            run_part(i + 1);
            std::lock_guard<std::mutex> g(mu_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, done_;
    uint64_t gen_ = 0;
    int pending_ = 0;
    bool stop_ = false;
    char* dst_ = nullptr;
    const char* src_ = nullptr;
    size_t n_ = 0;
    int parts_ = 1;
    JoinedThreads th_;     // last: the workers end before the state they wait on
};
