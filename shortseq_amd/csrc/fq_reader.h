// fq_reader.h — the FASTQ reader ring of ss_ingest_add_fastq_range, host-only (no HIP in here: it
// builds with a plain host compiler and runs under ThreadSanitizer / ASan in
// tests/host/host_threads_main.cpp).
//
// A range [begin, size) of a file is cut into chunks that end right after a newline (the last one at
// the range's end).  A reader thread fills chunk k + 1 into slot (k + 1) & 1 -- the previous chunk's
// tail (the bytes after its last newline: the carry) first, then file reads in pieces, each piece's
// copy to the device queued as soon as it is read -- while the consumer indexes and counts chunk k
// from slot k & 1.  A chunk in which one line fills the whole slot makes the slot grow to twice the
// size (for every later chunk too); the bytes kept are queued once more, as the carry of the retry.
//
// The slots' buffers, the copies and their stream belong to the owner and are reached through
// FqSlotOps; the reader keeps the framing, the hand-off and the thread.  A chunk is never empty: the
// owner returns before it builds a reader for an empty range, and every fill of a nonempty rest
// reads at least one byte or fails, so nothing here tests for n == 0.
#pragma once
#include <unistd.h>

#include <chrono>
#include <string>

#include "../../include/shortseq_amd.h"
#include "host_threads.h"

constexpr uint64_t kFqPiece = 64ull << 20;     // file read / H2D piece
constexpr uint64_t kFqParMin = 32ull << 20;    // a read at least this long is split over threads

inline uint64_t pread_full(int fd, uint8_t* dst, uint64_t len, uint64_t pos) {
    uint64_t got = 0;
    while (got < len) {
        const ssize_t k = pread(fd, dst + got, len - got, (off_t)(pos + got));
        if (k <= 0) break;
        got += (uint64_t)k;
    }
    return got;
}

// [pos, pos + len) of the file into dst over up to `threads` threads (shares aligned to `align`, a
// power of two); the bytes read, short at the file's end.  Whatever threads started are joined on
// every way out.
inline uint64_t read_parallel(int fd, uint8_t* dst, uint64_t len, uint64_t pos, unsigned threads,
                              uint64_t par_min, uint64_t align = 1 << 20) {
    if (len < par_min || threads <= 1) return pread_full(fd, dst, len, pos);
    const uint64_t per = ((len + threads - 1) / threads + align - 1) & ~(align - 1);
    std::vector<uint64_t> got(threads, 0);
    JoinedThreads th;
    for (unsigned t = 0; t < threads; ++t) {
        const uint64_t a = (uint64_t)t * per;
        if (a >= len) break;
        const uint64_t b = std::min(len, a + per);
        th.ts.emplace_back([&got, fd, dst, pos, t, a, b] { got[t] = pread_full(fd, dst + a, b - a, pos + a); });
    }
    th.join();
    uint64_t sum = 0;
    for (uint64_t n : got) sum += n;
    return sum;
}

// What the reader needs from the owner of the two slots.  Every call but last_error returns SS_OK or
// a code whose message last_error() then gives on the same thread.  All calls come from the reader's
// thread (the constructing thread in inline mode).
struct FqSlotOps {
    // once, before anything else on the reader's thread
    virtual void thread_start() = 0;
    // slot i: a host buffer of at least cap bytes (*host) and device room for cap + 16
    virtual int ensure(int i, uint64_t cap, uint8_t** host) = 0;
    // queue the copy of [off, off + len) of slot i to the device: piece number `piece` of this fill
    virtual int queue_copy(int i, uint32_t piece, uint64_t off, uint64_t len) = 0;
    // wait for the queued copies (a grow replaces the host buffer they read)
    virtual int wait_copies() = 0;
    // replace slot i's host buffer by one of cap bytes that keeps the first `keep` bytes (*host)
    virtual int grow(int i, uint64_t cap, uint64_t keep, uint8_t** host) = 0;
    // every piece of slot i's chunk is queued
    virtual int complete(int i) = 0;
    virtual const char* last_error() = 0;

  protected:
    ~FqSlotOps() = default;
};

// a slot's first capacity for chunks of chunk_bytes over a range of `bytes`
inline uint64_t fq_cap0(uint64_t chunk_bytes, uint64_t bytes) {
    return std::max<uint64_t>(16, std::min<uint64_t>(chunk_bytes, bytes + 16));
}

struct FqRange {
    int fd;
    uint64_t begin, size;            // the bytes [begin, size) of the file, begin < size
    uint64_t cap0;                   // a slot's first capacity (>= 16)
    unsigned threads;                // read_parallel's
    double* read_ms = nullptr;       // += the host ms of the file reads
    uint64_t piece = kFqPiece, par_min = kFqParMin;
};

// a filled slot, as the consumer sees it
struct FqChunk {
    uint64_t n = 0, use = 0;         // bytes in the slot, bytes up to its last newline (n at the range's end)
    bool at_eof = false;
    uint32_t np = 0;                 // pieces queued for it
    int rc = SS_OK;
    std::string err;                 // rc's message: the consumer raises it on its own thread
};

class FqReader {
  public:
    // A range that fits one chunk has nothing to overlap: it is filled on this thread, here (no
    // thread start), unless the reader is to run on `cpus` (the caller's affinity is left alone).
    FqReader(FqSlotOps& ops, const FqRange& r, const std::vector<int>& cpus)
        : ops_(ops), r_(r), cpus_(cpus), pos_(r.begin), cap_(r.cap0) {
        if (r.size - r.begin <= r.cap0 && cpus.empty()) {
            run();
            return;
        }
        try {
            th_ = std::thread([this] { run(); });
        } catch (...) {
            publish(0, SS_EHIP, "cannot start the FASTQ reader thread");
        }
    }
    ~FqReader() { stop(); }

    // wait for chunk k (in slot k & 1); it stays the consumer's until release(k)
    const FqChunk& acquire(uint64_t k) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return state_[k & 1] == 1; });
        return slot_[k & 1];
    }
    void release(uint64_t k) { signal(state_[k & 1], 0); }
    // End the reader (after the fill it is in, if any) and join it, whatever the consumer holds.
    void stop() {
        signal(stop_, 1);
        if (th_.joinable()) th_.join();
    }

  private:
    using Clock = std::chrono::steady_clock;

    // one word of the hand-off changed under the lock, both sides woken
    void signal(int& word, int v) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            word = v;
        }
        cv_.notify_all();
    }
    void publish(int i, int rc, const char* err) {
        slot_[i].rc = rc;
        if (rc) slot_[i].err = err;
        signal(state_[i], 1);
    }

    void run() {
        ops_.thread_start();
        pin_thread(pthread_self(), cpus_);      // (read_parallel's threads inherit the mask)
        for (uint64_t k = 0;; ++k) {
            const int i = (int)(k & 1);
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || state_[i] == 0; });
                if (stop_) return;
            }
            const FqChunk& sl = slot_[i];
            const char* err = "";
            int rc;
            try {
                rc = fill(i, &err);
            } catch (...) {     // (the owner's event vector, read_parallel's threads)
                rc = SS_ENOMEM, err = "FASTQ reader: out of host memory";
            }
            publish(i, rc, err);
            if (rc || sl.at_eof) return;
            csrc_ = host_[i] + sl.use;
            carry_ = sl.n - sl.use;
        }
    }

    int send(int i, uint64_t off, uint64_t len) { return ops_.queue_copy(i, slot_[i].np++, off, len); }

    // the next chunk into slot i; an error's message in *err
    int fill(int i, const char** err) {
        FqChunk& sl = slot_[i];
        sl.np = 0;
        int rc = SS_OK;
        while (!rc) {
            if (cap_ >= (1ull << 32)) {
                *err = "a FASTQ line is longer than 2 GiB";
                return SS_EARG;
            }
            if ((rc = ops_.ensure(i, cap_, &host_[i]))) break;
            uint8_t* hv = host_[i];
            if (carry_ && csrc_ != hv) memcpy(hv, csrc_, carry_);
            const uint64_t want = std::min(cap_ - carry_, r_.size - pos_);
            if (carry_) rc = send(i, 0, carry_);
            for (uint64_t off = 0; off < want && !rc; off += r_.piece) {
                const uint64_t len = std::min(r_.piece, want - off);
                const auto t0 = Clock::now();
                const uint64_t got = read_parallel(r_.fd, hv + carry_ + off, len, pos_ + off, r_.threads, r_.par_min);
                if (r_.read_ms) *r_.read_ms += std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
                if (got != len) {
                    *err = "short read of the FASTQ file";
                    return SS_EHIP;
                }
                rc = send(i, carry_ + off, len);
            }
            if (rc) break;
            pos_ += want;
            sl.n = carry_ + want;
            sl.at_eof = pos_ >= r_.size;
            sl.use = sl.at_eof ? sl.n : 0;
            for (uint64_t q = sl.n; q > 0 && !sl.use; --q)
                if (hv[q - 1] == '\n') sl.use = q;
            if (sl.use) {
                rc = ops_.complete(i);
                break;
            }
            // one line fills the chunk: grow this slot (its bytes kept, sent again as the carry)
            if ((rc = ops_.wait_copies()) || (rc = ops_.grow(i, 2 * cap_, sl.n, &host_[i]))) break;
            cap_ *= 2;
            carry_ = sl.n;
            csrc_ = host_[i];
        }
        if (rc) *err = ops_.last_error();
        return rc;
    }

    FqSlotOps& ops_;
    const FqRange r_;
    const std::vector<int> cpus_;
    FqChunk slot_[2];
    uint8_t* host_[2] = {nullptr, nullptr};
    uint64_t pos_, cap_, carry_ = 0;     // next file byte; the slots' capacity; bytes carried into the next fill
    const uint8_t* csrc_ = nullptr;      // where the carry lies (the previous slot, or this one after a grow)
    std::mutex mu_;
    std::condition_variable cv_;
    int state_[2] = {0, 0};              // 0 the reader's, 1 filled (the consumer's)
    int stop_ = 0;
    std::thread th_;
};
