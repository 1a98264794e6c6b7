// host_threads_main.cpp — the library's host threads (csrc/fq_reader.h: the FASTQ reader ring,
// read_parallel; csrc/host_threads.h: CopyPool) driven on the CPU, with no HIP and no Python, so that
// ThreadSanitizer and ASan/UBSan can watch them (tests/test_host_threads.py builds this file with
// each and runs it).  The "device" of the reader's slots is a malloc'ed buffer of exactly the size
// the reader asked for, filled by memcpy as each piece is queued.  Exit status 0 = every check held.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "../../shortseq_amd/csrc/fq_reader.h"

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "FAILED %s:%d: %s | ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
            ++g_failed;                                          \
            return false;                                        \
        }                                                        \
    } while (0)

using Bytes = std::vector<uint8_t>;

void nap(int ms) {
    if (ms) std::this_thread::sleep_for(std::chrono::milliseconds(ms));
}

// The owner's side of the ring.  A slot's records (its log, its capacity) are written by the reader
// during a fill and read by the consumer while it holds the slot, as the real owner's are.
struct MockOps final : FqSlotOps {
    struct Rec {
        bool grow;
        uint64_t off, len;      // a piece, or (grow) len = the bytes kept
    };
    struct Slot {
        uint8_t* h = nullptr;
        uint8_t* d = nullptr;
        uint64_t hcap = 0, dcap = 0, cap = 0;    // cap: what the last ensure asked for
        std::vector<Rec> log;                    // of the fill in the slot
        uint32_t np = 0;                         // its pieces so far
        std::thread::id filler;
    } slot[2];
    uint64_t queued = 0, kept = 0;           // (read after the reader has ended)
    int slow_ms = 0;
    bool started = false;

    ~MockOps() {
        for (Slot& s : slot) free(s.h), free(s.d);
    }
    void thread_start() override { started = true; }
    int ensure(int i, uint64_t cap, uint8_t** host) override {
        Slot& s = slot[i];
        s.filler = std::this_thread::get_id();
        s.cap = cap;
        if (cap > s.hcap) {
            free(s.h);
            s.h = (uint8_t*)malloc(cap);
            s.hcap = cap;
        }
        if (cap + 16 > s.dcap) {
            free(s.d);
            s.d = (uint8_t*)malloc(cap + 16);
            s.dcap = cap + 16;
        }
        *host = s.h;
        return s.h && s.d ? SS_OK : SS_ENOMEM;
    }
    int queue_copy(int i, uint32_t piece, uint64_t off, uint64_t len) override {
        Slot& s = slot[i];
        if (piece == 0) s.log.clear(), s.np = 0;
        if (piece != s.np++) return SS_EARG;      // pieces are numbered 0, 1, ... through the grows of a fill
        if (off + len > s.hcap || off + len > s.dcap) return SS_EARG;
        memcpy(s.d + off, s.h + off, len);
        s.log.push_back({false, off, len});
        queued += len;
        return SS_OK;
    }
    int wait_copies() override { return SS_OK; }
    int grow(int i, uint64_t cap, uint64_t keep, uint8_t** host) override {
        Slot& s = slot[i];
        uint8_t* nh = (uint8_t*)malloc(cap);
        if (!nh) return SS_ENOMEM;
        memcpy(nh, s.h, keep);
        free(s.h);
        s.h = nh;
        s.hcap = cap;
        s.log.push_back({true, 0, keep});
        kept += keep;
        *host = nh;
        return SS_OK;
    }
    int complete(int) override {
        nap(slow_ms);
        return SS_OK;
    }
    const char* last_error() override { return "mock owner error"; }
};

struct TempFile {
    std::string path;
    int fd = -1;
    Bytes data;
    TempFile(const TempFile&) = delete;
    TempFile(const std::string& dir, const char* name, const Bytes& bytes) : path(dir + "/" + name), data(bytes) {
        FILE* f = fopen(path.c_str(), "wb");
        if (f) {
            if (!data.empty() && fwrite(data.data(), 1, data.size(), f) != data.size()) perror("fwrite");
            fclose(f);
        }
        fd = open(path.c_str(), O_RDONLY);
    }
    ~TempFile() {
        if (fd >= 0) close(fd);
        unlink(path.c_str());
    }
};

// ~300 lines of 0 .. 300 bytes, two of them ~5000 bytes
Bytes make_lines(uint32_t seed, bool final_newline) {
    std::mt19937 rng(seed);
    Bytes out;
    for (int i = 0; i < 300; ++i) {
        uint32_t len = rng() % 301;
        if (i == 90 || i == 210) len = 4900 + rng() % 200;
        for (uint32_t k = 0; k < len; ++k) out.push_back((uint8_t)(' ' + rng() % 90));
        out.push_back('\n');
    }
    if (!final_newline) out.pop_back();
    return out;
}

struct Case {
    uint64_t begin, end;          // the range; end past the file's size: the short-read case
    uint64_t chunk, piece;
    int consumer_ms = 0, reader_ms = 0;
    int stop_at = -1;             // early stop: 0 after taking chunk 0, 1 after chunk 1 (chunk 0 released), 2 holding both
    bool pin = false;             // give the reader a CPU list (forces the thread even for one chunk)
};

// One range through the ring, every chunk checked against the file's bytes.
bool run_case(const TempFile& f, const Case& c) {
    const uint64_t fsize = f.data.size(), size = c.end;
    const bool expect_short = size > fsize;
    const uint64_t cap0 = fq_cap0(c.chunk, size - c.begin);
    std::vector<int> cpus;
    if (c.pin) cpus.push_back(sched_getcpu());
    const bool inline_mode = size - c.begin <= cap0 && cpus.empty();
    MockOps ops;
    ops.slow_ms = c.reader_ms;
    double read_ms = 0;
    uint64_t sum_n = 0, done = c.begin, grows = 0;
    Bytes carry;                  // chunk k's [use, n)
    bool ended = false;
    {
        FqReader rd(ops, {f.fd, c.begin, size, cap0, 3, &read_ms, c.piece, 1024}, cpus);
        if (c.stop_at == 2) {
            CHECK(rd.acquire(0).rc == SS_OK && rd.acquire(1).rc == SS_OK, "holding both");
            return true;          // (the reader ends in its destructor, both slots taken)
        }
        for (uint64_t k = 0; !ended; ++k) {
            const FqChunk& ch = rd.acquire(k);
            const MockOps::Slot& sl = ops.slot[k & 1];
            if (ch.rc) {
                CHECK(expect_short, "chunk %llu: rc %d %s", (unsigned long long)k, ch.rc, ch.err.c_str());
                CHECK(ch.rc == SS_EHIP && ch.err == "short read of the FASTQ file", "rc %d '%s'", ch.rc, ch.err.c_str());
                return true;
            }
            CHECK(inline_mode == (sl.filler == std::this_thread::get_id()), "inline %d", (int)inline_mode);
            // the fill's log: [the carry] pieces from there on in order, (grow: all of it kept, sent again) ...
            uint64_t at = 0, expect_carry = carry.size(), bytes = 0, kept = 0;
            size_t q = 0;
            for (;;) {
                if (expect_carry) {
                    CHECK(q < sl.log.size() && !sl.log[q].grow && sl.log[q].off == 0 && sl.log[q].len == expect_carry,
                          "chunk %llu: carry piece", (unsigned long long)k);
                    bytes += sl.log[q++].len;
                }
                at = expect_carry;
                for (; q < sl.log.size() && !sl.log[q].grow; ++q) {
                    CHECK(sl.log[q].off == at && sl.log[q].len > 0 && sl.log[q].len <= c.piece, "chunk %llu piece %zu",
                          (unsigned long long)k, q);
                    at += sl.log[q].len;
                    bytes += sl.log[q].len;
                }
                if (q == sl.log.size()) break;
                CHECK(sl.log[q].len == at, "grow keeps %llu of %llu", (unsigned long long)sl.log[q].len, (unsigned long long)at);
                expect_carry = at;
                kept += at;
                ++grows, ++q;
            }
            CHECK(at == ch.n && bytes == ch.n + kept, "chunk %llu: pieces cover %llu of %llu", (unsigned long long)k,
                  (unsigned long long)at, (unsigned long long)ch.n);
            CHECK(ch.np == sl.np, "np %u, %u pieces queued", ch.np, sl.np);
            CHECK(sl.cap == cap0 << grows && ch.n <= sl.cap, "capacity %llu after %llu grows", (unsigned long long)sl.cap,
                  (unsigned long long)grows);
            // the bytes, as the "device" holds them
            CHECK(ch.use >= 1 && ch.use <= ch.n && done + ch.use <= fsize, "use %llu n %llu", (unsigned long long)ch.use,
                  (unsigned long long)ch.n);
            CHECK(memcmp(sl.d, f.data.data() + done, ch.use) == 0, "chunk %llu differs from the file", (unsigned long long)k);
            CHECK(carry.empty() || memcmp(sl.d, carry.data(), carry.size()) == 0, "chunk %llu: carry", (unsigned long long)k);
            CHECK(ch.at_eof == (done + ch.use == size), "chunk %llu at_eof %d", (unsigned long long)k, (int)ch.at_eof);
            CHECK(ch.at_eof ? ch.use == ch.n : sl.d[ch.use - 1] == '\n', "chunk %llu: end", (unsigned long long)k);
            carry.assign(sl.d + ch.use, sl.d + ch.n);
            done += ch.use;
            sum_n += ch.n;
            ended = ch.at_eof;
            if (c.stop_at == (int)k) return true;      // leaves holding chunk k
            nap(c.consumer_ms);
            if (!ended) rd.release(k);
        }
    }
    CHECK(!expect_short, "no short read reported");
    CHECK(done == size, "read %llu of %llu", (unsigned long long)done, (unsigned long long)size);
    CHECK(ops.started && ops.queued == sum_n + ops.kept, "queued %llu, chunks %llu + kept %llu", (unsigned long long)ops.queued,
          (unsigned long long)sum_n, (unsigned long long)ops.kept);
    // (every range of the long files holds a ~5000-byte line)
    CHECK(grows >= 1 || c.chunk > 4096 || size - c.begin < 20000, "no slot grew at chunk %llu", (unsigned long long)c.chunk);
    CHECK(read_ms > 0, "read_ms");
    return true;
}

// the position right after the newline at or past `from` (the file's size when there is none)
uint64_t after_newline(const Bytes& d, uint64_t from) {
    for (uint64_t p = from; p < d.size(); ++p)
        if (d[p] == '\n') return p + 1;
    return d.size();
}

bool test_reader(const std::string& dir) {
    const uint8_t one[] = {'A', 'C', 'G', 'T', '\n'};
    const TempFile files[] = {{dir, "nl.txt", make_lines(1, true)},
                              {dir, "nonl.txt", make_lines(2, false)},
                              {dir, "empty.txt", Bytes()},
                              {dir, "one.txt", Bytes(one, one + 5)}};
    for (const TempFile& f : files) {
        CHECK(f.fd >= 0, "cannot write %s", f.path.c_str());
        const uint64_t size = f.data.size();
        if (size == 0) continue;      // (an empty range never reaches the reader: its owner returns first)
        const uint64_t b = after_newline(f.data, size / 3), e = after_newline(f.data, 2 * size / 3);
        const uint64_t ranges[3][2] = {{0, size}, {b, size}, {0, e}};
        for (const auto& r : ranges) {
            if (r[0] >= r[1]) continue;
            for (uint64_t chunk : {16ull, 64ull, 1000ull, 4096ull, (unsigned long long)size + 100})
                for (uint64_t piece : {7ull, 64ull, 1ull << 20})
                    if (!run_case(f, {r[0], r[1], chunk, piece})) {
                        fprintf(stderr, "  in %s [%llu, %llu) chunk %llu piece %llu\n", f.path.c_str(), (unsigned long long)r[0],
                                (unsigned long long)r[1], (unsigned long long)chunk, (unsigned long long)piece);
                        return false;
                    }
        }
        // both wait orders, early stops (while the reader grows a slot, reads, or waits), a short read,
        // and one chunk on a thread of its own (the same view as inline, checked by the same code)
        const Case more[] = {{0, size, 4096, 64, 3, 0},        {0, size, 4096, 64, 0, 3},
                             {0, size, 16, 7, 0, 0, 0},        {0, size, 16, 7, 0, 0, 1},
                             {0, size, 16, 7, 0, 0, 2},        {0, size, 1000, 1 << 20, 0, 0, 0},
                             {0, size, 1000, 1 << 20, 2, 0, 1}, {0, size, 1000, 64, 0, 2, 2},
                             {0, size + 1000, 4096, 64},       {0, size + 1000, size + 5000, 1 << 20},
                             {0, size, size + 100, 64, 0, 0, -1, true}};
        for (const Case& c : more) {
            if (c.stop_at >= 1 && size < 100) continue;      // (needs two chunks)
            if (!run_case(f, c)) {
                fprintf(stderr, "  in %s chunk %llu piece %llu stop_at %d\n", f.path.c_str(), (unsigned long long)c.chunk,
                        (unsigned long long)c.piece, c.stop_at);
                return false;
            }
        }
    }
    return true;
}

bool test_read_parallel(const std::string& dir) {
    std::mt19937 rng(3);
    Bytes data(10000);
    for (uint8_t& v : data) v = (uint8_t)rng();
    const TempFile f(dir, "par.bin", data);
    CHECK(f.fd >= 0, "cannot write %s", f.path.c_str());
    for (unsigned threads : {1u, 3u, 8u})
        for (uint64_t pos : {0ull, 777ull}) {
            const uint64_t len = data.size() - pos;
            Bytes a(len + 500, 0xEE), b(len + 500, 0xEE);
            CHECK(pread_full(f.fd, a.data(), len, pos) == len, "pread_full");
            CHECK(read_parallel(f.fd, b.data(), len, pos, threads, 1024, 1024) == len, "read_parallel %u", threads);
            CHECK(a == b && memcmp(a.data(), data.data() + pos, len) == 0, "read_parallel %u at %llu differs", threads,
                  (unsigned long long)pos);
            // past the file's end: the short count, the same bytes
            CHECK(read_parallel(f.fd, b.data(), len + 500, pos, threads, 1024, 1024) == len, "short count %u", threads);
            CHECK(memcmp(b.data(), data.data() + pos, len) == 0, "short read %u differs", threads);
        }
    return true;
}

bool test_copy_pool() {
    std::mt19937 rng(4);
    const size_t sizes[] = {0, 1, (4u << 20) - 1, (4u << 20) + 4097, 9u << 20};
    Bytes src(9u << 20), dst(9u << 20);
    for (size_t i = 0; i < src.size(); i += 8) src[i] = (uint8_t)rng();
    for (int workers : {0, 1, 4}) {
        { CopyPool idle(workers, {}); }      // no copy made
        CopyPool pool(workers, workers == 4 ? std::vector<int>{sched_getcpu()} : std::vector<int>{});
        for (size_t n : sizes) {
            std::fill(dst.begin(), dst.end(), (uint8_t)0xEE);
            pool.copy(dst.data(), src.data(), n);
            CHECK(memcmp(dst.data(), src.data(), n) == 0, "%d workers: copy of %zu differs", workers, n);
            CHECK(n == dst.size() || dst[n] == 0xEE, "%d workers: copy of %zu wrote past its end", workers, n);
        }
        if (workers != 4) continue;
        for (int k = 0; k < 50; ++k) {
            const size_t n = (4u << 20) + 4097 + (size_t)k, off = (size_t)k * 3;
            pool.copy(dst.data(), src.data() + off, n);
            CHECK(memcmp(dst.data(), src.data() + off, n) == 0, "copy %d of 50 differs", k);
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    const bool ok = test_reader(dir) & test_read_parallel(dir) & test_copy_pool();
    if (ok && !g_failed) printf("host threads: all checks held\n");
    return ok && !g_failed ? 0 : 1;
}
