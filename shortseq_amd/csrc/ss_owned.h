// ss_owned.h — owners of the library's buffers, streams and events, host-only (no HIP in here: it
// builds with a plain host compiler and runs under ASan / UBSan in tests/host/owned_main.cpp, as
// fq_reader.h does).  The HIP side -- where memory comes from, how a handle is destroyed -- is a
// policy given by ss_internal.h.  Both types are move-only (a copy would make two owners of one
// allocation), so a struct of them frees what it holds when it goes, members in reverse declaration
// order: it declares its streams before the buffers used on them and needs no release list.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>

// A grow-only buffer of at least Min elements of T.  Mem is its memory:
//   static int alloc(void** p, uint64_t bytes)   0, or an error code with its message recorded
//   static void free(void* p)
//   static int copy_keep(void* dst, const void* src, uint64_t bytes, void* stream)
//       the copy (bytes may be 0) and the wait for `stream`: nothing queued reads src after it
//   static void before_regrow()   ensure() is about to free a buffer that queued work may still read
template <typename T, typename Mem, uint64_t Min = 1>
struct Buf {
    T* p = nullptr;
    uint64_t cap = 0;

    Buf() = default;
    Buf(const Buf&) = delete;      // (copy assignment too: the moves below are declared)
    Buf(Buf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~Buf() { release(); }

    // room for n elements; the contents are not kept across a grow
    int ensure(uint64_t n) {
        if (n <= cap) return 0;
        if (p) Mem::before_regrow();
        release();
        const uint64_t want = std::max<uint64_t>(n, Min);
        if (int rc = Mem::alloc((void**)&p, want * sizeof(T))) return rc;
        cap = want;
        return 0;
    }
    // grow keeping the first `used` elements (geometric: appended-to buffers such as row maps); the old
    // buffer is freed once the copy on `stream` is complete
    int ensure_keep(uint64_t n, uint64_t used, void* stream) {
        if (n <= cap) return 0;
        T* q = nullptr;
        const uint64_t want = std::max<uint64_t>(n, 2 * cap);
        if (int rc = Mem::alloc((void**)&q, want * sizeof(T))) return rc;
        const int rc = Mem::copy_keep(q, p, used * sizeof(T), stream);
        release();
        p = q;
        cap = want;
        return rc;
    }
    void release() {
        if (p) Mem::free(p);
        p = nullptr;
        cap = 0;
    }
};

// A handle (a stream, an event, a table) destroyed by Destroy when its owner goes; H{} is no handle.
// Reads as the handle wherever one is expected; put() is where a create call stores a new one.
template <typename H, auto Destroy>
struct Handle {
    H h{};

    Handle() = default;
    Handle(const Handle&) = delete;     // (copy assignment too)
    Handle(Handle&& o) noexcept : h(std::exchange(o.h, H{})) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) {
            reset();
            h = std::exchange(o.h, H{});
        }
        return *this;
    }
    ~Handle() { reset(); }

    operator H() const { return h; }
    H* put() {
        reset();
        return &h;
    }
    void reset() {
        if (h != H{}) (void)Destroy(h);
        h = H{};
    }
};
