// owned_main.cpp — the owning buffer and handle of csrc/ss_owned.h driven on the CPU, with no HIP and
// no Python, so that ASan / UBSan can watch them (tests/test_owned.py builds this file and runs it).
// The buffer's memory is a counting malloc policy, the handle a number with a counting destroy; the
// program keeps its own books of what is live, so a leak or a second free shows without
// LeakSanitizer.  Exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <type_traits>
#include <vector>

#include "../../shortseq_amd/csrc/ss_owned.h"

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

// the books: what is allocated / created now, every call so far, and the call that is made to fail
std::set<void*> g_bufs;
std::set<int> g_handles;
long g_calls = 0, g_fail_at = -1, g_bad_frees = 0, g_regrows = 0, g_copies = 0;
int g_next_handle = 1;
constexpr int kNoMem = -3;

long live() { return (long)g_bufs.size() + (long)g_handles.size(); }
bool fail_now() { return g_calls++ == g_fail_at; }

struct CountMem {
    static int alloc(void** p, uint64_t bytes) {
        if (fail_now()) return kNoMem;
        *p = malloc(bytes ? bytes : 1);
        g_bufs.insert(*p);
        return 0;
    }
    static void free(void* p) {
        if (!g_bufs.erase(p)) {      // not ours, or freed before
            ++g_bad_frees;
            return;
        }
        ::free(p);
    }
    static int copy_keep(void* dst, const void* src, uint64_t bytes, void*) {
        if (bytes) memcpy(dst, src, bytes);
        ++g_copies;
        return 0;
    }
    static void before_regrow() { ++g_regrows; }
};
template <typename T, uint64_t Min = 1>
using TBuf = Buf<T, CountMem, Min>;

int fake_create(int* out) {
    if (fail_now()) return kNoMem;
    *out = g_next_handle++;
    g_handles.insert(*out);
    return 0;
}
int fake_destroy(int h) {
    if (!g_handles.erase(h)) ++g_bad_frees;
    return 0;
}
using FakeTable = Handle<int, fake_destroy>;
static_assert(!std::is_copy_constructible<TBuf<int>>::value && !std::is_copy_assignable<TBuf<int>>::value &&
                  !std::is_copy_constructible<FakeTable>::value && !std::is_copy_assignable<FakeTable>::value,
              "owners are move-only");

bool test_ensure() {
    const long live0 = live();
    {
        TBuf<uint32_t, 16> b;
        CHECK(b.p == nullptr && b.cap == 0, "a new buffer is empty");
        CHECK(b.ensure(3) == 0 && b.cap == 16 && b.p, "the minimum element count, cap %llu", (unsigned long long)b.cap);
        uint32_t* p0 = b.p;
        for (uint32_t i = 0; i < 16; ++i) b.p[i] = i;
        CHECK(b.ensure(16) == 0 && b.p == p0 && b.cap == 16, "n <= cap keeps the buffer");
        CHECK(g_regrows == 0, "no wait before a first allocation");
        CHECK(b.ensure(17) == 0 && b.cap == 17 && live() == live0 + 1, "a grow frees the old buffer");
        CHECK(g_regrows == 1, "the wait before a grow frees a used buffer");
        b.p[16] = 1;        // (ASan: the whole new size is ours)
        g_fail_at = g_calls;
        CHECK(b.ensure(100) == kNoMem && b.p == nullptr && b.cap == 0 && live() == live0, "a failed grow leaves it empty");
        g_fail_at = -1;
        b.release();
        b.release();
        CHECK(live() == live0, "release twice");
    }
    CHECK(live() == live0 && g_bad_frees == 0, "nothing left, nothing freed twice");
    return true;
}

bool test_ensure_keep() {
    const long live0 = live();
    {
        TBuf<uint64_t> b;
        int stream = 0;
        CHECK(b.ensure_keep(10, 0, &stream) == 0 && b.cap == 10, "first allocation");
        for (uint64_t i = 0; i < 10; ++i) b.p[i] = 1000 + i;
        uint64_t* p0 = b.p;
        CHECK(b.ensure_keep(10, 10, &stream) == 0 && b.p == p0, "n <= cap keeps the buffer");
        const long copies0 = g_copies;
        CHECK(b.ensure_keep(11, 7, &stream) == 0 && b.cap == 20, "at least doubles: cap %llu", (unsigned long long)b.cap);
        CHECK(g_copies == copies0 + 1, "the copy (and its wait) before the old buffer goes");
        for (uint64_t i = 0; i < 7; ++i) CHECK(b.p[i] == 1000 + i, "element %llu kept", (unsigned long long)i);
        b.p[19] = 1;
        CHECK(b.ensure_keep(100, 7, &stream) == 0 && b.cap == 100 && b.p[6] == 1006, "n past the double");
        CHECK(live() == live0 + 1, "one buffer live");
        g_fail_at = g_calls;
        CHECK(b.ensure_keep(1000, 7, &stream) == kNoMem && b.cap == 100 && b.p[6] == 1006, "a failed grow keeps the old buffer");
        g_fail_at = -1;
    }
    CHECK(live() == live0 && g_bad_frees == 0, "nothing left, nothing freed twice");
    return true;
}

bool test_moves() {
    const long live0 = live();
    {
        TBuf<uint8_t> a, b;
        CHECK(a.ensure(100) == 0 && b.ensure(200) == 0 && live() == live0 + 2, "two buffers");
        uint8_t* pa = a.p;
        TBuf<uint8_t> c(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && c.p == pa && c.cap == 100 && live() == live0 + 2, "move-construct");
        b = std::move(c);
        CHECK(c.p == nullptr && c.cap == 0 && b.p == pa && b.cap == 100, "move-assign");
        CHECK(live() == live0 + 1, "the overwritten target freed once");
        TBuf<uint8_t>& self = b;
        b = std::move(self);
        CHECK(b.p == pa && live() == live0 + 1, "self-assignment");
        b = TBuf<uint8_t>();
        CHECK(b.p == nullptr && live() == live0, "assigned an empty one");

        FakeTable t, u;
        CHECK(!t && fake_create(t.put()) == 0 && fake_create(u.put()) == 0 && live() == live0 + 2, "two handles");
        const int ht = t;
        FakeTable v(std::move(t));
        CHECK(!t && (int)v == ht && live() == live0 + 2, "handle move-construct");
        u = std::move(v);
        CHECK(!v && (int)u == ht && live() == live0 + 1, "handle move-assign destroys the target's once");
        CHECK(fake_create(u.put()) == 0 && (int)u != ht && live() == live0 + 1, "put() destroys what was held");
        u.reset();
        u.reset();
        CHECK(!u && live() == live0, "reset twice");
    }
    CHECK(live() == live0 && g_bad_frees == 0, "nothing left, nothing freed twice");
    return true;
}

// a struct of owners, as the engine's Group: no destructor, no release list
struct S {
    FakeTable table;
    TBuf<uint64_t> rowmap, words;
    TBuf<uint32_t> lens;
};
bool fill(S& s, uint64_t n) {
    return fake_create(s.table.put()) == 0 && s.rowmap.ensure(n) == 0 && s.words.ensure(2 * n) == 0 && s.lens.ensure(n) == 0;
}

bool test_containers() {
    const long live0 = live();
    std::map<uint32_t, S> m;
    for (uint32_t k = 0; k < 5; ++k) CHECK(fill(m[k * 7], 10 + k), "map entry %u", k);
    CHECK(live() == live0 + 20, "five structs of four");
    m.erase(7);
    CHECK(live() == live0 + 16, "an erased entry frees its own");
    m.clear();
    CHECK(live() == live0, "map clear");
    std::vector<S> v;
    for (uint32_t k = 0; k < 9; ++k) {       // (grows by moves: nothing is freed or copied on the way)
        v.emplace_back();
        CHECK(fill(v.back(), 3 + k), "vector entry %u", k);
        CHECK(live() == live0 + 4 * (long)(k + 1), "entry %u: live %ld", k, live());
    }
    v.erase(v.begin() + 2);
    CHECK(live() == live0 + 32 && v[2].rowmap.cap == 6, "erase moves the rest down");
    v.resize(3);
    CHECK(live() == live0 + 12, "resize");
    v.clear();
    CHECK(live() == live0 && g_bad_frees == 0, "vector clear");
    return true;
}

// The shape of the engine's group_room: a new table owned locally until it is installed, six local
// buffers, a return on the first failure; the old table goes to the pool.
int room_like(S& gr, std::vector<FakeTable>& pool, uint64_t cap) {
    FakeTable nt;
    int rc = fake_create(nt.put());
    if (rc) return rc;
    TBuf<uint64_t> k, c, f, pc, wd;
    TBuf<uint32_t> l;
    if ((rc = k.ensure(cap)) || (rc = c.ensure(cap)) || (rc = f.ensure(cap)) || (rc = l.ensure(cap)) ||
        (rc = pc.ensure(1)) || (rc = wd.ensure(cap * 3)))
        return rc;
    pool.push_back(std::move(gr.table));
    gr.table = std::move(nt);
    return 0;
}

bool test_early_returns() {
    const long live0 = live();
    {
        S gr;
        std::vector<FakeTable> pool;
        pool.reserve(4);
        CHECK(fill(gr, 8), "the group");
        const long live1 = live();
        const int t0 = gr.table;
        for (long k = 0; k < 7; ++k) {          // the table, then the six buffers
            g_fail_at = g_calls + k;
            CHECK(room_like(gr, pool, 64) == kNoMem, "allocation %ld fails", k);
            CHECK(live() == live1, "allocation %ld: live %ld, was %ld", k, live(), live1);
            CHECK((int)gr.table == t0 && pool.empty(), "allocation %ld: the group keeps its table", k);
        }
        g_fail_at = -1;
        CHECK(room_like(gr, pool, 64) == 0, "no failure");
        CHECK(live() == live1 + 1 && pool.size() == 1 && (int)pool[0] == t0 && (int)gr.table != t0, "the new table installed, the old one pooled");
    }
    CHECK(live() == live0 && g_bad_frees == 0, "nothing left, nothing freed twice");
    return true;
}

}  // namespace

int main() {
    test_ensure();
    test_ensure_keep();
    test_moves();
    test_containers();
    test_early_returns();
    if (live() != 0 || g_bad_frees != 0) {
        fprintf(stderr, "FAILED: %ld live allocations, %ld bad frees at exit\n", live(), g_bad_frees);
        ++g_failed;
    }
    if (g_failed) return 1;
    printf("all checks held\n");
    return 0;
}
