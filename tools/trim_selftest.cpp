// trim_selftest.cpp — csrc/host_trim.h against a naive byte loop, in a stand-alone program meant to be
// built with -fsanitize=address,undefined: every read sits in a heap block of exactly its length, so a
// load past r[L - 1] (the SWAR step reads 8 bytes at a time) is caught by the sanitizer.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/trim_selftest.cpp -o trim_selftest && ./trim_selftest
// Prints "all checks held" and exits 0, or names the first difference and exits 1.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../shortseq_amd/csrc/host_trim.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t m) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 32) % m);
}

uint32_t naive(const uint8_t* r, uint32_t L, const uint8_t* a, uint32_t A, uint32_t mo, uint32_t ed) {
    if (L > 1024) return L;
    for (uint32_t p = 0; p < L; ++p) {
        const uint32_t ov = L - p < A ? L - p : A;
        if (ov < mo) continue;
        uint32_t mm = 0;
        for (uint32_t k = 0; k < ov; ++k) mm += a[k] != 'N' && r[p + k] != a[k];
        if (mm <= (ed ? ov / ed : 0u)) return p;
    }
    return L;
}

int failures = 0;

void check(const std::vector<uint8_t>& read, const std::vector<uint8_t>& ad, uint32_t mo, uint32_t ed) {
    const uint32_t L = (uint32_t)read.size();
    std::unique_ptr<uint8_t[]> block(new uint8_t[L]);       // exactly L bytes
    for (uint32_t k = 0; k < L; ++k) block[k] = read[k];
    std::unique_ptr<uint8_t[]> ablock(new uint8_t[ad.size()]);
    for (size_t k = 0; k < ad.size(); ++k) ablock[k] = ad[k];
    ssh::TrimAdapter t;
    if (!ssh::trim_prepare(&t, ablock.get(), (uint32_t)ad.size(), mo, ed)) {
        std::fprintf(stderr, "FAILED: trim_prepare refused A=%zu mo=%u\n", ad.size(), mo);
        ++failures;
        return;
    }
    const uint32_t got = ssh::trim_read(t, block.get(), L);
    const uint32_t exp = naive(block.get(), L, ablock.get(), (uint32_t)ad.size(), mo, ed);
    if (got != exp && failures++ < 10)
        std::fprintf(stderr, "FAILED: L=%u A=%zu mo=%u ed=%u: got %u, expected %u\n", L, ad.size(), mo, ed, got, exp);
}

std::vector<uint8_t> random_bases(uint32_t n) {
    std::vector<uint8_t> v(n);
    for (auto& c : v) c = "ACGT"[rnd(4)];
    return v;
}

}  // namespace

int main() {
    const uint32_t As[] = {1, 7, 8, 9, 16, 17, 33, 64};
    const uint32_t eds[] = {0, 1, 4, 8, 10};
    const uint8_t hostile[] = {'N', 'a', 0x00, 0xFF, '\n'};
    uint64_t cases = 0;
    for (uint32_t A : As) {
        for (int wild = 0; wild < 2; ++wild) {
            std::vector<uint8_t> ad = random_bases(A);
            if (wild) ad[0] = ad[A / 2] = ad[A - 1] = 'N';
            const uint32_t mos[] = {1, 3, A};
            for (uint32_t mo : mos) {
                for (uint32_t ed : eds) {
                    const uint32_t Ls[] = {0, 1, mo - 1, mo, A - 1, A, A + 1, 15, 16, 17, 63, 64, 65, 150, 1023, 1024};
                    for (uint32_t L : Ls) {
                        check(random_bases(L), ad, mo, ed);
                        ++cases;
                        if (L == 0) continue;
                        // the adapter's first k bytes at the 3' end, with 0..2 substitutions and a hostile byte
                        for (int rep = 0; rep < 4; ++rep) {
                            std::vector<uint8_t> r = random_bases(L);
                            const uint32_t k = 1 + rnd(A < L ? A : L);
                            for (uint32_t q = 0; q < k; ++q) r[L - k + q] = ad[q];
                            for (uint32_t s = 0; s < (uint32_t)rep % 3; ++s) r[L - 1 - rnd(k)] = "ACGT"[rnd(4)];
                            if (rep == 3) r[L - 1 - rnd(k)] = hostile[rnd(5)];
                            check(r, ad, mo, ed);
                            ++cases;
                        }
                    }
                    // the adapter, cut at the read's end, at every position of a 40-byte read
                    for (uint32_t p = 0; p < 40; ++p) {
                        std::vector<uint8_t> r = random_bases(40);
                        for (uint32_t q = 0; q < A && p + q < 40; ++q) r[p + q] = ad[q];
                        check(r, ad, mo, ed);
                        ++cases;
                    }
                }
            }
        }
    }
    // arguments the ABI rejects
    ssh::TrimAdapter t;
    const uint8_t one[1] = {'A'};
    if (ssh::trim_prepare(&t, one, 0, 3, 10) || ssh::trim_prepare(&t, one, 65, 3, 10) || ssh::trim_prepare(&t, one, 1, 0, 10) ||
        ssh::trim_prepare(&t, nullptr, 1, 3, 10)) {
        std::fprintf(stderr, "FAILED: trim_prepare accepted a bad argument\n");
        ++failures;
    }
    if (failures) {
        std::fprintf(stderr, "FAILED: %d of %llu cases\n", failures, (unsigned long long)cases);
        return 1;
    }
    std::printf("%llu cases, all checks held\n", (unsigned long long)cases);
    return 0;
}
