// qtrim_selftest.cpp — csrc/host_qtrim.h against naive byte loops, in a stand-alone program meant to be
// built with -fsanitize=address,undefined: every quality run and every FASTQ text sits in a heap block of
// exactly its size, so a load before q[0], past q[L - 1] or past blob[nbytes - 1] is caught by the sanitizer.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/qtrim_selftest.cpp -o qtrim_selftest && ./qtrim_selftest
// Prints "all checks held" and exits 0, or names the first differences and exits 1.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../shortseq_amd/csrc/host_qtrim.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t m) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 32) % m);
}

// the rule as the header states it, with every partial sum kept: the greatest sum before the first
// negative one, the rightmost position among equals
uint32_t naive_read(const uint8_t* q, uint32_t L, int c, int b) {
    if (L > 1024) return L;
    std::vector<long> sums(L);
    long s = 0;
    for (uint32_t k = 0; k < L; ++k) {
        s += c - ((int)q[L - 1 - k] - b);
        sums[k] = s;                       // the sum after byte L - 1 - k
    }
    long best = 0;
    uint32_t stop = L;
    for (uint32_t k = 0; k < L && sums[k] >= 0; ++k)
        if (sums[k] > best) {
            best = sums[k];
            stop = L - 1 - k;
        }
    return stop;
}

// the newlines of the text by index, then the three that matter
bool naive_locate(const uint8_t* blob, uint64_t nbytes, uint64_t off, uint32_t L, uint64_t* qoff, uint64_t* Q) {
    std::vector<uint64_t> nl;
    for (uint64_t k = 0; k < nbytes; ++k)
        if (blob[k] == '\n' && k >= off + L) nl.push_back(k);
    if (nl.size() < 2) return false;
    *qoff = nl[1] + 1;
    *Q = (nl.size() > 2 ? nl[2] : nbytes) - nl[1] - 1;
    return true;
}

int failures = 0;
unsigned long long cases = 0;

void check_read(const std::vector<uint8_t>& q, uint32_t c, uint32_t b) {
    const uint32_t L = (uint32_t)q.size();
    std::unique_ptr<uint8_t[]> block(new uint8_t[L]);       // exactly L bytes
    for (uint32_t k = 0; k < L; ++k) block[k] = q[k];
    const uint32_t got = ssh::qtrim_read(block.get(), L, c, b);
    const uint32_t exp = naive_read(block.get(), L, (int)c, (int)b);
    ++cases;
    if (got != exp && failures++ < 10) std::fprintf(stderr, "FAILED: qtrim_read L=%u c=%u b=%u: got %u, expected %u\n", L, c, b, got, exp);
}

void check_locate(const std::string& text, uint64_t off, uint32_t L) {
    const uint64_t n = text.size();
    std::unique_ptr<uint8_t[]> block(new uint8_t[n]);       // exactly nbytes bytes
    for (uint64_t k = 0; k < n; ++k) block[k] = (uint8_t)text[k];
    uint64_t qo = 777, Q = 777, eo = 777, eQ = 777;
    const bool got = ssh::qtrim_locate(block.get(), n, off, L, &qo, &Q);
    const bool exp = off + L <= n && naive_locate(block.get(), n, off, L, &eo, &eQ);
    ++cases;
    if ((got != exp || qo != eo || Q != eQ) && failures++ < 10)
        std::fprintf(stderr, "FAILED: qtrim_locate n=%llu off=%llu L=%u: got %d (%llu, %llu), expected %d (%llu, %llu)\n",
                     (unsigned long long)n, (unsigned long long)off, L, (int)got, (unsigned long long)qo, (unsigned long long)Q,
                     (int)exp, (unsigned long long)eo, (unsigned long long)eQ);
    // the layout form on the whole read
    bool usable = false;
    const uint32_t k = off + L <= n ? ssh::qtrim_read_fastq(block.get(), n, off, L, 20, 33, &usable) : L;
    uint32_t ek = L;
    if (L != 0 && L <= 1024 && exp && eQ >= L) ek = naive_read(block.get() + eo, L, 20, 33);
    if (k != ek && failures++ < 10) std::fprintf(stderr, "FAILED: qtrim_read_fastq n=%llu off=%llu L=%u: got %u, expected %u\n",
                                                  (unsigned long long)n, (unsigned long long)off, L, k, ek);
}

std::vector<uint8_t> random_quals(uint32_t n, uint32_t lo, uint32_t span) {
    std::vector<uint8_t> v(n);
    for (auto& c : v) c = (uint8_t)(lo + rnd(span));
    return v;
}

}  // namespace

int main() {
    const uint32_t Ls[] = {0, 1, 2, 15, 16, 17, 63, 64, 65, 150, 255, 256, 257, 1023, 1024};
    const uint32_t cutoffs[] = {1, 2, 20, 30, 93};
    const uint32_t bases[] = {33, 64};
    const uint8_t hostile[] = {0x00, 0x20, 0x7F, 0xFF, '\n'};
    for (uint32_t c : cutoffs)
        for (uint32_t b : bases) {
            for (uint32_t L : Ls) {
                check_read(random_quals(L, b + c + 1, 20), c, b);            // all high
                check_read(random_quals(L, b, c), c, b);                      // all low
                check_read(std::vector<uint8_t>(L, (uint8_t)(b + c)), c, b);  // all at the cutoff
                for (int rep = 0; rep < 6; ++rep) {                           // around the cutoff, with a hostile byte
                    std::vector<uint8_t> q = random_quals(L, b + (c > 4 ? c - 4 : 0), 9);
                    if (L && rep >= 3) q[rnd(L)] = hostile[rnd(5)];
                    check_read(q, c, b);
                }
            }
            for (uint32_t k = 0; k <= 40; ++k) {      // a low tail of every length on a 40-byte read
                std::vector<uint8_t> q(40, (uint8_t)(b + c + 10));
                for (uint32_t j = 40 - k; j < 40; ++j) q[j] = (uint8_t)(b + (c > 1 ? c - 1 : 0));
                check_read(q, c, b);
            }
        }
    // a read too long to be looked at: a null pointer is never dereferenced
    if (ssh::qtrim_read(nullptr, 1025, 20, 33) != 1025 || ssh::qtrim_read(nullptr, 0xFFFFFFFFu, 20, 33) != 0xFFFFFFFFu) {
        std::fprintf(stderr, "FAILED: a read past 1024 bytes was changed\n");
        ++failures;
    }
    // FASTQ text: '+' lines of several lengths, short and long quality lines, texts cut at every byte
    const uint32_t plus[] = {1, 15, 16, 17, 300};
    for (uint32_t P : plus)
        for (int dq = -1; dq <= 1; ++dq) {
            const uint32_t L = 30;
            std::string rec = "@h\n" + std::string(L, 'A') + "\n" + "+" + std::string(P - 1, 'x') + "\n";
            for (uint32_t k = 0; k < L + dq; ++k) rec += (char)(33 + (k < 20 ? 40 : 5));
            const std::string two = rec + "\n" + rec + "\n";
            for (uint64_t cut = 0; cut <= two.size(); cut += (P == 300 && cut > 40 && cut + 40 < two.size()) ? 7 : 1) {
                const std::string text = two.substr(0, cut);
                if (3 + L <= text.size()) check_locate(text, 3, L);
                if (rec.size() + 1 + 3 + L <= text.size()) check_locate(text, rec.size() + 1 + 3, L);
            }
        }
    {
        std::string nul = std::string("@h\nAC") + '\0' + "GT\n+\nIIIII\n";   // a sequence line shortened by a NUL: L = 1
        check_locate(nul, 3, 1);
        check_locate(nul, 3, 0);
        check_locate("@h\nACGT\n+\n", 3, 4);                                  // Q = 0
        check_locate("@h\nACGT\n+\n\n", 3, 4);
        check_locate("@h\nACGT", 3, 3);                                       // no newline at all behind the read
        check_locate("", 0, 0);
    }
    if (ssh::qtrim_args_ok(0, 33) || ssh::qtrim_args_ok(94, 33) || ssh::qtrim_args_ok(20, 32) || ssh::qtrim_args_ok(20, 0) ||
        !ssh::qtrim_args_ok(1, 33) || !ssh::qtrim_args_ok(93, 64)) {
        std::fprintf(stderr, "FAILED: qtrim_args_ok\n");
        ++failures;
    }
    if (failures) {
        std::fprintf(stderr, "FAILED: %d of %llu cases\n", failures, cases);
        return 1;
    }
    std::printf("%llu cases, all checks held\n", cases);
    return 0;
}
