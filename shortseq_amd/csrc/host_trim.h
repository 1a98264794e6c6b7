// host_trim.h — 3' adapter trim of one read on the host, header-only, no HIP.
//
// The rule (include/shortseq_amd.h, "3' adapter trim"): for a read r[0..L), an adapter a[0..A)
// (1 <= A <= 64), min_overlap >= 1 and err_div >= 0, position p (0 <= p < L) has
//   ov(p) = min(A, L - p)
//   mm(p) = #{k < ov(p) : a[k] != 'N' and r[p + k] != a[k]}      (bytewise, case-sensitive)
// and matches iff ov(p) >= min_overlap and mm(p) <= (err_div ? ov(p) / err_div : 0).  The trimmed
// length is the LEAST matching p, or L.  Only an 'N' in the adapter is a wildcard; any byte of the
// read is compared as it is.  Leftmost, not best-scoring; no indels.
//
// The same SWAR step as the device kernel (k_trim_adapter3, ss_trim.hip): 8 bytes of the read xor
// the adapter word, masked by the wildcard and overlap masks, nonzero bytes counted.  Reads are
// loaded with memcpy of exactly the bytes that exist: nothing past r[L - 1] is touched.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace ssh {

constexpr uint32_t kTrimMaxAdapter = 64;
constexpr uint32_t kTrimMaxRead = 1024;    // SS_MAX_NT: longer reads stay as they are

struct TrimAdapter {
    uint64_t w[8];      // the adapter's bytes, little-endian, zero past A
    uint64_t m[8];      // 0xFF per compared byte (k < A and a[k] != 'N'), else 0
    uint64_t cmp;       // the same as one bit per adapter byte (the kernel's argument)
    uint32_t A, min_overlap, err_div;
};

// false (and *t untouched) for arguments the ABI rejects: a null adapter, A == 0, A > 64, min_overlap == 0
inline bool trim_prepare(TrimAdapter* t, const uint8_t* a, uint32_t A, uint32_t min_overlap, uint32_t err_div) {
    if (!a || A == 0 || A > kTrimMaxAdapter || min_overlap == 0) return false;
    TrimAdapter r;
    memset(&r, 0, sizeof r);
    for (uint32_t k = 0; k < A; ++k) {
        r.w[k >> 3] |= (uint64_t)a[k] << (8 * (k & 7));
        if (a[k] != 'N') {
            r.m[k >> 3] |= 0xFFull << (8 * (k & 7));
            r.cmp |= 1ull << k;
        }
    }
    r.A = A;
    r.min_overlap = min_overlap;
    r.err_div = err_div;
    *t = r;
    return true;
}

// 0x80 in every nonzero byte of x (constexpr: the device kernel calls it too)
constexpr uint64_t trim_nonzero_bytes(uint64_t x) {
    const uint64_t k7 = 0x7F7F7F7F7F7F7F7Full;
    return (((x & k7) + k7) | x) & ~k7;
}

// The trimmed length of one read of L bytes (L > 1024: L itself, nothing is read).
inline uint32_t trim_read(const TrimAdapter& t, const uint8_t* r, uint32_t L) {
    // (an adapter shorter than min_overlap never has enough overlap)
    if (L > kTrimMaxRead || L < t.min_overlap || t.A < t.min_overlap) return L;
    for (uint32_t p = 0; p + t.min_overlap <= L; ++p) {
        const uint32_t ov = L - p < t.A ? L - p : t.A;
        const uint32_t budget = t.err_div ? ov / t.err_div : 0u;
        uint32_t mm = 0;
        for (uint32_t k = 0; k < ov && mm <= budget; k += 8) {
            const uint32_t nb = ov - k < 8 ? ov - k : 8u;
            uint64_t x = 0;
            memcpy(&x, r + p + k, nb);
            x = (x ^ t.w[k >> 3]) & t.m[k >> 3];
            if (nb < 8) x &= (1ull << (8 * nb)) - 1;
            mm += (uint32_t)__builtin_popcountll(trim_nonzero_bytes(x));
        }
        if (mm <= budget) return p;
    }
    return L;
}

}  // namespace ssh
