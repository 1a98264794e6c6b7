// host_qtrim.h — 3' quality trim of one read on the host, header-only, no HIP.
//
// The rule (include/shortseq_amd.h, "3' quality trim"): for a read of L <= 1024 bytes with quality
// bytes q[0..L), a cutoff c in 1..93 and a base b of 33 or 64,
//   s = 0; best = 0; stop = L
//   for i = L-1 down to 0:
//       s += c - (int(q[i]) - b)          (q[i] as an unsigned byte: any value is legal)
//       if s < 0: break
//       if s > best: best = s; stop = i
// and the new length is stop: BWA's running sum, the rule behind cutadapt's -q for the 3' end.  A tie
// keeps the rightmost position, s == 0 neither ends the walk nor moves stop.  The sum stays inside
// 1024 * 255 in magnitude, far inside an int32.
//
// qtrim_locate finds a read's quality line in FASTQ text (the layout form of ss_trim_quality3).  Both
// functions touch only q[0..L) and blob[0..nbytes).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace ssh {

constexpr uint32_t kQtrimMaxRead = 1024;     // SS_MAX_NT: longer reads stay as they are
constexpr uint32_t kQtrimMaxCutoff = 93;

// the arguments the ABI accepts
inline bool qtrim_args_ok(uint32_t cutoff, uint32_t base) {
    return cutoff >= 1 && cutoff <= kQtrimMaxCutoff && (base == 33 || base == 64);
}

// The trimmed length of a read whose L quality bytes are q[0..L) (L > 1024: L itself, nothing is read).
inline uint32_t qtrim_read(const uint8_t* q, uint32_t L, uint32_t cutoff, uint32_t base) {
    if (L > kQtrimMaxRead) return L;
    const int32_t cb = (int32_t)(cutoff + base);
    int32_t s = 0, best = 0;
    uint32_t stop = L;
    for (uint32_t i = L; i-- > 0;) {
        s += cb - (int32_t)q[i];
        if (s < 0) break;
        if (s > best) {
            best = s;
            stop = i;
        }
    }
    return stop;
}

// The quality line of the sequence line blob[off .. off + L) of FASTQ text blob[0..nbytes):
//   e1 = the first '\n' at a position >= off + L (the end of the sequence line; further right than
//        off + L where a NUL shortened the line), e2 = the first '\n' after e1 (the end of the '+' line),
//   the quality line is [e2 + 1, e3) with e3 = the next '\n' or nbytes.
// true: *qoff = e2 + 1, *Q = e3 - e2 - 1.  false (outputs untouched): e1 or e2 does not exist.
inline bool qtrim_locate(const uint8_t* blob, uint64_t nbytes, uint64_t off, uint32_t L, uint64_t* qoff, uint64_t* Q) {
    if (off > nbytes || L > nbytes - off) return false;
    uint64_t p = off + L;
    for (int k = 0; k < 2; ++k) {
        if (p >= nbytes) return false;
        const void* e = memchr(blob + p, '\n', nbytes - p);
        if (!e) return false;
        p = (uint64_t)((const uint8_t*)e - blob) + 1;
    }
    const void* e3 = p < nbytes ? memchr(blob + p, '\n', nbytes - p) : nullptr;
    *qoff = p;
    *Q = (e3 ? (uint64_t)((const uint8_t*)e3 - blob) : nbytes) - p;
    return true;
}

// The layout form on one read: the new length, and *usable = false where the read has no quality
// line of at least L bytes (it keeps its length).
inline uint32_t qtrim_read_fastq(const uint8_t* blob, uint64_t nbytes, uint64_t off, uint32_t L, uint32_t cutoff,
                                 uint32_t base, bool* usable) {
    *usable = true;
    if (L > kQtrimMaxRead || L == 0) return L;
    uint64_t qoff = 0, Q = 0;
    if (!qtrim_locate(blob, nbytes, off, L, &qoff, &Q) || Q < L) {
        *usable = false;
        return L;
    }
    return qtrim_read(blob + qoff, L, cutoff, base);
}

}  // namespace ssh
