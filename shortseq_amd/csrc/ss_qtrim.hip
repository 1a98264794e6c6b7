// ss_qtrim.hip — 3' quality trim of a ragged batch: d_out_lens[i] = read i's length after BWA's
// running-sum rule over its quality bytes (include/shortseq_amd.h, "3' quality trim"; the rule on one
// read is csrc/host_qtrim.h).  No read is moved: lowering a length is the whole trim, as for the
// adapter (ss_trim.hip), and the two compose -- quality first, then the adapter on the kept prefix.
//
// k_trim_quality3<G>: a group of G lanes per read, 256 / G reads per block.
//   - Where the quality bytes are.  Explicit form: d_qual + d_qoffsets[i].  FASTQ layout form: the
//     group looks for the '\n' that ends the sequence line from offsets[i] + L on (G 16-B aligned chunks
//     per step, the '\n' bytes of a chunk as a 16-bit mask, the group's first from the wave ballot), then
//     for the '\n' that ends the '+' line; where both sit in one chunk ("\n+\n", the usual record) the
//     second comes out of the first's mask and there is no second load.  Nothing at or past nbytes is
//     looked at, and no chunk past the one holding byte nbytes - 1 is loaded.
//   - The walk goes from the right in rounds of G chunks (G = 2 in the library): lane t takes the t-th
//     chunk from the right, replaces the bytes outside the read by cutoff + base (a score of 0), sums
//     its 16 scores with v_sad_u8, the group prefix-sums the totals by shuffles, and each lane then walks
//     its own 16 bytes
//     exactly from its starting sum: where the sum first goes negative, and the greatest sum right of
//     that with its rightmost position.  The rightmost lane that went negative ends the read; the lanes
//     right of it (and its own bytes before the break) give the maximum as one packed (sum, position)
//     key reduced by shuffles, which replaces the carried best only where it is greater (earlier rounds
//     lie further right and win ties).  A read whose first round decides it does no second.
//   - FASTQ layout form: the walk uses the L bytes after the '+' line if they lie below nbytes.  A '\n'
//     among them means the quality line is short (Q < L).  Only a read with stop < L can be changed by
//     that, so only such a read has the chunks that the walk did not visit searched (a '\n' in a visited
//     chunk is seen in the walk: one zero-byte test per dword); with d_stats every read is checked, so
//     that stats[2] is exact.  A read without a usable quality line keeps its length.
//   - Grid-stride over the reads with one trip count for every thread (ballots and shuffles need whole
//     groups); reads of more than SS_MAX_NT bytes (0xFFFFFFFF included) and empty reads leave with their
//     length, nothing of them is read.
//   - d_stats: per-lane sums, reduced per wave by shuffles and per block through LDS, then up to three
//     64-bit atomic adds per block.
// d_out_lens may be d_lens: a read's length is loaded by its own group before that group's one store.
#include <algorithm>

#include "ss_device.h"
#include "ss_internal.h"
#include "host_qtrim.h"

namespace {

using namespace ssd;

constexpr int kQtThreads = 256;
constexpr uint64_t kQtReadsPerLaunch = 1ull << 28;
// The library's lane group, measured (profiles/qtrim/README.md): one lane is 9 % faster where nine reads in
// ten end at their first byte and 70 % slower where every read walks 50..150 bytes; four lanes tie with two
// on long walks and lose 35 % on short ones (three of four lanes load a chunk nobody needs).
constexpr int kQtG = 2;
constexpr uint64_t kQtNone = ~0ull;

// 0x80 in every zero byte of y (exact per byte)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t y) {
    return ((((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u) ^ 0x80808080u;
}

// bit j: byte j of the chunk is '\n'
__device__ __forceinline__ uint32_t nl_mask16(uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)      // the four 0x80 flags to four adjacent bits: one multiply, no carries
        m |= ((((zero_bytes(w[k] ^ 0x0A0A0A0Au) >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * k);
    return m;
}

// bits [lo, hi) of 16 (0 <= lo < 16, 1 <= hi <= 16)
__device__ __forceinline__ uint32_t range16(uint32_t lo, uint32_t hi) { return (0xFFFFu << lo) & (0xFFFFu >> (16u - hi)) & 0xFFFFu; }

// Chunk ck (0 .. lastc) of the quality run that starts sh bytes into chunk 0 of `a` and has L bytes:
// its four dwords, with every byte outside the run replaced by `fill` (in all four bytes of fill4).
__device__ __forceinline__ void load_chunk(const uint4* a, uint32_t ck, uint32_t sh, uint32_t lastc, uint32_t L,
                                           uint32_t fill4, uint32_t (&w)[4]) {
    const uint4 v = ld_stream(a + ck);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    const uint32_t lo = ck == 0 ? sh : 0u, hi = ck == lastc ? ((sh + L - 1u) & 15u) + 1u : 16u;
    if (lo != 0 || hi != 16) {
        const uint32_t vm = range16(lo, hi);
#pragma unroll
        for (int k = 0; k < 4; ++k) {    // nibble -> one 0xFF per set bit
            const uint32_t bm = ((((vm >> (4 * k)) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu;
            w[k] = (w[k] & bm) | (fill4 & ~bm);
        }
    }
}

__device__ __forceinline__ bool has_nl(const uint32_t (&w)[4]) {
    return (zero_bytes(w[0] ^ 0x0A0A0A0Au) | zero_bytes(w[1] ^ 0x0A0A0A0Au) | zero_bytes(w[2] ^ 0x0A0A0A0Au) |
            zero_bytes(w[3] ^ 0x0A0A0A0Au)) != 0;
}

// The first '\n' of blob[p .. nbytes) or kQtNone (the same in every lane of the group; p is), and in
// *next the '\n' after it where the same 16-B chunk holds one (else kQtNone).
template <int G>
__device__ __forceinline__ uint64_t find_nl(const uint8_t* blob, uint64_t nbytes, uint64_t p, uint32_t t, uint32_t gsh,
                                            uint64_t gmask, uint64_t* next) {
    *next = kQtNone;
    if (p >= nbytes) return kQtNone;
    const uintptr_t addr = (uintptr_t)blob;
    const uint4* a = (const uint4*)(addr & ~(uintptr_t)15);
    const uint64_t sh0 = addr & 15, x = sh0 + p, xend = sh0 + nbytes;      // in bytes from a
    const uint64_t clast = (xend - 1) >> 4;                                 // the chunk holding byte nbytes - 1
    for (uint64_t c = x >> 4; c <= clast; c += G) {
        const uint64_t mc = c + t;
        uint32_t m = 0;
        if (mc <= clast) {
            const uint4 v = a[mc];
            const uint32_t lo = x > mc * 16 ? (uint32_t)(x - mc * 16) : 0u;
            const uint32_t hi = xend - mc * 16 >= 16 ? 16u : (uint32_t)(xend - mc * 16);
            m = nl_mask16(v) & range16(lo, hi);
        }
        const uint64_t b = (__ballot(m != 0) >> gsh) & gmask;
        if (b) {
            const uint32_t src = (uint32_t)__builtin_ctzll(b);
            const uint32_t ms = (uint32_t)__shfl((int)m, (int)(gsh + src), 64);
            const uint64_t at = (c + src) * 16 - sh0;
            const uint32_t rest = ms & (ms - 1u);
            if (rest) *next = at + (uint32_t)__builtin_ctz(rest);
            return at + (uint32_t)__builtin_ctz(ms);
        }
    }
    return kQtNone;
}

template <int G>
__global__ __launch_bounds__(kQtThreads) void k_trim_quality3(const uint8_t* blob, uint64_t nbytes,
                                                              const uint64_t* __restrict__ offs, const uint32_t* lens,
                                                              uint64_t n, const uint8_t* qual,
                                                              const uint64_t* __restrict__ qoffs, uint32_t cb, uint32_t* out,
                                                              unsigned long long* stats, uint32_t iters) {
    constexpr int kGroups = kQtThreads / G;
    __shared__ unsigned long long red[3][kQtThreads / 64];
    const uint32_t t = threadIdx.x % G, grp = threadIdx.x / G;
    const uint32_t gsh = threadIdx.x & 63u & ~(uint32_t)(G - 1);
    const uint64_t gmask = G == 64 ? ~0ull : (1ull << G) - 1;
    const uint32_t cb4 = cb * 0x01010101u;         // cutoff + base <= 157 in every byte: a score of 0
    const bool fq = qoffs == nullptr;              // (uniform)
    unsigned long long nshort = 0, nremoved = 0, nnoqual = 0;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint64_t i = ((uint64_t)it * gridDim.x + blockIdx.x) * kGroups + grp;
        const bool live = i < n;
        const uint32_t L = live ? lens[i] : 0u;
        uint32_t res = L;
        bool noqual = false;
        // (everything below is the same in every lane of a group)
        if (live && L != 0 && L <= SS_MAX_NT) {
            const uint8_t* q = nullptr;
            if (fq) {
                uint64_t e2 = kQtNone;
                const uint64_t e1 = find_nl<G>(blob, nbytes, offs[i] + L, t, gsh, gmask, &e2);
                if (e1 != kQtNone && e2 == kQtNone) {
                    uint64_t unused;
                    e2 = find_nl<G>(blob, nbytes, e1 + 1, t, gsh, gmask, &unused);
                }
                if (e2 != kQtNone && e2 + 1 + L <= nbytes) q = blob + e2 + 1;
                else noqual = true;
            } else {
                q = qual + qoffs[i];
            }
            if (q) {
                const uintptr_t addr = (uintptr_t)q;
                const uint4* a = (const uint4*)(addr & ~(uintptr_t)15);
                const uint32_t sh = (uint32_t)(addr & 15);
                const uint32_t lastc = (sh + L - 1u) >> 4;       // the chunk holding the last quality byte
                int32_t carry = 0, best = 0;
                uint32_t stop = L;
                bool nl = false, done = false;
                int32_t c0 = (int32_t)lastc;                     // lane 0's chunk of this round
                for (; c0 >= 0 && !done; c0 -= G) {
                    const int32_t ck = c0 - (int32_t)t;
                    uint32_t w[4] = {cb4, cb4, cb4, cb4};
                    if (ck >= 0) {
                        load_chunk(a, (uint32_t)ck, sh, lastc, L, cb4, w);
                        if (fq) nl |= has_nl(w);
                    }
                    // the chunk's total score, then this lane's starting sum: the carry plus the lanes right of it
                    uint32_t qsum = __builtin_amdgcn_sad_u8(w[0], 0u, 0u);
                    qsum = __builtin_amdgcn_sad_u8(w[1], 0u, qsum);
                    qsum = __builtin_amdgcn_sad_u8(w[2], 0u, qsum);
                    qsum = __builtin_amdgcn_sad_u8(w[3], 0u, qsum);
                    int32_t incl = 16 * (int32_t)cb - (int32_t)qsum;
#pragma unroll
                    for (int d = 1; d < G; d <<= 1) {
                        const int32_t y = __shfl_up(incl, d, G);
                        if ((int)t >= d) incl += y;
                    }
                    incl += carry;
                    int32_t s = incl - (16 * (int32_t)cb - (int32_t)qsum);
                    // the exact walk over this lane's 16 bytes, right to left
                    int32_t m = s, pj = -1;
                    bool broke = false;
#pragma unroll
                    for (int j = 15; j >= 0; --j) {
                        s += (int32_t)cb - (int32_t)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
                        broke |= s < 0;
                        if (!broke && s > m) {
                            m = s;
                            pj = j;
                        }
                    }
                    const uint64_t bm = (__ballot(broke) >> gsh) & gmask;
                    const uint32_t tb = bm ? (uint32_t)__builtin_ctzll(bm) : (uint32_t)G;
                    // (a lane at or right of the break started from a sum >= 0, so its m > 0; m <= 1024 * 157 < 2^18)
                    uint32_t key = (t <= tb && pj >= 0) ? ((uint32_t)m << 10) | (uint32_t)(ck * 16 + pj - (int32_t)sh) : 0u;
#pragma unroll
                    for (int d = 1; d < G; d <<= 1) key = max(key, (uint32_t)__shfl_xor((int)key, d, 64));
                    if ((int32_t)(key >> 10) > best) {
                        best = (int32_t)(key >> 10);
                        stop = key & 1023u;
                    }
                    done = bm != 0;
                    carry = __shfl(incl, (int)(gsh + G - 1), 64);
                }
                res = stop;
                if (fq && (stop < L || stats)) {
                    // Q < L iff a '\n' lies among the L bytes: seen in the visited chunks, or in the ones left of them
                    bool any = (__ballot(nl) >> gsh) & gmask;
                    for (int32_t c1 = c0; c1 >= 0 && !any; c1 -= G) {      // (c0 = the first chunk not visited)
                        const int32_t ck = c1 - (int32_t)t;
                        bool f = false;
                        if (ck >= 0) {
                            uint32_t w[4];
                            load_chunk(a, (uint32_t)ck, sh, lastc, L, cb4, w);
                            f = has_nl(w);
                        }
                        any = (__ballot(f) >> gsh) & gmask;
                    }
                    if (any) {
                        res = L;
                        noqual = true;
                    }
                }
            }
        }
        if (live && t == 0) {
            out[i] = res;
            if (res < L) {
                ++nshort;
                nremoved += L - res;
            }
            nnoqual += noqual;
        }
    }
    if (stats) {           // (the same in every thread)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            nshort += __shfl_xor(nshort, d, 64);
            nremoved += __shfl_xor(nremoved, d, 64);
            nnoqual += __shfl_xor(nnoqual, d, 64);
        }
        if ((threadIdx.x & 63u) == 0) {
            red[0][threadIdx.x >> 6] = nshort;
            red[1][threadIdx.x >> 6] = nremoved;
            red[2][threadIdx.x >> 6] = nnoqual;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            unsigned long long v = 0;
            for (int k = 0; k < kQtThreads / 64; ++k) v += red[threadIdx.x][k];
            if (v) atomicAdd(stats + threadIdx.x, v);
        }
    }
}

template <int G>
int qtrim_launch(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offs, const uint32_t* d_lens, uint64_t m,
                 const uint8_t* d_qual, const uint64_t* d_qoffs, uint32_t cb, uint32_t* d_out, uint64_t* d_stats,
                 hipStream_t s) {
    constexpr uint64_t kGroups = kQtThreads / G;
    const uint64_t blocks = (m + kGroups - 1) / kGroups;
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks, 256 * 8);
    const uint32_t iters = (uint32_t)((blocks + grid - 1) / grid);
    hipLaunchKernelGGL((k_trim_quality3<G>), dim3(grid), dim3(kQtThreads), 0, s, d_blob, nbytes, d_offs, d_lens, m, d_qual,
                       d_qoffs, cb, d_out, (unsigned long long*)d_stats, iters);
    return ss_check(hipGetLastError(), "k_trim_quality3");
}

const char* qtrim_check(const void* blob, const void* offs, const void* lens, const void* out, uint64_t n, const void* qual,
                        const void* qoffs, uint32_t cutoff, uint32_t base) {
    if (cutoff == 0 || cutoff > ssh::kQtrimMaxCutoff) return "quality trim: cutoff in 1 .. 93";
    if (base != 33 && base != 64) return "quality trim: base of 33 or 64";
    if (qoffs && !qual) return "quality trim: quality offsets without quality bytes";
    if (n >= (1ull << 32)) return "quality trim: n < 2^32";
    if (n && (!offs || !lens || !out || (!qoffs && !blob))) return "quality trim: null buffer";
    return nullptr;
}

}  // namespace

extern "C" {

// The entry behind ss_trim_quality3 / _ex with the lane group open (tools/probe_qtrim.py): group = lanes
// per read (1, 2, 4, 8, 16; 0 = the library's).
int ss_trim_quality3_shape(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                           uint64_t n, const uint8_t* d_qual, const uint64_t* d_qoffsets, uint32_t cutoff, uint32_t base,
                           uint32_t* d_out_lens, uint64_t* d_stats, uint64_t reads_per_launch, uint32_t group, void* stream) {
    if (const char* e = qtrim_check(d_blob, d_offsets, d_lens, d_out_lens, n, d_qual, d_qoffsets, cutoff, base))
        return ss_fail(SS_EARG, e);
    if (group == 0) group = kQtG;
    if (group != 1 && group != 2 && group != 4 && group != 8 && group != 16)
        return ss_fail(SS_EARG, "quality trim: lane group of 1, 2, 4, 8 or 16");
    hipStream_t s = (hipStream_t)stream;
    int rc = SS_OK;
    if (d_stats) rc = ss_check(hipMemsetAsync(d_stats, 0, 3 * sizeof(uint64_t), s), "quality trim stats reset");
    if (rc || n == 0) return rc;
    const uint32_t cb = cutoff + base;
    const uint64_t per = reads_per_launch ? std::min(reads_per_launch, kQtReadsPerLaunch) : kQtReadsPerLaunch;
    for (uint64_t i0 = 0; i0 < n && !rc; i0 += per) {
        const uint64_t m = std::min(per, n - i0);
        const uint64_t* o = d_offsets + i0;
        const uint32_t* l = d_lens + i0;
        const uint64_t* qo = d_qoffsets ? d_qoffsets + i0 : nullptr;
        uint32_t* d = d_out_lens + i0;
        if (group == 1) rc = qtrim_launch<1>(d_blob, nbytes, o, l, m, d_qual, qo, cb, d, d_stats, s);
        else if (group == 2) rc = qtrim_launch<2>(d_blob, nbytes, o, l, m, d_qual, qo, cb, d, d_stats, s);
        else if (group == 4) rc = qtrim_launch<4>(d_blob, nbytes, o, l, m, d_qual, qo, cb, d, d_stats, s);
        else if (group == 8) rc = qtrim_launch<8>(d_blob, nbytes, o, l, m, d_qual, qo, cb, d, d_stats, s);
        else rc = qtrim_launch<16>(d_blob, nbytes, o, l, m, d_qual, qo, cb, d, d_stats, s);
    }
    return rc;
}

int ss_trim_quality3_ex(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                        uint64_t n, const uint8_t* d_qual, const uint64_t* d_qoffsets, uint32_t cutoff, uint32_t base,
                        uint32_t* d_out_lens, uint64_t* d_stats, uint64_t reads_per_launch, void* stream) {
    return ss_trim_quality3_shape(d_blob, nbytes, d_offsets, d_lens, n, d_qual, d_qoffsets, cutoff, base, d_out_lens,
                                  d_stats, reads_per_launch, 0, stream);
}

int ss_trim_quality3(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens, uint64_t n,
                     const uint8_t* d_qual, const uint64_t* d_qoffsets, uint32_t cutoff, uint32_t base, uint32_t* d_out_lens,
                     uint64_t* d_stats, void* stream) {
    return ss_trim_quality3_ex(d_blob, nbytes, d_offsets, d_lens, n, d_qual, d_qoffsets, cutoff, base, d_out_lens, d_stats,
                               0, stream);
}

int ss_host_trim_quality3(const uint8_t* h_blob, uint64_t nbytes, const uint64_t* h_offsets, const uint32_t* h_lens,
                          uint64_t n, const uint8_t* h_qual, uint64_t qbytes, const uint64_t* h_qoffsets, uint32_t cutoff,
                          uint32_t base, uint32_t* h_out_lens, uint64_t* h_stats) {
    if (const char* e = qtrim_check(h_blob, h_offsets, h_lens, h_out_lens, n, h_qual, h_qoffsets, cutoff, base))
        return ss_fail(SS_EARG, e);
    for (uint64_t i = 0; i < n; ++i) {
        if (h_lens[i] > SS_MAX_NT) continue;
        if (h_offsets[i] > nbytes || h_lens[i] > nbytes - h_offsets[i])
            return ss_fail(SS_EARG, "quality trim: a read ends past the blob");
        if (h_qoffsets && (h_qoffsets[i] > qbytes || h_lens[i] > qbytes - h_qoffsets[i]))
            return ss_fail(SS_EARG, "quality trim: a quality run ends past the quality bytes");
    }
    uint64_t nshort = 0, nremoved = 0, nnoqual = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t L = h_lens[i];
        uint32_t k = L;
        if (L != 0 && L <= SS_MAX_NT) {
            bool usable = true;
            if (h_qoffsets) k = ssh::qtrim_read(h_qual + h_qoffsets[i], L, cutoff, base);
            else k = ssh::qtrim_read_fastq(h_blob, nbytes, h_offsets[i], L, cutoff, base, &usable);
            nnoqual += !usable;
        }
        h_out_lens[i] = k;
        if (k < L) {
            ++nshort;
            nremoved += L - k;
        }
    }
    if (h_stats) {
        h_stats[0] = nshort;
        h_stats[1] = nremoved;
        h_stats[2] = nnoqual;
    }
    return SS_OK;
}

}  // extern "C"
