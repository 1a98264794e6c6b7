// ss_trim.hip — 3' adapter trim of a ragged batch: d_out_lens[i] = the least position of read i at
// which the adapter matches (include/shortseq_amd.h, "3' adapter trim"; the rule on one read is
// csrc/host_trim.h), or the read's length.  No read is moved: every later phase of the engine works
// from (d_offsets, d_lens), so lowering a length is the whole trim.
//
// k_trim_adapter3<G, STAGED>: a group of G lanes per read, 256 / G reads per block.
//   - The adapter (8 words) and its compare mask (one bit per adapter byte, 0 for 'N' and past A)
//     arrive by value in the kernel arguments; each thread expands the mask to the 0x80-per-byte form
//     once (uniform, scalar registers).
//   - STAGED: the group copies the read's 16-B aligned chunks into its own LDS region, one window of
//     kWin positions (22 chunks: the window, the 15 bytes of misalignment, 63 bytes of adapter
//     overhang and the funnel's look-ahead) at a time: a read of up to 256 bytes is one window.
//     Chunks past the one holding the read's last byte are never loaded (the blob must be readable to
//     the end of its last 16-B chunk, as for ss_encode_var).  !STAGED (kept for the probe,
//     tools/probe_trim.py): the lanes read aligned dwords of those same chunks straight from global
//     memory through the vector L1, the index clamped to the read's last chunk.
//   - Lane t takes positions t, t + G, ... of the window.  One position is up to 8 SWAR steps over 8
//     bytes: three aligned dwords realigned by v_alignbyte, xor the adapter word, nonzero-byte mask,
//     and with the compare and overlap masks, popcount; the position is dropped as soon as its
//     mismatches pass the budget (random sequence: after the first step).  The group walks the window
//     in rounds of G consecutive positions; after a round the lowest matching lane of the group's part
//     of the wave ballot is the least matching position (one v_cmp into a scalar pair, no shuffle
//     chain), every lane of the group knows it, and the group stops: nothing right of the adapter's
//     start is looked at.  (A lane stopping at its own first match with a shuffle minimum at the end
//     measured 7-10 % slower on adapter-bearing reads and 3-8 % faster on reads without the adapter:
//     profiles/trim/README.md.)  Lane 0 stores.
//   - The budget ov / err_div is (ov * M) >> 24 with M = ceil(2^24 / err_div): exact for ov <= 64
//     (the error term ov * (M * err_div - 2^24) * err_div < 2^18); err_div of 0 or past 64 gives 0.
//   - Grid-stride over the reads with one trip count for every thread (the ballots need whole groups).
//   - Reads of more than SS_MAX_NT bytes (0xFFFFFFFF included) and reads shorter than min_overlap
//     leave with their length; nothing of them is read.
//   - d_stats: per-lane sums, reduced per wave by shuffles and per block through LDS, then two 64-bit
//     atomic adds per block.
// d_out_lens may be d_lens: a read's length is loaded by its own group before that group's one store.
#include <algorithm>

#include "ss_device.h"
#include "ss_internal.h"
#include "host_trim.h"

namespace {

using namespace ssd;

constexpr int kTrimThreads = 256;
constexpr uint32_t kWin = 256;                     // positions per staged window
constexpr uint32_t kRegionChunks = 22;             // 16-B chunks of one group's LDS region (352 B)
constexpr uint64_t kTrimReadsPerLaunch = 1ull << 28;
constexpr int kTrimG = 4;                          // the library's lane group (profiles/trim/README.md)
constexpr bool kTrimStaged = true;

struct TrimArgs {
    uint64_t w[8];            // adapter bytes, little-endian, zero past A
    uint64_t cmp;             // bit k: adapter byte k is compared (k < A, not 'N')
    uint32_t A, min_overlap, budget_mul;
};

// LDS writes of this wave's lanes are visible to its other lanes after this (and the reads before it
// are done before the writes after it): the groups never span waves, so no block barrier is needed
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Does the adapter match at the position whose first byte is byte `rel` of d32 (aligned dwords)?
// ov = compared bytes (1..64); lim = the last dword index that may be read (CLAMP).
template <bool CLAMP, typename P>
__device__ __forceinline__ bool trim_match(P d32, uint32_t rel, uint32_t ov, uint32_t lim, const uint64_t (&w)[8],
                                           const uint64_t (&c80)[8], uint32_t budget) {
    const uint32_t i = rel >> 2, sb = rel & 3u;
    uint32_t lo = d32[CLAMP ? min(i, lim) : i];
    uint32_t mm = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        if (8 * j >= ov) break;
        const uint32_t i1 = i + 2 * j + 1, i2 = i + 2 * j + 2;
        const uint32_t mid = d32[CLAMP ? min(i1, lim) : i1], hi = d32[CLAMP ? min(i2, lim) : i2];
        const uint64_t x = (((uint64_t)__builtin_amdgcn_alignbyte(hi, mid, sb) << 32) |
                            __builtin_amdgcn_alignbyte(mid, lo, sb)) ^ w[j];
        uint64_t nz = ssh::trim_nonzero_bytes(x) & c80[j];
        const uint32_t nb = ov - 8 * j;                  // compared bytes left, this word's included
        if (nb < 8) nz &= (1ull << (8 * nb)) - 1;
        mm += __popcll(nz);
        if (mm > budget) return false;
        lo = hi;
    }
    return true;
}

template <int G, bool STAGED>
__global__ __launch_bounds__(kTrimThreads) void k_trim_adapter3(const uint8_t* blob, const uint64_t* __restrict__ offs,
                                                                const uint32_t* lens, uint64_t n, TrimArgs a,
                                                                uint32_t* out, unsigned long long* stats, uint32_t iters) {
    constexpr int kGroups = kTrimThreads / G;
    __shared__ uint4 region[STAGED ? kGroups * kRegionChunks : 1];
    __shared__ unsigned long long red[2][kTrimThreads / 64];
    const uint32_t t = threadIdx.x % G, grp = threadIdx.x / G;
    uint64_t c80[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint64_t bits = (a.cmp >> (8 * j)) & 0xFFull;
        c80[j] = (((bits * 0x0101010101010101ull) & 0x8040201008040201ull) + 0x7F7F7F7F7F7F7F7Full) & 0x8080808080808080ull;
    }
    unsigned long long nshort = 0, nremoved = 0;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint64_t i = ((uint64_t)it * gridDim.x + blockIdx.x) * kGroups + grp;
        const bool live = i < n;
        const uint32_t L = live ? lens[i] : 0u;
        uint32_t best = L;
        // (the same in every lane of a group; an adapter shorter than min_overlap never has enough overlap)
        if (live && L <= SS_MAX_NT && L >= a.min_overlap && a.A >= a.min_overlap) {
            const uintptr_t addr = (uintptr_t)blob + offs[i];
            const uint4* q = (const uint4*)(addr & ~(uintptr_t)15);
            const uint32_t sh = (uint32_t)(addr & 15);
            const uint32_t lastc = (sh + L - 1u) >> 4;                // the chunk holding the read's last byte
            const uint32_t pmax = L - a.min_overlap;                  // the last position with enough overlap
            // a round = G consecutive positions, one per lane; the first lane of the group's ballot that
            // matched is the least matching position, and the group (every lane alike) stops there
            const uint32_t gsh = threadIdx.x & 63u & ~(uint32_t)(G - 1);
            const uint64_t gmask = G == 64 ? ~0ull : (1ull << G) - 1;
            if (STAGED) {
                uint4* reg = region + grp * kRegionChunks;
                const uint32_t* reg32 = (const uint32_t*)reg;
                for (uint32_t w0 = 0; w0 <= pmax && best == L; w0 += kWin) {
                    wave_lds_sync();
                    const uint32_t nch = min(kRegionChunks, lastc - (w0 >> 4) + 1u);
                    for (uint32_t k = t; k < nch; k += G) reg[k] = ld_stream(q + (w0 >> 4) + k);
                    wave_lds_sync();
                    const uint32_t pend = min(pmax, w0 + kWin - 1u);
                    for (uint32_t p0 = w0; p0 <= pend && best == L; p0 += G) {
                        const uint32_t p = p0 + t, ov = min(a.A, L - min(p, pend));
                        const bool hit = p <= pend &&
                                         trim_match<false>(reg32, sh + p - w0, ov, 0u, a.w, c80, (ov * a.budget_mul) >> 24);
                        const uint64_t m = (__ballot(hit) >> gsh) & gmask;
                        if (m) best = p0 + (uint32_t)__builtin_ctzll(m);
                    }
                }
            } else {
                const uint32_t* q32 = (const uint32_t*)q;
                for (uint32_t p0 = 0; p0 <= pmax && best == L; p0 += G) {
                    const uint32_t p = p0 + t, ov = min(a.A, L - min(p, pmax));
                    const bool hit = p <= pmax &&
                                     trim_match<true>(q32, sh + p, ov, 4u * lastc + 3u, a.w, c80, (ov * a.budget_mul) >> 24);
                    const uint64_t m = (__ballot(hit) >> gsh) & gmask;
                    if (m) best = p0 + (uint32_t)__builtin_ctzll(m);
                }
            }
        }
        if (live && t == 0) {
            out[i] = best;
            if (best < L) {
                ++nshort;
                nremoved += L - best;
            }
        }
    }
    if (stats) {           // (the same in every thread)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            nshort += __shfl_xor(nshort, d, 64);
            nremoved += __shfl_xor(nremoved, d, 64);
        }
        if ((threadIdx.x & 63u) == 0) {
            red[0][threadIdx.x >> 6] = nshort;
            red[1][threadIdx.x >> 6] = nremoved;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            unsigned long long v = 0;
            for (int k = 0; k < kTrimThreads / 64; ++k) v += red[threadIdx.x][k];
            if (v) atomicAdd(stats + threadIdx.x, v);
        }
    }
}

template <int G, bool STAGED>
int trim_launch(const uint8_t* d_blob, const uint64_t* d_offs, const uint32_t* d_lens, uint64_t m, const TrimArgs& a,
                uint32_t* d_out, uint64_t* d_stats, hipStream_t s) {
    constexpr uint64_t kGroups = kTrimThreads / G;
    const uint64_t blocks = (m + kGroups - 1) / kGroups;
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks, 256 * 8);
    const uint32_t iters = (uint32_t)((blocks + grid - 1) / grid);
    hipLaunchKernelGGL((k_trim_adapter3<G, STAGED>), dim3(grid), dim3(kTrimThreads), 0, s, d_blob, d_offs, d_lens, m, a,
                       d_out, (unsigned long long*)d_stats, iters);
    return ss_check(hipGetLastError(), "k_trim_adapter3");
}

const char* trim_check(const void* blob, const void* offs, const void* lens, const void* out, uint64_t n,
                       const uint8_t* adapter, uint32_t A, uint32_t min_overlap) {
    if (A == 0 || A > ssh::kTrimMaxAdapter) return "trim: adapter length in 1 .. 64";
    if (min_overlap == 0) return "trim: min_overlap >= 1";
    if (n >= (1ull << 32)) return "trim: n < 2^32";
    if (n && (!adapter || !blob || !offs || !lens || !out)) return "trim: null buffer";
    return nullptr;
}

}  // namespace

extern "C" {

// The entry behind ss_trim_adapter3 / _ex with the kernel's shape open (tools/probe_trim.py): group =
// lanes per read (2, 4, 8, 16, 32; 0 = the library's), staged = 1 LDS staging, 0 direct aligned loads, < 0
// the library's.
int ss_trim_adapter3_shape(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                           uint64_t n, const uint8_t* h_adapter, uint32_t A, uint32_t min_overlap, uint32_t err_div,
                           uint32_t* d_out_lens, uint64_t* d_stats, uint64_t reads_per_launch, uint32_t group, int staged,
                           void* stream) {
    (void)nbytes;              // trusted, as ss_encode_var trusts its offsets
    if (const char* e = trim_check(d_blob, d_offsets, d_lens, d_out_lens, n, h_adapter, A, min_overlap))
        return ss_fail(SS_EARG, e);
    if (group == 0) group = kTrimG;
    const bool st = staged < 0 ? kTrimStaged : staged != 0;
    if (group != 2 && group != 4 && group != 8 && group != 16 && group != 32)
        return ss_fail(SS_EARG, "trim: lane group of 2, 4, 8, 16 or 32");
    hipStream_t s = (hipStream_t)stream;
    int rc = SS_OK;
    if (d_stats) rc = ss_check(hipMemsetAsync(d_stats, 0, 2 * sizeof(uint64_t), s), "trim stats reset");
    if (rc || n == 0) return rc;
    ssh::TrimAdapter t;
    ssh::trim_prepare(&t, h_adapter, A, min_overlap, err_div);
    TrimArgs a;
    for (int j = 0; j < 8; ++j) a.w[j] = t.w[j];
    a.cmp = t.cmp;
    a.A = A;
    a.min_overlap = min_overlap;
    a.budget_mul = (err_div == 0 || err_div > 64) ? 0u : (uint32_t)(((1u << 24) + err_div - 1) / err_div);
    const uint64_t per = reads_per_launch ? std::min(reads_per_launch, kTrimReadsPerLaunch) : kTrimReadsPerLaunch;
    for (uint64_t i0 = 0; i0 < n && !rc; i0 += per) {
        const uint64_t m = std::min(per, n - i0);
        const uint64_t* o = d_offsets + i0;
        const uint32_t* l = d_lens + i0;
        uint32_t* d = d_out_lens + i0;
        if (group == 2) rc = st ? trim_launch<2, true>(d_blob, o, l, m, a, d, d_stats, s) : trim_launch<2, false>(d_blob, o, l, m, a, d, d_stats, s);
        else if (group == 4) rc = st ? trim_launch<4, true>(d_blob, o, l, m, a, d, d_stats, s) : trim_launch<4, false>(d_blob, o, l, m, a, d, d_stats, s);
        else if (group == 8) rc = st ? trim_launch<8, true>(d_blob, o, l, m, a, d, d_stats, s) : trim_launch<8, false>(d_blob, o, l, m, a, d, d_stats, s);
        else if (group == 16) rc = st ? trim_launch<16, true>(d_blob, o, l, m, a, d, d_stats, s) : trim_launch<16, false>(d_blob, o, l, m, a, d, d_stats, s);
        else rc = st ? trim_launch<32, true>(d_blob, o, l, m, a, d, d_stats, s) : trim_launch<32, false>(d_blob, o, l, m, a, d, d_stats, s);
    }
    return rc;
}

int ss_trim_adapter3_ex(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                        uint64_t n, const uint8_t* h_adapter, uint32_t A, uint32_t min_overlap, uint32_t err_div,
                        uint32_t* d_out_lens, uint64_t* d_stats, uint64_t reads_per_launch, void* stream) {
    return ss_trim_adapter3_shape(d_blob, nbytes, d_offsets, d_lens, n, h_adapter, A, min_overlap, err_div, d_out_lens,
                                  d_stats, reads_per_launch, 0, -1, stream);
}

int ss_trim_adapter3(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens, uint64_t n,
                     const uint8_t* h_adapter, uint32_t A, uint32_t min_overlap, uint32_t err_div, uint32_t* d_out_lens,
                     uint64_t* d_stats, void* stream) {
    return ss_trim_adapter3_ex(d_blob, nbytes, d_offsets, d_lens, n, h_adapter, A, min_overlap, err_div, d_out_lens,
                               d_stats, 0, stream);
}

int ss_host_trim_adapter3(const uint8_t* h_blob, uint64_t nbytes, const uint64_t* h_offsets, const uint32_t* h_lens,
                          uint64_t n, const uint8_t* h_adapter, uint32_t A, uint32_t min_overlap, uint32_t err_div,
                          uint32_t* h_out_lens, uint64_t* h_stats) {
    if (const char* e = trim_check(h_blob, h_offsets, h_lens, h_out_lens, n, h_adapter, A, min_overlap))
        return ss_fail(SS_EARG, e);
    for (uint64_t i = 0; i < n; ++i)
        if (h_lens[i] <= SS_MAX_NT && (h_offsets[i] > nbytes || h_lens[i] > nbytes - h_offsets[i]))
            return ss_fail(SS_EARG, "trim: a read ends past the blob");
    ssh::TrimAdapter t;
    if (n) ssh::trim_prepare(&t, h_adapter, A, min_overlap, err_div);
    uint64_t nshort = 0, nremoved = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t L = h_lens[i];
        const uint32_t k = L <= SS_MAX_NT ? ssh::trim_read(t, h_blob + h_offsets[i], L) : L;
        h_out_lens[i] = k;
        if (k < L) {
            ++nshort;
            nremoved += L - k;
        }
    }
    if (h_stats) {
        h_stats[0] = nshort;
        h_stats[1] = nremoved;
    }
    return SS_OK;
}

}  // extern "C"
