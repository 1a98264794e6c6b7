// ss_grouped.hip — all-pairs thresholded hamming restricted to groups (UMI dedup per cell x gene or
// per mapping position): the rows arrive sorted by group, group g is rows [off[g], off[g + 1]), and
// only pairs inside one group are compared.  Distance, counts, pair list and total are those of
// ss_hamming_all_pairs (ss_allpairs.hip); indices are global rows, so ss_cluster_pairs runs on the
// result as it stands.
//
// The all-pairs tile kernels launch one block per pair of tiles; with 10^5 - 10^7 groups of a few rows
// almost every tile pair is empty.  Here the grid is one block per ROW tile of kGpTile = 256 consecutive
// rows of the batch, whatever the groups are.  Lane t owns row i = 256 b + t: its bit planes live in
// registers (the bit-plane form of k_allpairs: per word lo_a ^ lo_b, hi_a ^ hi_b, OR, v_bcnt), and it
// knows end_i, the end of its group, from one binary search over the offsets (L2-resident: the lanes
// of a wave walk the same upper levels).  Partners of row i are the rows (i, end_i): they start inside
// the tile, so the block walks column chunks of C rows from its own tile's first row up to its
// largest end, each chunk's planes staged in LDS and read with broadcast reads; a hit is
// d <= k && j > i && j < end_i.  The column loop is bounded per wave, [wave's first row + 1, the wave's
// largest end): a wave of tiny groups runs ~64 + g columns, not 256, and a tile whose groups all end
// inside it (the common case) stages one chunk.  A group that spans t tiles costs t (t + 1) / 2 chunk
// walks in all: the VALU all-pairs tiles' work, no MFMA -- ss_hamming_all_pairs is the tool for one group
// of 10^5 rows ("Grouped all-pairs").  Hits leave the loop through a wave ballot: row
// counts stay in registers, column counts go to LDS, pairs gather in the waves' LDS buffers
// (WaveHits, ss_hamming.h) and are appended with one global atomic per block.
//
// Malformed offsets are not detected on the device, but nothing depends on them for memory safety:
// the search reads off[1 .. ngroups] only, every end is clamped to n, end <= i means "no partners",
// and a written index is a row index i < n or a column j < end <= n.
#include <algorithm>

#include "ss_hamming.h"
#include "ss_internal.h"
#include "host_codec.h"   // after the public header (it declares ss_err only without it)

namespace {

using namespace ssd;

constexpr int kGpTile = 256;                              // rows per block = threads per block
constexpr uint64_t kGpMaxTilesPerLaunch = 1ull << 23;     // a launch's work-item count must fit 32 bits

struct GpArgs {
    const uint64_t* words;
    const uint32_t* off;    // ngroups + 1 offsets
    uint64_t n, ngroups;
    uint64_t tile0;         // first row tile of this launch
    uint32_t wpr, W, k;
    uint32_t* counts;       // nullable
    uint32_t* pairs;        // nullable
    uint64_t max_pairs;
    unsigned long long* npairs;
};

// End of row i's group: off[g + 1] of the first g with off[g + 1] > i, clamped to n; 0 ("no partners")
// when no offset lies above i.  Reads off[1 .. ngroups] only, whatever the offsets hold.
__device__ __forceinline__ uint32_t gp_row_end(const GpArgs& a, uint32_t i) {
    uint64_t lo = 0, hi = a.ngroups;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a.off[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= a.ngroups) return 0u;
    const uint32_t e = a.off[lo + 1];
    return (uint64_t)e < a.n ? e : (uint32_t)a.n;
}

template <int WT>
__global__ __launch_bounds__(256) void k_gp_pairs(GpArgs a) {
    constexpr int C = WT <= 8 ? kGpTile : 2048 / WT;     // columns per LDS chunk (<= 16 KiB of planes)
    // columns per step of the inner loop (chosen from the ISA: one column per step waits for its LDS
    // read before every compare; not measured against it)
    constexpr int U = WT <= 2 ? 4 : (WT <= 8 ? 2 : 1);
    __shared__ uint2 pl[C * WT];                          // {lo, hi} planes per column word
    __shared__ uint32_t colcnt[C];
    __shared__ uint2 pbuf[4][kPairBuf];                   // the waves' pair buffers (WaveHits)
    __shared__ uint32_t s_wend[4], s_fill[4];
    __shared__ unsigned long long blkhits, s_base;        // count-only calls: the block's hits
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t row0 = (a.tile0 + blockIdx.x) * kGpTile;
    const uint64_t i = row0 + threadIdx.x;
    uint32_t end = i < a.n ? gp_row_end(a, (uint32_t)i) : 0u;
    if ((uint64_t)end <= i) end = 0u;                     // (also every lane past the batch)
    const uint32_t span = end ? end - (uint32_t)i - 1u : 0u;   // partners: the span rows after i
    uint32_t alo[WT], ahi[WT];
    load_planes<WT>(a.words, a.n, a.wpr, a.W, i, alo, ahi);
    // the wave's and the block's last partner row + 1 (ends are nondecreasing in i for well-formed
    // offsets; the maximum is right for any)
    uint32_t wend = end;
    for (int o = 32; o; o >>= 1) wend = max(wend, (uint32_t)__shfl_xor((int)wend, o));
    wend = (uint32_t)__builtin_amdgcn_readfirstlane((int)wend);
    if (lane == 0) s_wend[wave] = wend;
    if (threadIdx.x == 0) blkhits = 0;
    __syncthreads();
    const uint64_t bend = max(max(s_wend[0], s_wend[1]), max(s_wend[2], s_wend[3]));
    const uint64_t wfirst = row0 + 64u * wave + 1u;       // the first column a lane of this wave can pair with
    uint32_t rowcnt = 0;
    WaveHits wh;
    wh.buf = pbuf[wave];
    for (uint64_t j0 = row0; j0 < bend; j0 += C) {
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            uint32_t lo[WT], hi[WT];
            load_planes<WT>(a.words, a.n, a.wpr, a.W, j0 + c, lo, hi);
#pragma unroll
            for (int w = 0; w < WT; ++w) pl[c * WT + w] = make_uint2(lo[w], hi[w]);
            colcnt[c] = 0;
        }
        __syncthreads();
        // this wave's columns of the chunk: wave-uniform bounds (wend <= n, so every column is a row)
        const uint64_t jlo = max(j0, wfirst), jhi = min(j0 + C, (uint64_t)wend);
        const uint32_t c_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(jlo - j0)) & ~(uint32_t)(U - 1);
        const uint32_t c_hi = jhi > jlo ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(jhi - j0)) : c_lo;
        // column c is a partner of this lane's row iff i < j0 + c < end: one unsigned compare of
        // c - rel against span (mod 2^32: a column at or below i wraps far above any span, n < 2^32)
        const uint32_t rel = (uint32_t)(i + 1 - j0);
        // U columns per step (U divides C and c is a multiple of U, so c + u < C): their LDS reads are in
        // flight together and one ballot tests them all.  The columns a step adds below jlo or at and
        // past jhi are partners of no lane of this wave.
        for (uint32_t c = c_lo; c < c_hi; c += U) {
            uint32_t d[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = 0;
#pragma unroll
                for (int w = 0; w < WT; ++w) {
                    const uint2 p = pl[(c + u) * WT + w];
                    d[u] += __popc((alo[w] ^ p.x) | (ahi[w] ^ p.y));
                }
            }
            bool hit[U], any = false;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                hit[u] = d[u] <= a.k && c + u - rel < span;
                any |= hit[u];
            }
            if (!__ballot(any)) continue;
#pragma unroll
            for (int u = 0; u < U; ++u) {                 // rare: row and column count, pair output
                const uint64_t mask = __ballot(hit[u]);
                if (!mask) continue;
                rowcnt += hit[u] ? 1u : 0u;
                if (hit[u] && a.counts) atomicAdd(&colcnt[c + u], 1u);
                hits_add(a, wh, hit[u], mask, (uint32_t)i, (uint32_t)(j0 + c + u));
            }
        }
        __syncthreads();
        if (a.counts) {
            for (int c = threadIdx.x; c < C; c += 256)
                if (colcnt[c]) atomicAdd(&a.counts[j0 + c], colcnt[c]);   // (a counted column is a row < n)
        }
    }
    // what the waves' buffers still hold (a full buffer left on its own: hits_add) and the count-only
    // hits leave with ONE atomic on the pair counter per block: with a hit in every fourth row, one per
    // wave and hit column made the whole call wait on that single address
    if (lane == 0) {
        s_fill[wave] = wh.fill;
        if (wh.nh) atomicAdd(&blkhits, (unsigned long long)wh.nh);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long add = blkhits + s_fill[0] + s_fill[1] + s_fill[2] + s_fill[3];
        s_base = add ? atomicAdd(a.npairs, add) : 0ull;
    }
    __syncthreads();
    if (wh.fill) {
        uint64_t base = s_base;
        for (uint32_t w = 0; w < wave; ++w) base += s_fill[w];
        for (uint32_t e = lane; e < wh.fill; e += 64) {
            const uint64_t slot = base + e;
            if (slot < a.max_pairs) {
                const uint2 pr = wh.buf[e];
                a.pairs[2 * slot] = pr.x;
                a.pairs[2 * slot + 1] = pr.y;
            }
        }
    }
    if (a.counts && rowcnt) atomicAdd(&a.counts[i], rowcnt);              // (rowcnt != 0 only for i < n)
}

const char* gp_check(uint64_t n, uint64_t ngroups, uint32_t L, uint32_t wpr) {
    if (L < 1 || L > SS_MAX_NT) return "grouped all-pairs: L must be 1 .. 1024";
    if (wpr < ham_shape(L).W) return "grouped all-pairs: wpr below the words of L";
    if (n >= (1ull << 32)) return "grouped all-pairs: n must be < 2^32";
    if (n && !ngroups) return "grouped all-pairs: rows without a group";
    return nullptr;
}

}  // namespace

extern "C" {

uint64_t ss_hamming_all_pairs_grouped_ws_bytes(uint64_t, uint64_t, uint32_t) { return 0; }

int ss_hamming_all_pairs_grouped_ex(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                                    const uint32_t* d_group_offsets, uint64_t ngroups, uint32_t* d_counts,
                                    uint32_t* d_pairs, uint64_t max_pairs, uint64_t* d_npairs, void* d_ws,
                                    uint64_t ws_bytes, uint64_t tiles_per_launch, void* stream) {
    (void)d_ws;
    (void)ws_bytes;                                       // no workspace: 0 bytes are always enough
    if (const char* e = gp_check(n, ngroups, L, wpr)) return ss_fail(SS_EARG, e);
    if (n && (!d_words || !d_group_offsets || !d_npairs)) return ss_fail(SS_EARG, "grouped all-pairs: null buffer");
    hipStream_t s = (hipStream_t)stream;
    int rc = SS_OK;
    if (d_npairs) rc = ss_check(hipMemsetAsync(d_npairs, 0, sizeof(uint64_t), s), "npairs reset");
    if (!rc && d_counts && n) rc = ss_check(hipMemsetAsync(d_counts, 0, n * sizeof(uint32_t), s), "counts reset");
    if (rc || n < 2) return rc;
    GpArgs a{};
    a.words = d_words;
    a.off = d_group_offsets;
    a.n = n;
    a.ngroups = ngroups;
    a.wpr = wpr;
    a.W = ham_shape(L).W;
    a.k = max_dist;
    a.counts = d_counts;
    a.pairs = max_pairs ? d_pairs : nullptr;
    a.max_pairs = a.pairs ? max_pairs : 0;
    a.npairs = (unsigned long long*)d_npairs;
    const uint64_t tiles = (n + kGpTile - 1) / kGpTile;
    const uint64_t per = tiles_per_launch ? std::min(tiles_per_launch, kGpMaxTilesPerLaunch) : kGpMaxTilesPerLaunch;
    for (uint64_t t0 = 0; t0 < tiles; t0 += per) {
        a.tile0 = t0;
        const dim3 grid((unsigned)std::min(per, tiles - t0));
        if (a.W <= 1) hipLaunchKernelGGL(k_gp_pairs<1>, grid, dim3(256), 0, s, a);
        else if (a.W <= 2) hipLaunchKernelGGL(k_gp_pairs<2>, grid, dim3(256), 0, s, a);
        else if (a.W <= 4) hipLaunchKernelGGL(k_gp_pairs<4>, grid, dim3(256), 0, s, a);
        else if (a.W <= 8) hipLaunchKernelGGL(k_gp_pairs<8>, grid, dim3(256), 0, s, a);
        else if (a.W <= 16) hipLaunchKernelGGL(k_gp_pairs<16>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_gp_pairs<32>, grid, dim3(256), 0, s, a);
        rc = ss_check(hipGetLastError(), "k_gp_pairs");
        if (rc) return rc;
    }
    return SS_OK;
}

int ss_hamming_all_pairs_grouped(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                                 const uint32_t* d_group_offsets, uint64_t ngroups, uint32_t* d_counts,
                                 uint32_t* d_pairs, uint64_t max_pairs, uint64_t* d_npairs, void* d_ws, uint64_t ws_bytes,
                                 void* stream) {
    return ss_hamming_all_pairs_grouped_ex(d_words, n, L, wpr, max_dist, d_group_offsets, ngroups, d_counts, d_pairs,
                                           max_pairs, d_npairs, d_ws, ws_bytes, 0, stream);
}

int ss_host_hamming_all_pairs_grouped(const uint64_t* h_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                                      const uint32_t* h_group_offsets, uint64_t ngroups, uint32_t* h_counts,
                                      uint32_t* h_pairs, uint64_t max_pairs, uint64_t* h_npairs) {
    if (const char* e = gp_check(n, ngroups, L, wpr)) return ss_fail(SS_EARG, e);
    if (n && (!h_words || !h_group_offsets || !h_npairs)) return ss_fail(SS_EARG, "grouped all-pairs: null buffer");
    if (ngroups) {
        if (!h_group_offsets) return ss_fail(SS_EARG, "grouped all-pairs: null buffer");
        bool ok = h_group_offsets[0] == 0 && h_group_offsets[ngroups] == n;
        for (uint64_t g = 0; ok && g < ngroups; ++g) ok = h_group_offsets[g] <= h_group_offsets[g + 1];
        if (!ok) return ss_fail(SS_EARG, "grouped all-pairs: offsets must start at 0, not decrease, and end at n");
    }
    if (h_npairs) *h_npairs = 0;
    if (h_counts) std::fill(h_counts, h_counts + n, 0u);
    if (n < 2) return SS_OK;
    if (!max_pairs) h_pairs = nullptr;
    uint64_t total = 0;
    for (uint64_t g = 0; g < ngroups; ++g) {
        const uint64_t beg = h_group_offsets[g], end = h_group_offsets[g + 1];
        for (uint64_t i = beg; i + 1 < end; ++i) {
            for (uint64_t j = i + 1; j < end; ++j) {
                if (ssh::hamming(h_words + i * wpr, h_words + j * wpr, L) > max_dist) continue;
                if (h_counts) {
                    ++h_counts[i];
                    ++h_counts[j];
                }
                if (h_pairs && total < max_pairs) {
                    h_pairs[2 * total] = (uint32_t)i;
                    h_pairs[2 * total + 1] = (uint32_t)j;
                }
                ++total;
            }
        }
    }
    *h_npairs = total;
    return SS_OK;
}

}  // extern "C"
