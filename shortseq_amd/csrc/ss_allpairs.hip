// ss_allpairs.hip — all-pairs thresholded hamming (UMI-style dedup; the reference
// benchmark compares its __xor__ against UMI-tools' edit_distance, benchmark.py:11,153).
//
// Distance = the reference's ShortSeq.__xor__ (short_seq_64.pyx:77-84, short_seq_192.pyx:74-91,
// short_seq_var.pyx:64-81): over W words, popcount(((x >> 1) | x) & 0x5555...), x = a ^ b, i.e. the
// number of nucleotide positions whose 2-bit codes differ.
//
// This is the one compute-bound piece of the path (O(n^2) pairs over O(n) bytes).  Each packed word
// (32 nt) is split once into two bit-planes (lo = even bits, hi = odd bits, 32 bits each), so a
// pair costs, per word: lo_a^lo_b, hi_a^hi_b, OR, v_bcnt (accumulating) — then one compare and
// one add for the row count: ~6 VALU ops per pair per word instead of ~10 on the interleaved form.
// Tiling: a block owns a row tile of S = 256 reads held in registers (one per lane, converted to
// planes on load) and a column tile of S reads, staged through LDS in chunks (planes), read by
// every lane with broadcast LDS reads.  Only tile pairs bj >= bi run (unordered pairs once; the
// diagonal tile masks j <= i).  Hits are rare for UMI thresholds, so they leave the inner loop
// through a wave ballot: row counts stay in registers, column counts go to LDS counters, pairs
// are appended with one global atomic per wave.
#include <mutex>

#include "ss_hamming.h"
#include "ss_internal.h"

namespace {

using namespace ssd;

struct AllPairsArgs {
    const uint64_t* words;
    uint64_t n;
    uint32_t wpr;       // words per read in memory
    uint32_t W;         // words compared (ham_shape(L).W); words W..WT-1 of the template are zero
    uint32_t k;         // max distance
    uint32_t* counts;   // nullable
    uint32_t* pairs;    // nullable: (i, j) u32 pairs
    uint64_t max_pairs;
    unsigned long long* npairs;
};

template <int WT>
struct Tile {
    static constexpr int S = 256;                            // reads per tile: one per lane
    static constexpr int C0 = (WT <= 4) ? 1024 : (4096 / WT);
    static constexpr int C = C0 < S ? C0 : S;               // columns per LDS chunk (divides S)
};

template <int WT>
__global__ __launch_bounds__(256) void k_allpairs(AllPairsArgs a) {
    constexpr int S = Tile<WT>::S, C = Tile<WT>::C;
    const uint32_t bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;                                    // unordered pairs: upper triangle only
    __shared__ uint2 pl[C * WT];                             // {lo, hi} planes per column word
    __shared__ uint32_t colcnt[C];
    __shared__ unsigned long long blkhits;   // count-only calls: the block's hits, one global atomic
    if (threadIdx.x == 0) blkhits = 0;
    const bool diag = bi == bj;
    uint32_t alo[WT], ahi[WT];
    {
        const uint64_t i = (uint64_t)bi * S + threadIdx.x;     // this lane's row
        load_planes<WT>(a.words, a.n, a.wpr, a.W, i, alo, ahi);
    }
    uint32_t rowcnt = 0;
    // WT <= 16: one chunk (C == S), and the loop is unrolled away (a count past the trip count is a
    // full unroll; left to itself the compiler keeps the loop, at 8 .. 12 VGPRs).  WT 32: two chunks, a loop.
    // (The chunk as a lambda under `if constexpr (C == S)`, with i defined once, measured 7 .. 12 % slower
    // at 150, 250 and 1024 nt: profiles/hamming_refactor.)
    constexpr int kChunkUnroll = C == S ? 2 : 1;
#pragma unroll kChunkUnroll
    for (int c0 = 0; c0 < S; c0 += C) {
        const uint64_t j0 = (uint64_t)bj * S + c0;
        if (j0 >= a.n) break;
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            uint32_t lo[WT], hi[WT];
            load_planes<WT>(a.words, a.n, a.wpr, a.W, j0 + c, lo, hi);
#pragma unroll
            for (int w = 0; w < WT; ++w) pl[c * WT + w] = make_uint2(lo[w], hi[w]);
            colcnt[c] = 0;
        }
        __syncthreads();
        const uint32_t ncols = (uint32_t)min<uint64_t>(C, a.n - j0);

        for (uint32_t c = 0; c < ncols; ++c) {
            uint32_t blo[WT], bhi[WT];
#pragma unroll
            for (int w = 0; w < WT; ++w) {
                const uint2 p = pl[c * WT + w];
                blo[w] = p.x;
                bhi[w] = p.y;
            }
            const uint64_t j = j0 + c;
            const uint64_t i = (uint64_t)bi * S + threadIdx.x;
            uint32_t d = 0;
#pragma unroll
            for (int w = 0; w < WT; ++w) d += __popc((alo[w] ^ blo[w]) | (ahi[w] ^ bhi[w]));
            bool hit = d <= a.k && i < a.n;
            if (diag) hit = hit && j > i;
            rowcnt += hit ? 1u : 0u;
            if (__ballot(hit)) {                            // rare: column count + pair output
                if (hit && a.counts) atomicAdd(&colcnt[c], 1u);
                if (a.pairs) {
                    const uint64_t mask = __ballot(hit);
                    const uint32_t lane = threadIdx.x & 63u;
                    const uint32_t rank = __popcll(mask & ((1ull << lane) - 1ull));
                    unsigned long long base = 0;
                    if (lane == (uint32_t)__ffsll((unsigned long long)mask) - 1u)
                        base = atomicAdd(a.npairs, (unsigned long long)__popcll(mask));
                    base = __shfl(base, __ffsll((unsigned long long)mask) - 1);
                    const uint64_t slot = base + rank;
                    if (hit && slot < a.max_pairs) {
                        a.pairs[2 * slot] = (uint32_t)i;
                        a.pairs[2 * slot + 1] = (uint32_t)j;
                    }
                } else {
                    const uint64_t mask = __ballot(hit);   // all lanes, before the leader's branch
                    if ((threadIdx.x & 63u) == (uint32_t)__ffsll((unsigned long long)mask) - 1u)
                        atomicAdd(&blkhits, (unsigned long long)__popcll(mask));
                }
            }
        }
        __syncthreads();
        if (a.counts) {
            for (int c = threadIdx.x; c < (int)ncols; c += 256)
                if (colcnt[c]) atomicAdd(&a.counts[j0 + c], colcnt[c]);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && blkhits) atomicAdd(a.npairs, blkhits);
    const uint64_t i = (uint64_t)bi * S + threadIdx.x;
    if (a.counts && i < a.n && rowcnt) atomicAdd(&a.counts[i], rowcnt);
}

// ------------------------------------------------------------------------------------------------
// MFMA form for one-word reads (L <= 32, the UMI case).  Matching positions are a dot product of
// one-hot codes: position p of a read -> 4 int8 lanes with a 1 at its code, so for reads i, j
// D[i][j] = sum_k A[i][k] B[k][j] = number of positions with equal codes, and distance = P - D.
// P = min(L + 1, 32) positions: positions > L are code 0 in every packed word, position L can
// carry the table-path alias bit, which the reference's whole-word __xor__ counts.
// v_mfma_i32_32x32x32_i8 takes 8 positions per k-step: lane l (r = l & 31, h = l >> 5) holds
// row / column r and positions 8s + 4h + q (q = 0..3) in its 4 VGPRs, VGPR q = 1 << (8 * code);
// D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h (tools/probe_mfma_i8.hip checks the maps).
// Block: 4 waves x RB row blocks of 32 rows = S rows (A fragments in registers), the S columns
// of the paired tile staged in LDS as packed words; per 32-column block each wave builds its B
// fragments once and runs RB x KS MFMAs.  A hit needs D >= P - k; the 16 results of a tile are
// OR-reduced (bits 7-8 after a 128 - thr bias) and tested with one ballot, so the (rare) hit path runs
// only for tiles that have one.
// Rows / columns past n get zero fragments (D = 0); the hit path checks indices.
// Fragments come from a 256-entry LDS table (4 codes of a byte -> the 4 one-hot VGPRs of a k-step
// half, one ds_read_b128), not per-VGPR bit arithmetic (tools/tune_allpairs.hip measured the table
// ahead).  The table, the tile choice and the sweep of a column block are ss_hamming.h's:
// ss_nearest.hip runs the same tiles.
// ------------------------------------------------------------------------------------------------
// Hit path of one 32 x 32 result tile (st = its 16 result registers per lane, [reg][lane], hit =
// result >= 128: bit 7 or 8): index checks, LDS row / column counts, wave-aggregated pair append.
__device__ __noinline__ void ap_hits(const AllPairsArgs& a, const int* st, uint32_t rl0, uint32_t cl, uint64_t row0,
                                     uint64_t col0, bool diag, uint32_t* rowcnt, uint32_t* colcnt,
                                     unsigned long long* blkhits) {
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5;
#pragma unroll 1
    for (int q = 0; q < 16; ++q) {
        const uint32_t rl = rl0 + (q & 3) + 8 * (q >> 2) + 4 * h;
        const uint64_t i = row0 + rl, j = col0 + cl;
        bool hit = (st[q * 64 + lane] & 0x180) && i < a.n && j < a.n;
        if (diag) hit = hit && j > i;
        const uint64_t mask = __ballot(hit);
        if (!mask) continue;
        if (hit && a.counts) {
            atomicAdd(&rowcnt[rl], 1u);
            atomicAdd(&colcnt[cl], 1u);
        }
        const int leader = __ffsll((unsigned long long)mask) - 1;
        if (!a.pairs) {         // count only: the block's LDS total, one global atomic per block
            if ((int)lane == leader) atomicAdd(blkhits, (unsigned long long)__popcll(mask));
            continue;
        }
        unsigned long long base = 0;
        if ((int)lane == leader) base = atomicAdd(a.npairs, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader);
        if (hit) {
            const uint64_t slot = base + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < a.max_pairs) {
                a.pairs[2 * slot] = (uint32_t)i;
                a.pairs[2 * slot + 1] = (uint32_t)j;
            }
        }
    }
}

// Upper-triangle tile pair (bi <= bj) of linear block k over t tiles, row-major: row bi holds
// t - bi pairs.  A float estimate of bi, corrected by integer steps.
__device__ __forceinline__ void tri_pair(uint64_t k, uint64_t t, uint32_t& bi, uint32_t& bj) {
    const double b = 2.0 * (double)t + 1.0;
    int64_t i = (int64_t)((b - sqrt(b * b - 8.0 * (double)k)) / 2.0);
    auto before = [&](int64_t r) { return (uint64_t)(r * (int64_t)t - r * (r - 1) / 2); };   // pairs in rows < r
    if (i < 0) i = 0;
    while (i > 0 && before(i) > k) --i;
    while (before(i + 1) <= k) ++i;
    bi = (uint32_t)i;
    bj = (uint32_t)(i + (int64_t)(k - before(i)));
}

// TRI: the launch may be a 1-D grid over upper-triangle tile pairs (kept out of the RB >= 4
// instantiations: its registers cost them a wave per SIMD)
template <int KS, int RB, bool TRI>
__global__ __launch_bounds__(256) void k_allpairs_mfma(AllPairsArgs a, uint32_t P) {
    using T = MfmaTiles<KS, RB>;
    constexpr int S = T::S, NW = T::NW;
    // one block per upper-triangle tile pair (a 1-D grid while its work-item count fits 32 bits;
    // beyond that the square 2-D grid, lower-triangle blocks exiting at once)
    uint32_t bi = blockIdx.y, bj = blockIdx.x;
    if (TRI && gridDim.y == 1) tri_pair(blockIdx.x, (a.n + S - 1) / S, bi, bj);
    if (bj < bi) return;
    __shared__ uint64_t cw[S * NW];
    __shared__ uint32_t rowcnt[S], colcnt[S];
    __shared__ int stash[4 * 1024];                        // hit path: [wave][result reg][lane]
    __shared__ v4i32 ohtab[256];
    __shared__ unsigned long long blkhits;
    const bool diag = bi == bj;
    if (threadIdx.x == 0) blkhits = 0;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, h = lane >> 5, r = lane & 31u;
    const uint64_t row0 = (uint64_t)bi * S, col0 = (uint64_t)bj * S;
    ohtab[threadIdx.x] = onehot_entry(threadIdx.x);
    for (int c = threadIdx.x; c < S; c += 256) {
        const uint64_t j = col0 + c;
#pragma unroll
        for (int w = 0; w < NW; ++w) cw[c * NW + w] = (j < a.n && (uint32_t)w < a.W) ? a.words[j * a.wpr + w] : 0ull;
        rowcnt[c] = 0;
        colcnt[c] = 0;
    }
    __syncthreads();                                       // the table
    v4i32 A[RB][KS];
    T::load_a(ohtab, a.words, a.n, a.wpr, a.W, row0, A);
    __syncthreads();
    const v16i32 Cinit = T::c_init(T::thr(P, a.k));
    const uint32_t ncb = (uint32_t)min<uint64_t>(S / 32, (a.n - col0 + 31) / 32);
    for (uint32_t cb = 0; cb < ncb; ++cb) {
        const uint32_t cl = cb * 32 + r;                 // this lane's column (local)
        v4i32 B[KS];
        onehot_frag_tab<KS>(ohtab, &cw[cl * NW], true, h, B);   // a padding column is "A..A" (filtered)
        T::sweep(A, B, Cinit, stash, [&](int rb, const int* st) {
            ap_hits(a, st, (wave * RB + rb) * 32, cl, row0, col0, diag, rowcnt, colcnt, &blkhits);
        });
    }
    __syncthreads();
    if (threadIdx.x == 0 && blkhits) atomicAdd(a.npairs, blkhits);
    if (a.counts) {
        for (int c = threadIdx.x; c < S; c += 256) {
            if (rowcnt[c]) atomicAdd(&a.counts[row0 + c], rowcnt[c]);
            if (colcnt[c]) atomicAdd(&a.counts[col0 + c], colcnt[c]);
        }
    }
}

template <int KS, int RB = mfma_rb(KS)>
int launch_allpairs_mfma(AllPairsArgs a, uint32_t P, hipStream_t s) {
    constexpr int S = MfmaTiles<KS, RB>::S;
    const uint64_t t = (a.n + S - 1) / S;
    if (t > 65535) return ss_fail(SS_EARG, "all-pairs: n too large for one launch (split the batch)");
    const uint64_t tri = t * (t + 1) / 2;
    // measured: the 1-D triangle is faster at RB <= 2 (50k x 32 nt 7.45 -> 8.16 T pairs/s, 20k x 96 nt
    // 1.80 -> 1.92), slower at RB 8 (100k x 12 nt 15.6 -> 13.3), where the square grid stays
    constexpr bool TRI = RB <= 2;
    const dim3 grid = (TRI && t > 1 && tri * 256 < (1ull << 32)) ? dim3((unsigned)tri) : dim3((unsigned)t, (unsigned)t);
    hipLaunchKernelGGL((k_allpairs_mfma<KS, RB, TRI>), grid, dim3(256), 0, s, a, P);
    return ss_check(hipGetLastError(), "k_allpairs_mfma");
}

template <int WT>
int launch_allpairs(AllPairsArgs a, hipStream_t s) {
    constexpr int S = Tile<WT>::S;
    const uint64_t t = (a.n + S - 1) / S;
    if (t > 65535) return ss_fail(SS_EARG, "all-pairs: n too large for one launch (split the batch)");
    hipLaunchKernelGGL((k_allpairs<WT>), dim3((unsigned)t, (unsigned)t), dim3(256), 0, s, a);
    return ss_check(hipGetLastError(), "k_allpairs");
}

// ------------------------------------------------------------------------------------------------
// Pigeonhole form (one-word reads, small max_dist k): split the P compared positions into G = k + 1
// contiguous segments.  Two reads within distance k differ in at most k positions, so at least one
// segment is equal in both.  Per segment g the reads are bucketed by that segment's value (counting
// sort: histogram -> tile sums -> scan -> scatter of {word, index}); only pairs sharing a bucket are
// candidates, and a candidate (i, j) is reported by segment g only when segment g is equal and
// every segment g' < g differs (the pair's first equal segment), so each pair is reported once.
// Work is sum over buckets of c (c - 1) / 2 per segment instead of n (n - 1) / 2: for n random UMIs
// of 12 nt and k = 1, 2 segments of 6 nt (the alias position L joins the last), ~n^2 / 4096
// candidates.  Skewed batches (one UMI repeated many times, low-complexity segments) make buckets
// large; AUTO reads the candidate totals back after the histogram and hands such batches to the
// tiled MFMA form.  Kernels: k_pig_hist (bucket counts, each read's rank), k_pig_tile (tile sums;
// its last block scans them), k_pig_apply (bucket starts), k_pig_scatter, k_pig_pairs.
// Buckets: the segment value itself when it has <= nbmax bits, else a 64-bit multiplicative hash of
// it (colliding values only add candidates: the equality test is on the segment value).
// ------------------------------------------------------------------------------------------------
constexpr int kPigMaxG = 16;             // segments of the forms with row copies (k_pig_*, k_pigw_*)
constexpr int kPiglMaxG = 32;            // the long form's segment bound (k_pigl_*, below)
constexpr uint32_t kPigTile = 4096;      // buckets per scan tile: 256 threads x 16
constexpr uint32_t kPigMaxBits = 22;     // <= 1024 tiles per segment (4 per thread of the scanning block)
constexpr uint64_t kPigRatio = 16;       // auto: pigeonhole when candidates < all pairs / kPigRatio

// One argument struct for the three forms: one-word rows (k_pig_*), W = 2 .. 4 with row copies
// (k_pigw_*), and the long form without them (k_pigl_*, further below).  The one-word form's shift /
// mask and the other forms' seg share their bytes (no kernel reads both): side by side the struct is
// 608 B of kernel arguments, and past ~520 B the compiler builds k_pig_pairs' walks, unchanged in
// source, with more exec-mask branches (100k x 16 nt, k 2: 0.099 -> 0.114 ms; profiles/hamming_refactor).
struct PigArgs {
    const uint64_t* words;
    uint64_t n;
    uint32_t wpr, W, k, G, nbmax, maxtiles, exact, P;   // exact: bit g = segment g buckets by value
    uint32_t nb[kPiglMaxG];
    union {
        struct {   // one-word rows (G <= kPigMaxG): segment g = (word >> shift[g]) & mask[g]
            uint32_t shift[kPigMaxG];
            uint64_t mask[kPigMaxG];
        };
        // multi-word rows: segment g = positions [seg[g], seg[g + 1]) of the row's P (it may cross a
        // word boundary)
        uint32_t seg[kPiglMaxG + 1];
    };
    uint32_t* hist;       // G << nbmax: counts, then bucket starts (k_pig_apply)
    uint32_t* tile_cnt;   // G * maxtiles: bucket sums, then tile bases
    uint64_t* tile_cand;  // G * maxtiles
    uint64_t* cand;       // G: candidate pairs per segment
    uint32_t* done;       // k_pig_tile's finished-block count (zeroed with hist)
    uint32_t zero_out;    // k_pig_hist zeroes counts and *npairs (the entry point left them)
    uint64_t* sw;         // G * n * W words: the rows in bucket order (null in the long form)
    uint32_t* sid;        // G * n read indices in bucket order
    // G * n: read i's rank in its bucket of segment g (the hist kernels' atomics); the long form's
    // scatter then overwrites it with that bucket's end
    uint32_t* rank;
    uint32_t* counts;
    uint32_t* pairs;
    uint64_t max_pairs;
    unsigned long long* npairs;
};

__device__ __forceinline__ uint64_t shfl64x(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t pig_key(const PigArgs& a, uint32_t g, uint64_t w) {
    return (w >> a.shift[g]) & a.mask[g];
}
__device__ __forceinline__ uint32_t pig_bucket(const PigArgs& a, uint32_t g, uint64_t w) {
    const uint64_t key = pig_key(a, g, w);
    return (a.exact >> g) & 1u ? (uint32_t)key : (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - a.nb[g]));
}

__global__ __launch_bounds__(256) void k_pig_hist(PigArgs a) {
    if (a.zero_out && blockIdx.x == 0 && threadIdx.x == 0) *a.npairs = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256) {
        if (a.zero_out && a.counts) a.counts[i] = 0u;
        const uint64_t w = a.words[i * a.wpr];
        for (uint32_t g = 0; g < a.G; ++g)
            a.rank[g * a.n + i] = atomicAdd(&a.hist[((uint64_t)g << a.nbmax) + pig_bucket(a, g, w)], 1u);
    }
}

// block sums of a 256-thread block: returns the total to every thread
template <typename T>
__device__ __forceinline__ T block_sum256(T v, T* red) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const T t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}

// per tile of 4096 buckets: number of reads and candidate pairs; the grid's last block to finish
// then scans every segment's tile sums (<= 1024 tiles: 4 per thread) into tile bases and the
// segment's candidate total -- no separate scan launch
__global__ __launch_bounds__(256) void k_pig_tile(PigArgs a) {
    const uint32_t g = blockIdx.y, t0 = blockIdx.x * kPigTile, nbk = 1u << a.nb[g];
    __shared__ uint32_t r32[4];
    __shared__ uint64_t r64[4];
    __shared__ uint32_t s_last;
    if (t0 < nbk) {
        const uint32_t* h = a.hist + ((uint64_t)g << a.nbmax) + t0;
        uint32_t c = 0;
        uint64_t cand = 0;
        for (uint32_t j = threadIdx.x; j < kPigTile && t0 + j < nbk; j += 256) {
            const uint64_t v = h[j];
            c += (uint32_t)v;
            cand += v * (v - (v ? 1 : 0)) / 2;
        }
        c = block_sum256(c, r32);
        cand = block_sum256(cand, r64);
        if (threadIdx.x == 0) {
            a.tile_cnt[g * a.maxtiles + blockIdx.x] = c;
            a.tile_cand[g * a.maxtiles + blockIdx.x] = cand;
        }
    }
    if (threadIdx.x == 0) {
        __threadfence();                                          // this block's sums before its count
        s_last = atomicAdd(a.done, 1u) + 1u == gridDim.x * gridDim.y;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();                                              // every block's sums visible
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t gg = 0; gg < a.G; ++gg) {
        const uint32_t nt = ((1u << a.nb[gg]) + kPigTile - 1) / kPigTile;
        uint32_t* tc = a.tile_cnt + gg * a.maxtiles;
        uint64_t* td = a.tile_cand + gg * a.maxtiles;
        uint32_t v[4], sum = 0;
        uint64_t cand = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t t = 4 * threadIdx.x + k;
            // device-scope loads (other blocks wrote them): past this CU's cache
            v[k] = t < nt ? __hip_atomic_load(&tc[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            cand += t < nt ? __hip_atomic_load(&td[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            sum += v[k];
        }
        uint32_t inc = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(inc, o);
            if (lane >= (uint32_t)o) inc += y;
        }
        if (lane == 63) r32[wv] = inc;
        const uint64_t ctot = block_sum256(cand, r64);              // (its barriers order r32 too)
        uint32_t run = inc - sum;
        for (uint32_t i = 0; i < wv; ++i) run += r32[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t t = 4 * threadIdx.x + k;
            if (t < nt) tc[t] = run;
            run += v[k];
        }
        if (threadIdx.x == 0) a.cand[gg] = ctot;
        __syncthreads();                                          // r32 of the next segment
    }
}

// bucket starts: each thread owns 16 consecutive buckets of the tile
__global__ __launch_bounds__(256) void k_pig_apply(PigArgs a) {
    const uint32_t g = blockIdx.y, t0 = blockIdx.x * kPigTile, nbk = 1u << a.nb[g];
    if (t0 >= nbk) return;
    uint32_t* h = a.hist + ((uint64_t)g << a.nbmax) + t0;
    const uint32_t b0 = threadIdx.x * 16u;
    const uint32_t m = b0 < nbk - t0 ? min(16u, nbk - t0 - b0) : 0u;
    uint32_t v[16];
    uint32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        v[j] = j < m ? h[b0 + j] : 0u;
        s += v[j];
    }
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t inc = s;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += y;
    }
    __shared__ uint32_t ws[4];
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    uint32_t run = a.tile_cnt[g * a.maxtiles + blockIdx.x] + inc - s;
    for (uint32_t i = 0; i < wv; ++i) run += ws[i];
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        if (j < m) h[b0 + j] = run;
        run += v[j];
    }
}

__global__ __launch_bounds__(256) void k_pig_scatter(PigArgs a) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w = a.words[i * a.wpr];
        for (uint32_t g = 0; g < a.G; ++g) {
            const uint32_t pos = a.hist[((uint64_t)g << a.nbmax) + pig_bucket(a, g, w)] + a.rank[g * a.n + i];
            a.sw[g * a.n + pos] = w;
            a.sid[g * a.n + pos] = (uint32_t)i;
        }
    }
}

constexpr uint64_t kPigTileWalk = 256;     // a wave's entry run past this: walked as broadcast tiles

// one lane per read in bucket order of segment g = blockIdx.y, compared with the reads after it in its
// bucket (see the walk below).  Hits leave through wave ballots into the wave's hit buffer; a
// count-only call sums the block's hits in LDS and adds them with one atomic per block (one per
// wave on the single pair counter measured a third of the kernel).
template <int GM>   // G <= GM segments: the first-equal-segment test unrolled over GM - 1 masks
__global__ __launch_bounds__(256) void k_pig_pairs(PigArgs a) {
    __shared__ uint2 pbuf[4][kPairBuf];
    __shared__ unsigned long long s_hits;
    if (threadIdx.x == 0) s_hits = 0;
    __syncthreads();
    const uint32_t g = blockIdx.y, lane = threadIdx.x & 63u;
    // the wave's first position, made scalar (threadIdx.x & ~63 is wave-uniform)
    const uint64_t p0 = (uint64_t)blockIdx.x * 256 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    const uint64_t p = p0 + lane;
    const bool valid = p < a.n;                              // (a wave past the batch walks nothing)
    const uint64_t* sw = a.sw + g * a.n;
    const uint32_t* sid = a.sid + g * a.n;
    const uint32_t* start = a.hist + ((uint64_t)g << a.nbmax);
    const uint32_t nbk = 1u << a.nb[g];
    const uint64_t w = valid ? sw[p] : 0ull;
    const uint32_t id = valid ? sid[p] : 0u;
    const uint32_t b = pig_bucket(a, g, w);
    uint64_t end = valid ? (b + 1 < nbk ? start[b + 1] : a.n) : 0ull;
    // segment h's positions as one bit per position (the low bit of its 2-bit code): with
    // d = the positions where two words differ, the pair is segment g's iff d misses segment g and
    // meets every segment before it (g is the pair's first equal segment) and popcount(d) <= k
    constexpr uint64_t kLo = 0x5555555555555555ull;
    uint64_t segm[GM];
#pragma unroll
    for (int h = 0; h < GM; ++h) segm[h] = (uint32_t)h < g ? (a.mask[h] << a.shift[h]) & kLo : 0ull;
    const uint64_t mg = (a.mask[g] << a.shift[g]) & kLo;
    const uint32_t kmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.k);
    WaveHits wh;
    wh.buf = pbuf[threadIdx.x >> 6];
    uint32_t row = 0;
    // the wave's run of entries, [p0 + 1, its largest bucket end): long (large buckets: heavy
    // duplicates, short segments) -> the wave walks it in 64-entry tiles, one coalesced load per tile
    // and each entry broadcast to the wave by v_readlane (the 64 compares of a tile wait on no
    // memory); short (the UMI case) -> each lane walks its own run (below)
    uint64_t wend = end;
    for (int o = 32; o; o >>= 1) {
        const uint64_t y = shfl64x(wend, o);
        wend = y > wend ? y : wend;
    }
    wend = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(wend >> 32)) << 32 |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wend);   // uniform: scalar loop bounds
    if (wend > p0 + kPigTileWalk) {
        for (uint64_t t0 = p0 + 1; t0 < wend; t0 += 64) {
            const uint64_t qt = t0 + lane;
            const uint64_t tw = qt < a.n ? sw[qt] : 0ull;
            const uint32_t tid = qt < a.n ? sid[qt] : 0u;
            const uint32_t twl = (uint32_t)tw, twh = (uint32_t)(tw >> 32);
            const uint32_t ne = (uint32_t)((wend - t0) < 64 ? (wend - t0) : 64);
            for (uint32_t e = 0; e < ne; ++e) {
                const uint64_t q = t0 + e;
                const uint64_t w2 = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)twh, (int)e) << 32 |
                                    (uint32_t)__builtin_amdgcn_readlane((int)twl, (int)e);
                const uint64_t x = w ^ w2, d = (x | (x >> 1)) & kLo;
                bool hit = (q > p) & (q < end) & ((uint32_t)__popcll(d) <= kmax) & !(d & mg);
#pragma unroll
                for (int h = 0; h < GM - 1; ++h) hit = hit && ((uint32_t)h >= g || (d & segm[h]) != 0ull);
                const uint64_t mask = __ballot(hit);
                if (!mask) continue;
                const uint32_t jd = (uint32_t)__builtin_amdgcn_readlane((int)tid, (int)e);
                row += hit ? 1u : 0u;
                if (a.counts && lane == (uint32_t)__ffsll((unsigned long long)mask) - 1u)
                    atomicAdd(&a.counts[jd], (uint32_t)__popcll(mask));
                hits_add(a, wh, hit, mask, id, jd);
            }
        }
        end = 0;                                           // (the lane walk below has nothing left)
    }
    // each lane walks its own bucket run (p, end): consecutive lanes read consecutive entries, so a
    // step's 64 loads are one coalesced run; kPigStep entries per step, the next step's in flight
    constexpr int kPigStep = 4;
    uint64_t nx[kPigStep];
#pragma unroll
    for (int u = 0; u < kPigStep; ++u) nx[u] = p + 1 + u < end ? sw[p + 1 + u] : 0ull;
    for (uint64_t q0 = p + 1;; q0 += kPigStep) {
        if (!__ballot(q0 < end)) break;
        uint64_t cur[kPigStep];
#pragma unroll
        for (int u = 0; u < kPigStep; ++u) {
            cur[u] = nx[u];
            const uint64_t qn = q0 + kPigStep + u;
            nx[u] = qn < end ? sw[qn] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kPigStep; ++u) {
            const uint64_t q = q0 + u;
            const uint64_t x = w ^ cur[u], d = (x | (x >> 1)) & kLo;
            bool hit = (q < end) & ((uint32_t)__popcll(d) <= kmax) & !(d & mg);
#pragma unroll
            for (int h = 0; h < GM - 1; ++h) hit = hit && ((uint32_t)h >= g || (d & segm[h]) != 0ull);
            const uint64_t mask = __ballot(hit);
            if (!mask) continue;
            const uint32_t jd = hit ? sid[q] : 0u;
            row += hit ? 1u : 0u;
            if (hit && a.counts) atomicAdd(&a.counts[jd], 1u);
            hits_add(a, wh, hit, mask, id, jd);
        }
    }
    if (a.pairs) hits_flush(a, wh);
    else if (lane == 0 && wh.nh) atomicAdd(&s_hits, (unsigned long long)wh.nh);
    if (a.counts && row) atomicAdd(&a.counts[id], row);
    __syncthreads();
    if (threadIdx.x == 0 && s_hits) atomicAdd(a.npairs, s_hits);
}

// ---- Multi-word reads (W = 2 .. 4 words: 33 .. 128 nt).  The same pigeonhole
// argument over the P = min(L + 1, 32 W) compared positions of the row: G = k + 1 contiguous segments
// (a segment may cross a word boundary and be longer than 32 positions).  A segment's bucket is its
// value when it has <= nbmax bits, else a hash of its (up to 128-bit) value; equality, the distance
// and the first-equal-segment rule are decided on the words of both rows, so a hash collision only
// adds candidates.  Rows live W words apiece in the bucket-ordered arrays (sw: G x n x W words).
template <int W>
__device__ __forceinline__ void pig_row(const PigArgs& a, uint64_t i, uint64_t (&w)[W]) {
#pragma unroll
    for (int q = 0; q < W; ++q) w[q] = a.words[i * a.wpr + q];
}
// A row's words for the bucket function: in registers (W a template constant: selected, never
// indexed) or in memory (a runtime W; no word at or past W is read).  word(q) = 0 for q >= W.
template <int W>
struct RegRow {
    const uint64_t (&w)[W];
    __device__ __forceinline__ uint64_t word(uint32_t q) const {
        uint64_t v = 0;
#pragma unroll
        for (int k = 0; k < W; ++k)
            if ((uint32_t)k == q) v = w[k];
        return v;
    }
};
struct MemRow {
    const uint64_t* r;
    uint32_t W;
    __device__ __forceinline__ uint64_t word(uint32_t q) const { return q < W ? r[q] : 0ull; }
};
// bits [2 b0, 2 b0 + 64) of a row (b0 in positions, < 32 W)
template <typename Row>
__device__ __forceinline__ uint64_t row_bits64(const Row& row, uint32_t b0) {
    const uint32_t q = b0 >> 5, sh = 2u * (b0 & 31u);
    const uint64_t lo = row.word(q);
    if (!sh) return lo;
    return (lo >> sh) | (row.word(q + 1u) << (64u - sh));
}
// bucket of segment g of a multi-word row: its value when it has <= nbmax bits, else a hash of it;
// an empty segment is bucket 0
template <typename Row>
__device__ __forceinline__ uint32_t pigw_bucket(const PigArgs& a, uint32_t g, const Row& row) {
    const uint32_t p0 = a.seg[g], len = a.seg[g + 1] - p0;
    if (!len) return 0u;
    if ((a.exact >> g) & 1u) return (uint32_t)(row_bits64(row, p0) & ((1ull << (2u * len)) - 1ull));
    uint64_t h = 0x243F6A8885A308D3ull ^ len;
    for (uint32_t b = 0; b < len; b += 32) {          // the segment's 64-bit pieces, the last masked
        const uint32_t m = len - b < 32u ? len - b : 32u;
        uint64_t v = row_bits64(row, p0 + b);
        if (m < 32u) v &= (1ull << (2u * m)) - 1ull;
        h = (h ^ v) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    return (uint32_t)(h >> (64 - a.nb[g]));
}

template <int W>
__global__ __launch_bounds__(256) void k_pigw_hist(PigArgs a) {
    if (a.zero_out && blockIdx.x == 0 && threadIdx.x == 0) *a.npairs = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256) {
        if (a.zero_out && a.counts) a.counts[i] = 0u;
        uint64_t w[W];
        pig_row<W>(a, i, w);
        for (uint32_t g = 0; g < a.G; ++g)
            a.rank[g * a.n + i] = atomicAdd(&a.hist[((uint64_t)g << a.nbmax) + pigw_bucket(a, g, RegRow<W>{w})], 1u);
    }
}

template <int W>
__global__ __launch_bounds__(256) void k_pigw_scatter(PigArgs a) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256) {
        uint64_t w[W];
        pig_row<W>(a, i, w);
        for (uint32_t g = 0; g < a.G; ++g) {
            const uint64_t pos = a.hist[((uint64_t)g << a.nbmax) + pigw_bucket(a, g, RegRow<W>{w})] + a.rank[g * a.n + i];
            uint64_t* dst = a.sw + ((uint64_t)g * a.n + pos) * W;
#pragma unroll
            for (int q = 0; q < W; ++q) dst[q] = w[q];
            a.sid[g * a.n + pos] = (uint32_t)i;
        }
    }
}

// one lane per row in bucket order of segment g = blockIdx.y, each walking its own bucket run (p, end)
// with kPigStep rows in flight (consecutive lanes on consecutive rows: coalesced).  A candidate is a
// hit when its distance is <= k and g is the first segment the rows agree on: the <= k differing
// positions are walked and their segments marked (segment of a position: the boundaries in a.seg).
template <int W>
__global__ __launch_bounds__(256) void k_pigw_pairs(PigArgs a) {
    __shared__ uint2 pbuf[4][kPairBuf];
    __shared__ unsigned long long s_hits;
    if (threadIdx.x == 0) s_hits = 0;
    __syncthreads();
    const uint32_t g = blockIdx.y, lane = threadIdx.x & 63u;
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = p < a.n;
    const uint64_t* sw = a.sw + (uint64_t)g * a.n * W;
    const uint32_t* sid = a.sid + g * a.n;
    const uint32_t* start = a.hist + ((uint64_t)g << a.nbmax);
    const uint32_t nbk = 1u << a.nb[g];
    uint64_t w[W];
#pragma unroll
    for (int q = 0; q < W; ++q) w[q] = valid ? sw[p * W + q] : 0ull;
    const uint32_t id = valid ? sid[p] : 0u;
    const uint32_t b = pigw_bucket(a, g, RegRow<W>{w});
    const uint64_t end = valid ? (b + 1 < nbk ? start[b + 1] : a.n) : 0ull;
    constexpr uint64_t kLo = 0x5555555555555555ull;
    const uint32_t kmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.k);
    const uint32_t want = (1u << g) - 1u;             // segments 0 .. g - 1 differ, g agrees
    WaveHits wh;
    wh.buf = pbuf[threadIdx.x >> 6];
    uint32_t row = 0;
    constexpr int kPigStep = 4;
    uint64_t nx[kPigStep][W];
#pragma unroll
    for (int u = 0; u < kPigStep; ++u)
#pragma unroll
        for (int q = 0; q < W; ++q) nx[u][q] = p + 1 + u < end ? sw[(p + 1 + u) * W + q] : 0ull;
    for (uint64_t q0 = p + 1;; q0 += kPigStep) {
        if (!__ballot(q0 < end)) break;
        uint64_t cur[kPigStep][W];
#pragma unroll
        for (int u = 0; u < kPigStep; ++u) {
            const uint64_t qn = q0 + kPigStep + u;
#pragma unroll
            for (int q = 0; q < W; ++q) {
                cur[u][q] = nx[u][q];
                nx[u][q] = qn < end ? sw[qn * W + q] : 0ull;
            }
        }
#pragma unroll
        for (int u = 0; u < kPigStep; ++u) {
            const uint64_t qq = q0 + u;
            uint64_t d[W];
            uint32_t dd = 0;
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const uint64_t x = w[q] ^ cur[u][q];
                d[q] = (x | (x >> 1)) & kLo;
                dd += (uint32_t)__popcll(d[q]);
            }
            bool hit = (qq < end) & (dd <= kmax);
            if (hit) {     // the segments the differing positions fall in
                uint32_t segs = 0;
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    uint64_t m = d[q];
                    while (m) {
                        const uint32_t pos = 32u * q + ((uint32_t)__ffsll((long long)m) - 1u) / 2u;
                        uint32_t sgi = 0;
                        while (sgi + 1 < a.G && pos >= a.seg[sgi + 1]) ++sgi;
                        segs |= 1u << sgi;
                        m &= m - 1ull;
                    }
                }
                hit = (segs & (want | (1u << g))) == want;
            }
            const uint64_t mask = __ballot(hit);
            if (!mask) continue;
            const uint32_t jd = hit ? sid[qq] : 0u;
            row += hit ? 1u : 0u;
            if (hit && a.counts) atomicAdd(&a.counts[jd], 1u);
            hits_add(a, wh, hit, mask, id, jd);
        }
    }
    if (a.pairs) hits_flush(a, wh);
    else if (lane == 0 && wh.nh) atomicAdd(&s_hits, (unsigned long long)wh.nh);
    if (a.counts && row) atomicAdd(&a.counts[id], row);
    __syncthreads();
    if (threadIdx.x == 0 && s_hits) atomicAdd(a.npairs, s_hits);
}

// Per-device scratch of the pigeonhole form, grow-only and stream-ordered: a call holds the device's
// lock, waits (on its stream) for the previous call's kernels before reusing the buffer, and records
// its own end.
struct PigScratch {
    std::mutex mu;
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    uint64_t* h_cand = nullptr;   // pinned: the candidate totals read back
};
PigScratch g_pig[64];

// A call's hold on the scratch of the device that holds `words` (the kernels run there, on the
// caller's stream), not of whichever device is current: that device made current and the
// scratch locked until the hold goes.  acquire() leaves ps->p with >= need bytes, ordered after the
// previous call's kernels; *have = false (rc 0) when the memory could not be had and the call was
// not forced: the outputs are then zeroed for the tiled form, which needs no scratch.
struct PigHold {
    int prev = 0, now = 0;
    PigScratch* ps = nullptr;
    std::unique_lock<std::mutex> lock;
    ~PigHold() {
        if (lock.owns_lock()) lock.unlock();
        if (prev != now) (void)hipSetDevice(prev);
    }
    int acquire(const void* words, size_t need, bool forced, hipStream_t s, unsigned long long* npairs,
                uint32_t* counts, uint64_t n, bool* have) {
        *have = false;
        int rc = ss_check(hipGetDevice(&prev), "hipGetDevice");
        now = prev;
        if (rc) return rc;
        hipPointerAttribute_t pa{};
        rc = ss_check(hipPointerGetAttributes(&pa, words), "all-pairs: words pointer attributes");
        if (rc) return rc;
        if (pa.device < 0 || pa.device >= 64) return ss_fail(SS_EARG, "all-pairs: device index past 63");
        if (pa.device != prev) {
            rc = ss_check(hipSetDevice(pa.device), "all-pairs: hipSetDevice");
            if (rc) return rc;
            now = pa.device;
        }
        ps = &g_pig[now];
        lock = std::unique_lock<std::mutex>(ps->mu);
        if (!ps->done) rc = ss_check(hipEventCreateWithFlags(&ps->done, hipEventDisableTiming), "pig event");
        if (!rc && !ps->h_cand)
            rc = ss_check(hipHostMalloc((void**)&ps->h_cand, kPiglMaxG * 8, hipHostMallocDefault), "pinned totals");
        if (!rc && ps->bytes < need) {
            if (ps->p) {
                rc = ss_check(hipEventSynchronize(ps->done), "pig scratch idle");
                if (!rc) rc = ss_check(hipFree(ps->p), "pig scratch free");
                ps->p = nullptr;
                ps->bytes = 0;
            }
            const size_t want = need + need / 4;
            if (!rc && hipMalloc(&ps->p, want) != hipSuccess) {
                (void)hipGetLastError();
                ps->p = nullptr;
                if (forced) return ss_fail(SS_ENOMEM, "pigeonhole all-pairs scratch: out of device memory");
                // auto: the tiled form gets the outputs zeroed as the entry skipped that
                rc = ss_check(hipMemsetAsync(npairs, 0, sizeof(uint64_t), s), "npairs reset");
                if (!rc && counts) rc = ss_check(hipMemsetAsync(counts, 0, n * sizeof(uint32_t), s), "counts reset");
                return rc;
            }
            if (!rc) ps->bytes = want;
        } else if (!rc) {
            rc = ss_check(hipStreamWaitEvent(s, ps->done, 0), "pig scratch wait");
        }
        if (!rc) *have = true;
        return rc;
    }
};

// ------------------------------------------------------------------------------------------------
// Long form (SS_ALLPAIRS_BUCKETED past the range of the forms above: W = 5 .. 32 words, or max_dist 16 .. 31
// at any W).  The same pigeonhole argument and segment split, for a runtime W and G <= 32.  Two
// things differ from k_pigw_*:
//  - no row copies: bucket order holds read indices only (sid), and candidate rows are read from
//    `words` through them.  Scratch per call = G (4 << nbmax) B of histogram + 12 B per scan tile
//    + G * n * 8 B (sid + rank); copied rows would add G * n * 8 W B (8 GB at n = 1M, W = G = 32).
//  - load shape: a group of LG = 4 / 8 / 16 / 32 lanes (the power of two >= W) per entry, one 8-byte
//    word of the row per lane, so a candidate row is one contiguous 8 W-byte piece of a wave load
//    instead of 64 lanes in 64 rows.  8-byte pieces are aligned for every wpr (a 16-byte piece is
//    not when wpr is odd, the 129 .. 160-nt case); lanes at word >= W load nothing and add zero, so
//    no read goes past a row's W words (wpr may equal W).
// k_pigl_scatter overwrites rank[g][i] with the end of read i's bucket, so the pairs kernel gets an
// entry's run (p, end) from its index alone and never hashes.  A group walks its run kPiglStep
// candidates per step (their indices fetched a step ahead, the rows in flight together); the wave
// leaves the loop when no group has candidates left.  Nothing is sized by a run's length, so a
// bucket of n entries (one repeated read) is walked correctly, in n / kPiglStep steps.
// Measured and not kept (profiles/r7/ab_four_entries_per_group.log): four consecutive entries per
// group, each candidate row loaded once for the four and the tile's own rows its first candidates
// (112 VGPRs, 4 waves per SIMD): sparse buckets 0.124 -> 0.103 ms (100k x 150 nt, pool 2^16) and
// 0.454 -> 0.358 ms (50k x 1024 nt), but buckets of ~400 reads 1.73 -> 2.16 ms and 2.52 -> 3.09 ms.
// ------------------------------------------------------------------------------------------------
// a thread per read, every segment in turn (a thread per (segment, read) measured no faster at 100k x
// 150 nt, 20 vs 20 us, and slower at 50k x 1024 nt, G = 17: hist 38 -> 43 us, scatter 27 -> 35 us)
__global__ __launch_bounds__(256) void k_pigl_hist(PigArgs a) {
    if (a.zero_out && blockIdx.x == 0 && threadIdx.x == 0) *a.npairs = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256) {
        if (a.zero_out && a.counts) a.counts[i] = 0u;
        const uint64_t* r = a.words + i * a.wpr;
        for (uint32_t g = 0; g < a.G; ++g)
            a.rank[g * a.n + i] = atomicAdd(&a.hist[((uint64_t)g << a.nbmax) + pigw_bucket(a, g, MemRow{r, a.W})], 1u);
    }
}

__global__ __launch_bounds__(256) void k_pigl_scatter(PigArgs a) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t* r = a.words + i * a.wpr;
        for (uint32_t g = 0; g < a.G; ++g) {
            const uint32_t* start = a.hist + ((uint64_t)g << a.nbmax);
            const uint32_t b = pigw_bucket(a, g, MemRow{r, a.W}), nbk = 1u << a.nb[g];
            const uint32_t pos = start[b] + a.rank[g * a.n + i];
            a.sid[g * a.n + pos] = (uint32_t)i;
            a.rank[g * a.n + i] = b + 1u < nbk ? start[b + 1u] : (uint32_t)a.n;   // this read's bucket end
        }
    }
}

constexpr int kPiglStep = 4;
template <int LG>   // lanes per entry, one row word each: W <= LG
__global__ __launch_bounds__(256) void k_pigl_pairs(PigArgs a) {
    __shared__ uint2 pbuf[4][kPairBuf];
    __shared__ uint32_t s_seg[kPiglMaxG + 1];
    __shared__ unsigned long long s_hits;
    if (threadIdx.x == 0) {
        s_hits = 0;
        for (uint32_t h = 0; h <= a.G; ++h) s_seg[h] = a.seg[h];   // (lanes index it per position below)
    }
    __syncthreads();
    const uint32_t g = blockIdx.y, lane = threadIdx.x & 63u, l = threadIdx.x & (LG - 1u);
    const uint64_t p = (uint64_t)blockIdx.x * (256 / LG) + threadIdx.x / LG;   // the group's entry
    const bool valid = p < a.n, live = l < a.W;
    const uint32_t* sid = a.sid + g * a.n;
    const uint32_t id = valid ? sid[p] : 0u;
    const uint64_t end = valid ? a.rank[g * a.n + id] : 0ull;
    const uint64_t w = valid && live ? a.words[(uint64_t)id * a.wpr + l] : 0ull;
    // this lane's word holds positions [32 l, 32 l + 32); those below P compare (the low bit of each code)
    const uint32_t np = live && a.P > 32u * l ? min(32u, a.P - 32u * l) : 0u;
    const uint64_t pm = np >= 32u ? 0x5555555555555555ull : 0x5555555555555555ull & ((1ull << (2u * np)) - 1ull);
    uint32_t s0 = 0;                                   // the segment of this word's first position
    while (s0 + 1 < a.G && 32u * l >= s_seg[s0 + 1]) ++s0;
    const uint32_t kmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.k);
    const uint32_t want = (1u << g) - 1u;             // segments 0 .. g - 1 differ, g agrees
    WaveHits wh;
    wh.buf = pbuf[threadIdx.x >> 6];
    uint32_t row = 0;
    uint32_t nx[kPiglStep];
#pragma unroll
    for (int u = 0; u < kPiglStep; ++u) nx[u] = p + 1 + u < a.n ? sid[p + 1 + u] : 0u;   // (not "< end": issued with sid[p])
    for (uint64_t q0 = p + 1;; q0 += kPiglStep) {
        if (!__ballot(q0 < end)) break;
        uint32_t jd[kPiglStep];
        uint64_t c[kPiglStep];
#pragma unroll
        for (int u = 0; u < kPiglStep; ++u) {
            jd[u] = nx[u];
            c[u] = q0 + u < end && live ? a.words[(uint64_t)jd[u] * a.wpr + l] : 0ull;
            const uint64_t qn = q0 + kPiglStep + u;
            nx[u] = qn < end ? sid[qn] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kPiglStep; ++u) {
            const uint64_t x = w ^ c[u], d = (x | (x >> 1)) & pm;
            uint32_t dd = (uint32_t)__popcll(d);
#pragma unroll
            for (int o = LG / 2; o; o >>= 1) dd += __shfl_xor(dd, o);
            const bool near = (q0 + u < end) & (dd <= kmax);
            if (!__ballot(near)) continue;
            // g must be the first segment the rows agree on: each lane marks the segments of its
            // word's differing positions (ascending, so the segment index only moves up)
            uint32_t segs = 0;
            if (near) {
                uint32_t sgi = s0;
                for (uint64_t m = d; m; m &= m - 1ull) {
                    const uint32_t pos = 32u * l + ((uint32_t)__ffsll((long long)m) - 1u) / 2u;
                    while (sgi + 1 < a.G && pos >= s_seg[sgi + 1]) ++sgi;
                    segs |= 1u << sgi;
                }
            }
#pragma unroll
            for (int o = LG / 2; o; o >>= 1) segs |= __shfl_xor(segs, o);
            const bool hit = near && l == 0 && (segs & (want | (1u << g))) == want;   // one lane per group
            const uint64_t mask = __ballot(hit);
            if (!mask) continue;
            row += hit ? 1u : 0u;
            if (hit && a.counts) atomicAdd(&a.counts[jd[u]], 1u);
            hits_add(a, wh, hit, mask, id, jd[u]);
        }
    }
    if (a.pairs) hits_flush(a, wh);
    else if (lane == 0 && wh.nh) atomicAdd(&s_hits, (unsigned long long)wh.nh);
    if (a.counts && row) atomicAdd(&a.counts[id], row);
    __syncthreads();
    if (threadIdx.x == 0 && s_hits) atomicAdd(a.npairs, s_hits);
}

// AUTO keeps the long form when candidates < all pairs / kPiglRatio.  Not kPigRatio: the other side
// is the bit-plane form (slower than the MFMA tiles), and a candidate here costs a gathered row.
// Measured (tools/probe_f4.py longsweep, profiles/r7/probe_f4_longsweep.log: pools drawn uniformly,
// candidate fraction (k + 1) / pool, every candidate of segment 0 a hit): forced bucketed against
// forced tiles at 100k x 150 nt, k 3: 1/16 6.48 vs 5.46 ms, 1/32 3.43 vs 5.14 ms; at 50k x 1024 nt,
// k 16: 1/15 4.85 vs 4.22 ms, 1/30 2.72 vs 4.14 ms.  Both cross near 1/18 .. 1/20; 32 leaves the long
// form ~1.5x ahead at the threshold, for batches whose rows no longer sit in L2 as these did.
constexpr uint64_t kPiglRatio = 32;

// The three forms of one chain (memset -> hist -> k_pig_tile -> [totals read back] -> k_pig_apply ->
// scatter -> pairs): they differ in the kernels at those three points, in the per-row scratch and in
// AUTO's ratio.
enum PigForm { kPigWord, kPigRows, kPigLong };   // one-word rows; W = 2 .. 4 with row copies; long, without

template <typename K>
void pig_launch_w(K k2, K k3, K k4, uint32_t W, dim3 grid, hipStream_t s, const PigArgs& a) {
    hipLaunchKernelGGL(W == 2 ? k2 : (W == 3 ? k3 : k4), grid, dim3(256), 0, s, a);
}

// returns 0 with *done = false when the auto choice hands the batch to the tiled form
int pig_all_pairs(const AllPairsArgs& b, PigForm form, uint32_t L, uint32_t P, bool forced, hipStream_t s, bool* done) {
    *done = false;
    PigArgs a{};
    a.words = b.words;
    a.n = b.n;
    a.wpr = b.wpr;
    a.W = b.W;
    a.k = b.k;
    a.G = b.k + 1;
    a.P = P;
    a.counts = b.counts;
    a.pairs = b.pairs;
    a.max_pairs = b.max_pairs;
    a.npairs = b.npairs;
    a.zero_out = 1;
    uint32_t lg = 0;
    while ((1ull << lg) < a.n) ++lg;
    a.nbmax = lg < 10 ? 10 : (lg > kPigMaxBits ? kPigMaxBits : lg);
    a.maxtiles = ((1u << a.nbmax) + kPigTile - 1) / kPigTile;
    // the L read positions split evenly (the first L % G segments one longer, a segment may be empty
    // when L < G); the alias position L (P = L + 1: nearly always code 0, so no bucketing entropy)
    // joins the last segment
    const uint32_t Lr = P < L ? P : L;
    for (uint32_t g = 0, pos = 0; g < a.G; ++g) {
        uint32_t len = Lr / a.G + (g < Lr % a.G ? 1u : 0u);
        if (g + 1 == a.G) len = P - pos;
        if (form == kPigWord) {
            a.shift[g] = 2 * pos;
            a.mask[g] = len >= 32 ? ~0ull : ((1ull << (2 * len)) - 1ull);
        } else {
            a.seg[g] = pos;
        }
        a.nb[g] = 2 * len < a.nbmax ? 2 * len : a.nbmax;
        if (2 * len <= a.nbmax) a.exact |= 1u << g;
        pos += len;
    }
    if (form != kPigWord) a.seg[a.G] = P;
    // per (segment, read): sid + rank, and the row's W words in the forms that keep a copy
    const size_t ids_n = (size_t)a.G * a.n, sw_n = form == kPigLong ? 0 : ids_n * a.W;
    const size_t hist_n = (size_t)a.G << a.nbmax, tiles_n = (size_t)a.G * a.maxtiles;
    const size_t need = tiles_n * 8 + a.G * 8 + (hist_n + 2) * 4 + tiles_n * 4 + 64 + sw_n * 8 + ids_n * 8;
    PigHold hold;
    bool have = false;
    int rc = hold.acquire(b.words, need, forced, s, a.npairs, a.counts, a.n, &have);
    if (rc || !have) return rc;
    PigScratch& ps = *hold.ps;
    a.tile_cand = (uint64_t*)ps.p;
    a.cand = a.tile_cand + tiles_n;
    a.sw = sw_n ? a.cand + a.G : nullptr;
    a.hist = (uint32_t*)(a.cand + a.G + sw_n);
    a.done = a.hist + hist_n;                 // zeroed with hist
    a.tile_cnt = a.done + 2;
    a.sid = a.tile_cnt + tiles_n;
    a.rank = a.sid + ids_n;
    const dim3 rgrid((unsigned)std::min<uint64_t>((a.n + 255) / 256, 2048));
    const dim3 tgrid(a.maxtiles, a.G);
    rc = ss_check(hipMemsetAsync(a.hist, 0, (hist_n + 2) * 4, s), "pig hist reset");
    if (!rc) {
        if (form == kPigWord) hipLaunchKernelGGL(k_pig_hist, rgrid, dim3(256), 0, s, a);
        else if (form == kPigRows) pig_launch_w(k_pigw_hist<2>, k_pigw_hist<3>, k_pigw_hist<4>, a.W, rgrid, s, a);
        else hipLaunchKernelGGL(k_pigl_hist, rgrid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_pig_tile, tgrid, dim3(256), 0, s, a);
        rc = ss_check(hipGetLastError(), "pigeonhole hist / k_pig_tile");
    }
    bool use = forced;
    if (!rc && !forced) {
        rc = ss_check(hipMemcpyAsync(ps.h_cand, a.cand, a.G * 8, hipMemcpyDeviceToHost, s), "pig totals");
        if (!rc) rc = ss_check(hipStreamSynchronize(s), "pig totals sync");
        uint64_t cand = 0;
        for (uint32_t g = 0; !rc && g < a.G; ++g) cand += ps.h_cand[g];
        // measured (tools/probe_f4.py, profiles/r5/probe_f4_*.log, profiles/r7/probe_f4_longsweep.log):
        // see kPigRatio, kPiglRatio
        use = cand < a.n * (a.n - 1) / 2 / (form == kPigLong ? kPiglRatio : kPigRatio);
    }
    if (!rc && use) {
        hipLaunchKernelGGL(k_pig_apply, tgrid, dim3(256), 0, s, a);
        if (form == kPigWord) hipLaunchKernelGGL(k_pig_scatter, rgrid, dim3(256), 0, s, a);
        else if (form == kPigRows) pig_launch_w(k_pigw_scatter<2>, k_pigw_scatter<3>, k_pigw_scatter<4>, a.W, rgrid, s, a);
        else hipLaunchKernelGGL(k_pigl_scatter, rgrid, dim3(256), 0, s, a);
        // entries per block of the pairs kernel: a lane each, or in the long form a group of lgn lanes
        // (the power of two >= W, at least 4)
        const int lgn = form != kPigLong ? 1 : (a.W <= 4 ? 4 : (a.W <= 8 ? 8 : (a.W <= 16 ? 16 : 32)));
        const uint64_t pb = (a.n + 256 / lgn - 1) / (256 / lgn);
        const dim3 pgrid((unsigned)pb, a.G);
        if (pb > 0x7FFFFFFFull) {
            rc = ss_fail(SS_EARG, "all-pairs: n too large");
        } else if (form == kPigWord) {
            if (a.G <= 2) hipLaunchKernelGGL(k_pig_pairs<2>, pgrid, dim3(256), 0, s, a);
            else if (a.G <= 4) hipLaunchKernelGGL(k_pig_pairs<4>, pgrid, dim3(256), 0, s, a);
            else if (a.G <= 8) hipLaunchKernelGGL(k_pig_pairs<8>, pgrid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL(k_pig_pairs<kPigMaxG>, pgrid, dim3(256), 0, s, a);
        } else if (form == kPigRows) {
            pig_launch_w(k_pigw_pairs<2>, k_pigw_pairs<3>, k_pigw_pairs<4>, a.W, pgrid, s, a);
        } else {
            if (lgn == 4) hipLaunchKernelGGL(k_pigl_pairs<4>, pgrid, dim3(256), 0, s, a);
            else if (lgn == 8) hipLaunchKernelGGL(k_pigl_pairs<8>, pgrid, dim3(256), 0, s, a);
            else if (lgn == 16) hipLaunchKernelGGL(k_pigl_pairs<16>, pgrid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL(k_pigl_pairs<32>, pgrid, dim3(256), 0, s, a);
        }
        if (!rc) rc = ss_check(hipGetLastError(), "k_pig_apply / pigeonhole scatter / pairs");
        if (!rc) *done = true;
    }
    const int r2 = ss_check(hipEventRecord(ps.done, s), "pig scratch event");
    return rc ? rc : r2;
}

}  // namespace

extern "C" {

int ss_hamming_all_pairs(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                         uint32_t* d_counts, uint32_t* d_pairs, uint64_t max_pairs, uint64_t* d_npairs,
                         void* stream) {
    return ss_hamming_all_pairs_ex(d_words, n, L, wpr, max_dist, d_counts, d_pairs, max_pairs, d_npairs,
                                   SS_ALLPAIRS_AUTO, stream);
}

int ss_hamming_all_pairs_ex(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                            uint32_t* d_counts, uint32_t* d_pairs, uint64_t max_pairs, uint64_t* d_npairs,
                            uint32_t method, void* stream) {
    if (method > SS_ALLPAIRS_BUCKETED) return ss_fail(SS_EARG, "unknown all-pairs method");
    if (method == SS_ALLPAIRS_BUCKETED && max_dist >= (uint32_t)kPiglMaxG)
        return ss_fail(SS_EARG, "bucketed all-pairs needs max_dist <= 31");
    if (L > SS_MAX_NT) return ss_fail(SS_EARG, "L must be <= 1024");
    const uint32_t W = ham_shape(L).W;
    if (wpr < W || wpr > 32) return ss_fail(SS_EARG, "bad wpr");
    if (!d_npairs) return ss_fail(SS_EARG, "d_npairs is required");
    if (n >= (1ull << 32)) return ss_fail(SS_EARG, "n must be < 2^32");
    hipStream_t s = (hipStream_t)stream;
    // the pigeonhole form (tried first when it may apply) zeroes the outputs in its first kernel
    const uint32_t Pw = ham_shape(L).P;
    // the methods' ranges are the caller's max_dist (forced methods refuse by it); the work below runs
    // on max_dist clamped to Pw (no distance exceeds the Pw compared positions, so the results are
    // the same), which keeps Gw = max_dist + 1 in [1, Pw + 1]: max_dist = 2^32 - 1 would wrap it to 0
    const bool pig_range = max_dist < (uint32_t)kPigMaxG, pigl_range = max_dist < (uint32_t)kPiglMaxG;
    if (max_dist > Pw) max_dist = Pw;
    const uint32_t Gw = max_dist + 1;
    // AUTO on a stream being captured into a hipGraph stays on the tiles: the pigeonhole decision
    // allocates and reads the candidate totals back (a host sync), neither of which a capture allows
    // (the entry point was capturable before AUTO existed)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (method == SS_ALLPAIRS_AUTO && hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) {
        (void)hipGetLastError();
        cap = hipStreamCaptureStatusNone;
    }
    const bool capturing = cap != hipStreamCaptureStatusNone;
    // BUCKETED: pig_all_pairs where it applies (W <= 4, max_dist < 16), the long form past that
    const bool pig_fits = W <= 4 && pig_range;
    const bool pig_forced = method == SS_ALLPAIRS_PIGEONHOLE || (method == SS_ALLPAIRS_BUCKETED && pig_fits);
    const bool pig_try = n >= 2 && W <= 4 && method != SS_ALLPAIRS_TILES && !(capturing && method == SS_ALLPAIRS_AUTO) &&
                         wpr >= W && d_words && !(method == SS_ALLPAIRS_BUCKETED && !pig_fits) &&
                         (pig_forced ? pig_range : pig_range && Pw / Gw >= 3 && n >= (1u << 15));
    // the long form: forced past pig_all_pairs' range; auto for W >= 5 and a batch large enough to
    // pay the host read of the totals (never under capture, as above)
    const bool pigl_try = n >= 2 && d_words && pigl_range &&
                          (method == SS_ALLPAIRS_BUCKETED ? !pig_fits
                                                          : method == SS_ALLPAIRS_AUTO && !capturing && W >= 5 && n >= (1u << 15));
    int rc = SS_OK;
    if (!pig_try && !pigl_try) {
        rc = ss_check(hipMemsetAsync(d_npairs, 0, sizeof(uint64_t), s), "npairs reset");
        if (!rc && d_counts && n) rc = ss_check(hipMemsetAsync(d_counts, 0, n * sizeof(uint32_t), s), "counts reset");
    }
    if (rc || n < 2) return rc;
    if (!d_words || (d_pairs && max_pairs == 0)) return ss_fail(SS_EARG, "null buffer");
    AllPairsArgs a;
    a.words = d_words;
    a.n = n;
    a.wpr = wpr;
    a.W = W;
    a.k = max_dist;
    a.counts = d_counts;
    a.pairs = d_pairs;
    a.max_pairs = d_pairs ? max_pairs : 0;
    a.npairs = (unsigned long long*)d_npairs;
    if (method == SS_ALLPAIRS_PIGEONHOLE && (W > 4 || !pig_range))
        return ss_fail(SS_EARG, "pigeonhole all-pairs needs L <= 128 and max_dist < 16");
    // auto: segments of >= 3 nt and a batch large enough to pay the host read of the totals
    if (pig_try) {
        bool done = false;
        rc = pig_all_pairs(a, W == 1 ? kPigWord : kPigRows, L, Pw, pig_forced, s, &done);
        if (rc || done) return rc;
    }
    if (pigl_try) {
        bool done = false;
        rc = pig_all_pairs(a, kPigLong, L, Pw, method == SS_ALLPAIRS_BUCKETED, s, &done);
        if (rc || done) return rc;
    }
    if (W <= 4) {
        // MFMA form: the Pw compared positions, 8 per k-step, k-steps rounded up to an instantiated count
        return with_mfma_ks(mfma_ks(Pw), [&](auto ks) { return launch_allpairs_mfma<decltype(ks)::value>(a, Pw, s); });
    }
    if (W <= 8) return launch_allpairs<8>(a, s);
    if (W <= 16) return launch_allpairs<16>(a, s);
    return launch_allpairs<32>(a, s);
}

}  // extern "C"
