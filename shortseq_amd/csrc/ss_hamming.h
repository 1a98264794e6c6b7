// ss_hamming.h — what the hamming pair kernels share (ss_allpairs.hip, ss_nearest.hip, ss_grouped.hip):
// the compared shape of an L-nt row, bit planes, the waves' LDS pair buffers, and the one-hot
// v_mfma_i32_32x32x32_i8 tiles (fragment table, tile choice, the sweep of one 32-column block).
#pragma once
#include <type_traits>

#include "ss_device.h"

namespace ssd {

// What a distance over L-nt rows compares (the reference's __xor__ runs over whole words): W words,
// P = min(L + 1, 32 W) positions.  Positions > L are code 0 in every packed word; position L can
// carry the table-path alias bit, which the whole-word __xor__ counts.
struct HamShape {
    uint32_t W, P;
};
__host__ __device__ inline HamShape ham_shape(uint32_t L) {
    const uint32_t W = L <= 32u ? 1u : (L + 31u) / 32u;
    return {W, L + 1 < 32u * W ? L + 1 : 32u * W};
}

// even bits of x (nt codes' low bits) -> 32-bit plane; odd bits -> the other plane
// (the bit-plane hamming tiles of ss_allpairs.hip / ss_nearest.hip)
__device__ __forceinline__ uint32_t even_bits(uint64_t x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}

// {lo, hi} planes of the W compared words of row r of a packed batch (stride wpr); a row past n and the
// words W .. WT-1 of the template are zero (k_allpairs, k_gp_pairs)
template <int WT>
__device__ __forceinline__ void load_planes(const uint64_t* words, uint64_t n, uint32_t wpr, uint32_t W, uint64_t r,
                                            uint32_t* lo, uint32_t* hi) {
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        uint64_t x = 0;
        if (r < n && (uint32_t)w < W) x = words[r * wpr + w];
        lo[w] = even_bits(x);
        hi[w] = even_bits(x >> 1);
    }
}

// Hit output of a wave without one global atomic per hit ballot (the pigeonhole pair kernels of
// ss_allpairs.hip, k_gp_pairs): pairs gather in a per-wave LDS buffer and leave in runs (one
// pair-counter atomic per run of up to kPairBuf); count-only calls keep the wave's hit count in a
// register and add it once.  A: any argument struct with pairs, max_pairs and npairs.
constexpr uint32_t kPairBuf = 512;
struct WaveHits {
    uint2* buf;          // this wave's kPairBuf LDS entries
    uint32_t fill = 0;   // wave-uniform
    uint64_t nh = 0;     // wave-uniform (count-only)
};
__device__ __forceinline__ void lds_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <typename A>
__device__ __forceinline__ void hits_flush(const A& a, WaveHits& wh) {
    if (!wh.fill) return;
    lds_wave_sync();
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(a.npairs, (unsigned long long)wh.fill);
    base = __shfl(base, 0);
    for (uint32_t e = lane; e < wh.fill; e += 64) {
        const uint64_t slot = base + e;
        if (slot < a.max_pairs) {
            const uint2 pr = wh.buf[e];
            a.pairs[2 * slot] = pr.x;
            a.pairs[2 * slot + 1] = pr.y;
        }
    }
    lds_wave_sync();
    wh.fill = 0;
}
template <typename A>
__device__ __forceinline__ void hits_add(const A& a, WaveHits& wh, bool hit, uint64_t mask, uint32_t i, uint32_t j) {
    const uint32_t c = (uint32_t)__popcll(mask);
    if (!a.pairs) {
        wh.nh += c;
        return;
    }
    if (wh.fill + c > kPairBuf) hits_flush(a, wh);
    const uint32_t lane = threadIdx.x & 63u;
    if (hit) wh.buf[wh.fill + __popcll(mask & ((1ull << lane) - 1ull))] = make_uint2(min(i, j), max(i, j));
    wh.fill += c;
}

// One-hot i8 fragments of v_mfma_i32_32x32x32_i8 for the hamming tiles (ss_allpairs.hip's header
// has the scheme): position p of a read -> 4 int8 lanes with a 1 at its code.  A 256-entry LDS
// table maps the 4 codes of a byte to the 4 one-hot VGPRs of a k-step half (one ds_read_b128):
// thread t of a 256-thread block writes tab[t] = onehot_entry(t).  k-step s covers positions
// 8s .. 8s+7 = byte 2(s % 4) + h of word s / 4 (h = lane >> 5).
typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef int v16i32 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ v4i32 onehot_entry(uint32_t byte) {
    v4i32 e;
#pragma unroll
    for (int q = 0; q < 4; ++q) e[q] = (int)(1u << (8u * ((byte >> (2 * q)) & 3u)));
    return e;
}

template <int KS>
__device__ __forceinline__ void onehot_frag_tab(const v4i32* tab, const uint64_t* word, bool valid, uint32_t h, v4i32* f) {
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
        const v4i32 z = {0, 0, 0, 0};
        const uint32_t byte = (uint32_t)(word[s2 / 4] >> (16 * (s2 % 4) + 8 * h)) & 0xFFu;
        f[s2] = valid ? tab[byte] : z;
    }
}

// The tile choice.  k-steps: 8 positions each, rounded up to an instantiated count (the padding
// positions P .. 8 KS - 1 are code 0 on both sides and add the constant 8 KS - P to every result,
// folded into the threshold).  Row blocks per wave: more A reuse for short reads, fewer registers
// for long ones (tools/tune_allpairs.hip: KS 2 -> RB 8, KS 4 -> RB 2).
inline uint32_t mfma_ks(uint32_t P) {
    const uint32_t ks = (P + 7) / 8;
    return ks <= 4 ? ks : (ks <= 6 ? 6 : (ks <= 8 ? 8 : (ks <= 12 ? 12 : 16)));
}
constexpr int mfma_rb(int ks) { return ks <= 2 ? 8 : (ks == 3 ? 4 : (ks == 4 ? 2 : 1)); }

// f(std::integral_constant<int, KS>) for ks = mfma_ks(P)
template <typename F>
auto with_mfma_ks(uint32_t ks, F&& f) -> decltype(f(std::integral_constant<int, 1>{})) {
    switch (ks) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 12: return f(std::integral_constant<int, 12>{});
        default: return f(std::integral_constant<int, 16>{});
    }
}

// The tiles of a 256-thread block: 4 waves x RB row blocks of 32 rows = S rows, their A fragments in
// registers; per 32-column block a wave builds its B fragments once and runs RB x KS MFMAs.
template <int KS, int RB>
struct MfmaTiles {
    static constexpr int S = 4 * RB * 32;
    static constexpr int NW = (KS + 3) / 4;                // packed words per row (32 positions each)

    // hit iff matches >= thr over the 8 KS table positions.  The accumulators start at 128 - thr, so a
    // hit is a result >= 128.  thr lies in [0, 8 KS] and matches in [0, 8 KS], 8 KS <= 128, so results
    // lie in [0, 256] (256: identical 128-position rows at max distance >= 128): result >= 128 is bit 7
    // or bit 8, and an OR-reduction of the 16 non-negative registers has one of the two set exactly
    // when one of them is >= 128, so one ballot tests a tile.  Max distance >= P: thr = 0 over the P
    // positions, every pair hits.
    static __device__ __forceinline__ int thr(uint32_t P, uint32_t k) { return max(0, (int)P - (int)k) + (8 * KS - (int)P); }
    static __device__ __forceinline__ v16i32 c_init(int thr) {
        v16i32 c;
#pragma unroll
        for (int q = 0; q < 16; ++q) c[q] = 128 - thr;
        return c;
    }

    // A fragments of this wave's RB row blocks; the block's rows start at row0, rows past n are zero
    static __device__ __forceinline__ void load_a(const v4i32* tab, const uint64_t* rows, uint64_t n, uint32_t wpr,
                                                  uint32_t W, uint64_t row0, v4i32 (*A)[KS]) {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const uint64_t i = row0 + (wave * RB + rb) * 32 + (lane & 31u);
            uint64_t rw[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) rw[w] = (i < n && (uint32_t)w < W) ? rows[i * wpr + w] : 0ull;
            onehot_frag_tab<KS>(tab, rw, i < n, lane >> 5, A[rb]);
        }
    }

    // One 32-column block (B: its fragments) against the wave's RB row blocks.  on_hit(rb) runs for
    // every tile with a result >= 128, the tile's 16 results per lane in st ([reg][lane], this
    // wave's 1024 ints of LDS): an out-of-line loop there keeps the sweep's registers.
    template <typename F>
    static __device__ __forceinline__ void sweep(const v4i32 (*A)[KS], const v4i32* B, const v16i32& Cinit, int* stash,
                                                 F&& on_hit) {
        // RB >= 4 (short reads): all RB tiles of the column block first, one ballot for all of
        // them: no branch between the tiles' MFMA chains, so they interleave; a hit (rare)
        // recomputes the tiles below.  (100k x 12 nt: 14.7 -> 15.6 T pairs/s; at RB <= 2 the
        // per-tile form measured faster.  Two tiles' chains explicitly interleaved with independent
        // accumulators measured level at RB 8, slower at RB 4: profiles/r2/r2f/tune_ap_pair.log.)
        if constexpr (RB >= 4) {
            int any_all = 0;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                v16i32 D = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[rb][0], B[0], Cinit, 0, 0, 0);
#pragma unroll
                for (int s2 = 1; s2 < KS; ++s2) D = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[rb][s2], B[s2], D, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 16; ++q) any_all |= D[q];
            }
            if (!__ballot(any_all & 0x180)) return;
        }
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            v16i32 D = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[rb][0], B[0], Cinit, 0, 0, 0);
#pragma unroll
            for (int s2 = 1; s2 < KS; ++s2) D = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[rb][s2], B[s2], D, 0, 0, 0);
            int any = D[0];
#pragma unroll
            for (int q = 1; q < 16; ++q) any |= D[q];
            if (!__ballot(any & 0x180)) continue;
            int* st = stash + wave * 1024;
#pragma unroll
            for (int q = 0; q < 16; ++q) st[q * 64 + lane] = D[q];
            on_hit(rb, st);
        }
    }
};

}  // namespace ssd
