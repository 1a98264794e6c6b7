// ss_nearest.hip — nearest-reference hamming match: every query row against a second set of rows
// (barcode correction against a whitelist, demultiplexing, feature barcodes).  Per query: the
// minimum distance over the references when it is <= max_dist, the lowest reference index at that
// distance and how many references lie at it (include/shortseq_amd.h has the contract).
//
// Distance = ss_hamming_all_pairs' (the reference __xor__ over W whole words).  L <= 128 runs the
// one-hot v_mfma_i32_32x32x32_i8 tiles of k_allpairs_mfma on a rectangular grid: a block owns S =
// 4 waves x RB row blocks x 32 query rows (A fragments in registers) and sweeps its share of the
// references, staged kStage columns at a time as packed words in LDS; per 32-column block each wave
// builds its B fragments once and runs RB x KS MFMAs.  Same KS / P / table scheme and the same
// folded padding constant as all-pairs: the accumulators start at 128 - thr, a hit is a result >=
// 128, and the distance of a result v is 8 KS + (128 - thr) - v.
// Hits are NOT rare here (a corrected barcode has one reference within the threshold, so a 32 x 32
// tile holds a hit with chance ~min(1, 1024 / nr)): the hit path takes no atomics.  In the D layout
// a result register holds, over the 32 lanes of a half-wave, 32 columns of ONE row; the half-wave
// reduces to (best distance, ballot of the lanes at it -> count and lowest column) and its lane 0
// folds that into the row's LDS state.  A row belongs to one wave and is always folded by the same
// lane, so program order is all the ordering the state needs.  Tiles without a hit leave through
// one ballot as in all-pairs.
// Few row tiles (small nq, large nr): the references are cut into `splits` contiguous ranges
// (blockIdx.y), one partial (dist, idx, count) per (split, query) goes to the caller's workspace and
// k_nearest_finish merges them in split order: lower distance wins, equal distances add their
// counts and keep the lower index.  That rule is associative and commutative, and every fold in the
// tile kernels is the same rule, so the outputs do not depend on the geometry.
// L > 128 (W >= 5): the bit-plane VALU arithmetic of k_allpairs, one query row per lane (planes in
// registers, its running best in registers), reference planes staged in LDS.  Correct, not tuned.
#include <algorithm>

#include "ss_hamming.h"
#include "ss_internal.h"
#include "host_codec.h"   // after the public header (it declares ss_err only without it)

namespace {

using namespace ssd;

constexpr uint32_t kNone = SS_NEAREST_NONE;
constexpr int kStage = 1024;                 // reference columns per LDS stage (MFMA form)
constexpr uint32_t kMaxSplits = 1024;
// Row tiles per launch: x 256 threads must stay below 2^32 work-items (2^24 tiles).  Far lower, so
// that the several-launch path runs at sizes a test can afford (8.4 M rows of 33 .. 128 nt); 2^16
// blocks of >= 128 rows each still fill the device some 60 times over per launch.
constexpr uint64_t kMaxTilesPerLaunch = 1ull << 16;

struct NearArgs {
    const uint64_t* q;
    const uint64_t* ref;
    uint64_t nq, nr;
    uint32_t q_wpr, r_wpr;
    uint32_t W;            // words compared
    uint32_t k;            // max distance, clamped to the compared positions
    uint64_t tile0;        // first row tile of this launch
    uint64_t per_split;    // reference columns per split (a multiple of 32)
    // splits == 1: the outputs themselves (nbest nullable); else the workspace's partials,
    // [split][query] in each of the three arrays
    uint32_t* dist;
    uint32_t* idx;
    uint32_t* nbest;
};

// the merge rule: (d, i, n) <- (d, i, n) + (d2, i2, n2); n2 = 0 (with d2 = i2 = none) is neutral
__device__ __forceinline__ void near_fold(uint32_t& d, uint32_t& i, uint32_t& n, uint32_t d2, uint32_t i2, uint32_t n2) {
    if (d2 < d) {
        d = d2;
        i = i2;
        n = n2;
    } else if (d2 == d && n2) {
        i = i2 < i ? i2 : i;
        n += n2;
    }
}

// Hit path of one 32 x 32 result tile (st = its 16 result registers per lane, [reg][lane]; a hit is
// a result >= 128 in a valid column).  rl0: the tile's first local row, j0: its first column (global
// reference index), valid: this lane's column lies inside the block's reference range.
__device__ __noinline__ void near_hits(const int* st, uint32_t rl0, uint32_t j0, bool valid, int bias, uint32_t* rs_d,
                                       uint32_t* rs_i, uint32_t* rs_n) {
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5;
#pragma unroll 1
    for (int q = 0; q < 16; ++q) {
        const int v = st[q * 64 + lane];
        const bool hit = valid && v >= 128;
        if (!__ballot(hit)) continue;
        int m = hit ? v : -1;
#pragma unroll
        for (int o = 16; o; o >>= 1) m = max(m, __shfl_xor(m, o));       // the half-wave's (= the row's) best
        const uint64_t eq = __ballot(hit && v == m);
        const uint32_t mine = (uint32_t)(eq >> (32u * h));
        if ((lane & 31u) == 0 && mine) {
            const uint32_t rl = rl0 + (q & 3) + 8 * (q >> 2) + 4 * h;
            uint32_t d = rs_d[rl], i = rs_i[rl], n = rs_n[rl];
            near_fold(d, i, n, (uint32_t)(bias - m), j0 + (uint32_t)__ffs((int)mine) - 1u, (uint32_t)__popc(mine));
            rs_d[rl] = d;
            rs_i[rl] = i;
            rs_n[rl] = n;
        }
    }
}

__device__ __forceinline__ void near_store(const NearArgs& a, uint64_t i, uint32_t d, uint32_t j, uint32_t n) {
    const uint64_t o = (uint64_t)blockIdx.y * a.nq + i;      // blockIdx.y = 0 when the outputs are written directly
    a.dist[o] = d;
    a.idx[o] = j;
    if (a.nbest) a.nbest[o] = n;
}

template <int KS, int RB>
__global__ __launch_bounds__(256) void k_nearest_mfma(NearArgs a, uint32_t P) {
    using T = MfmaTiles<KS, RB>;
    constexpr int S = T::S, NW = T::NW;
    __shared__ uint64_t cw[kStage * NW];
    __shared__ uint32_t rs_d[S], rs_i[S], rs_n[S];         // per query row: best distance, lowest index, count
    __shared__ int stash[4 * 1024];                        // hit path: [wave][result reg][lane]
    __shared__ v4i32 ohtab[256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, h = lane >> 5, r = lane & 31u;
    const uint64_t row0 = (a.tile0 + blockIdx.x) * S;
    const uint64_t c_beg = (uint64_t)blockIdx.y * a.per_split;
    const uint64_t c_end = min(a.nr, c_beg + a.per_split);
    ohtab[threadIdx.x] = onehot_entry(threadIdx.x);
    for (int c = threadIdx.x; c < S; c += 256) {
        rs_d[c] = kNone;
        rs_i[c] = kNone;
        rs_n[c] = 0;
    }
    v4i32 A[RB][KS];
    __syncthreads();                                       // the table
    T::load_a(ohtab, a.q, a.nq, a.q_wpr, a.W, row0, A);
    const int thr = T::thr(P, a.k);
    const int bias = 8 * KS + 128 - thr;                   // distance of a result v = bias - v
    const v16i32 Cinit = T::c_init(thr);
    for (uint64_t s0 = c_beg; s0 < c_end; s0 += kStage) {
        __syncthreads();                                   // the previous stage is read
        for (int c = threadIdx.x; c < kStage; c += 256) {
            const uint64_t j = s0 + c;
#pragma unroll
            for (int w = 0; w < NW; ++w) cw[c * NW + w] = (j < c_end && (uint32_t)w < a.W) ? a.ref[j * a.r_wpr + w] : 0ull;
        }
        __syncthreads();
        const uint32_t ncb = (uint32_t)min<uint64_t>(kStage / 32, (c_end - s0 + 31) / 32);
        for (uint32_t cb = 0; cb < ncb; ++cb) {
            const uint32_t cl = cb * 32 + r;               // this lane's column in the stage
            const bool cvalid = s0 + cl < c_end;           // a padding column is "A..A": filtered by index
            v4i32 B[KS];
            onehot_frag_tab<KS>(ohtab, &cw[cl * NW], true, h, B);
            T::sweep(A, B, Cinit, stash, [&](int rb, const int* st) {
                near_hits(st, (wave * RB + rb) * 32, (uint32_t)(s0 + cb * 32), cvalid, bias, rs_d, rs_i, rs_n);
            });
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < S; c += 256) {
        const uint64_t i = row0 + c;
        if (i < a.nq) near_store(a, i, rs_d[c], rs_i[c], rs_n[c]);
    }
}

// L > 128: one query row per lane, bit planes in registers; reference planes staged in LDS
template <int WT>
__global__ __launch_bounds__(256) void k_nearest_valu(NearArgs a) {
    constexpr int C = 4096 / WT;                           // columns per LDS stage
    __shared__ uint2 pl[C * WT];                           // {lo, hi} planes per column word
    const uint64_t i = (a.tile0 + blockIdx.x) * 256 + threadIdx.x;
    const uint64_t c_beg = (uint64_t)blockIdx.y * a.per_split;
    const uint64_t c_end = min(a.nr, c_beg + a.per_split);
    uint32_t alo[WT], ahi[WT];
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        const uint64_t x = (i < a.nq && (uint32_t)w < a.W) ? a.q[i * a.q_wpr + w] : 0ull;
        alo[w] = even_bits(x);
        ahi[w] = even_bits(x >> 1);
    }
    uint32_t bd = kNone, bi = kNone, bn = 0;
    for (uint64_t s0 = c_beg; s0 < c_end; s0 += C) {
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            const uint64_t j = s0 + c;
#pragma unroll
            for (int w = 0; w < WT; ++w) {
                const uint64_t x = (j < c_end && (uint32_t)w < a.W) ? a.ref[j * a.r_wpr + w] : 0ull;
                pl[c * WT + w] = make_uint2(even_bits(x), even_bits(x >> 1));
            }
        }
        __syncthreads();
        const uint32_t ncols = (uint32_t)min<uint64_t>(C, c_end - s0);
        for (uint32_t c = 0; c < ncols; ++c) {
            uint32_t d = 0;
#pragma unroll
            for (int w = 0; w < WT; ++w) {
                const uint2 p = pl[c * WT + w];
                d += __popc((alo[w] ^ p.x) | (ahi[w] ^ p.y));
            }
            if (d <= a.k) near_fold(bd, bi, bn, d, (uint32_t)(s0 + c), 1u);
        }
    }
    if (i < a.nq) near_store(a, i, bd, bi, bn);
}

// splits partials per query -> the outputs, merged in split order (splits = 0: nr = 0, all "none")
__global__ __launch_bounds__(256) void k_nearest_finish(const uint32_t* pd, const uint32_t* pi, const uint32_t* pn,
                                                        uint32_t splits, uint64_t nq, uint32_t* dist, uint32_t* idx,
                                                        uint32_t* nbest) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * 256) {
        uint32_t d = kNone, j = kNone, n = 0;
        for (uint32_t s = 0; s < splits; ++s) {
            const uint64_t o = (uint64_t)s * nq + i;
            near_fold(d, j, n, pd[o], pi[o], pn[o]);
        }
        dist[i] = d;
        idx[i] = j;
        if (nbest) nbest[i] = n;
    }
}

struct NearPlan {
    uint32_t W, P, ks;      // words compared, positions compared, k-steps (MFMA form; 0: VALU form)
    uint32_t S;             // query rows per block
    uint32_t splits;        // reference ranges in use (>= 1 when nr > 0)
    uint64_t per_split;     // columns per range, a multiple of 32
};

NearPlan near_plan(uint64_t nq, uint64_t nr, uint32_t L, uint32_t ref_splits) {
    NearPlan p{};
    const HamShape sh = ham_shape(L);
    p.W = sh.W;
    p.P = sh.P;
    p.ks = p.W <= 4 ? mfma_ks(p.P) : 0;
    p.S = p.ks ? 4 * mfma_rb((int)p.ks) * 32 : 256;
    const uint64_t cblocks = (nr + 31) / 32;
    uint64_t want = ref_splits;
    if (!want) {
        // auto: enough blocks for two per CU when the row tiles alone are fewer, each range at least
        // four LDS stages long.  One point measured (tools/probe_nearest.py splits, 4096 x 2^20 x 16 nt):
        // 1 range 12.8 ms, 8 1.62, 32 0.44, 64 0.317, 128 0.325, 256 0.354; this rule picks 64
        const uint64_t tiles = (nq + p.S - 1) / p.S;
        want = tiles >= 512 ? 1 : std::min<uint64_t>((512 + tiles - 1) / std::max<uint64_t>(tiles, 1), nr / (4 * kStage));
    }
    want = std::max<uint64_t>(1, std::min<uint64_t>({want, cblocks, (uint64_t)kMaxSplits}));
    p.per_split = std::max<uint64_t>(1, (cblocks + want - 1) / want) * 32;
    p.splits = nr ? (uint32_t)((nr + p.per_split - 1) / p.per_split) : 1u;   // no empty range
    return p;
}

uint64_t near_ws(const NearPlan& p, uint64_t nq) { return p.splits > 1 ? 12ull * p.splits * nq : 0ull; }

const char* near_check(uint64_t nq, uint32_t q_wpr, uint64_t nr, uint32_t r_wpr, uint32_t L) {
    if (L < 1 || L > SS_MAX_NT) return "nearest: L must be 1 .. 1024";
    const uint32_t W = ham_shape(L).W;
    if (q_wpr < W || r_wpr < W) return "nearest: q_wpr / r_wpr below the words of L";
    if (nq >= (1ull << 32) || nr >= (1ull << 32)) return "nearest: nq and nr must be < 2^32";
    return nullptr;
}

}  // namespace

extern "C" {

uint64_t ss_hamming_nearest_ws_bytes(uint64_t nq, uint64_t nr, uint32_t L, uint32_t ref_splits) {
    if (L < 1 || L > SS_MAX_NT || nq >= (1ull << 32) || nr >= (1ull << 32)) return 0;
    return near_ws(near_plan(nq, nr, L, ref_splits), nq);
}

int ss_hamming_nearest_ex(const uint64_t* d_q, uint64_t nq, uint32_t q_wpr, const uint64_t* d_ref, uint64_t nr,
                          uint32_t r_wpr, uint32_t L, uint32_t max_dist, uint32_t* d_idx, uint32_t* d_dist,
                          uint32_t* d_nbest, void* d_ws, uint64_t ws_bytes, uint32_t ref_splits, void* stream) {
    if (const char* e = near_check(nq, q_wpr, nr, r_wpr, L)) return ss_fail(SS_EARG, e);
    if (nq == 0) return SS_OK;
    if (!d_q || !d_idx || !d_dist || (nr && !d_ref)) return ss_fail(SS_EARG, "nearest: null buffer");
    const NearPlan p = near_plan(nq, nr, L, ref_splits);
    const uint64_t need = near_ws(p, nq);
    if (need && (!d_ws || ws_bytes < need)) return ss_fail(SS_EARG, "nearest: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const unsigned fgrid = (unsigned)std::min<uint64_t>((nq + 255) / 256, 4096);
    if (nr == 0) {
        hipLaunchKernelGGL(k_nearest_finish, dim3(fgrid), dim3(256), 0, s, nullptr, nullptr, nullptr, 0u, nq, d_dist, d_idx,
                           d_nbest);
        return ss_check(hipGetLastError(), "k_nearest_finish");
    }
    NearArgs a{};
    a.q = d_q;
    a.ref = d_ref;
    a.nq = nq;
    a.nr = nr;
    a.q_wpr = q_wpr;
    a.r_wpr = r_wpr;
    a.W = p.W;
    a.k = max_dist < p.P ? max_dist : p.P;      // no distance exceeds the P compared positions
    a.per_split = p.per_split;
    if (p.splits == 1) {
        a.dist = d_dist;
        a.idx = d_idx;
        a.nbest = d_nbest;
    } else {
        a.dist = (uint32_t*)d_ws;
        a.idx = a.dist + (uint64_t)p.splits * nq;
        a.nbest = a.idx + (uint64_t)p.splits * nq;
    }
    // a launch's work-item count must fit 32 bits: row tiles in runs of kMaxTilesPerLaunch
    const uint64_t tiles = (nq + p.S - 1) / p.S;
    for (uint64_t t0 = 0; t0 < tiles; t0 += kMaxTilesPerLaunch) {
        a.tile0 = t0;
        const dim3 grid((unsigned)std::min<uint64_t>(kMaxTilesPerLaunch, tiles - t0), p.splits);
        if (p.ks) {
            with_mfma_ks(p.ks, [&](auto ks) {
                constexpr int KS = decltype(ks)::value;
                hipLaunchKernelGGL((k_nearest_mfma<KS, mfma_rb(KS)>), grid, dim3(256), 0, s, a, p.P);
            });
        } else if (p.W <= 8) {
            hipLaunchKernelGGL(k_nearest_valu<8>, grid, dim3(256), 0, s, a);
        } else if (p.W <= 16) {
            hipLaunchKernelGGL(k_nearest_valu<16>, grid, dim3(256), 0, s, a);
        } else {
            hipLaunchKernelGGL(k_nearest_valu<32>, grid, dim3(256), 0, s, a);
        }
        const int rc = ss_check(hipGetLastError(), "k_nearest tiles");
        if (rc) return rc;
    }
    if (p.splits > 1) {
        hipLaunchKernelGGL(k_nearest_finish, dim3(fgrid), dim3(256), 0, s, a.dist, a.idx, a.nbest, p.splits, nq, d_dist,
                           d_idx, d_nbest);
        return ss_check(hipGetLastError(), "k_nearest_finish");
    }
    return SS_OK;
}

int ss_hamming_nearest(const uint64_t* d_q, uint64_t nq, uint32_t q_wpr, const uint64_t* d_ref, uint64_t nr,
                       uint32_t r_wpr, uint32_t L, uint32_t max_dist, uint32_t* d_idx, uint32_t* d_dist, uint32_t* d_nbest,
                       void* d_ws, uint64_t ws_bytes, void* stream) {
    return ss_hamming_nearest_ex(d_q, nq, q_wpr, d_ref, nr, r_wpr, L, max_dist, d_idx, d_dist, d_nbest, d_ws, ws_bytes, 0u,
                                 stream);
}

int ss_host_hamming_nearest(const uint64_t* h_q, uint64_t nq, uint32_t q_wpr, const uint64_t* h_ref, uint64_t nr,
                            uint32_t r_wpr, uint32_t L, uint32_t max_dist, uint32_t* h_idx, uint32_t* h_dist,
                            uint32_t* h_nbest) {
    if (const char* e = near_check(nq, q_wpr, nr, r_wpr, L)) return ss_fail(SS_EARG, e);
    if (nq == 0) return SS_OK;
    if (!h_q || !h_idx || !h_dist || (nr && !h_ref)) return ss_fail(SS_EARG, "nearest: null buffer");
    for (uint64_t i = 0; i < nq; ++i) {
        const uint64_t* a = h_q + i * q_wpr;
        uint64_t bd = ~0ull;
        uint32_t bi = kNone, bn = 0;
        for (uint64_t j = 0; j < nr; ++j) {
            const uint64_t d = ssh::hamming(a, h_ref + j * r_wpr, L);
            if (d < bd) {
                bd = d;
                bi = (uint32_t)j;
                bn = 1;
            } else if (d == bd) {
                ++bn;
            }
        }
        const bool found = nr && bd <= max_dist;
        h_dist[i] = found ? (uint32_t)bd : kNone;
        h_idx[i] = found ? bi : kNone;
        if (h_nbest) h_nbest[i] = found ? bn : 0u;
    }
    return SS_OK;
}

}  // extern "C"
