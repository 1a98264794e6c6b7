// ss_cluster.hip — UMI clustering over the pair list of ss_hamming_all_pairs*: the `cluster`
// (connected components) and `directional` methods of UMI-tools as one min-label fixpoint, and its
// `adjacency` method as a min-rank cover on top of the `cluster` fixpoint (below, "Adjacency").
//
// order = the nodes by count descending, ties by index (identity without d_order); rank = its inverse.
// label[v] starts at rank[v]; a round is a hook pass over the pairs (label[v] = min(label[v], label[u])
// over every edge u -> v; `cluster` takes both directions of every pair, `directional` the directions
// with c[u] + 1 >= 2 c[v]) and a shortcut pass over the nodes (label[v] = label[order[label[v]]],
// chased to its end: the node a label names is v itself or an ancestor of v, and an ancestor's ancestors
// are ancestors, so this holds for directed edges too).  The fixpoint is the lowest rank among v and its
// ancestors, a minimum over integers: it does not depend on pair order or scheduling.
//
// Visibility: labels are lowered only by device-scope atomicMin; they are read by plain loads, which may
// return a value another XCD has since lowered.  A stale value is larger than the true one and still
// names an ancestor, so the atomicMin that follows it lowers less or nothing: safe.  "Lowered" is taken
// only from atomicMin's returned old value; a round in which no atomic lowered a label started from
// labels no kernel has written since the last kernel boundary, so every load in it was fresh and the
// fixpoint test is sound.  The round loop runs on the host (one 16-B read of the changed and bad-index
// flags per round through a pinned word); there is no grid-wide barrier.
//
// Adjacency (UMI-tools: per component, the shortest count-ordered prefix whose nodes and their
// neighbours cover the component are the leads; a lead's group is itself and its neighbours that are
// neither leads nor taken by an earlier lead).  In ranks:
//   1. cover[v] = min(rank[v], rank[u] over v's neighbours u)      one pass over the pairs, before the rounds
//   2. comp[v]  = the lowest rank in v's component                 the `cluster` fixpoint, unchanged
//   3. thr[c]   = max cover[v] over comp[v] == c                   one pass over the nodes
//   4. v leads iff rank[v] <= thr[comp[v]]; rep[v] = v for a lead, order[cover[v]] otherwise
// A prefix of ranks 0 .. i covers a component iff every node has a closed-neighbourhood member of rank
// <= i, so the shortest covering prefix ends at rank thr; global ranks keep the order inside a
// component.  A non-lead's lowest-rank neighbour has rank cover[v] <= thr: a lead, and the first lead in
// order that reaches v.  Every step is a min or a max over integers.  cover is lowered only by
// atomicMin and thr raised only by atomicMax; the plain read in front of either may be stale, which is
// larger (cover) or smaller (thr) than the true value, so the atomic still runs where it matters.
// Kernel boundaries separate the steps: after its own pass each array is read by plain loads.
#include <stdint.h>

#include <vector>

#include "ss_internal.h"

namespace {

constexpr uint32_t kClT = 256;          // threads per block (4 waves; the hook's ballots need whole waves)
constexpr uint32_t kClMaxBlocks = 2048; // grid-stride past this
constexpr uint64_t kClHdrBytes = 64;

// workspace header (u32 words): [0], [1] = the changed flags of even / odd rounds, [2] = a pair named a
// node >= n, [3] = direction bits of the unaligned first pair (bits 0-1) and the odd last pair (2-3)
enum { kHdrChanged = 0, kHdrBad = 2, kHdrEdgeBits = 3 };

struct ClWs {
    uint32_t* hdr;
    uint32_t* label;
    unsigned long long* bits;   // per 64 body units (128 pairs): 4 ballots, bit b of a unit in word b
    uint32_t* cover;            // adjacency only, after the layout of the other methods: u32 [n] each
    uint32_t* thr;
    uint32_t* rank;
};

inline uint64_t cl_label_bytes(uint64_t n) { return (4 * n + 63) / 64 * 64; }
inline uint64_t cl_bits_bytes(uint64_t m) { return ((m / 2 + 63) / 64) * 32 + 32; }

inline uint64_t cl_base_bytes(uint64_t n, uint64_t m) { return kClHdrBytes + cl_label_bytes(n) + cl_bits_bytes(m); }

inline ClWs cl_ws(void* d_ws, uint64_t n, uint64_t m) {
    ClWs w;
    w.hdr = (uint32_t*)d_ws;
    w.label = (uint32_t*)((char*)d_ws + kClHdrBytes);
    w.bits = (unsigned long long*)((char*)d_ws + kClHdrBytes + cl_label_bytes(n));
    w.cover = (uint32_t*)((char*)d_ws + cl_base_bytes(n, m));      // only valid in an adjacency workspace
    w.thr = (uint32_t*)((char*)w.cover + cl_label_bytes(n));
    w.rank = (uint32_t*)((char*)w.thr + cl_label_bytes(n));
    return w;
}

inline unsigned cl_grid(uint64_t items) {
    const uint64_t b = (items + kClT - 1) / kClT;
    return (unsigned)(b < 1 ? 1 : (b > kClMaxBlocks ? kClMaxBlocks : b));
}

// label[order[r]] = r (the inverse rank); the outputs the finish adds into and the header zeroed
__global__ __launch_bounds__(kClT) void k_cl_init(const uint32_t* __restrict__ order, uint32_t* __restrict__ label,
                                                  uint32_t* __restrict__ hdr, uint64_t n, uint32_t* __restrict__ sizes,
                                                  unsigned long long* __restrict__ sums,
                                                  unsigned long long* __restrict__ nclusters) {
    const uint64_t stride = (uint64_t)gridDim.x * kClT;
    const uint64_t t = (uint64_t)blockIdx.x * kClT + threadIdx.x;
    if (t < 4) hdr[t] = 0;
    if (t == 4) *nclusters = 0;
    for (uint64_t r = t; r < n; r += stride) {
        label[order ? order[r] : r] = (uint32_t)r;
        if (sizes) sizes[r] = 0;
        if (sums) sums[r] = 0;
    }
}

// the count rule of `directional` for the edge u -> v (UMI-tools: c[u] >= 2 c[v] - 1; counts <= 2^62)
__device__ __forceinline__ bool cl_dir(unsigned long long cu, unsigned long long cv) { return cu + 1 >= 2 * cv; }

// label[dst] = min(label[dst], ls) where the value read says that lowers it
__device__ __forceinline__ void cl_lower(uint32_t* label, uint32_t dst, uint32_t ls, uint32_t ld, bool& changed) {
    if (ls < ld && atomicMin(&label[dst], ls) > ls) changed = true;
}

// one pair (i, j) with direction bits d (1: i -> j, 2: j -> i)
__device__ __forceinline__ void cl_hook_pair(uint32_t* label, uint32_t i, uint32_t j, uint32_t d, bool& changed) {
    if (!d) return;
    const uint32_t li = label[i], lj = label[j];
    if (d & 1) cl_lower(label, j, li, lj, changed);
    if (d & 2) cl_lower(label, i, lj, li, changed);
}

// direction bits of one pair from scratch: 0 and *bad for a node >= n (never dereferenced), 3 for
// `cluster` (counts null), the count rule otherwise
__device__ __forceinline__ uint32_t cl_pair_bits(uint32_t i, uint32_t j, uint64_t n, const unsigned long long* counts,
                                                 bool& bad) {
    if (i >= n || j >= n) {
        bad = true;
        return 0;
    }
    if (!counts) return 3;
    const unsigned long long ci = counts[i], cj = counts[j];
    return (cl_dir(ci, cj) ? 1u : 0u) | (cl_dir(cj, ci) ? 2u : 0u);
}

// Hook pass.  The pair stream is `head` (0 / 1) pairs up to the first 16-B boundary, nu body units of two
// pairs (one 16-B load per lane) and `tail` (0 / 1) last pair.  MODE 0: `cluster` (both directions; the
// indices are range-checked every round, two compares).  MODE 1: the first `directional` pass: the count
// rule evaluated once, each unit's 4 bits kept as 4 wave ballots.  MODE 2: later `directional` passes,
// from the kept bits (a pair that named a node >= n kept 0: skipped).
template <int MODE>
__global__ __launch_bounds__(kClT) void k_cl_hook(const uint32_t* __restrict__ pairs, uint32_t head, uint64_t nu,
                                                  uint32_t tail, uint64_t n,
                                                  const unsigned long long* __restrict__ counts,
                                                  unsigned long long* __restrict__ bits, uint32_t* __restrict__ label,
                                                  uint32_t* __restrict__ hdr, uint32_t round) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * kClT;
    const uint4* body = (const uint4*)(pairs + 2 * head);
    bool changed = false, bad = false;
    // every lane of a wave runs the same trips (base is wave-uniform): the ballots see whole waves
    for (uint64_t base = (uint64_t)blockIdx.x * kClT + (threadIdx.x & ~63u); base < nu; base += stride) {
        const uint64_t u = base + lane;
        uint4 p = make_uint4(0, 0, 0, 0);
        uint32_t d = 0;
        if (u < nu) {
            p = body[u];
            if (MODE == 2) {
                const unsigned long long* bp = bits + (u >> 6) * 4;
                d = (uint32_t)((bp[0] >> lane) & 1) | (uint32_t)((bp[1] >> lane) & 1) << 1 |
                    (uint32_t)((bp[2] >> lane) & 1) << 2 | (uint32_t)((bp[3] >> lane) & 1) << 3;
            } else {
                d = cl_pair_bits(p.x, p.y, n, MODE == 1 ? counts : nullptr, bad) |
                    cl_pair_bits(p.z, p.w, n, MODE == 1 ? counts : nullptr, bad) << 2;
            }
        }
        if (MODE == 1) {
            const unsigned long long b0 = __ballot(d & 1), b1 = __ballot(d & 2), b2 = __ballot(d & 4),
                                     b3 = __ballot(d & 8);
            if (lane < 4) bits[(base >> 6) * 4 + lane] = lane == 0 ? b0 : lane == 1 ? b1 : lane == 2 ? b2 : b3;
        }
        cl_hook_pair(label, p.x, p.y, d & 3, changed);
        cl_hook_pair(label, p.z, p.w, d >> 2, changed);
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {   // thread 0: the unaligned first pair, thread 1: the odd last one
        const bool is_tail = threadIdx.x == 1;
        if (is_tail ? tail : head) {
            const uint32_t* q = is_tail ? pairs + 2 * ((uint64_t)head + 2 * nu) : pairs;
            const uint32_t i = q[0], j = q[1], sh = is_tail ? 2 : 0;
            uint32_t d;
            if (MODE == 2) {
                d = (hdr[kHdrEdgeBits] >> sh) & 3;
            } else {
                d = cl_pair_bits(i, j, n, MODE == 1 ? counts : nullptr, bad);
                if (MODE == 1 && d) atomicOr(&hdr[kHdrEdgeBits], d << sh);
            }
            cl_hook_pair(label, i, j, d, changed);
        }
    }
    if (bad) atomicOr(&hdr[kHdrBad], 1u);
    if (changed) atomicOr(&hdr[kHdrChanged + (round & 1)], 1u);
}

// Shortcut pass: label[v] follows label[order[.]] to its end.  Zeroes the next round's changed flag.
__global__ __launch_bounds__(kClT) void k_cl_shortcut(const uint32_t* __restrict__ order, uint32_t* __restrict__ label,
                                                      uint32_t* __restrict__ hdr, uint64_t n, uint32_t round) {
    const uint64_t stride = (uint64_t)gridDim.x * kClT;
    const uint64_t t = (uint64_t)blockIdx.x * kClT + threadIdx.x;
    if (t == 0) hdr[kHdrChanged + ((round + 1) & 1)] = 0;
    bool changed = false;
    for (uint64_t v = t; v < n; v += stride) {
        const uint32_t l0 = label[v];
        uint32_t l = l0;
        for (;;) {
            const uint32_t up = label[order ? order[l] : l];
            if (up >= l) break;
            l = up;
        }
        if (l < l0 && atomicMin(&label[v], l) > l) changed = true;
    }
    if (changed) atomicOr(&hdr[kHdrChanged + (round & 1)], 1u);
}

// rep[v] = order[label[v]]; size and count sum added at the representative; clusters counted at their
// representatives.  A cluster that holds most of the nodes would otherwise take one atomic per node on
// one word (measured: 1M nodes, 0.8M in one component, 12 of the call's 13 ms): the lanes of a wave that
// share a representative add once.
constexpr int kPeel = 4;
// One wave's 64 nodes (lane `on`: node v with representative r and count c; called by whole waves):
// the clusters counted, sizes and sums added.
__device__ __forceinline__ void cl_accumulate(uint32_t lane, bool on, uint64_t v, uint32_t r, unsigned long long c,
                                              uint32_t* __restrict__ sizes, unsigned long long* __restrict__ sums,
                                              unsigned long long* __restrict__ nclusters) {
    const unsigned long long roots = __ballot(on && r == (uint32_t)v);
    if (lane == 0 && roots) atomicAdd(nclusters, (unsigned long long)__popcll(roots));
    if (!sizes && !sums) return;
    // up to kPeel representatives per wave are summed in the wave and added once (rem and every
    // branch on it are wave-uniform); what is left after that adds per lane
    unsigned long long rem = __ballot(on);
    bool mine = on;
    for (int it = 0; it < kPeel && rem; ++it) {
        const uint32_t rl = (uint32_t)__shfl((int)r, __ffsll((long long)rem) - 1);
        const bool in = mine && r == rl;
        const unsigned long long mask = __ballot(in);
        rem &= ~mask;
        if (__popcll(mask) == 1) continue;      // its one lane adds below
        unsigned long long s = in ? c : 0;
        if (sums) {
            for (int o = 32; o; o >>= 1) {
                const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)s, o);
                const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(s >> 32), o);
                s += (unsigned long long)hi << 32 | lo;
            }
        }
        if (lane == 0) {
            if (sizes) atomicAdd(&sizes[rl], (uint32_t)__popcll(mask));
            if (sums) atomicAdd(&sums[rl], s);
        }
        mine = mine && !in;
    }
    if (mine) {
        if (sizes) atomicAdd(&sizes[r], 1u);
        if (sums) atomicAdd(&sums[r], c);
    }
}

__global__ __launch_bounds__(kClT) void k_cl_finish(const uint32_t* __restrict__ order, const uint32_t* __restrict__ label,
                                                    const unsigned long long* __restrict__ counts, uint64_t n,
                                                    uint32_t* __restrict__ rep, uint32_t* __restrict__ sizes,
                                                    unsigned long long* __restrict__ sums,
                                                    unsigned long long* __restrict__ nclusters) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * kClT;
    for (uint64_t base = (uint64_t)blockIdx.x * kClT + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t v = base + lane;
        const bool on = v < n;
        uint32_t r = 0;
        unsigned long long c = 0;
        if (on) {
            const uint32_t l = label[v];
            r = order ? order[l] : l;
            rep[v] = r;
            if (sums) c = counts[v];
        }
        cl_accumulate(lane, on, v, r, c, sizes, sums, nclusters);
    }
}

// ---- adjacency ------------------------------------------------------------------------------------
// After k_cl_init (label = rank): cover[v] = rank[v], the rank kept for the finish (label loses it in
// the rounds; null without an order: rank[v] = v), thr[c] = c (a component's lowest rank c is its
// root's own cover, so the maximum is never below it: nodes whose cover is c never need the atomic).
__global__ __launch_bounds__(kClT) void k_cl_adj_init(const uint32_t* __restrict__ label, uint64_t n,
                                                      uint32_t* __restrict__ cover, uint32_t* __restrict__ thr,
                                                      uint32_t* __restrict__ rank) {
    const uint64_t stride = (uint64_t)gridDim.x * kClT;
    for (uint64_t v = (uint64_t)blockIdx.x * kClT + threadIdx.x; v < n; v += stride) {
        const uint32_t r = label[v];
        cover[v] = r;
        if (rank) rank[v] = r;
        thr[v] = (uint32_t)v;
    }
}

// cover[dst] = min(cover[dst], rs) where the value read says that lowers it (cl_lower's idiom)
__device__ __forceinline__ void cl_cover_lower(uint32_t* cover, uint32_t dst, uint32_t rs) {
    if (rs < cover[dst]) atomicMin(&cover[dst], rs);
}

// one pair (i, j): each end's cover takes the other's rank; a node >= n is never dereferenced
__device__ __forceinline__ void cl_cover_pair(const uint32_t* __restrict__ rank, uint32_t* cover, uint32_t i, uint32_t j,
                                              uint64_t n, bool& bad) {
    if (i >= n || j >= n) {
        bad = true;
        return;
    }
    const uint32_t ri = rank[i], rj = rank[j];
    cl_cover_lower(cover, j, ri);
    cl_cover_lower(cover, i, rj);
}

// Cover pass (step 1), over the hook's stream shape: the unaligned head pair, nu 16-B body units, the
// odd tail pair.  Runs before the first round, while label still equals rank and no kernel writes it.
__global__ __launch_bounds__(kClT) void k_cl_cover(const uint32_t* __restrict__ pairs, uint32_t head, uint64_t nu,
                                                   uint32_t tail, uint64_t n, const uint32_t* __restrict__ rank,
                                                   uint32_t* __restrict__ cover, uint32_t* __restrict__ hdr) {
    const uint64_t stride = (uint64_t)gridDim.x * kClT;
    const uint4* body = (const uint4*)(pairs + 2 * head);
    bool bad = false;
    for (uint64_t u = (uint64_t)blockIdx.x * kClT + threadIdx.x; u < nu; u += stride) {
        const uint4 p = body[u];
        cl_cover_pair(rank, cover, p.x, p.y, n, bad);
        cl_cover_pair(rank, cover, p.z, p.w, n, bad);
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {   // thread 0: the unaligned first pair, thread 1: the odd last one
        const bool is_tail = threadIdx.x == 1;
        if (is_tail ? tail : head) {
            const uint32_t* q = is_tail ? pairs + 2 * ((uint64_t)head + 2 * nu) : pairs;
            cl_cover_pair(rank, cover, q[0], q[1], n, bad);
        }
    }
    if (bad) atomicOr(&hdr[kHdrBad], 1u);
}

// thr[c] = max(thr[c], x) where the value read says that raises it
__device__ __forceinline__ void cl_raise(uint32_t* thr, uint32_t c, uint32_t x) {
    if (x > thr[c]) atomicMax(&thr[c], x);
}

// Threshold pass (step 3), after the fixpoint (label = comp).  A giant component sends every node to
// one word (k_cl_finish's note): up to kPeel components per wave take their maximum in the wave and
// one lane raises thr, what is left raises per lane; either only where the value read is lower.
__global__ __launch_bounds__(kClT) void k_cl_thr(const uint32_t* __restrict__ label, const uint32_t* __restrict__ cover,
                                                 uint64_t n, uint32_t* __restrict__ thr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * kClT;
    for (uint64_t base = (uint64_t)blockIdx.x * kClT + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t v = base + lane;
        uint32_t c = 0, x = 0;
        if (v < n) {
            c = label[v];
            x = cover[v];
        }
        bool mine = v < n && x > c;             // cover == comp: thr[c] started there
        unsigned long long rem = __ballot(mine);
        for (int it = 0; it < kPeel && rem; ++it) {
            const uint32_t cl = (uint32_t)__shfl((int)c, __ffsll((long long)rem) - 1);
            const bool in = mine && c == cl;
            const unsigned long long mask = __ballot(in);
            rem &= ~mask;
            if (__popcll(mask) == 1) continue;      // its one lane raises below
            uint32_t mx = in ? x : 0;
            for (int o = 32; o; o >>= 1) {
                const uint32_t other = (uint32_t)__shfl_down((int)mx, o);
                mx = other > mx ? other : mx;
            }
            if (lane == 0) cl_raise(thr, cl, mx);
            mine = mine && !in;
        }
        if (mine) cl_raise(thr, c, x);
    }
}

// Finish (step 4): a lead (rank[v] <= thr[comp[v]]) represents itself, any other node goes to its
// lowest-rank neighbour order[cover[v]]; then as k_cl_finish.
__global__ __launch_bounds__(kClT) void k_cl_adj_finish(const uint32_t* __restrict__ order, const uint32_t* __restrict__ label,
                                                        const uint32_t* __restrict__ cover, const uint32_t* __restrict__ thr,
                                                        const uint32_t* __restrict__ rank,
                                                        const unsigned long long* __restrict__ counts, uint64_t n,
                                                        uint32_t* __restrict__ rep, uint32_t* __restrict__ sizes,
                                                        unsigned long long* __restrict__ sums,
                                                        unsigned long long* __restrict__ nclusters) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * kClT;
    for (uint64_t base = (uint64_t)blockIdx.x * kClT + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t v = base + lane;
        const bool on = v < n;
        uint32_t r = 0;
        unsigned long long c = 0;
        if (on) {
            const uint32_t rk = rank ? rank[v] : (uint32_t)v;
            r = (uint32_t)v;
            if (rk > thr[label[v]]) {
                const uint32_t cv = cover[v];
                r = order ? order[cv] : cv;
            }
            rep[v] = r;
            if (sums) c = counts[v];
        }
        cl_accumulate(lane, on, v, r, c, sizes, sums, nclusters);
    }
}

// the pinned {changed[2], bad, edge bits} copy the host loop reads, one per host thread, made at its first call
uint32_t* cl_pinned_hdr() {
    static thread_local uint32_t* h = nullptr;
    if (!h && hipHostMalloc((void**)&h, 16, hipHostMallocPortable) != hipSuccess) h = nullptr;
    return h;
}

int cl_check_args(uint64_t n, const void* counts, uint32_t method, const void* sums) {
    if (n >= (1ull << 32)) return ss_fail(SS_EARG, "cluster: n must be < 2^32");
    if (method != SS_CLUSTER_COMPONENTS && method != SS_CLUSTER_DIRECTIONAL && method != SS_CLUSTER_ADJACENCY)
        return ss_fail(SS_EARG, "cluster: unknown method");
    // n = 0: an empty array may well be a null pointer
    if (method == SS_CLUSTER_DIRECTIONAL && !counts && n) return ss_fail(SS_EARG, "cluster: directional needs counts");
    if (sums && !counts && n) return ss_fail(SS_EARG, "cluster: sums need counts");
    return SS_OK;
}

}  // namespace

extern "C" {

// header 64 B | label u32 [n] (to 64 B) | direction bits, 32 B per 128 pairs
uint64_t ss_cluster_ws_bytes(uint64_t n, uint64_t m) { return cl_base_bytes(n, m); }

// adjacency: the same, then cover, thr and rank, u32 [n] (to 64 B) each
uint64_t ss_cluster_ws_bytes_method(uint64_t n, uint64_t m, uint32_t method) {
    return cl_base_bytes(n, m) + (method == SS_CLUSTER_ADJACENCY ? 3 * cl_label_bytes(n) : 0);
}

int ss_cluster_pairs(const uint32_t* d_pairs, uint64_t m, uint64_t n, const uint64_t* d_counts, const uint32_t* d_order,
                     uint32_t method, void* d_ws, uint64_t ws_bytes, uint32_t* d_rep, uint32_t* d_sizes, uint64_t* d_sums,
                     uint64_t* d_nclusters, uint32_t* h_rounds, void* stream) {
    int rc = cl_check_args(n, d_counts, method, d_sums);
    if (rc) return rc;
    if (!d_ws || !d_nclusters || (n && !d_rep) || (m && !d_pairs)) return ss_fail(SS_EARG, "cluster: null buffer");
    if ((((uintptr_t)d_ws) & 7) || (((uintptr_t)d_pairs) & 7)) return ss_fail(SS_EARG, "cluster: d_ws and d_pairs must be 8-B aligned");
    if (ws_bytes < ss_cluster_ws_bytes_method(n, m, method)) return ss_fail(SS_EARG, "cluster: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) {
        (void)hipGetLastError();
        cap = hipStreamCaptureStatusNone;
    }
    if (cap != hipStreamCaptureStatusNone) return ss_fail(SS_EARG, "cluster: synchronises per round, cannot be captured");
    uint32_t* h_hdr = cl_pinned_hdr();
    if (!h_hdr) return ss_fail(SS_ENOMEM, "cluster: pinned flag word");

    const ClWs w = cl_ws(d_ws, n, m);
    const unsigned long long* counts = (const unsigned long long*)d_counts;
    unsigned long long* sums = (unsigned long long*)d_sums;
    unsigned long long* ncl = (unsigned long long*)d_nclusters;
    const unsigned gn = cl_grid(n);
    hipLaunchKernelGGL(k_cl_init, dim3(gn), dim3(kClT), 0, s, d_order, w.label, w.hdr, n, d_sizes, sums, ncl);

    const uint32_t head = (m && (((uintptr_t)d_pairs) & 15)) ? 1u : 0u;
    const uint64_t nu = (m - head) / 2;
    const uint32_t tail = (uint32_t)((m - head) & 1);
    const unsigned gm = cl_grid(nu);
    const bool dir = method == SS_CLUSTER_DIRECTIONAL;
    const bool adj = method == SS_CLUSTER_ADJACENCY;
    uint32_t* const rank = d_order ? w.rank : nullptr;
    if (adj) {
        hipLaunchKernelGGL(k_cl_adj_init, dim3(gn), dim3(kClT), 0, s, (const uint32_t*)w.label, n, w.cover, w.thr, rank);
        if (m)
            hipLaunchKernelGGL(k_cl_cover, dim3(gm), dim3(kClT), 0, s, d_pairs, head, nu, tail, n, (const uint32_t*)w.label,
                               w.cover, w.hdr);
    }
    uint32_t rounds = 0;
    while (m) {
        if (!dir)
            hipLaunchKernelGGL(k_cl_hook<0>, dim3(gm), dim3(kClT), 0, s, d_pairs, head, nu, tail, n, counts, w.bits, w.label,
                               w.hdr, rounds);
        else if (rounds == 0)
            hipLaunchKernelGGL(k_cl_hook<1>, dim3(gm), dim3(kClT), 0, s, d_pairs, head, nu, tail, n, counts, w.bits, w.label,
                               w.hdr, rounds);
        else
            hipLaunchKernelGGL(k_cl_hook<2>, dim3(gm), dim3(kClT), 0, s, d_pairs, head, nu, tail, n, counts, w.bits, w.label,
                               w.hdr, rounds);
        hipLaunchKernelGGL(k_cl_shortcut, dim3(gn), dim3(kClT), 0, s, d_order, w.label, w.hdr, n, rounds);
        rc = ss_check(hipGetLastError(), "k_cl_hook/k_cl_shortcut");
        if (!rc) rc = ss_check(hipMemcpyAsync(h_hdr, w.hdr, 16, hipMemcpyDeviceToHost, s), "cluster flag copy");
        if (!rc) rc = ss_check(hipStreamSynchronize(s), "cluster round");
        if (rc) return rc;
        const uint32_t changed = h_hdr[kHdrChanged + (rounds & 1)];
        ++rounds;
        if (h_hdr[kHdrBad]) return ss_fail(SS_EARG, "cluster: a pair names a node >= n");
        if (!changed) break;
    }
    if (adj) {
        if (m) hipLaunchKernelGGL(k_cl_thr, dim3(gn), dim3(kClT), 0, s, (const uint32_t*)w.label, (const uint32_t*)w.cover, n, w.thr);
        hipLaunchKernelGGL(k_cl_adj_finish, dim3(gn), dim3(kClT), 0, s, d_order, (const uint32_t*)w.label,
                           (const uint32_t*)w.cover, (const uint32_t*)w.thr, (const uint32_t*)rank, counts, n, d_rep, d_sizes,
                           sums, ncl);
    } else {
        hipLaunchKernelGGL(k_cl_finish, dim3(gn), dim3(kClT), 0, s, d_order, (const uint32_t*)w.label, counts, n, d_rep,
                           d_sizes, sums, ncl);
    }
    if (h_rounds) *h_rounds = rounds;
    return ss_check(hipGetLastError(), "k_cl_init/k_cl_finish");
}

// The same on the host: union-find keeping each set's lowest rank for `cluster`; for `directional` a
// worklist over the directed edges (CSR by source) that lowers label[v] to label[u] until nothing moves;
// for `adjacency` the union-find for the components, then steps 1, 3 and 4 of the note at the top.
int ss_host_cluster_pairs(const uint32_t* h_pairs, uint64_t m, uint64_t n, const uint64_t* h_counts,
                          const uint32_t* h_order, uint32_t method, uint32_t* h_rep, uint32_t* h_sizes, uint64_t* h_sums,
                          uint64_t* h_nclusters) {
    int rc = cl_check_args(n, h_counts, method, h_sums);
    if (rc) return rc;
    if (!h_nclusters || (n && !h_rep) || (m && !h_pairs)) return ss_fail(SS_EARG, "cluster: null buffer");
    for (uint64_t e = 0; e < 2 * m; ++e)
        if (h_pairs[e] >= n) return ss_fail(SS_EARG, "cluster: a pair names a node >= n");
    std::vector<uint32_t> label(n);
    for (uint64_t r = 0; r < n; ++r) label[h_order ? h_order[r] : r] = (uint32_t)r;
    if (method != SS_CLUSTER_DIRECTIONAL) {
        std::vector<uint32_t> parent(n);
        for (uint64_t v = 0; v < n; ++v) parent[v] = (uint32_t)v;
        auto find = [&](uint32_t v) {
            while (parent[v] != v) {
                parent[v] = parent[parent[v]];
                v = parent[v];
            }
            return v;
        };
        for (uint64_t e = 0; e < m; ++e) {
            const uint32_t a = find(h_pairs[2 * e]), b = find(h_pairs[2 * e + 1]);
            if (a == b) continue;
            if (label[a] < label[b]) parent[b] = a;   // the root of a set is its lowest-rank node
            else parent[a] = b;
        }
        for (uint64_t v = 0; v < n; ++v) h_rep[v] = find((uint32_t)v);
        if (method == SS_CLUSTER_ADJACENCY) {
            std::vector<uint32_t> cover(label), thr(n, 0);          // thr at a component's root node
            for (uint64_t e = 0; e < m; ++e) {
                const uint32_t i = h_pairs[2 * e], j = h_pairs[2 * e + 1];
                if (label[j] < cover[i]) cover[i] = label[j];
                if (label[i] < cover[j]) cover[j] = label[i];
            }
            for (uint64_t v = 0; v < n; ++v)
                if (cover[v] > thr[h_rep[v]]) thr[h_rep[v]] = cover[v];
            for (uint64_t v = 0; v < n; ++v) {
                if (label[v] <= thr[h_rep[v]]) h_rep[v] = (uint32_t)v;
                else h_rep[v] = h_order ? h_order[cover[v]] : cover[v];
            }
        }
    } else {
        std::vector<uint64_t> start(n + 1, 0);
        auto edge = [&](uint32_t u, uint32_t v) { return h_counts[u] + 1 >= 2 * h_counts[v]; };
        for (uint64_t e = 0; e < m; ++e) {
            const uint32_t i = h_pairs[2 * e], j = h_pairs[2 * e + 1];
            if (edge(i, j)) ++start[i + 1];
            if (edge(j, i)) ++start[j + 1];
        }
        for (uint64_t v = 0; v < n; ++v) start[v + 1] += start[v];
        std::vector<uint32_t> dst(start[n]);
        std::vector<uint64_t> fill(start.begin(), start.end() - 1);
        for (uint64_t e = 0; e < m; ++e) {
            const uint32_t i = h_pairs[2 * e], j = h_pairs[2 * e + 1];
            if (edge(i, j)) dst[fill[i]++] = j;
            if (edge(j, i)) dst[fill[j]++] = i;
        }
        // nodes enter the worklist in rank order, so most labels are final the first time they are set
        std::vector<uint32_t> work(n);
        std::vector<uint8_t> queued(n, 1);
        for (uint64_t v = 0; v < n; ++v) work[label[v]] = (uint32_t)v;
        for (size_t head = 0; head < work.size(); ++head) {
            const uint32_t u = work[head];
            queued[u] = 0;
            for (uint64_t k = start[u]; k < start[u + 1]; ++k) {
                const uint32_t v = dst[k];
                if (label[u] < label[v]) {
                    label[v] = label[u];
                    if (!queued[v]) {
                        queued[v] = 1;
                        work.push_back(v);
                    }
                }
            }
        }
        if (h_order) {
            for (uint64_t v = 0; v < n; ++v) h_rep[v] = h_order[label[v]];
        } else {
            for (uint64_t v = 0; v < n; ++v) h_rep[v] = label[v];
        }
    }
    uint64_t ncl = 0;
    for (uint64_t v = 0; v < n; ++v) {
        if (h_sizes) h_sizes[v] = 0;
        if (h_sums) h_sums[v] = 0;
        ncl += h_rep[v] == v;
    }
    for (uint64_t v = 0; v < n; ++v) {
        if (h_sizes) ++h_sizes[h_rep[v]];
        if (h_sums) h_sums[h_rep[v]] += h_counts[v];
    }
    *h_nclusters = ncl;
    return SS_OK;
}

}  // extern "C"
