/*
 * shortseq_amd.h — C ABI of the MI355X (gfx950) batch 2-bit DNA engine.
 *
 * Drop-in boundary for the reference's native kernel layer (AlexTate/ShortSeq, Cython cdef functions
 * exported as PyCapsules in each module's __pyx_capi__).  The reference kernels work
 * on ONE read per call; each entry point below does the same work for a whole batch on the GPU.
 *
 * Conventions
 *   - Plain C types only.  `d_*` arguments are device pointers (hipMalloc / torch CUDA tensors);
 *     `h_*` arguments are host pointers.  `stream` is a hipStream_t passed as void* (NULL = default).
 *   - Device entry points are asynchronous on `stream`, never allocate, never synchronise, and are
 *     safe to capture in a hipGraph.  They return SS_OK or a launch/argument error immediately.
 *     Exceptions, each documented at its declaration: the counter and ingest handles (their own
 *     workspaces; the ingest calls are synchronous), and ss_hamming_all_pairs / _ex when they take
 *     the pigeonhole / bucketed form (a per-device scratch buffer cached across calls; AUTO reads its
 *     candidate totals back with one stream sync), and ss_cluster_pairs (one stream sync per round;
 *     never capturable).  SS_ALLPAIRS_TILES keeps the plain contract.
 *   - Validation mirrors util.pxd:98-99 (bloom filter 0xFFFFFFFFFFEFFF75, util.pyx:75).  A kernel
 *     that meets an invalid byte writes the index of the FIRST invalid read (input order) into
 *     *d_first_bad (atomicMin; the entry point resets it to UINT64_MAX first).  The caller re-scans
 *     that read with ss_host_encode() to obtain the reference's exact error (byte or 8-byte chunk).
 *   - Layouts: read i of a fixed-length batch starts at d_ascii + i*stride (bytes); its packed words
 *     are d_words[i*wpr .. i*wpr + wpr), nt j in word j/32 at bits 2*(j%32) (nt 0 = LSBs), codes
 *     A=0 C=1 T=2 G=3 (README.md:101-112).  wpr >= ceil(L/32) (>= 1); extra words are written 0.
 *
 * Error codes (ss_status): negative = API/runtime error, positive = data error.
 */
#ifndef SHORTSEQ_AMD_H
#define SHORTSEQ_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_ABI_VERSION 1

enum ss_status {
    SS_OK = 0,
    SS_EINVALID_BASE = 1,   /* "Unsupported base character: ..."  (short_seq_64.pyx:105, util.pyx:115/137) */
    SS_ETOO_LONG = 2,       /* "Sequences longer than 1024 bases are not supported." (short_seq.pyx:74) */
    SS_EARG = -1,           /* bad argument (NULL pointer, L out of range, wpr too small, misalignment) */
    SS_EHIP = -2,           /* HIP runtime error; see ss_last_error_string() */
    SS_ENOMEM = -3,         /* device allocation failed (counter handles, forced all-pairs scratch) */
    SS_EFULL = -4           /* counter table full */
};

#define SS_MAX_NT 1024u     /* short_seq_var.pyx:9 */
#define SS_MAX_64_NT 32u    /* short_seq_64.pyx:28 */
#define SS_MAX_192_NT 96u   /* short_seq_192.pyx:22 */

/* Error detail for the host codec (ss_host_encode).  kind = ss_status; for SS_EINVALID_BASE,
 * [byte_offset, byte_offset + nbytes) are the bytes the reference names in its message: 1 byte on
 * the table path (the LAST offending byte, reverse scan), 8 bytes (the chunk) on the full-block path
 * (blocks in order, chunks 3->0 within a block). */
typedef struct ss_err {
    int32_t kind;
    int32_t nbytes;
    int64_t read_index;
    int64_t byte_offset;
} ss_err;

/* ------------------------------------------------------------------------------------------------
 * Library / runtime
 * ---------------------------------------------------------------------------------------------- */
int ss_abi_version(void);
const char* ss_last_error_string(void);          /* thread-local message of the last SS_EHIP/EARG */
int ss_device_count(int* h_count);
int ss_set_device(int device);
int ss_get_device(int* h_device);                   /* the calling thread's current device */

/* Pinned host staging buffers (hipHostMalloc / hipHostFree) for H2D batch staging. */
int ss_pinned_alloc(void** h_ptr, size_t bytes);
int ss_pinned_free(void* h_ptr);

/* ------------------------------------------------------------------------------------------------
 * Batch encode — replaces, per read:
 *   _marshall_bytes_64   (short_seq_64.pyx:96-108)   L <= 32: table path (SURVEY Q1 carry kept)
 *   _marshall_bytes_192  (short_seq_192.pyx:103-108) 33..96  -> _marshall_bytes_array
 *   _marshall_bytes_var  (short_seq_var.pyx:123-132) 97..1024 -> _marshall_bytes_array
 *   _marshall_bytes_array/_full_blocks/_partial_block (util.pyx:78-140): full 32-nt blocks by the
 *   PEXT rule (c>>1)&3, the L%32 tail by the table rule.
 * Fixed length L (1..1024) for every read.  Fast path when L % 16 == 0, stride % 16 == 0 and
 * d_ascii is 16-byte aligned; otherwise a general path (any L, stride >= L).
 * ---------------------------------------------------------------------------------------------- */
int ss_encode_fixed(const uint8_t* d_ascii, uint64_t n, uint32_t L, uint64_t stride,
                    uint64_t* d_words, uint32_t wpr, uint64_t* d_first_bad, void* stream);

/* Variable-length batch: read i = d_ascii[d_offsets[i] .. + d_lens[i]), 0 <= len <= 1024
 * (short_seq.pyx:54-74 length-class switch: 0 -> packed 0, <= 32 table path, else array path).
 * Reads longer than 1024 are reported through *d_first_bad like invalid bases.  The kernel reads the
 * blob in whole 16-B-aligned chunks around each read (device allocations are at least 256-B aligned,
 * so this never leaves the allocation). */
int ss_encode_var(const uint8_t* d_ascii, const uint64_t* d_offsets, const uint32_t* d_lens,
                  uint64_t n, uint64_t* d_words, uint32_t wpr, uint64_t* d_first_bad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batch decode — replaces _unmarshall_bytes_64/_192/_var (short_seq_64.pyx:114-121,
 * short_seq_192.pyx:114-127, short_seq_var.pyx:98-120): nt j -> "ACTG"[code] (util.pyx:52).
 * Writes exactly L bytes per read at d_ascii + i*stride (no terminator).
 * ---------------------------------------------------------------------------------------------- */
int ss_decode_fixed(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr,
                    uint8_t* d_ascii, uint64_t stride, void* stream);

int ss_decode_var(const uint64_t* d_words, const uint32_t* d_lens, uint64_t n, uint32_t wpr,
                  uint8_t* d_ascii, const uint64_t* d_offsets, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Hamming — replaces ShortSeq64/192/Var.__xor__ (short_seq_64.pyx:77-84, short_seq_192.pyx:74-91,
 * short_seq_var.pyx:64-81): sum over W = (L <= 32 ? 1 : ceil(L/32)) words of
 * popcount(((x >> 1) | x) & 0x5555555555555555), x = a ^ b.  Whole-word, like the reference.
 * Dense rows (wpr == W) with 16-B aligned word arrays and an 8-B aligned d_out take the streaming
 * kernels (k_ham_dense / k_ham_dense3w); any other layout the lane-group kernel.  Same results.
 * ---------------------------------------------------------------------------------------------- */
int ss_hamming_ref(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr,
                   const uint64_t* d_ref, uint32_t* d_out, void* stream);
int ss_hamming_pair(const uint64_t* d_a, const uint64_t* d_b, uint64_t n, uint32_t L, uint32_t wpr,
                    uint32_t* d_out, void* stream);

/* Fused encode + hamming vs one packed reference read (d_ref_words, wpr words, e.g. read 0 encoded
 * first): one pass over the ASCII, writes the packed words (if d_words != NULL) and the distance. */
int ss_encode_hamming_ref(const uint8_t* d_ascii, uint64_t n, uint32_t L, uint64_t stride,
                          uint64_t* d_words, uint32_t wpr, const uint64_t* d_ref_words,
                          uint32_t* d_out, uint64_t* d_first_bad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batch slice / subscript — replaces ShortSeq64/192/Var.__getitem__ (short_seq_64.pyx:53-75,
 * short_seq_192.pyx:50-72, short_seq_var.pyx:37-59) -> _slice / _slice_to_ShortSeq64/192/Var /
 * _shift_copy_trim (short_seq.pyx:93-238) and _subscript (short_seq.pyx:78-90, a 1-nt slice):
 * out row r = nts [start, start + len) of read r, packed from bit 0, trimmed to 2*len bits, words
 * past the slice zero.  out_wpr >= max(1, ceil(len/32)).
 * fixed: one (start, len) for the batch, start + len <= L.
 * var:   per-read d_starts / d_lens; with d_read_lens (nullable) they are clamped to the read
 *        (start' = min(start, L_r), len' = min(len, L_r - start')), as Python slice bounds are.
 *        Without d_read_lens they are any u32: a start at or past 32*wpr gives a zero row, and a len
 *        past the row's wpr words ends there (whatever those words hold past the read is copied).
 *        out_wpr may be smaller than ceil(len/32): the row then holds the first 32*out_wpr nts of
 *        the slice.
 * ---------------------------------------------------------------------------------------------- */
int ss_slice_fixed(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t start, uint32_t len,
                   uint64_t* d_out, uint32_t out_wpr, void* stream);
int ss_slice_var(const uint64_t* d_words, uint64_t n, uint32_t wpr, const uint32_t* d_read_lens,
                 const uint32_t* d_starts, const uint32_t* d_lens, uint64_t* d_out, uint32_t out_wpr, void* stream);

/* All-pairs thresholded hamming (UMI-style dedup; distance = __xor__ above) over
 * one batch of n < 2^32 packed reads of length L: for every unordered pair i < j with distance
 * <= max_dist, d_counts[i] and d_counts[j] += 1 (neighbours per read; if d_counts != NULL) and the
 * pair (i, j) is appended as two u32 to d_pairs (if != NULL) while fewer than max_pairs were written.
 * *d_npairs = all such pairs (may exceed max_pairs).  The entry point zeroes d_counts / *d_npairs.
 * Pair order is unspecified (each pair is written as i < j).  n <= 65535 * 1024 per call (L <= 32).
 * Same as ss_hamming_all_pairs_ex(..., SS_ALLPAIRS_AUTO, stream). */
int ss_hamming_all_pairs(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                         uint32_t* d_counts, uint32_t* d_pairs, uint64_t max_pairs, uint64_t* d_npairs,
                         void* stream);

/* Method of ss_hamming_all_pairs_ex; every method gives the same counts, total and pair set.
 * TILES: every pair checked (MFMA one-hot tiles for L <= 128, bit-plane tiles above).
 * PIGEONHOLE (L <= 128, max_dist < 16): the min(L + 1, 32 W) positions split into max_dist + 1
 *   segments (W = ceil(L/32) words; a segment may cross a word boundary); only pairs with an equal
 *   segment are checked (bucketed per segment on the device; a segment past 11 nt by a hash).
 *   Blocks the calling thread once on the stream (the candidate totals are read back) only in AUTO;
 *   forced, it queues everything.  Its scratch lives on the device that holds d_words.
 * BUCKETED (any L <= 1024, any wpr >= W, max_dist <= 31; more is SS_EARG): the same segment rule past
 *   PIGEONHOLE's range.  L <= 128 with max_dist < 16 runs PIGEONHOLE itself; everything else (W >= 5
 *   words, or max_dist 16 .. 31 at any W) runs the long form: rows are not copied into bucket order
 *   (only read indices are; candidate rows are read from d_words, a group of 4 .. 32 lanes per row),
 *   so its scratch does not grow with W.  Scratch per call, G = max_dist + 1 segments and
 *   b = clamp(ceil(log2 n), 10, 22) bucket bits: G * (4 << b) B of histogram, 12 B per 4096 buckets,
 *   and G * n * 8 B of indices (PIGEONHOLE adds G * n * 8 W B of copied rows).  Forced, a scratch
 *   that cannot be allocated is SS_ENOMEM; in AUTO the tiles run instead.  Padding words (wpr > W)
 *   are never read.
 * AUTO: PIGEONHOLE when L <= 128, segments >= 3 nt, n >= 32768 and the bucket histogram shows fewer
 *   than 1/16 of all pairs as candidates; the long form of BUCKETED when L > 128, max_dist <= 31,
 *   n >= 32768 and the histogram shows fewer than 1/32 of all pairs (kPiglRatio, measured apart from
 *   the 1/16: the other side is the slower bit-plane tiles and a candidate costs a gathered row);
 *   TILES otherwise.  A stream under hipGraph capture always gets TILES in AUTO (no allocation, no
 *   host read-back: the call stays capturable). */
#define SS_ALLPAIRS_AUTO 0u
#define SS_ALLPAIRS_TILES 1u
#define SS_ALLPAIRS_PIGEONHOLE 2u
#define SS_ALLPAIRS_BUCKETED 3u
int ss_hamming_all_pairs_ex(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                            uint32_t* d_counts, uint32_t* d_pairs, uint64_t max_pairs, uint64_t* d_npairs,
                            uint32_t method, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Grouped all-pairs thresholded hamming: ss_hamming_all_pairs restricted to groups (UMI dedup per cell
 * barcode x gene, or per mapping position: UMIs are only comparable inside one group, and a sample has
 * 10^5 - 10^7 groups, most of 1 - 20 rows; new in this ABI version, replaces no reference interface).
 * Rows: n < 2^32 packed rows of one length L, 1 .. 1024, at stride wpr >= W, sorted by group.
 * Groups: group g is rows [off[g], off[g + 1]); off has ngroups + 1 u32 entries, is nondecreasing,
 * off[0] = 0 and off[ngroups] = n.  Empty groups are allowed; ngroups == 0 requires n == 0.
 * Distance: exactly that of ss_hamming_all_pairs, the reference __xor__ over W = (L <= 32 ? 1 :
 * ceil(L/32)) whole words, so position L of a one-word row (the table-path alias bit) counts.  Words
 * W .. wpr-1 are never read.
 * Outputs (as ss_hamming_all_pairs): the entry point zeroes d_counts and *d_npairs; every unordered pair
 * i < j OF ONE GROUP within max_dist adds 1 to d_counts[i] and d_counts[j] (nullable) and is appended as
 * two u32 GLOBAL row indices to d_pairs (nullable; max_pairs == 0 also means none) while fewer than
 * max_pairs were written; *d_npairs = all such pairs (may exceed max_pairs).  Pair order is unspecified
 * (each pair is written as i < j).  max_dist is any u32.  The indices being global, ss_cluster_pairs runs
 * on the result as it stands: a pair list that never crosses a group gives clusters inside groups, and
 * its representative is the one a per-group run would choose ("Grouped all-pairs").
 * The device entry points keep the plain contract (asynchronous on `stream`, no allocation, no
 * synchronisation, no host read-back, capturable).  The caller supplies d_ws (8-B aligned) of
 * ss_hamming_all_pairs_grouped_ws_bytes(n, ngroups, L) bytes; this implementation needs none: the
 * function returns 0, d_ws may be NULL and no ws_bytes is too small.
 * Kernel: one block of 256 threads per row tile of 256 consecutive rows, whatever the groups are; a
 * lane owns a row (bit planes in registers) and finds its group's end by a binary search over the
 * offsets; the block walks column chunks from its own tile to its last row's group end, each wave only
 * over [its first row + 1, its last row's group end).  Every pair of a group is checked (bit-plane
 * VALU form at every L): no MFMA tiles and no pigeonhole form inside groups -- for ONE group of 10^5 or
 * more rows ss_hamming_all_pairs is the tool.  All three methods of ss_cluster_pairs, `adjacency`
 * included, run on the grouped pair list as it stands.  Not provided: a grouped form of the whitelist
 * match (ss_hamming_nearest).  tiles_per_launch (_ex; a test hook): row tiles per
 * kernel launch, 0 = the library's 2^23 (larger values are clamped to it); the results do not depend on it.
 * Malformed offsets are NOT detected on the device: the kernel still never reads or writes outside the
 * arrays (every end is clamped to n, an end <= i means "no partners", no index >= n is written to
 * d_pairs); the outputs are then unspecified.
 * SS_EARG (nothing is written): a NULL required pointer (n > 0: d_words, d_group_offsets, d_npairs), L
 * out of range, wpr < W, n >= 2^32, ngroups == 0 with n > 0, a workspace that is too small.
 * ss_host_hamming_all_pairs_grouped: the same function in plain C++ on host arrays over
 * ss_host_hamming's word rule, pairs in ascending (i, j) order; it DOES validate the offsets:
 * off[0] != 0, a decrease, or off[ngroups] != n is SS_EARG, checked before anything is written.
 * ---------------------------------------------------------------------------------------------- */
uint64_t ss_hamming_all_pairs_grouped_ws_bytes(uint64_t n, uint64_t ngroups, uint32_t L);
int ss_hamming_all_pairs_grouped(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                                 const uint32_t* d_group_offsets, uint64_t ngroups,
                                 uint32_t* d_counts, uint32_t* d_pairs, uint64_t max_pairs, uint64_t* d_npairs,
                                 void* d_ws, uint64_t ws_bytes, void* stream);
int ss_hamming_all_pairs_grouped_ex(const uint64_t* d_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                                    const uint32_t* d_group_offsets, uint64_t ngroups,
                                    uint32_t* d_counts, uint32_t* d_pairs, uint64_t max_pairs, uint64_t* d_npairs,
                                    void* d_ws, uint64_t ws_bytes, uint64_t tiles_per_launch, void* stream);
int ss_host_hamming_all_pairs_grouped(const uint64_t* h_words, uint64_t n, uint32_t L, uint32_t wpr, uint32_t max_dist,
                                      const uint32_t* h_group_offsets, uint64_t ngroups,
                                      uint32_t* h_counts, uint32_t* h_pairs, uint64_t max_pairs, uint64_t* h_npairs);

/* ------------------------------------------------------------------------------------------------
 * Nearest-reference hamming match: every query row against a SECOND set of rows (barcode correction
 * against a whitelist, demultiplexing against sample indices, guide / feature barcodes; new in this
 * ABI version, replaces no reference interface).
 * Inputs: nq packed query rows (stride q_wpr words) and nr packed reference rows (stride r_wpr words)
 * of one length L, 1 .. 1024; nq < 2^32, nr < 2^32.
 * Distance: exactly that of ss_hamming_all_pairs, the reference __xor__ over W = (L <= 32 ? 1 :
 * ceil(L/32)) whole words, so position L of a one-word row (the table-path alias bit) counts.  Words
 * W .. wpr-1 of either side are never read.
 * Outputs per query i (u32 each):
 *   d_dist[i]   the minimum distance to any reference if it is <= max_dist, else SS_NEAREST_NONE;
 *   d_idx[i]    the LOWEST reference index at that minimum distance, else SS_NEAREST_NONE;
 *   d_nbest[i]  (nullable) how many references lie at that minimum distance, 0 when none: duplicated
 *               whitelist entries and equidistant neighbours both show here, and a caller corrects a
 *               barcode only when it is 1.
 * max_dist is any u32 (at or above the number of compared positions every reference qualifies: the
 * outputs are the true nearest).  nr == 0 gives "none" for every query; nq == 0 is a no-op, SS_OK.
 * The results do not depend on the launch geometry, on ref_splits or on run order: every merge step
 * carries (distance, lowest index, count) and the rule -- the lower distance wins, equal distances
 * add their counts and keep the lower index -- is associative and commutative.
 * The device entry points keep the plain contract (asynchronous on `stream`, no allocation, no
 * synchronisation, no host read-back, capturable); a size past one launch's grid is split into
 * several launches inside the call.  The caller supplies d_ws (4-B aligned) of
 * ss_hamming_nearest_ws_bytes(nq, nr, L, ref_splits) bytes, with the same ref_splits as the call
 * (ss_hamming_nearest: 0); that is 0 bytes, and d_ws may be NULL, when one reference range is used.
 * Kernels: L <= 128 the one-hot MFMA tiles of the all-pairs form on a rectangular grid, a block of
 * 1024 / 512 / 256 / 128 query rows for min(L + 1, 32 W) <= 16 / 24 / 32 / 128 compared positions;
 * above 128 nt bit-plane tiles, 256 rows per block.  ref_splits (_ex; a test hook) cuts the
 * references into that many contiguous ranges of whole 32-row blocks, one partial result per (range,
 * query) in the workspace, merged in range order by a finishing kernel; a value above ceil(nr / 32)
 * (or 1024) is clamped, ranges are never empty; 0 chooses (more ranges when nq alone gives too few
 * blocks for the device).
 * SS_EARG: a NULL required pointer (nq > 0: d_q, d_idx, d_dist; d_ref when nr > 0), L out of range,
 * q_wpr or r_wpr below W, a workspace that is too small, nq or nr >= 2^32; nothing is written.
 * ss_host_hamming_nearest: the same function in plain C++ on host arrays (a loop over
 * ss_host_hamming's word rule), for small inputs and hosts without a GPU; the same SS_EARG cases,
 * checked before anything is written.
 * ---------------------------------------------------------------------------------------------- */
#define SS_NEAREST_NONE 0xFFFFFFFFu
uint64_t ss_hamming_nearest_ws_bytes(uint64_t nq, uint64_t nr, uint32_t L, uint32_t ref_splits);
int ss_hamming_nearest(const uint64_t* d_q, uint64_t nq, uint32_t q_wpr, const uint64_t* d_ref, uint64_t nr,
                       uint32_t r_wpr, uint32_t L, uint32_t max_dist, uint32_t* d_idx, uint32_t* d_dist, uint32_t* d_nbest,
                       void* d_ws, uint64_t ws_bytes, void* stream);
int ss_hamming_nearest_ex(const uint64_t* d_q, uint64_t nq, uint32_t q_wpr, const uint64_t* d_ref, uint64_t nr,
                          uint32_t r_wpr, uint32_t L, uint32_t max_dist, uint32_t* d_idx, uint32_t* d_dist,
                          uint32_t* d_nbest, void* d_ws, uint64_t ws_bytes, uint32_t ref_splits, void* stream);
int ss_host_hamming_nearest(const uint64_t* h_q, uint64_t nq, uint32_t q_wpr, const uint64_t* h_ref, uint64_t nr,
                            uint32_t r_wpr, uint32_t L, uint32_t max_dist, uint32_t* h_idx, uint32_t* h_dist,
                            uint32_t* h_nbest);

/* ------------------------------------------------------------------------------------------------
 * UMI clustering over a pair list (the step after ss_hamming_all_pairs* in a UMI dedup; new in this ABI
 * version, replaces no reference interface — the reference's shortseq/umi/ package is unfinished).
 * n < 2^32 nodes (distinct UMIs), m undirected pairs (i, j) as two u32 each (any order, duplicates
 * harmless; d_pairs 8-B aligned), optionally a count per node (u64, <= 2^62).  d_order = the nodes by
 * count descending, ties by ascending index (a stable descending sort; NULL = identity; trusted to be
 * a permutation); rank = its inverse.  Methods, named as in UMI-tools:
 *   COMPONENTS  ("cluster"): a node's representative is the lowest-rank node of its connected component.
 *   DIRECTIONAL: a pair gives the edge u -> v iff c[u] + 1 >= 2 c[v] (UMI-tools' c[u] >= 2 c[v] - 1;
 *                both directions may hold); a node's representative is the lowest-rank node among
 *                itself and its directed ancestors, which is the group UMI-tools' count-ordered BFS
 *                with first-observation-wins puts it in.
 *   ADJACENCY:   per connected component, the leads are the shortest prefix of its nodes in rank
 *                order whose members and their neighbours cover the component; a lead represents
 *                itself, any other node goes to its lowest-rank neighbour (a lead, and the first lead
 *                in order that reaches it: UMI-tools' walk over the leads).  In ranks, without the
 *                sequence: (1) cover[v] = min(rank[v], rank[u] over v's neighbours u); (2) comp[v] =
 *                the lowest rank in v's component, as COMPONENTS; (3) thr[c] = max cover[v] over
 *                comp[v] == c; (4) v leads iff rank[v] <= thr[comp[v]], rep[v] = v for a lead and
 *                order[cover[v]] otherwise.  Counts enter only through d_order (and d_sums).
 *                Tie rule: UMI-tools leaves nodes of equal count to set iteration order; here they
 *                rank by ascending index, as under the other methods.
 * The method ids are 0, 1 and 3: the value 2 is not a method and stays SS_EARG.
 * Outputs: d_rep[v] = v's representative; d_sizes / d_sums (nullable; d_sums needs d_counts): a
 * cluster's size and u64 count sum at its representative's index, 0 elsewhere; *d_nclusters.
 * ss_cluster_pairs allocates no device memory: the caller supplies d_ws (8-B aligned,
 * ss_cluster_ws_bytes_method(n, m, method) bytes: for COMPONENTS and DIRECTIONAL that is
 * ss_cluster_ws_bytes(n, m); ADJACENCY adds three u32 [n] arrays behind that layout).  It is NOT capturable and not asynchronous: rounds (a pass over the
 * pairs, a pass over the nodes) repeat until one lowers no label, and the host reads that flag once per
 * round, synchronising with `stream` (through a 16-B pinned word per host thread, made at the thread's
 * first call; SS_ENOMEM if that fails); on a capturing stream it returns SS_EARG.  *h_rounds (nullable)
 * = rounds run, the last, idle one included (0 when m = 0); ADJACENCY runs the rounds of COMPONENTS,
 * one pass over the pairs before them and one over the nodes after them.  The outputs are queued on `stream`.
 * SS_EARG: n >= 2^32, a workspace too small, DIRECTIONAL or d_sums without d_counts (n > 0), an unknown
 * method, or a pair naming a node >= n (never dereferenced: the pair is skipped, the call returns after
 * its first round and the outputs are unspecified).
 * ss_host_cluster_pairs: the same function in plain C++ on host arrays (union-find / a worklist /
 * union-find and the four steps), for
 * small inputs and hosts without a GPU; the same SS_EARG cases, checked before anything is written.
 * ---------------------------------------------------------------------------------------------- */
#define SS_CLUSTER_COMPONENTS 0u
#define SS_CLUSTER_DIRECTIONAL 1u
#define SS_CLUSTER_ADJACENCY 3u
uint64_t ss_cluster_ws_bytes(uint64_t n, uint64_t m);
uint64_t ss_cluster_ws_bytes_method(uint64_t n, uint64_t m, uint32_t method);
int ss_cluster_pairs(const uint32_t* d_pairs, uint64_t m, uint64_t n, const uint64_t* d_counts, const uint32_t* d_order,
                     uint32_t method, void* d_ws, uint64_t ws_bytes, uint32_t* d_rep, uint32_t* d_sizes, uint64_t* d_sums,
                     uint64_t* d_nclusters, uint32_t* h_rounds, void* stream);
int ss_host_cluster_pairs(const uint32_t* h_pairs, uint64_t m, uint64_t n, const uint64_t* h_counts,
                          const uint32_t* h_order, uint32_t method, uint32_t* h_rep, uint32_t* h_sizes, uint64_t* h_sums,
                          uint64_t* h_nclusters);

/* ------------------------------------------------------------------------------------------------
 * Dedup counter — replaces ShortSeqCounter._count_sequence (counter.pyx:41-54): key = (length,
 * packed words) (short_seq_64.pyx:41-44; short_seq_192.pyx:35-41), count += 1, first-occurrence
 * index kept so the host can rebuild dict insertion order.  Open-addressing table in HBM, one per
 * handle; all keys of one handle share one length L <= 1024 (the length is part of the key).
 * The packed word ~0 ("G" * 32) equals the table's EMPTY mark and is counted in a slot of its own,
 * whose key field says nothing: that key is present iff its count (the slot's u32 part plus its entry
 * of the u64 array below) is nonzero.
 * L <= 32: the slot key is the packed word.  L > 32: W = ceil(L/32) words per key, kept beside the
 * slots; the slot holds a 64-bit fingerprint of the words and equality is decided on the words.
 * A slot is 16 B (key u64, count u32, first index u32): global read indices of one handle stay below
 * 2^32 - 1 (inserts past that return SS_EARG).  Counts are u64 (ShortSeqCounter's are Python ints,
 * counter.pyx:53): before the reads inserted since the last spill could wrap a slot's u32, every
 * count moves into a per-slot u64 array (allocated then, 8 B per slot) and ss_counter_merge /
 * _merge_words carry past 32 bits into it; extracts return the sum.  The packed exchange records
 * (ss_counter_pack_ranges) carry u32 counts and flag bit 2 for a count past that.  Packed-word
 * handles (ss_counter_set_words) keep u32 slot counts: the drop-in engine that keys them spills
 * their counts per row itself (its per-row u64 counts).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ss_counter ss_counter;

int ss_counter_create(uint64_t capacity, ss_counter** out);      /* capacity rounded up to 2^k */
int ss_counter_destroy(ss_counter* c);
int ss_counter_reset(ss_counter* c, void* stream);
uint64_t ss_counter_capacity(const ss_counter* c);

/* Reserve workspace (~100 B per read + a small per-region table) so inserts of up to max_reads
 * reads take the partitioned path: reads are bucketed by table region and each region is
 * aggregated by one workgroup in LDS (no per-read global atomics).  Host call (allocates).  L 16/32
 * with 16-B aligned rows encode inside the first partition pass (a key repeated within a 4096-read
 * tile leaves it as one weighted record when its bin is heavy, so skewed inputs keep the partition
 * balanced; records finding their bucket full are counted by a direct insert afterwards); any other
 * L <= 32 / layout is packed into the workspace first.  Inserts larger than the reservation use the
 * direct atomic-insert kernels.  Requires capacity <= 2^26 (32768 regions).  max_reads < 2^31. */
int ss_counter_reserve(ss_counter* c, uint64_t max_reads);
uint64_t ss_counter_reserved(const ss_counter* c);
int ss_counter_release(ss_counter* c);       /* free the workspace (inserts take the direct path) */

/* Encode + count a fixed-length batch (L <= 1024).  Read i gets global index base_index + i.
 * Multi-word handles (L > 32) always take the partitioned path and grow the workspace to n reads
 * (plus n * W words for the packed batch) when the reservation is smaller. 
 * If the batch holds an invalid read (reported through *d_first_bad) the table's contents are
 * unspecified afterwards, like the reference counter that raises mid-list (counter.pyx:22-29). */
int ss_counter_insert_fixed(ss_counter* c, const uint8_t* d_ascii, uint64_t n, uint32_t L,
                            uint64_t stride, uint64_t base_index, uint64_t* d_first_bad, void* stream);

/* Merge already-counted entries (e.g. received from other GPUs): counts add, first index = min. */
int ss_counter_merge(ss_counter* c, const uint64_t* d_keys, const uint32_t* d_lens,
                     const uint64_t* d_counts, const uint64_t* d_first, uint64_t m, void* stream);

/* Merge already-counted multi-word entries (L > 32): d_words[m * W] the key words of entry i (row
 * i), counts add, first index = min.  The m entries must be distinct keys (e.g. the extraction of
 * another handle of the same length, ss_counter_extract_words); keys already in the table are
 * found by their words.  Used to grow a per-length table (ss_ingest).  New in this ABI version;
 * replaces no reference interface (the reference's dict grows by itself, counter.pyx:41-54). */
int ss_counter_merge_words(ss_counter* c, const uint64_t* d_words, const uint64_t* d_counts,
                           const uint64_t* d_first, uint64_t m, void* stream);

/* Test hook: spill the u32 slot counts into the u64 array once more than `reads` (1 .. 2^32 - 1,
 * default 2^32 - 1) reads were inserted since the last spill.  New in this ABI version. */
int ss_counter_set_spill_limit(ss_counter* c, uint64_t reads);

/* Fix the key length of an empty handle (also done by the first insert); -1 from ss_counter_length
 * means not fixed yet, -2 a packed-word handle (ss_counter_set_words). */
int ss_counter_set_length(ss_counter* c, uint32_t L);
int ss_counter_length(const ss_counter* c);

/* Packed-word keys: an empty handle (or one after ss_counter_reset) set to keys of W = 2..64 words,
 * compared whole; ss_counter_insert_words counts n rows d_words[n * W] already packed on the device
 * (row i gets global index base_index + i; partitioned path, workspace grown to n as for multi-word
 * ss_counter_insert_fixed).  The drop-in engine keys one handle per length class this way: the
 * ceil(L/32) words of a read of 32(W-2)+1 .. 32(W-1) nt plus its length as the last word, so one
 * table holds every length of the class (key = (length, words), short_seq_192.pyx:35-41 /
 * short_seq_var.pyx:22-28).  Extract with ss_counter_extract_words (lens = 0: the length is the
 * caller's word); grow with ss_counter_merge_words.  New in this ABI version; replaces no
 * reference interface. */
int ss_counter_set_words(ss_counter* c, uint32_t W);
int ss_counter_insert_words(ss_counter* c, const uint64_t* d_words, uint64_t n, uint64_t base_index, void* stream);

/* Copy the handle's overflow word to *d_flag (device u64): bit 0 = table full during an insert or
 * merge, bit 1 = an extract found more entries than `cap`, bit 2 = a merged count did not fit 32
 * bits, bit 3 = a read index did not fit 32 bits.  Nonzero means the result is invalid. */
int ss_counter_overflow(ss_counter* c, uint64_t* d_flag, void* stream);

/* Per-pass timing of the optimistic partitioned insert (tracing: bench.py's C5 lines attribute the
 * insert's time to its passes).  With on != 0 every such insert records HIP events on its stream
 * between its passes (a ring of 64 inserts, folded as it wraps); ss_counter_pass_times returns the
 * mean ms per insert since the last call of: [0] coarse partition (k_prep + k_pf_coarse), [1] sub-bin
 * order (k_pf_order), [2] fine scatter (k_pf_scatter), [3] aggregate (k_pc_aggregate_slice), [4]
 * spill insert (k_spill_insert), and *h_inserts; then resets the sums.  Host calls.  New in this
 * ABI version; replaces no reference interface. */
int ss_counter_set_timing(ss_counter* c, int on);
int ss_counter_pass_times(ss_counter* c, double* h_ms, uint64_t* h_inserts);

/* Number of occupied slots -> *d_size (device u64). */
int ss_counter_size(ss_counter* c, uint64_t* d_size, void* stream);

/* Compact the table into arrays of capacity `cap` (>= size).  Entries are grouped by owner
 * (hash % n_parts); d_part_counts[n_parts] receives the entries per part, in part order.
 * n_parts = 1 gives a plain compaction.  Order inside a part is unspecified (sort by first index
 * on the host to recover insertion order). */
int ss_counter_extract(ss_counter* c, uint32_t n_parts, uint64_t* d_keys, uint32_t* d_lens,
                       uint64_t* d_counts, uint64_t* d_first, uint64_t cap,
                       uint64_t* d_part_counts, void* stream);

/* Words per key of the handle: 1 for L <= 32, ceil(L/32) for multi-word keys (L 33..1024, the
 * ShortSeq192 / ShortSeqVar keys of short_seq_192.pyx:35-41 / short_seq_var.pyx:22-28; counted
 * under a 64-bit fingerprint of the words, equality always on the full words).  0 for NULL. */
int ss_counter_words(const ss_counter* c);

/* ss_counter_extract for any key length: as ss_counter_extract, plus d_words[cap * W] receives the
 * W packed words of each entry (row i = entry i).  For multi-word handles d_fps gets the entries'
 * fingerprints (the owner partition is owner_of(fingerprint)); for single-word handles d_fps and
 * d_words both get the packed word.  ss_counter_extract itself rejects multi-word handles, and
 * ss_counter_merge takes single-word keys only. */
int ss_counter_extract_words(ss_counter* c, uint32_t n_parts, uint64_t* d_fps, uint32_t* d_lens,
                             uint64_t* d_words, uint64_t* d_counts, uint64_t* d_first, uint64_t cap,
                             uint64_t* d_part_counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FASTQ ingest on the device — replaces _read_fastq_short_seqs (fast_read.pyx:3-20) + _from_chars
 * (short_seq.pyx:49-52) as called by read_and_count_fastq (counter.pyx:57-70): lines split at '\n',
 * 0-based line j kept iff j % 4 == 1, length = strlen(line) - 1 (the '\n' dropped; a final line
 * without '\n' loses its last character; an embedded NUL ends the line).
 * A chunk is < 4 GiB, starts at a line boundary and ends right after a '\n' (or at EOF: at_eof != 0);
 * line0 = lines before the chunk.  d_buf 16-B aligned.
 *   1. ss_fastq_scan: newlines per 16-KiB tile + scan into d_ws (ss_fastq_scan_ws_bytes(nbytes)
 *      bytes); *d_nlines = newlines in the chunk.
 *   2. ss_fastq_index (same d_ws): d_offsets[i] / d_lens[i] of sequence line i (chunk-relative),
 *      *d_nreads = sequence lines in the chunk (may exceed max_reads: then only max_reads are
 *      written; size max_reads from *d_nlines: at most nlines / 4 + 1).  d_aux: max_reads u64 of
 *      scratch.  d_lens[i] = 0xFFFFFFFF where strlen is 0 (the reference's size_t underflow, i.e.
 *      the too-long error); > 1024 is the too-long error as well.
 * or, reading the chunk once:
 *   ss_fastq_index_onepass: the same outputs from one read of the chunk (each 32-KiB tile stages its
 *      newline positions, 4 B per line, and the line numbers are resolved from the tile counts);
 *      d_ws of ss_fastq_onepass_ws_bytes(nbytes, max_reads) bytes; d_counts[3] = {newlines,
 *      sequence lines, staging full}.  max_reads is the caller's bound (a sequence line takes >= 4
 *      bytes of the file: nbytes / 4 + 2 always suffices); the outputs are complete iff
 *      d_counts[2] == 0 and d_counts[1] <= max_reads, otherwise the call is repeated with a larger
 *      max_reads (>= d_counts[1]; doubled when d_counts[2] != 0).
 * The (d_offsets, d_lens) pair is the ragged layout of ss_encode_var and ss_gather_rows.
 * ---------------------------------------------------------------------------------------------- */
uint64_t ss_fastq_scan_ws_bytes(uint64_t nbytes);
int ss_fastq_scan(const uint8_t* d_buf, uint64_t nbytes, void* d_ws, uint64_t ws_bytes, uint64_t* d_nlines,
                  void* stream);
int ss_fastq_index(const uint8_t* d_buf, uint64_t nbytes, uint64_t line0, int at_eof, void* d_ws,
                   uint64_t* d_offsets, uint32_t* d_lens, uint64_t* d_aux, uint64_t max_reads,
                   uint64_t* d_nreads, void* stream);
uint64_t ss_fastq_onepass_ws_bytes(uint64_t nbytes, uint64_t max_reads);
int ss_fastq_index_onepass(const uint8_t* d_buf, uint64_t nbytes, uint64_t line0, int at_eof, void* d_ws,
                           uint64_t ws_bytes, uint64_t* d_offsets, uint32_t* d_lens, uint64_t* d_aux,
                           uint64_t max_reads, uint64_t* d_counts, void* stream);

/* Gather ragged rows into a dense batch: dst row r = d_src[d_offsets[s] .. + L) with s = d_sel[r]
 * (or r when d_sel is NULL); dst_stride % 16 == 0, >= round_up(L, 16); d_dst 16-B aligned; bytes of
 * the last 16-B chunk past L are 'A'.  Reads of d_src stay below src_bytes.  Feeds one length
 * group of a ragged batch (FASTQ, ShortSeqCounter lists) to the fixed-length encode / counter. */
int ss_gather_rows(const uint8_t* d_src, uint64_t src_bytes, const uint64_t* d_offsets, const uint64_t* d_sel,
                   uint64_t m, uint32_t L, uint8_t* d_dst, uint64_t dst_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3' adapter trim of a ragged batch (small-RNA and amplicon libraries: almost every read runs through
 * the insert into the 3' adapter; new in this ABI version, replaces no reference interface).  No read
 * is moved: d_out_lens[i] is read i's length lowered to the adapter's position, and (d_offsets,
 * d_out_lens) is again the ragged layout of ss_encode_var, ss_gather_rows and ss_ingest_add_device.
 * The rule, for a read r[0..L), an adapter a[0..A) with 1 <= A <= 64, min_overlap >= 1, err_div >= 0:
 *   for a position p in 0 .. L-1:  ov(p) = min(A, L - p);
 *     mm(p) = the number of k < ov(p) with a[k] != 'N' and r[p + k] != a[k];
 *     p matches iff ov(p) >= min_overlap and mm(p) <= (err_div ? ov(p) / err_div : 0)  (integer division);
 *   the trimmed length is the LEAST matching p, or L when none matches.
 * Comparison is bytewise and case-sensitive: an 'N', a lower-case letter or any other byte in the READ
 * is an ordinary mismatch; only an 'N' in the adapter is a wildcard.  The match is leftmost, not
 * best-scoring, and has no indels; err_div = 10 is the floor(0.1 * overlap) mismatch budget.  With
 * err_div = 1 every position with enough overlap matches (a read of L >= min_overlap trims to 0), and
 * a short overlap matches by chance (3 bytes: one time in 64), as in every adapter trimmer.
 * Reads with d_lens[i] > SS_MAX_NT (0xFFFFFFFF, the strlen - 1 underflow of ss_fastq_index, included)
 * are left as they are and none of their bytes is read: they stay the too-long error.  Length 0 stays 0.
 * The device entry points keep the plain contract (asynchronous on `stream`, no allocation, no
 * synchronisation, capturable); the adapter travels in the kernel arguments (h_adapter is read before
 * the call returns).  d_out_lens may be d_lens itself.  d_stats (nullable): u64[2] = {reads shortened,
 * bytes removed}, zeroed by the entry point.  n < 2^32.  The blob is read in whole 16-B aligned chunks
 * around each read, as by ss_encode_var: it must be readable to the end of its last 16-B chunk (every
 * device allocation is); offsets and lengths are trusted to lie inside it.
 * reads_per_launch (_ex; a test hook): reads per kernel launch, 0 = the library's 2^28 (larger values
 * are clamped to it); the results do not depend on it.
 * Kernel (k_trim_adapter3): a group of 4 lanes per read stages the read's chunks in LDS and shares its
 * positions in rounds; one position is a SWAR pass over 8 bytes at a time (xor the adapter word, wildcard and
 * overlap masks, nonzero-byte mask, popcount), left as soon as the budget is passed; the group's
 * least match from the wave ballot ("3' adapter trim").
 * SS_EARG (nothing is written): a NULL required pointer with n > 0 (d_blob, d_offsets, d_lens,
 * h_adapter, d_out_lens), A == 0 or A > 64, min_overlap == 0, n >= 2^32.
 * ss_host_trim_adapter3: the same function in plain C++ on host arrays (csrc/host_trim.h per read); it
 * also validates h_offsets[i] + h_lens[i] <= nbytes for every read with h_lens[i] <= SS_MAX_NT
 * (SS_EARG, checked before anything is written).
 * ---------------------------------------------------------------------------------------------- */
int ss_trim_adapter3(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                     uint64_t n, const uint8_t* h_adapter, uint32_t A, uint32_t min_overlap, uint32_t err_div,
                     uint32_t* d_out_lens, uint64_t* d_stats, void* stream);
int ss_trim_adapter3_ex(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                        uint64_t n, const uint8_t* h_adapter, uint32_t A, uint32_t min_overlap, uint32_t err_div,
                        uint32_t* d_out_lens, uint64_t* d_stats, uint64_t reads_per_launch, void* stream);
int ss_host_trim_adapter3(const uint8_t* h_blob, uint64_t nbytes, const uint64_t* h_offsets, const uint32_t* h_lens,
                          uint64_t n, const uint8_t* h_adapter, uint32_t A, uint32_t min_overlap, uint32_t err_div,
                          uint32_t* h_out_lens, uint64_t* h_stats);

/* ------------------------------------------------------------------------------------------------
 * 3' quality trim of a ragged batch (the -q of cutadapt, fastp and BWA: the step that small-RNA and
 * amplicon pipelines run before the adapter cut; new in this ABI version, replaces no reference
 * interface).  As for the adapter no read is moved: d_out_lens[i] is read i's length lowered, and
 * (d_offsets, d_out_lens) is again the ragged layout of ss_encode_var, ss_trim_adapter3 and
 * ss_ingest_add_device.  The rule, for a read of length L <= 1024 with Q >= L quality bytes q[0..Q) of
 * which only q[0..L) are used, a cutoff c in 1..93 and a base b of 33 or 64:
 *   s = 0; best = 0; stop = L
 *   for i = L-1 down to 0:
 *       s += c - (int(q[i]) - b)        (q[i] as an unsigned byte 0..255; the sum fits in 32 bits)
 *       if s < 0: break
 *       if s > best: best = s; stop = i
 *   new length = stop
 * This is BWA's running-sum rule, which cutadapt's -q uses for the 3' end: ties keep the rightmost
 * position (the first maximum met wins), s == 0 neither stops the walk nor moves stop, and any byte
 * value is legal in q (a byte below b is a negative score).  No parity with any tool is claimed or
 * tested.  Reads with d_lens[i] > SS_MAX_NT (0xFFFFFFFF included) stay as they are and none of their
 * bytes is read; length 0 stays 0; neither counts in the statistics.
 * Where the quality bytes are:
 *   explicit form (d_qoffsets != NULL): read i's qualities are the d_lens[i] bytes at d_qual +
 *     d_qoffsets[i] (Q == L by contract; '\n' is an ordinary byte).  d_blob is not read.
 *   FASTQ layout form (d_qoffsets == NULL; d_qual is ignored): d_blob[0..nbytes) is FASTQ text and
 *     (d_offsets, d_lens) come from ss_fastq_index* over it.  e1 = the first '\n' at a position >=
 *     d_offsets[i] + L (exactly there on a normal line, further right on one shortened by a NUL), e2 =
 *     the first '\n' after e1 (the end of the '+' line, which may repeat the header), and the quality
 *     line is [e2 + 1, e3) with e3 = the next '\n' or nbytes, so Q = e3 - e2 - 1.  A read whose e1 or e2
 *     does not exist below nbytes, or with Q < L, keeps its length and counts in stats[2]; with Q > L
 *     the first L bytes are used.  Nothing at or past nbytes is looked at.
 * The device entry points keep the plain contract (asynchronous on `stream`, no allocation, no
 * synchronisation, capturable).  d_out_lens may be d_lens itself.  d_stats (nullable): u64[3] = {reads
 * shortened, bytes removed, reads without a usable quality line}, zeroed by the entry point.  n < 2^32.
 * Memory is read in whole 16-B aligned chunks, as by ss_trim_adapter3: the blob (layout form) or the
 * quality bytes (explicit form) must be readable from the start of their first to the end of their last
 * 16-B chunk (every device allocation is); offsets are trusted.
 * reads_per_launch (_ex; a test hook): reads per kernel launch, 0 = the library's 2^28 (larger values
 * are clamped to it); the results do not depend on it.
 * Kernel (k_trim_quality3): a small group of lanes per read locates the quality line, then walks it from
 * the right in rounds of one 16-B chunk per lane: chunk totals prefix-summed by shuffles, each lane's 16
 * bytes walked exactly from its starting sum, the rightmost lane that goes negative ends the read
 * ("3' quality trim").
 * SS_EARG (nothing is written): a NULL required pointer with n > 0 (d_offsets, d_lens, d_out_lens;
 * d_blob in the layout form), d_qoffsets without d_qual, cutoff 0 or above 93, base not 33 or 64,
 * n >= 2^32.
 * ss_host_trim_quality3: the same function in plain C++ on host arrays (csrc/host_qtrim.h per read);
 * qbytes = the size of h_qual (explicit form).  It also validates, before anything is written, that
 * every read of at most SS_MAX_NT bytes lies inside the blob and, in explicit form, its quality run
 * inside h_qual[0..qbytes) (SS_EARG).
 * ---------------------------------------------------------------------------------------------- */
int ss_trim_quality3(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                     uint64_t n, const uint8_t* d_qual, const uint64_t* d_qoffsets, uint32_t cutoff, uint32_t base,
                     uint32_t* d_out_lens, uint64_t* d_stats, void* stream);
int ss_trim_quality3_ex(const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                        uint64_t n, const uint8_t* d_qual, const uint64_t* d_qoffsets, uint32_t cutoff, uint32_t base,
                        uint32_t* d_out_lens, uint64_t* d_stats, uint64_t reads_per_launch, void* stream);
int ss_host_trim_quality3(const uint8_t* h_blob, uint64_t nbytes, const uint64_t* h_offsets, const uint32_t* h_lens,
                          uint64_t n, const uint8_t* h_qual, uint64_t qbytes, const uint64_t* h_qoffsets, uint32_t cutoff,
                          uint32_t base, uint32_t* h_out_lens, uint64_t* h_stats);

/* Multi-GPU counter with region-range ownership: part p of n owns the table regions
 * [ceil(p R / n), ceil((p + 1) R / n)) (R = capacity / slice slots, ss_counter_geometry); the sentinel
 * key ~0 belongs to the owner of its hash region.  Every rank counts its own reads into its own
 * table, extracts the entries of the OTHER ranks' regions (ss_counter_extract_ranges: grouped by
 * part, each part sorted by region, the sentinel last), exchanges them (all-to-all), and folds what it
 * receives into its own table's owned regions (ss_counter_merge_runs).  The regions a rank does not own
 * are stale afterwards; the union of all ranks' owned regions is the exact counter.
 *   ss_counter_geometry:       host query, log2(capacity) and log2(slots per region).
 *   ss_counter_extract_ranges: as ss_counter_extract with parts = region ranges (single-word keys).
 *   ss_counter_merge_runs:     d_run_offsets = n_runs (begin, end) u64 pairs (device) into the received
 *                              arrays; every run sorted by region and all keys in `part`'s regions;
 *                              d_bounds: n_runs * (regions of part + 1) u32 of scratch. */
int ss_counter_geometry(const ss_counter* c, uint32_t* h_log2cap, uint32_t* h_slice_log);
int ss_counter_extract_ranges(ss_counter* c, uint32_t n_parts, uint64_t* d_keys, uint32_t* d_lens,
                              uint64_t* d_counts, uint64_t* d_first, uint64_t cap, uint64_t* d_part_counts,
                              void* stream);
int ss_counter_merge_runs(ss_counter* c, const uint64_t* d_keys, const uint64_t* d_counts, const uint64_t* d_first,
                          const uint64_t* d_run_offsets, uint32_t n_runs, uint64_t m, uint32_t part,
                          uint32_t n_parts, uint32_t L, uint32_t* d_bounds, void* stream);

/* Packed exchange (the multi-GPU counter's one exchange step in 16-B records instead of three u64
 * arrays): record = {key u64, count u32 | (first - first_base) u32 << 32}.
 * ss_counter_pack_ranges: the entries of every part except skip_part (-1 = none; the caller's own
 *   part stays in its table), grouped by part in part order, inside a part by table region, the
 *   sentinel key ~0 last in its owner's segment; written to d_rec (16-byte aligned, cap records);
 *   d_part_counts[n_parts] (0 for skip_part).  One pass over the table after a partitioned insert
 *   (its aggregate keeps the per-region occupancy), two otherwise.  A count or first - first_base
 *   that does not fit 32 bits, or more than cap records, raises the overflow word (values 4 / 2,
 *   i.e. bits 2 / 1 of ss_counter_overflow); a record's count is the entry's whole u64 count, so one
 *   that fits is never flagged, however it is split between the slot and the u64 array.
 * ss_counter_merge_packed: as ss_counter_merge_runs for packed runs; run r's first indices are
 *   relative to d_run_first_base[r] (the source rank's first_base). */
int ss_counter_pack_ranges(ss_counter* c, uint32_t n_parts, int32_t skip_part, uint64_t first_base, void* d_rec,
                           uint64_t cap, uint64_t* d_part_counts, void* stream);
int ss_counter_merge_packed(ss_counter* c, const void* d_rec, const uint64_t* d_run_offsets,
                            const uint64_t* d_run_first_base, uint32_t n_runs, uint64_t m, uint32_t part,
                            uint32_t n_parts, uint32_t L, uint32_t* d_bounds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ragged read streams counted on the GPU — the batch engine behind the drop-in ShortSeqCounter(list)
 * (counter.pyx:22-39: _count_py_bytes_list -> _from_py_bytes -> _count_sequence) and
 * read_and_count_fastq (counter.pyx:57-70 + fast_read.pyx:3-20).  Host calls, synchronous, one
 * engine per thread; the engine owns its stream, pinned staging and counter tables (one for lengths 1-31 --
 * the packed word with a length marker at bit 2L + 1 -- one for 32, one per length class).
 *   ss_ingest_staging:  a pinned buffer of >= nbytes the caller fills with the reads back to back
 *                       (valid until the next staging / add call).
 *   ss_ingest_add_blob: count n reads of h_blob (read i = the next h_lens[i] bytes); global indices
 *                       continue across calls.
 *   ss_ingest_add_fastq: the sequence lines of a FASTQ file (the fast_read.pyx rule; lengths as
 *                       ss_fastq_index), read in chunks of chunk_bytes (0 = 1 GiB); *h_nseqs = lines.
 *   ss_ingest_error:    the first rejected read in input order: *h_index (UINT64_MAX = none), *h_kind
 *                       (SS_EINVALID_BASE, its bytes -> h_read[0..cap), *h_len; or SS_ETOO_LONG).  The
 *                       caller raises the reference's exception for it (ss_host_encode gives the
 *                       message of an invalid base); nothing after that read is counted.
 *   ss_ingest_finish:   orders the distinct keys by first occurrence (dict insertion order);
 *                       *h_nkeys entries, *h_nwords packed words in total.
 *   ss_ingest_results:  pinned arrays valid until the next reset: lengths u32 [nkeys], counts u64
 *                       [nkeys], words u64 (entry k's max(0, ceil(L/32)) words follow entry k-1's; a
 *                       length-0 entry is the empty read and has none).
 *   ss_ingest_reset:    drop the counts (tables are pooled for the next call).
 *   ss_ingest_set_exact: 1 = size every length class's table by its rows (the 2 x rows bound).  By
 *                       default a class table (lengths 33..1024, one per ceil(L/32)) is sized by a
 *                       HyperLogLog sketch of its distinct keys over the call (1.2 x the estimate +
 *                       256, at most half full); a table that still runs full makes the add call
 *                       return SS_EFULL, and the caller counts again with exact sizing (the drop-in
 *                       front does).  2 = size them by 1/64 of the sketch (a test hook that makes
 *                       the SS_EFULL path run).  3 = test hook: the classes' fingerprint count takes
 *                       its exact fallback (as if two keys shared a 64-bit fingerprint).  4 = as 3,
 *                       but found only after the deferred fold and the speculative finish were queued.
 *                       5 = test hook: the speculative finish's result bound as if the sketch said 0,
 *                       so it is dropped and the finish runs the ordinary way.  New in this ABI
 *                       version; the reference dict has no sizing.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ss_ingest ss_ingest;
int ss_ingest_create(int device, ss_ingest** h_out);
int ss_ingest_destroy(ss_ingest* g);
int ss_ingest_reset(ss_ingest* g);
int ss_ingest_set_exact(ss_ingest* g, int exact);
/* 3' adapter of the engine (the rule of ss_trim_adapter3; new in this ABI version): every later
 * ss_ingest_add_blob, _add_device, _add_fastq and _add_fastq_range trims each chunk's lengths once, on the
 * engine's stream, before anything else sees them (a FASTQ chunk in place right after its index, as
 * part of the index stage; a staged list never as a dense chunk; a caller's device lengths into the
 * engine's own array: the caller's are never written).  Everything after that is unchanged: the first
 * rejected read is judged on its kept prefix only (a bad byte in the removed tail is no error),
 * ss_ingest_error returns the trimmed bytes, a read trimmed to 0 counts as the empty read, and a line
 * of more than 1024 bytes is still the too-long error.  A == 0 clears the setting; it is sticky across
 * ss_ingest_reset, like ss_ingest_set_exact.  SS_EARG: A > 64, or A > 0 with a NULL adapter or
 * min_overlap == 0.  With no adapter set no kernel is queued and no buffer is touched. */
int ss_ingest_set_adapter(ss_ingest* g, const uint8_t* h_adapter, uint32_t A, uint32_t min_overlap, uint32_t err_div);
/* 3' quality cutoff of the engine (the rule of ss_trim_quality3, FASTQ layout form; new in this ABI
 * version): every later ss_ingest_add_fastq and _add_fastq_range lowers each chunk's lengths in place
 * right after its index, on the engine's stream, as part of the index stage and before the adapter trim
 * if one is set (quality first, then the adapter on the kept prefix: the order every trimmer uses).  A
 * chunk ends after a newline, not after a record: where its last sequence line has its quality line in
 * the next bytes of the file (also at the end of a multi-GPU range), the engine reads those one or two
 * lines from the file and applies csrc/host_qtrim.h to that one read, so the result does not depend on
 * the chunk size.  Everything after that is unchanged, as for the adapter: a read is judged on its kept
 * prefix only, a read trimmed to 0 is the empty read, a line of more than 1024 bytes is still the
 * too-long error, and a record whose quality line is missing or short keeps its length.
 * ss_ingest_add_blob and ss_ingest_add_device have no quality bytes: the setting does not apply to them.
 * cutoff 0 clears the setting; it is sticky across ss_ingest_reset.  SS_EARG: cutoff above 93, or a
 * cutoff with a base other than 33 or 64.  With no cutoff set no kernel is queued and no buffer is touched. */
int ss_ingest_set_quality(ss_ingest* g, uint32_t cutoff, uint32_t base);
/* Global read indices of one engine are u64 (a call counts any number of reads); a length's or class's
 * table indexes its rows with a u32 first index, so a group about to pass 2^32 - 1 rows is re-keyed
 * (its distinct keys become its first rows).  Test hook: lower that bound to `rows` (>= 1024) so the
 * re-keying runs at small sizes.  New in this ABI version. */
int ss_ingest_set_row_limit(ss_ingest* g, uint64_t rows);
/* A slot's count is u32: before the reads counted since the last spill pass 2^32 - 2, every table's
 * counts move into its group's u64 row counts (added back at finish / export), so a key's count is
 * exact past 2^32.  Test hook: spill once `reads` (1 .. 2^32 - 2) reads have been counted since the
 * last spill.  New in this ABI version. */
int ss_ingest_set_count_limit(ss_ingest* g, uint64_t reads);
int ss_ingest_staging(ss_ingest* g, uint64_t nbytes, uint8_t** h_ptr);
int ss_ingest_add_blob(ss_ingest* g, const uint8_t* h_blob, const uint32_t* h_lens, uint64_t n);
int ss_ingest_add_fastq(ss_ingest* g, const char* path, uint64_t chunk_bytes, uint64_t* h_nseqs);
/* Multi-GPU FASTQ (counter.pyx:57-70 over one file, split across devices): ss_fastq_split cuts the
 * file into nparts byte ranges h_begin[p] .. h_begin[p + 1] (h_begin has nparts + 1 entries), each
 * starting at a line start and ending after a newline or at the end of the file, and gives the
 * lines before each range (h_line0[p]).  ss_ingest_add_fastq_range counts one range (line0 = the
 * lines before it, so the j % 4 == 1 selection of fast_read.pyx:13 stays global); the ranges'
 * results, taken in range order, are the file's counter (first-occurrence order kept: every read of
 * range p precedes every read of range p + 1).  Host calls.  A range longer than one chunk
 * (chunk_bytes; 0 = 1 GiB) is read by a reader thread into two pinned chunk slots: chunk k + 1's
 * file reads and H2D copies (their own stream) run while chunk k is indexed and counted.  The reader
 * runs on the GPU's NUMA node's CPUs within the process's affinity mask (SHORTSEQ_FQ_PIN=0: not
 * pinned), so its pinned slots and the bytes copied into them are node-local. */
int ss_fastq_split(const char* path, uint32_t nparts, uint64_t* h_begin, uint64_t* h_line0);
int ss_ingest_add_fastq_range(ss_ingest* g, const char* path, uint64_t begin, uint64_t end, uint64_t line0,
                              uint64_t chunk_bytes, uint64_t* h_nseqs);
/* A ragged batch already on this engine's device: read i = d_blob[d_offsets[i], + d_lens[i]) of an
 * nbytes-byte blob (e.g. the output of ss_fastq_index_onepass, or a device-generated batch); counted
 * as ss_ingest_add_blob counts a staged list (same length split, tables and first-occurrence order).
 * Synchronous; the caller's buffers are not kept. */
int ss_ingest_add_device(ss_ingest* g, const uint8_t* d_blob, uint64_t nbytes, const uint64_t* d_offsets,
                         const uint32_t* d_lens, uint64_t n);
int ss_ingest_error(ss_ingest* g, uint64_t* h_index, int* h_kind, uint8_t* h_read, uint64_t cap, uint64_t* h_len);
int ss_ingest_finish(ss_ingest* g, uint64_t* h_nkeys, uint64_t* h_nwords);
/* Stage split of the engine's FASTQ calls since the last call of this (new,
 * replaces nothing): h_ms[5] = host ms of the file reads (pread into pinned memory, in pieces whose
 * H2D copies overlap the next piece's read), device ms of those H2D copies (summed), host ms of the
 * device index to its sync (incl. the wait for its chunk's copies), host ms of the chunk counts,
 * host ms of ss_ingest_finish (reads and copies of a later chunk overlap the index and count of an
 * earlier one, so the stages of a multi-chunk range sum to more than its wall time); *h_h2d_bytes =
 * the bytes the H2D copies moved (their rate = the PCIe rate the call saw). */
int ss_ingest_fastq_stages(ss_ingest* g, double* h_ms, uint64_t* h_h2d_bytes);
int ss_ingest_results(ss_ingest* g, const uint32_t** h_lens, const uint64_t** h_counts, const uint64_t** h_words);
/* Compact results (new in this ABI version; replaces nothing -- the reference's dict holds Python
 * ints): with ss_ingest_set_results_format(g, 1) the finish writes lengths as u16 and counts as u32
 * (*h_count_bytes = 4) unless a count needs u64 (8); the words are as above.  About 15 % fewer bytes
 * over PCIe for ragged keys.  ss_ingest_results refuses the compact format and
 * ss_ingest_results_compact the plain one.  Format 2: compact with u64 counts always (a test hook). */
int ss_ingest_set_results_format(ss_ingest* g, int compact);
int ss_ingest_results_compact(ss_ingest* g, const uint16_t** h_lens, const void** h_counts, uint32_t* h_count_bytes,
                              const uint64_t** h_words);

/* Multi-device reduce of one call (ShortSeqCounter(list) / read_and_count_fastq sharded over several
 * engines, counter.pyx:10-70; north_star: "an RCCL reduce over xGMI only for the final histogram
 * merge").  Engines that counted contiguous shards of one input fold into the first shard's engine on
 * the devices, so every distinct key crosses PCIe once and the host builds the dict from one
 * first-occurrence-ordered row list (no per-shard dict merge).
 *   ss_ingest_export: extract every table of the engine on its own device (entries, counts, and each
 *                     entry's first read); *h_nkeys = its distinct keys.  Run it in the shard's own
 *                     thread after its adds (the shards' exports run concurrently).
 *   ss_ingest_merge:  fold an exported engine into dst: its entries cross to dst's device (peer copies
 *                     over xGMI, hipMemcpyPeerAsync; a device copy when both share a device), become
 *                     rows of dst's tables (short group, length 32, classes) appended as one block (first read =
 *                     src_base + the entry's own), counts add, first index = min.  Sources follow
 *                     dst's reads in input order (src_base = the reads before the source's shard,
 *                     increasing from call to call).  Then ss_ingest_finish(dst) orders the union.
 *                     The caller checks ss_ingest_error of every shard first (the first rejected read
 *                     in input order raises).  Synchronous.  A dst that received merges may itself be
 *                     merged into an engine before it (a reduction tree of adjacent shards: export it
 *                     again first; the merge marks dst un-exported).  Merges into distinct dst
 *                     engines may run concurrently from different host threads.  New in this ABI
 *                     version; the reference has one process-wide dict (counter.pyx:41-54). */
int ss_ingest_export(ss_ingest* g, uint64_t* h_nkeys);
int ss_ingest_merge(ss_ingest* dst, ss_ingest* src, uint64_t src_base);
/* Optional, before a destination's merges: size dst's tables and row maps once for the union of
 * the nsrc (exported) sources' entries, so the merges that follow do not grow a table -- re-inserting
 * every entry it holds -- one merge at a time.  Synchronous.  New in this ABI version. */
int ss_ingest_reserve_merge(ss_ingest* dst, ss_ingest* const* srcs, uint32_t nsrc);

/* ------------------------------------------------------------------------------------------------
 * Synthetic reads on the device (SURVEY §8(d) generator; identical to oracle/ss_oracle.c):
 * read i word w: r = splitmix64(seed + i*W + w) masked to its nts, byte j = "ACTG"[(r >> 2j) & 3].
 * Pool variant: read i is pool item splitmix64(pool_seed ^ (i * 0xD1B54A32D192ED03)) % U.
 * Zipf variant (SURVEY §8(d) C5 skew): read i is pool item rank = #{k : d_cdf[k] <= u63}, u63 =
 * splitmix64(pool_seed ^ (i * 0xD1B54A32D192ED03)) >> 1, for a device table d_cdf[U] of the Zipf
 * CDF scaled to 2^63 (d_cdf[k] = floor(2^63 * P(rank <= k)), d_cdf[U-1] = 2^63; built on the host by
 * shortseq_amd.batch.zipf_cdf).  Item 0 is the most frequent.
 * ---------------------------------------------------------------------------------------------- */
int ss_synth_reads(uint8_t* d_ascii, uint64_t seed, uint64_t i0, uint64_t n, uint32_t L,
                   uint64_t stride, void* stream);
int ss_synth_pool_reads(uint8_t* d_ascii, uint64_t seed, uint64_t pool_seed, uint64_t U,
                        uint64_t i0, uint64_t n, uint32_t L, uint64_t stride, void* stream);
int ss_synth_zipf_reads(uint8_t* d_ascii, uint64_t seed, uint64_t pool_seed, const uint64_t* d_cdf, uint64_t U,
                        uint64_t i0, uint64_t n, uint32_t L, uint64_t stride, void* stream);
/* Ragged pool reads (mixed lengths): read i draws pool item
 * p = splitmix64(pool_seed ^ i * 0xD1B54A32D192ED03) % U of length
 * Lmin + splitmix64(seed ^ 0x6A09E667F3BCC909 ^ p) % (Lmax - Lmin + 1), word w = splitmix64(seed + 32 p + w)
 * masked.  ss_synth_ragged_lens writes the n lengths; the caller lays the blob out (d_offsets, e.g.
 * an exclusive prefix sum of the lengths) and ss_synth_ragged_reads writes the ASCII there. */
int ss_synth_ragged_lens(uint32_t* d_lens, uint64_t seed, uint64_t pool_seed, uint64_t U, uint64_t i0, uint64_t n,
                         uint32_t Lmin, uint32_t Lmax, void* stream);
int ss_synth_ragged_reads(uint8_t* d_blob, const uint64_t* d_offsets, uint64_t seed, uint64_t pool_seed, uint64_t U,
                          uint64_t i0, uint64_t n, uint32_t Lmin, uint32_t Lmax, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Host-resident batches (the host side stages read batches in pinned
 * memory).  Replaces, for a whole host array, the per-object marshal/unmarshal loops the Cython front
 * runs today (short_seq_64.pyx:96-121, util.pyx:78-140, short_seq_var.pyx:98-120).
 * A stager owns a ring of `nslots` (2..16) pinned + device chunk slots of `chunk_bytes` each and
 * three HIP streams (H2D, kernel, D2H); a call streams the batch through it chunk by chunk so the
 * copies and the kernel of neighbouring chunks overlap.  Host buffers may be pageable (staged by
 * `copy_threads` memcpy threads; 0 = the calling thread) or pinned (DMA'd directly, detected per
 * call).  Calls are synchronous (they return when the outputs are in host memory) and must not be
 * made concurrently on one stager.  *h_first_bad = first invalid read (input order) or UINT64_MAX;
 * the rc stays SS_OK for data errors, as for the device entry points.
 * ss_decode_host writes L bytes per read at h_ascii + i*stride; bytes L..stride of a row are
 * unspecified.  d_ref_words (encode_hamming) is a device pointer, ready before the call.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ss_stager ss_stager;
int ss_stager_create(int device, uint64_t chunk_bytes, uint32_t nslots, uint32_t copy_threads,
                     ss_stager** h_out);
int ss_stager_destroy(ss_stager* st);
/* Stage split and placement of a stager (new, replaces nothing).  With timing on,
 * every call records event pairs per chunk.  ss_stager_stats returns, per call since its last call
 * (timed calls), h_ms[6] = host ms of the pageable -> pinned copies, host ms of the pinned ->
 * pageable copies, device ms of the H2D copies, the kernels and the D2H copies (sums over chunks:
 * they overlap across chunks), host ms waiting on the D2H events; and h_info[4] = copy threads, CPUs
 * in the process's affinity mask, the GPU's NUMA node (-1 unknown), CPUs the copy threads are pinned
 * to (the node's CPUs within the mask; 0 = not pinned, also with SHORTSEQ_STAGE_PIN=0). */
int ss_stager_set_timing(ss_stager* st, int on);
int ss_stager_stats(ss_stager* st, double* h_ms, int32_t* h_info);
int ss_encode_host(ss_stager* st, const uint8_t* h_ascii, uint64_t n, uint32_t L, uint64_t stride,
                   uint64_t* h_words, uint32_t wpr, uint64_t* h_first_bad);
int ss_encode_hamming_ref_host(ss_stager* st, const uint8_t* h_ascii, uint64_t n, uint32_t L, uint64_t stride,
                               uint64_t* h_words, uint32_t wpr, const uint64_t* d_ref_words, uint32_t* h_out,
                               uint64_t* h_first_bad);
int ss_decode_host(ss_stager* st, const uint64_t* h_words, uint64_t n, uint32_t L, uint32_t wpr,
                   uint8_t* h_ascii, uint64_t stride);

/* ------------------------------------------------------------------------------------------------
 * Host codec (per-object path, no GPU): the drop-in Python objects use these for single reads,
 * where a kernel launch (~µs) would cost more than the work (SURVEY §7 hard parts).
 * ---------------------------------------------------------------------------------------------- */
int ss_host_encode(const uint8_t* h_seq, uint64_t L, uint64_t* h_words, ss_err* h_err);
void ss_host_decode(const uint64_t* h_words, uint64_t L, char* h_out);
uint64_t ss_host_hamming(const uint64_t* h_a, const uint64_t* h_b, uint64_t L);

#ifdef __cplusplus
}
#endif
#endif /* SHORTSEQ_AMD_H */
