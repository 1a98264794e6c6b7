"""Inputs for tests/test_allpairs_shapes.py: row counts at the edges of every tile and block of
ss_hamming_all_pairs_ex (shortseq_amd/csrc/ss_allpairs.hip), dense batches whose pair lists run
through the pigeonhole form's broadcast tile walk and the waves' hit buffers (hits_add / hits_flush in
ss_hamming.h), and the CPU reference.

Reference: the oracle's hamming_ref_batch over every pair (brute), as _brute of test_allpairs*.py, with
the expected pairs as one sorted int64 key array (i << 32 | j): the dense cases have 10^5 to 10^6 pairs.

Constants named k* and the functions tile_rows, split, nbmax and bucket restate ss_allpairs.hip /
ss_hamming.h; if one changes there, change it here.  They aim the inputs and state the CPU-side
conditions of tests/test_allpairs_shapes.py (a bucket run of >= 257 rows, more than kPairBuf hits in
a wave's run, a segment with two scan tiles); no expectation comes from them.  Seeded.
"""
import collections
import functools

import numpy as np

U32MAX = 2**32 - 1
ACGT = np.frombuffer(b"ACGT", np.uint8)

kPairBuf = 512          # hits a wave buffers in LDS before it flushes (ss_hamming.h)
kPigTileWalk = 256      # a wave's entry run past this is walked as broadcast tiles (k_pig_pairs)
kPigTile = 4096         # buckets per scan tile (k_pig_tile / k_pig_apply)
kPigMaxBits = 22
MUL = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


# ---- shapes ---------------------------------------------------------------------------------------
def shape(L):
    """ham_shape: W compared words, P = min(L + 1, 32 W) compared positions."""
    W = 1 if L <= 32 else (L + 31) // 32
    return W, min(L + 1, 32 * W)


def mfma_ks(P):
    ks = (P + 7) // 8
    return ks if ks <= 4 else (6 if ks <= 6 else (8 if ks <= 8 else (12 if ks <= 12 else 16)))


def tile_rows(L):
    """Rows per tile of the tiled form that serves L: 4 x RB x 32 of the MFMA tiles (W <= 4), 256 of
    the bit-plane tiles."""
    W, P = shape(L)
    if W > 4:
        return 256
    ks = mfma_ks(P)
    rb = 8 if ks <= 2 else (4 if ks == 3 else (2 if ks == 4 else 1))
    return 4 * rb * 32


def chunk_cols(L):
    """Columns per LDS chunk of the bit-plane tiles (Tile<WT>::C), None for the MFMA tiles."""
    W, _ = shape(L)
    if W <= 4:
        return None
    WT = 8 if W <= 8 else (16 if W <= 16 else 32)
    return min(256, 1024 if WT <= 4 else 4096 // WT)


# L -> (family, S) of the instantiated tile families
TILE_FAMILIES = {
    7: ("mfma-ks1", 1024), 12: ("mfma-ks2", 1024), 20: ("mfma-ks3", 512), 31: ("mfma-ks4", 256),
    32: ("mfma-ks4", 256), 33: ("mfma-ks6", 128), 64: ("mfma-ks8", 128), 65: ("mfma-ks12", 128),
    128: ("mfma-ks16", 128), 129: ("planes-wt8", 256), 300: ("planes-wt16", 256), 1000: ("planes-wt32", 256),
}


def tile_ns(L):
    S = TILE_FAMILIES[L][1]
    ns = {0, 1, 2, 3, 31, 32, 33, 64, 65, S - 1, S, S + 1, 2 * S + 1}
    C = chunk_cols(L)
    if C is not None and C < S:      # WT 32: the chunk edge and its `j0 >= a.n` break
        ns |= {C - 1, C, C + 1, S + C - 1, S + C + 1}
    return sorted(ns)


def small_k(L):
    return 1 if L <= 32 else 2


TILE_CASES = [(L, n) for L in TILE_FAMILIES for n in tile_ns(L)]

# (form, L, k, forced method): the template or lane-group size is in the comment of the issue's table
PIG_FORMS = [
    ("word-2", 12, 1, "pigeonhole"), ("word-4", 16, 3, "pigeonhole"), ("word-8", 31, 5, "pigeonhole"),
    ("word-16", 30, 12, "pigeonhole"),
    ("rows-w2", 40, 2, "pigeonhole"), ("rows-w3", 80, 2, "pigeonhole"), ("rows-w4", 128, 2, "pigeonhole"),
    ("long-lg4", 20, 20, "bucketed"), ("long-lg8", 150, 3, "bucketed"), ("long-lg16", 300, 3, "bucketed"),
    ("long-lg32", 993, 20, "bucketed"),
]
PIG_NS = [2, 3, 63, 64, 65, 255, 256, 257, 513, 1024, 1025]      # 1024 -> 1025: nbmax 10 -> 11


def lane_group(L):
    """Lanes per entry of the long form (k_pigl_pairs<LG>)."""
    W, _ = shape(L)
    return 4 if W <= 4 else (8 if W <= 8 else (16 if W <= 16 else 32))


def pig_ns(form, L):
    ns = set(PIG_NS)
    if form.startswith("long"):
        e = 256 // lane_group(L)          # entries per block of the long form
        ns |= {e - 1, e, e + 1}
    return sorted(ns)


PIG_CASES = [(form, L, k, m, n) for form, L, k, m in PIG_FORMS for n in pig_ns(form, L)]
# n = 4097: nbmax = 13 and a segment of >= 13 bits, so two scan tiles
PIG_TWO_TILES = [("word", 32, 1, "pigeonhole"), ("rows", 40, 1, "pigeonhole"), ("long", 150, 3, "bucketed")]

# (L, k): the forms of the dense batches: one-word <2> <4> <8>, MFMA P = 32, MFMA KS 6, row copies
# W = 2 and 4, the long form at W = 1, 5 and 32, the bit-plane tiles at WT 8 and 32
DENSE_SHAPES = [(12, 1), (16, 3), (31, 5), (32, 1), (33, 2), (40, 2), (128, 2), (20, 20), (150, 3), (993, 20), (1000, 3)]
ONE_READ_NS = [65, 257, 300, 600]
LADDER = [1, 2, 63, 64, 65, 192, 193, 255, 256, 257]


def methods(L, k):
    """Every forced method that serves (L, k), and the tiles.  Where the one-word / row-copy form
    applies, "bucketed" is that same form and is left out."""
    W, _ = shape(L)
    m = ["tiles"]
    if W <= 4 and k <= 15:
        m.append("pigeonhole")
    elif k <= 31:
        m.append("bucketed")
    return m


def is_word_form(L, k):
    return shape(L)[0] == 1 and k <= 15


def dense_cases():
    """(kind, L, k, arg): one repeated read at four n; heavy plus background at k = 1, 3 and the
    shape's own; the ladder at k = 0 and 1."""
    out = []
    for L, k in DENSE_SHAPES:
        out += [("one-read", L, k, n) for n in ONE_READ_NS]
        out += [("heavy", L, kk, 0) for kk in sorted({1, 3, k})]
        out += [("ladder", L, kk, 0) for kk in (0, 1)]
    return out


DENSE_CASES = dense_cases()
CAP_FORMS = [(12, 1, "pigeonhole"), (40, 2, "pigeonhole"), (150, 3, "bucketed"), (12, 1, "tiles"), (150, 3, "tiles")]
CAP_CASES = [(batch, L, k, m) for batch in ("heavy", "umi") for L, k, m in CAP_FORMS]


# ---- the reference --------------------------------------------------------------------------------
def encode(oracle, ascii):
    """ASCII rows (n, L) -> packed words (n, W), read-only."""
    n, L = ascii.shape
    if n == 0:
        words = np.zeros((0, shape(L)[0]), dtype=np.uint64)
    else:
        words, rc, _ = oracle.encode_batch(np.ascontiguousarray(ascii).reshape(-1), n, L)
        assert rc == 0
        words = np.ascontiguousarray(words).reshape(n, -1)
    assert words.shape[1] == shape(L)[0]
    words.setflags(write=False)
    return words


def brute(oracle, words, L, ks):
    """Oracle distances of every pair (hamming_ref_batch row by row), thresholded at each k of ks
    -> {k: (counts int64 [n], sorted keys int64 [m], i << 32 | j with i < j)}."""
    n = words.shape[0]
    cnt = {k: np.zeros(n, dtype=np.int64) for k in ks}
    parts = {k: [np.zeros(0, dtype=np.int64)] for k in ks}
    for i in range(n - 1):
        d = oracle.hamming_ref_batch(words[i + 1:], n - i - 1, L, words[i])
        for k in ks:
            js = np.flatnonzero(d <= k) + (i + 1)
            cnt[k][i] += js.size
            cnt[k][js] += 1
            parts[k].append((i << 32) | js.astype(np.int64))      # i, then j, ascending: sorted
    out = {}
    for k in ks:
        keys = np.concatenate(parts[k])
        keys.setflags(write=False)
        cnt[k].setflags(write=False)
        out[k] = (cnt[k], keys)
    return out


# ---- generators -----------------------------------------------------------------------------------
def umi_rows(oracle, n, L, U, seed):
    """n ASCII rows drawn from U distinct L-mers, 40 % with one substitution (a UMI-like pool)."""
    rng = np.random.default_rng(seed)
    base = oracle.gen_reads(seed, 0, U, L).reshape(U, L)
    pick = base[rng.integers(0, U, size=n)].copy()
    mut = rng.random(n) < 0.4
    pos = rng.integers(0, L, size=n)
    pick[mut, pos[mut]] = ACGT[rng.integers(0, 4, size=int(mut.sum()))]
    return pick


def edge_rows(L, n):
    """Rows of an n-row batch on either side of a tile edge (and of the WT 32 chunk edge), row 0 and
    row n - 1."""
    S = TILE_FAMILIES[L][1] if L in TILE_FAMILIES else tile_rows(L)
    e = {0, n - 1, S - 1, S, 2 * S - 1, 2 * S}
    C = chunk_cols(L)
    if C is not None and C < S:
        e |= {C - 1, C, S + C - 1, S + C}
    return sorted(x for x in e if 0 <= x < n)


@functools.lru_cache(maxsize=4)
def tile_case(L, n):
    """A UMI-like pool of n rows whose edge rows (edge_rows) are all "A...A" (packed word 0, what the
    MFMA tiles give a padding column), so copies of one another -> words, edge rows,
    {k: (counts, keys)} for k = 0, small_k(L) and 2^32 - 1."""
    import oracle
    ascii = umi_rows(oracle, n, L, max(2, n // 20), 1000 * L + n) if n else np.zeros((0, L), np.uint8)
    edges = edge_rows(L, n)
    ascii[np.array(edges, dtype=np.intp)] = ord("A")
    words = encode(oracle, ascii)
    return words, edges, brute(oracle, words, L, (0, small_k(L), U32MAX))


@functools.lru_cache(maxsize=4)
def pig_case(L, k, n):
    """A UMI-like pool of n rows -> words, (counts, keys) at k.  Where k >= L (every pair of plain
    reads is within k) and n >= 3, row 0 ends in "C" and row n - 2 is its complement with the last
    byte aliased (table code 4: "A" at position L - 1 and a set bit at position L): L + 1 apart."""
    import oracle
    ascii = umi_rows(oracle, n, L, max(2, n // 20), 7000 * L + 13 * k + n)
    if k >= L and n >= 3:
        assert L % 32 != 0
        comp = np.zeros(256, np.uint8)
        comp[ACGT] = np.frombuffer(b"CGTA", np.uint8)
        ascii[0, L - 1] = ord("C")
        ascii[n - 2] = comp[ascii[0]]
        ascii[n - 2, L - 1] = 0x01
    words = encode(oracle, ascii)
    return words, brute(oracle, words, L, (k,))[k]


def _substituted(row, pos, rng):
    out = row.copy()
    out[pos] = rng.choice(ACGT[ACGT != row[pos]])
    return out


@functools.lru_cache(maxsize=None)
def dense_ascii(kind, L, arg):
    """ASCII rows of a dense batch.
    one-read: arg copies of one read.
    heavy: 400 copies of a read A, 300 of A' (A with position 0 substituted: segment 0 of every
      split), 200 of A'' (position L - 1 substituted: the last segment of every split), 500 random
      rows; shuffled.  A-A' pairs differ in segment 0, so a later segment reports them.
    ladder: duplicate groups of sizes LADDER, shuffled."""
    import oracle
    rng = np.random.default_rng(100 * L + len(kind))
    if kind == "one-read":
        rows = np.tile(oracle.gen_reads(8 + L, 0, 1, L).reshape(1, L), (arg, 1))
    elif kind == "heavy":
        A = oracle.gen_reads(31 + L, 0, 1, L).reshape(L)
        rows = np.concatenate([np.tile(A, (400, 1)), np.tile(_substituted(A, 0, rng), (300, 1)),
                               np.tile(_substituted(A, L - 1, rng), (200, 1)),
                               oracle.gen_reads(57 + L, 0, 500, L).reshape(500, L)])
    elif kind == "ladder":
        base = oracle.gen_reads(91 + L, 0, len(LADDER), L).reshape(len(LADDER), L)
        assert len(np.unique(base, axis=0)) == len(LADDER)
        rows = np.repeat(base, LADDER, axis=0)
    elif kind == "umi":
        rows = umi_rows(oracle, 1000, L, 50, 3 * L + 1)
    else:
        raise KeyError(kind)
    if kind != "one-read":
        rows = rows[rng.permutation(len(rows))]
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=6)
def dense_case(kind, L, k, arg):
    """-> words, (counts, keys) at k; shared by the methods and the capacity tests (read-only)."""
    import oracle
    words = encode(oracle, dense_ascii(kind, L, arg))
    return words, brute(oracle, words, L, (k,))[k]


@functools.lru_cache(maxsize=2)
def two_tile_case(L, k):
    """n = 4097 rows of a UMI-like pool."""
    import oracle
    n = kPigTile + 1
    words = encode(oracle, umi_rows(oracle, n, L, n // 20, 5 * L + k))
    return words, brute(oracle, words, L, (k,))[k]


# ---- the bucket rule, as far as the CPU-side conditions need it -------------------------------------
def split(L, k):
    """Bounds of the G = k + 1 segments over the P compared positions: the L read positions split
    evenly (the first L % G one longer), position L joins the last segment."""
    _, P = shape(L)
    Lr, G = min(P, L), k + 1
    lens = [Lr // G + (1 if g < Lr % G else 0) for g in range(G)]
    b = [0]
    for x in lens:
        b.append(b[-1] + x)
    b[-1] = P
    return b


def nbmax(n):
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return max(10, min(kPigMaxBits, lg))


def row_ints(words):
    """Each row as one Python int (word q at bits 64 q)."""
    return [int.from_bytes(np.ascontiguousarray(r).tobytes(), "little") for r in words]


def segment_values(words, L, k):
    """[g][i] = the value of segment g of row i (2 bits per position)."""
    b = split(L, k)
    rows = row_ints(words)
    return [[(r >> (2 * b[g])) & ((1 << (2 * (b[g + 1] - b[g]))) - 1) for r in rows] for g in range(k + 1)]


def bucket(value, length, nb, exact, word_form):
    """pig_bucket (one-word rows) / pigw_bucket (multi-word rows) of a segment value of `length`
    positions."""
    if length == 0 and not word_form:
        return 0
    if exact:
        return value
    if word_form:
        return ((value * MUL) & MASK64) >> (64 - nb)
    h = 0x243F6A8885A308D3 ^ length
    for p in range(0, length, 32):           # the segment's 64-bit pieces
        h = ((h ^ ((value >> (2 * p)) & MASK64)) * MUL) & MASK64
        h ^= h >> 29
    return h >> (64 - nb)


def longest_equal_segment_run(words, L, k):
    """The most rows that share one value of one segment: a lower bound of the longest bucket run."""
    return max(max(collections.Counter(vals).values()) for vals in segment_values(words, L, k))


def largest_duplicate_group(words):
    return int(np.unique(words, axis=0, return_counts=True)[1].max()) if len(words) else 0
