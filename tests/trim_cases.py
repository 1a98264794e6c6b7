"""The 3' adapter trim sweep shared by test_trim.py (host rule against a Python restatement) and
test_trim_gpu.py (device against host): the smallest shapes at which the kernel can still go wrong --
adapter lengths around the 8-byte SWAR word edges, every parameter combination, read lengths around the
adapter, the 16-byte chunks and the 1024 limit, planted occurrences (every position, every partial
overlap, two occurrences, exactly the allowed mismatches and one more, mismatches at the word edges),
hostile bytes, wildcards, and every start residue mod 16 in three layouts.  Everything is seeded."""
import numpy as np

ADAPTER_LENS = (1, 7, 8, 9, 16, 17, 33, 64)
ERR_DIVS = (0, 1, 4, 8, 10)
BASES = b"ACGT"
HOSTILE = (ord("N"), ord("a"), 0x00, 0xFF, ord("\n"))


def ref_trim(read: bytes, adapter: bytes, min_overlap: int, err_div: int) -> int:
    """The rule, restated: the least p with enough overlap and few enough mismatches, else len(read)."""
    L, A = len(read), len(adapter)
    if L > 1024:
        return L
    for p in range(L):
        ov = min(A, L - p)
        if ov < min_overlap:
            continue
        mm = sum(1 for x, y in zip(read[p:p + ov], adapter) if y != ord("N") and x != y)
        if mm <= (ov // err_div if err_div else 0):
            return p
    return L


def rand_seq(rng, n: int) -> bytes:
    return bytes(rng.choice(np.frombuffer(BASES, np.uint8), n)) if n else b""


def combos():
    """(adapter length, min_overlap, err_div) for the whole sweep."""
    out = []
    for A in ADAPTER_LENS:
        for mo in sorted({1, 3, A}):
            for ed in ERR_DIVS:
                out.append((A, mo, ed))
    return out


def mutate(rng, seq: bytes, positions) -> bytes:
    """seq with another base at each of `positions`."""
    b = bytearray(seq)
    for k in positions:
        b[k] = rng.choice([c for c in BASES if c != b[k]])
    return bytes(b)


def mismatch_sets(ov: int, count: int):
    """`count` distinct adapter positions below ov, the word edges 0, 7, 8 and ov - 1 first."""
    order = [k for k in (0, 7, 8, ov - 1) if 0 <= k < ov]
    order = list(dict.fromkeys(order)) + [k for k in range(ov) if k not in (0, 7, 8, ov - 1)]
    return order[:count]


def sweep_reads(rng, adapter: bytes, min_overlap: int, err_div: int):
    """The reads of one parameter combination; a (fake length, None) entry is a read that must not be read."""
    A = len(adapter)
    reads = []
    for L in (0, 1, min_overlap - 1, min_overlap, A - 1, A, A + 1, 15, 16, 17, 63, 64, 65, 150, 1023, 1024):
        if L < 0:
            continue
        reads.append(rand_seq(rng, L))
        if L >= 1:                      # the adapter's start at the 3' end, as long as fits below L
            k = min(A, L, int(rng.integers(1, 66)))
            reads.append(rand_seq(rng, L - k) + adapter[:k])
        if L > A:                       # the whole adapter somewhere inside
            p = int(rng.integers(0, L - A + 1))
            reads.append(rand_seq(rng, p) + adapter + rand_seq(rng, L - A - p))
    reads += [(1025, None), (0xFFFFFFFF, None)]
    # the adapter (cut at the read's end) at every position of a 40-byte read: every partial overlap too
    for p in range(40):
        reads.append((rand_seq(rng, p) + adapter)[:40])
    # two occurrences: the left one wins
    reads.append(rand_seq(rng, 5) + adapter + rand_seq(rng, 3) + adapter)
    # exactly the allowed mismatches, and one more, at full and at partial overlap; the mismatches at
    # adapter bytes 0, 7, 8 and ov - 1 first
    for ov in sorted({A, max(1, A - 1), max(1, A // 2), min(A, 9)}):
        allowed = ov // err_div if err_div else 0
        for cnt in (allowed, allowed + 1):
            if cnt > ov:
                continue
            occ = mutate(rng, adapter[:ov], mismatch_sets(ov, cnt))
            tail = rand_seq(rng, 7) if ov == A else b""
            reads.append(rand_seq(rng, 11) + occ + tail)
            # a perfect occurrence further right than this worse one: the left one wins if it suffices
            if ov == A:
                reads.append(rand_seq(rng, 11) + occ + rand_seq(rng, 2) + adapter)
        for k in mismatch_sets(ov, 4):      # one mismatch at each word-edge byte
            reads.append(rand_seq(rng, 6) + mutate(rng, adapter[:ov], [k]) + (rand_seq(rng, 4) if ov == A else b""))
    # hostile bytes in the read at compared positions: each an ordinary mismatch
    for hb in HOSTILE:
        for k in sorted({0, A // 2, A - 1}):
            occ = bytearray(adapter)
            occ[k] = hb
            reads.append(rand_seq(rng, 9) + bytes(occ) + rand_seq(rng, 5))
    reads.append(rand_seq(rng, 9) + adapter.lower() + rand_seq(rng, 5))
    return reads


def wildcard_adapters(rng, A: int):
    """Adapters of length A with an N at the first, the middle and the last byte, and at all three."""
    base = rand_seq(rng, A)
    out = []
    for ks in ([0], [A // 2], [A - 1], [0, A // 2, A - 1]):
        b = bytearray(base)
        for k in ks:
            b[k] = ord("N")
        out.append(bytes(b))
    return out


def wildcard_reads(rng, adapter: bytes):
    """Occurrences whose bytes under the adapter's N are anything at all, N itself included."""
    A = len(adapter)
    reads = []
    for fill in (ord("A"), ord("N"), 0x00, 0xFF, ord("g")):
        occ = bytearray(adapter)
        for k in range(A):
            if adapter[k] == ord("N"):
                occ[k] = fill
        reads.append(rand_seq(rng, 13) + bytes(occ) + rand_seq(rng, 6))
        reads.append(rand_seq(rng, 13) + bytes(occ)[:max(1, A - 2)])
    reads.append(rand_seq(rng, 30))
    return reads


def layout(rng, reads, kind: str):
    """(blob u8, offsets u64, lens u32) of the reads: `back` back to back (the first read at byte 0, the
    last one ending at nbytes), `junk` FASTQ-like (a header before and a '+' line and qualities after each
    read), `residue` read k starting at residue k mod 16.  A (length, None) read gets an offset inside the
    blob and takes no bytes."""
    parts, offs, lens = [], [], []
    pos = 0
    for k, r in enumerate(reads):
        if isinstance(r, tuple):
            offs.append(pos // 2)
            lens.append(r[0])
            continue
        pre = b""
        if kind == "junk":
            pre = b"@r%d x\n" % k
        elif kind == "residue":
            pre = b"#" * ((k % 16 - pos) % 16)
        post = b"\n+\n" + b"I" * len(r) + b"\n" if kind == "junk" else b""
        offs.append(pos + len(pre))
        lens.append(len(r))
        parts += [pre, r, post]
        pos += len(pre) + len(r) + len(post)
    blob = np.frombuffer(b"".join(parts), np.uint8).copy() if pos else np.zeros(0, np.uint8)
    return blob, np.array(offs, np.uint64), np.array(lens, np.uint32)


def expected(reads, adapter: bytes, min_overlap: int, err_div: int, memo=None):
    """The Python rule on every read: (new lengths u32, [reads shortened, bytes removed])."""
    memo = {} if memo is None else memo
    out = []
    for r in reads:
        if isinstance(r, tuple):
            out.append(r[0])
            continue
        v = memo.get(r)
        if v is None:
            v = memo[r] = ref_trim(r, adapter, min_overlap, err_div)
        out.append(v)
    full = [r[0] if isinstance(r, tuple) else len(r) for r in reads]
    short = sum(1 for a, b in zip(out, full) if a < b)
    removed = sum(b - a for a, b in zip(out, full))
    return np.array(out, np.uint32), [short, removed]


def library_reads(rng, n: int, adapter: bytes, pool: int = 300, lo: int = 15, hi: int = 40, tail: int = 20,
                  err_rate: float = 0.01):
    """n small-RNA-like reads: an insert from a pool of `pool` inserts of lo..hi nt, then the adapter's
    first bytes, cut at insert + tail bytes, with substitutions sprinkled in at err_rate."""
    inserts = [rand_seq(rng, int(rng.integers(lo, hi + 1))) for _ in range(pool)]
    picks = rng.integers(0, pool, n)
    flips = rng.random(n) < err_rate * 40
    reads = []
    for i in range(n):
        r = inserts[picks[i]] + adapter[:tail]
        if flips[i]:
            r = mutate(rng, r, [int(rng.integers(0, len(r)))])
        reads.append(r)
    return reads
