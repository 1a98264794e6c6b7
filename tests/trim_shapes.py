"""Inputs of test_trim_shapes.py (no GPU import): the parts of k_trim_adapter3 that the sweep of
trim_cases.py does not reach -- the seams between the staged windows of 256 positions, the second and
later trips of the grid-stride loop, every compiled (lane group, staged) shape and the budget multiply --
and a second statement of the rule, vectorised in NumPy, as the expectation.  Everything is seeded and
cached per case; nothing here is changed by a test."""
import functools

import numpy as np

import trim_cases as T

KWIN = 256                              # positions per staged window (csrc/ss_trim.hip)
SEAMS = (256, 512, 768)
SEAM_ADAPTER_LENS = (9, 33, 64)
PREFILL = 0x5A5A5A5A
A21 = b"TGGAATTCTCGGGTGCCAAGG"
TRIM_THREADS, MAX_GRID = 256, 2048      # the launch geometry restated by trips()
SHAPES = tuple((g, s) for g in (2, 4, 8, 16, 32) for s in (1, 0))
LIB_GROUP = 4


# ---- the rule, vectorised ----------------------------------------------------------------------------

def np_trim(read: bytes, adapter: bytes, min_overlap: int, err_div: int) -> int:
    """The rule of include/shortseq_amd.h ("3' adapter trim") on one read: every window of the zero-padded
    read against the adapter, mismatches counted under the wildcard and the overlap mask, the first
    position with enough overlap and few enough mismatches, else the length."""
    L, A = len(read), len(adapter)
    if L > 1024 or L == 0:
        return L
    a = np.frombuffer(adapter, np.uint8)
    padded = np.zeros(L + A, np.uint8)
    padded[:L] = np.frombuffer(read, np.uint8)
    win = np.lib.stride_tricks.sliding_window_view(padded, A)[:L]           # [L, A]: row p = read[p : p + A]
    ov = np.minimum(A, L - np.arange(L, dtype=np.int64))
    counted = (a != ord("N"))[None, :] & (np.arange(A)[None, :] < ov[:, None])
    mm = ((win != a[None, :]) & counted).sum(axis=1)
    budget = ov // err_div if err_div else np.zeros(L, np.int64)
    hit = np.flatnonzero((ov >= min_overlap) & (mm <= budget))
    return int(hit[0]) if hit.size else L


def np_expected(reads, adapter: bytes, min_overlap: int, err_div: int, memo=None):
    """np_trim on every read (a (length, None) entry keeps its length): (new lengths u32, [reads
    shortened, bytes removed])."""
    memo = {} if memo is None else memo
    out, full = [], []
    for r in reads:
        if isinstance(r, tuple):
            out.append(r[0])
            full.append(r[0])
            continue
        v = memo.get(r)
        if v is None:
            v = memo[r] = np_trim(r, adapter, min_overlap, err_div)
        out.append(v)
        full.append(len(r))
    out, full = np.array(out, np.int64), np.array(full, np.int64)
    return out.astype(np.uint32), [int((out < full).sum()), int((full - out).sum())]


def blob_reads(blob, offs, lens):
    """The reads of a ragged batch as bytes ((length, None) for one longer than 1024)."""
    raw = blob.tobytes()
    return [(int(n), None) if n > 1024 else raw[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]


def layout_at(reads, residues):
    """trim_cases.layout's `residue`, the residue a parameter: read k starts at residues[k] mod 16 ('#'
    in between).  A (length, None) read gets an offset inside the blob and takes no bytes."""
    parts, offs, lens = [], [], []
    pos = 0
    for r, res in zip(reads, residues):
        if isinstance(r, tuple):
            offs.append(pos // 2)
            lens.append(r[0])
            continue
        pad = (int(res) - pos) % 16
        parts += [b"#" * pad, r]
        offs.append(pos + pad)
        lens.append(len(r))
        pos += pad + len(r)
    blob = np.frombuffer(b"".join(parts), np.uint8).copy() if pos else np.zeros(0, np.uint8)
    return blob, np.array(offs, np.uint64), np.array(lens, np.uint32)


# ---- A. window seams -----------------------------------------------------------------------------------

def seam_params(A: int):
    return ((3, 10), (A, 0))


def seam_lengths(A: int, min_overlap: int):
    """The last window holds a window's last position or the single first position of the next; 256 + A;
    and lengths inside and at the end of windows 1, 2 and 3."""
    ls = {s + d + min_overlap for s in SEAMS for d in (-1, 0)} | {KWIN + A, 300, 513, 1009, 1023, 1024}
    return sorted(x for x in ls if x <= 1024)


def seam_positions(A: int, min_overlap: int, L: int):
    ps = {0, L - A, L - A + 1, L - min_overlap - 1, L - min_overlap}
    for s in SEAMS:
        ps |= {s - A - 1, s - A, s - A + 1, s - 8, s - 1, s, s + 1}
    return sorted(p for p in ps if 0 <= p <= L - min_overlap)


def seam_cases(rng, adapter: bytes, min_overlap: int, err_div: int):
    """[(read, kind, planted position or None)]: kind `planted` the adapter at p, cut at the read's end
    or followed by a random tail; `plain` nothing planted; `nearmiss` (err_div 0) an occurrence with one
    mismatch at s - 1, the last position of a window, and a perfect one in the next window."""
    A = len(adapter)
    cases = []
    for L in seam_lengths(A, min_overlap):
        for p in seam_positions(A, min_overlap, L):
            cases.append(((T.rand_seq(rng, p) + adapter + T.rand_seq(rng, max(0, L - p - A)))[:L], "planted", p))
        cases.append((T.rand_seq(rng, L), "plain", None))
        if err_div == 0:
            for s in SEAMS:
                second = s - 1 + A + 3
                if second + A > L:
                    continue
                miss = T.mutate(rng, adapter, [int(rng.integers(0, A))])
                r = T.rand_seq(rng, s - 1) + miss + T.rand_seq(rng, 3) + adapter + T.rand_seq(rng, L - second - A)
                cases.append((r, "nearmiss", second))
    return cases


class SeamBatch:
    """One launch of part A: every case at every start residue, interleaved with short library reads and
    reads the kernel must skip, and the reference's answer."""

    def __init__(self, A: int, which: int):
        self.A = A
        self.min_overlap, self.err_div = seam_params(A)[which]
        rng = np.random.default_rng(9000 + 10 * A + which)
        self.adapter = T.rand_seq(rng, A)
        self.cases = seam_cases(rng, self.adapter, self.min_overlap, self.err_div)
        longs = [(ci, res) for ci in range(len(self.cases)) for res in range(16)]
        longs = [longs[k] for k in rng.permutation(len(longs))]
        shorts = T.library_reads(rng, 64, self.adapter)
        fillers = 0
        reads, residues, case_of = [], [], []          # case_of: the case's index, -1 for a filler
        self.filler_kind = {}                          # read index -> library / 1025 / 0xFFFFFFFF / short

        def filler():
            nonlocal fillers
            kind = fillers % 4
            fillers += 1
            if kind == 0:
                r = shorts[int(rng.integers(0, len(shorts)))]
            elif kind == 1:
                r = (1025, None)
            elif kind == 2:
                r = (0xFFFFFFFF, None)
            else:
                r = T.rand_seq(rng, int(rng.integers(0, self.min_overlap)))     # shorter than min_overlap
            self.filler_kind[len(reads)] = ("library", 1025, 0xFFFFFFFF, "short")[kind]
            reads.append(r)
            residues.append(int(rng.integers(0, 16)))
            case_of.append(-1)

        k = 0
        while k < len(longs):
            slots = set(rng.choice(16, int(rng.integers(1, 4)), replace=False).tolist())
            for j in range(16):
                if j in slots or k == len(longs):     # (the last wave is filled up with fillers)
                    filler()
                else:
                    ci, res = longs[k]
                    k += 1
                    reads.append(self.cases[ci][0])
                    residues.append(res)
                    case_of.append(ci)
        self.reads, self.residues, self.case_of = reads, np.array(residues), np.array(case_of)
        self.blob, self.offs, self.lens = layout_at(reads, residues)
        self.exp, self.stats = np_expected(reads, self.adapter, self.min_overlap, self.err_div)
        self.case_answer = {}
        for ci, e in zip(case_of, self.exp):
            if ci >= 0:
                self.case_answer[ci] = int(e)

    @property
    def name(self):
        return f"seam A{self.A} mo{self.min_overlap} ed{self.err_div}"


@functools.lru_cache(maxsize=None)
def seam_batch(A: int, which: int) -> SeamBatch:
    return SeamBatch(A, which)


SEAM_BATCHES = tuple((A, w) for A in SEAM_ADAPTER_LENS for w in (0, 1))


# ---- B. every compiled shape ---------------------------------------------------------------------------

SHAPE_SWEEP_COMBOS = ((1, 1, 0), (8, 3, 10), (17, 17, 4), (64, 3, 8))


@functools.lru_cache(maxsize=None)
def shape_inputs():
    """[(name, adapter, min_overlap, err_div, blob, offs, lens, expected lengths, expected stats)]: the
    A = 64 and A = 9 seam batches, four combinations of the trim_cases sweep (one per layout and one
    more) and a wildcard adapter's case set, each with the reference's answer."""
    out = []
    for A in (64, 9):
        for w in (0, 1):
            b = seam_batch(A, w)
            out.append((b.name, b.adapter, b.min_overlap, b.err_div, b.blob, b.offs, b.lens, b.exp, b.stats))
    rng = np.random.default_rng(31337)
    for k, (A, mo, ed) in enumerate(SHAPE_SWEEP_COMBOS):
        adapter = T.rand_seq(rng, A)
        reads = T.sweep_reads(rng, adapter, mo, ed)
        blob, offs, lens = T.layout(rng, reads, ("residue", "junk", "back", "residue")[k])
        exp, st = np_expected(reads, adapter, mo, ed)
        out.append((f"sweep A{A} mo{mo} ed{ed}", adapter, mo, ed, blob, offs, lens, exp, st))
    adapter = T.wildcard_adapters(rng, 17)[3]                  # N at the first, the middle and the last byte
    reads = T.wildcard_reads(rng, adapter) + [T.rand_seq(rng, 300) + bytes(adapter).replace(b"N", b"T")]
    blob, offs, lens = T.layout(rng, reads, "residue")
    exp, st = np_expected(reads, adapter, 3, 10)
    out.append(("wildcards A17 mo3 ed10", adapter, 3, 10, blob, offs, lens, exp, st))
    return out


# ---- C. grid-stride trips --------------------------------------------------------------------------------

def trips(n: int, group: int):
    """(reads per trip, trips) of one launch over n reads: blocks = ceil(n / (256 / G)), grid =
    min(blocks, 2048), iters = ceil(blocks / grid) -- trim_launch restated."""
    per_block = TRIM_THREADS // group
    blocks = -(-n // per_block)
    grid = min(blocks, MAX_GRID)
    return grid * per_block, -(-blocks // grid)


LIB_TRIP_N = 131072 + 64 + 1            # a second trip of one full block and one block with one live group
G32_TRIP_NS = (16384, 16385, 49153)


def _ragged_fill(blob, starts, lens, rows, row_index):
    """blob[starts[i] : starts[i] + lens[i]] = rows[row_index[i], : lens[i]] for every i, without a loop."""
    within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    blob[np.repeat(starts, lens) + within] = rows[np.repeat(row_index, lens), within]


@functools.lru_cache(maxsize=None)
def trip_batch(n: int, per_trip: int, seed: int = 0, pool: int = 300, tail: int = 20):
    """n library-like reads in the `junk` layout, made without a per-read loop: an insert from a pool
    (insert k of 15 + 7 k mod 26 nt, so neighbours in the pool differ in length), then the first `tail`
    bytes of A21; read i + per_trip takes the pool entry after read i's, so the reads of a later trip
    differ from those at the same block position in the trip before; one substitution in about 1 % of
    the reads.  -> (blob, offs u64, lens u32)."""
    rng = np.random.default_rng(500000 + n + seed)
    ilen = 15 + (7 * np.arange(pool)) % 26
    rows = rng.choice(np.frombuffer(T.BASES, np.uint8), (pool, 40 + tail))
    head = np.frombuffer(A21[:tail], np.uint8)
    for k in range(pool):                                   # (the pool, not the reads)
        rows[k, ilen[k]:ilen[k] + tail] = head
    pick = rng.integers(0, pool, n)
    for i in range(per_trip, n, per_trip):
        m = min(per_trip, n - i)
        pick[i:i + m] = (pick[i - per_trip:i - per_trip + m] + 1) % pool
    rl = (ilen[pick] + tail).astype(np.int64)
    hdr = 8                                                 # '@rrrrrr\n'
    rec = hdr + rl + 3 + rl + 1
    start = np.cumsum(rec) - rec
    offs = start + hdr
    blob = np.full(int(rec.sum()), ord("I"), np.uint8)
    blob[start] = ord("@")
    blob[start + hdr - 1] = ord("\n")
    _ragged_fill(blob, offs, rl, rows, pick)
    blob[offs + rl] = ord("\n")
    blob[offs + rl + 1] = ord("+")
    blob[offs + rl + 2] = ord("\n")
    blob[start + rec - 1] = ord("\n")
    sub = np.flatnonzero(rng.random(n) < 0.01)
    at = offs[sub] + (rng.random(sub.size) * rl[sub]).astype(np.int64)
    blob[at] = np.frombuffer(b"CGAT", np.uint8)[(blob[at] >> 1) & 3]        # A -> C, C -> G, T -> A, G -> T
    return blob, offs.astype(np.uint64), rl.astype(np.uint32)


_A21_MEMO = {}


@functools.lru_cache(maxsize=None)
def trip_reference(n: int, per_trip: int, sample: bool):
    """(read indices, the reference's lengths there) of trip_batch(n, per_trip) with A21 and the default
    parameters: trip_sample's reads, or every read."""
    blob, offs, lens = trip_batch(n, per_trip)
    idx = trip_sample(n, per_trip) if sample else np.arange(n)
    raw = blob.tobytes()
    reads = [raw[int(offs[i]):int(offs[i]) + int(lens[i])] for i in idx]
    return idx, np_expected(reads, A21, 3, 10, _A21_MEMO)[0]


def trip_sample(n: int, per_trip: int, extra: int = 2000, seed: int = 1):
    """Read indices: the first and the last 64 reads of every trip and `extra` others."""
    idx = set(np.random.default_rng(seed).integers(0, n, extra).tolist())
    for t0 in range(0, n, per_trip):
        t1 = min(n, t0 + per_trip)
        idx |= set(range(t0, min(t1, t0 + 64))) | set(range(max(t0, t1 - 64), t1))
    return np.array(sorted(idx))


# ---- D. the budget multiply --------------------------------------------------------------------------------

BUDGET_ERR_DIVS = (0,) + tuple(range(2, 67)) + (100, 1 << 16, (1 << 24) + 1, 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def budget_adapter() -> bytes:
    return T.rand_seq(np.random.default_rng(6464), 64)


@functools.lru_cache(maxsize=None)
def budget_case(err_div: int):
    """For every overlap 1..64 a read with exactly the allowed mismatches at random adapter bytes and one
    with one more, the occurrence at byte 11 and cut at the read's end (a 5-byte tail after a whole
    adapter).  -> (reads, at_budget bool [n], blob, offs, lens, expected lengths, expected stats)."""
    rng = np.random.default_rng(64000 + err_div % 99991)
    adapter = budget_adapter()
    reads, at_budget = [], []
    for ov in range(1, 65):
        allowed = ov // err_div if err_div else 0
        for cnt in (allowed, allowed + 1):
            where = sorted(rng.choice(ov, cnt, replace=False).tolist())
            occ = T.mutate(rng, adapter[:ov], where)
            reads.append(T.rand_seq(rng, 11) + occ + (T.rand_seq(rng, 5) if ov == 64 else b""))
            at_budget.append(cnt == allowed)
    blob, offs, lens = T.layout(rng, reads, "residue")
    exp, st = np_expected(reads, adapter, 1, err_div)
    return reads, np.array(at_budget), blob, offs, lens, exp, st


# ---- E. the engine with reads past one window ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def engine_reads(n_long: int = 1000, n_short: int = 1000, pool: int = 100, head: int = 20):
    """(reads, is_long): inserts of 260..600 nt from a pool, each followed by the first `head` bytes of
    A21 (the trim point lies in window 1 or 2), shuffled with 40-nt-insert library reads."""
    rng = np.random.default_rng(26000)
    inserts = [T.rand_seq(rng, int(rng.integers(260, 601))) for _ in range(pool)]
    longs = [inserts[int(k)] + A21[:head] for k in rng.integers(0, pool, n_long)]
    shorts = T.library_reads(rng, n_short, A21, pool=50, lo=40, hi=40)
    reads = longs + shorts
    order = rng.permutation(len(reads))
    return [reads[k] for k in order], np.array([k < n_long for k in order])
