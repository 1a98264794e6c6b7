"""Inputs of test_fastq_shapes.py (no GPU import): the branches of csrc/ss_fastq.hip that the texts of
test_fastq.py do not reach -- newlines at, before and after the tile seams of both paths, lines longer than
a tile, one-pass tiles of every density class, NUL bytes at both sides of the list and overflow switches
and next to sub-block and tile edges, every line phase on tiny texts, and more than 1024 tiles (a second
and third tile group) -- and a second statement of the rule, vectorised in NumPy, as the expectation.
Every text is seeded and cached; a census per family counts what the text reaches, so that a retuned
kernel or a changed generator fails a census and does not quietly empty a case.  Nothing here is changed
by a test."""
import collections
import functools
import itertools
import random
import re

import numpy as np

# ---- csrc/ss_fastq.hip restated ----------------------------------------------------------------------------

TILE2 = 16384                 # two-pass tile: kFqT * kFqU * 16
TILE1 = 32768                 # one-pass tile: kFqT * kFqU1 * 16
TILE_CAP = 2048               # kTileCap: a one-pass tile with at most this many newlines writes its own fixed run
LDS_POS = 4096                # kLdsPos: up to here a denser tile stages in LDS; above, every lane stores to the run
NUL_LIST_SCAN = 64            # kNulListScan: up to here nul_len searches the position list, above the masks
NUL_CAP = 65536               # kNulCap: entries the NUL list holds exactly
GROUP_TILES = 1024            # tiles per scan group
FIXED_ROUND = 512             # positions k_fq_place reads per round of a fixed run
STAGED_ROUND = 64             # ... per round of a shard run
NUL_SUB = 1024                # bytes per NUL sub-block mask bit
STAGE_SHARDS = 64             # a denser tile reserves in shard (tile mod 64)
NONE32 = 0xFFFFFFFF           # the length of a sequence line whose first byte is NUL

KERNEL_CONSTANTS = {"kFqT": 256, "kFqU": TILE2 // (256 * 16), "kFqU1": TILE1 // (256 * 16), "kTileCap": TILE_CAP,
                    "kLdsPos": LDS_POS, "kNulListScan": NUL_LIST_SCAN, "kNulCap": NUL_CAP}

KINDS = ("header", "sequence", "plus", "quality")

Case = collections.namedtuple("Case", "name data line0")


def source_constants(text: str) -> dict:
    """name -> value of the `constexpr` lines of a HIP source that reduce to integer arithmetic over
    earlier ones (casts and integer suffixes dropped); a line that does not is left out."""
    out = {}
    for m in re.finditer(r"^\s*constexpr\s+\w+\s+(\w+)\s*=\s*([^;]+);", text, re.M):
        expr = re.sub(r"\(\s*(?:u?int\d*_t|int|unsigned)\s*\)", "", m.group(2))
        expr = re.sub(r"\b(\d+)(?:ull|ul|u)\b", r"\1", expr).replace("/", "//")
        if not re.fullmatch(r"[\w\s()+\-*/<>]+", expr):
            continue
        try:
            out[m.group(1)] = int(eval(expr, {"__builtins__": {}}, dict(out)))     # noqa: S307 -- arithmetic only
        except Exception:  # noqa: BLE001 -- not an integer constant
            continue
    return out


# ---- the rule, vectorised ------------------------------------------------------------------------------------

def line_table(data: bytes, line0: int = 0):
    """(a, newline positions, kept line numbers inside the chunk, their starts, their stops): line k of the
    chunk has the global number line0 + k and is kept iff that is 1 mod 4; stop is one past the line's '\\n',
    or the end of the text for a final line without one."""
    a = np.frombuffer(data, np.uint8)
    nlpos = np.flatnonzero(a == 10).astype(np.int64)
    nlines = nlpos.size + (1 if a.size and a[-1] != 10 else 0)
    ks = np.arange((1 - line0) % 4, nlines, 4, dtype=np.int64)
    starts = np.concatenate((np.zeros(1, np.int64), nlpos + 1))
    stops = np.concatenate((nlpos + 1, np.full(1, a.size, np.int64)))
    return a, nlpos, ks, starts[ks], stops[ks]


def np_index(data: bytes, line0: int = 0):
    """The rule in the header of csrc/ss_fastq.hip on one chunk -> (offsets u64, lens u32, newlines): lines
    split at '\\n'; the line with global number j is kept iff j % 4 == 1; strlen covers the line and its
    '\\n' and stops at the line's first NUL; len = strlen - 1, or 0xFFFFFFFF where strlen is 0; a final
    line without '\\n' counts up to the end of the text."""
    a, nlpos, _ks, start, stop = line_table(data, line0)
    nul = np.flatnonzero(a == 0).astype(np.int64)
    at = np.searchsorted(nul, start)
    first = np.concatenate((nul, np.full(1, a.size, np.int64)))[at]            # the first NUL at or after start
    slen = np.minimum(first, stop) - start
    lens = np.where(slen == 0, NONE32, np.minimum(slen - 1, NONE32 - 1))
    return start.astype(np.uint64), lens.astype(np.uint32), int(nlpos.size)


def nul_lines(data: bytes, line0: int = 0) -> int:
    """Kept lines that hold a NUL byte."""
    a, _nl, _ks, start, stop = line_table(data, line0)
    nul = np.flatnonzero(a == 0)
    return int((np.searchsorted(nul, stop) > np.searchsorted(nul, start)).sum())


def tile_counts(data: bytes, tile: int):
    """Newlines per tile of `tile` bytes."""
    a = np.frombuffer(data, np.uint8)
    return np.bincount(np.flatnonzero(a == 10) // tile, minlength=-(-a.size // tile))


def edge_cuts(data: bytes, edges):
    """Chunk cuts right after the newline nearest to each edge: (the last newline before the edge, the
    first one at or after it), each list sorted, without 0 and the end of the text."""
    nl = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
    before, after = set(), set()
    for e in edges:
        i = int(np.searchsorted(nl, e))
        if i > 0:
            before.add(int(nl[i - 1]) + 1)
        if i < nl.size:
            after.add(int(nl[i]) + 1)
    keep = lambda s: sorted(c for c in s if 0 < c < len(data))                 # noqa: E731
    return keep(before), keep(after)


def first_line_cuts(data: bytes, n: int = 8):
    """A cut after every one of the first n lines."""
    nl = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)[:n]
    return [int(p) + 1 for p in nl if int(p) + 1 < len(data)]


def edges_of(data: bytes, tile: int):
    return list(range(tile, len(data) + 1, tile))


# ---- records -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _nt_pool() -> bytes:
    return np.random.default_rng(4242).choice(np.frombuffer(b"ACGT", np.uint8), 1 << 17).tobytes()


_HDR = b"read_0123456789:abcdefghijklmnopqrstuvwxyz/" * 24


def _nt(rnd, n: int) -> bytes:
    o = rnd.randrange(0, (1 << 17) - n)
    return _nt_pool()[o:o + n]


def record_lines(rnd, h=None, L=None, hmax: int = 30, lmax: int = 150):
    """The four lines of one record, without their newlines: a header of h bytes ('@' included), L nt,
    '+' and L quality bytes."""
    h = rnd.randint(2, hmax) if h is None else h
    L = rnd.randint(0, lmax) if L is None else L
    return [b"@" + _HDR[:h - 1], _nt(rnd, L), b"+", b"I" * L]


def _join(lines) -> bytes:
    return b"".join(ln + b"\n" for ln in lines)


def _newline_after(kind: int, L: int) -> int:
    """Bytes from a record's start to the newline that ends its line `kind`, less the header's length."""
    return (0, 1 + L, 3 + L, 4 + 2 * L)[kind]


def fill_to(rnd, parts, pos: int, P: int, kind: int, L=None, upto=3) -> int:
    """Appends records of mixed lengths 0..150 to parts, then one whose header is padded so that the
    newline ending its line `kind` lands on byte P of the text; that record's lines up to `upto` are
    appended.  -> the text's new length."""
    while P - pos > 700:                       # a filler takes at most 335 bytes: more than 365 are left
        rec = _join(record_lines(rnd))
        parts.append(rec)
        pos += len(rec)
    L = rnd.randint(0, 150) if L is None else L
    h = P - pos - _newline_after(kind, L)      # >= 365 - 304
    rec = _join(record_lines(rnd, h, L)[:upto + 1])
    parts.append(rec)
    return pos + len(rec)


# ---- 1. seams --------------------------------------------------------------------------------------------------

SEAM_DS = (-2, -1, 0, 1)
SEAM_COMBOS = tuple((k, d) for k in range(4) for d in SEAM_DS)
SEAM_COUNT = 32               # seams at m * 16384, m = 1..32: the odd m are seams of the two-pass tiles only


@functools.lru_cache(maxsize=None)
def seam_text(seed: int) -> bytes:
    """The newline ending a line of kind k lands at S + d for all 16 (k, d) at the seams S = 32768 i and
    again at S = 16384 (2 i - 1); records of mixed lengths in between.  An odd seed rotates the order of the
    combinations and ends in a sequence line without a newline."""
    rnd = random.Random(1000 + seed)
    parts, pos = [], 0
    for m in range(1, SEAM_COUNT + 1):
        kind, d = SEAM_COMBOS[((m - 1) // 2 + 5 * seed) % 16]
        pos = fill_to(rnd, parts, pos, m * TILE2 + d, kind)
    for _ in range(20):
        parts.append(_join(record_lines(rnd)))
    if seed & 1:
        parts.append(b"@open\n" + _nt(rnd, 37))
    return b"".join(parts)


SEAM_CUT_SEAMS = (5 * TILE2, 3 * TILE1)
SEAM_CUT_LEAVES = ("complete", "sequence", "other")


@functools.lru_cache(maxsize=None)
def seam_cut_texts():
    """[(name, text, S, end - S, leave)]: seam_text(0) up to a record boundary some way before a 16-KiB and
    a 32-KiB seam S, then continued so that the text ends at S - 1, S or S + 1 with a complete final line,
    inside a sequence line, or inside another line (a quality line, a header)."""
    base = seam_text(0)
    _a, nlpos, _ks, _s, _e = line_table(base)
    recs = nlpos[3::4] + 1
    out = []
    rnd = random.Random(77)
    for S in SEAM_CUT_SEAMS:
        for e in (-1, 0, 1):
            for n, leave in enumerate(SEAM_CUT_LEAVES):
                end = S + e
                at = int(recs[np.searchsorted(recs, end - 1500) - 1])
                parts, m = [base[:at]], rnd.randint(1, 60)
                if leave == "complete":
                    kind = (e + n + S // TILE2) % 4
                    fill_to(rnd, parts, at, end - 1, kind, upto=kind)
                elif leave == "sequence":
                    fill_to(rnd, parts, at, end - 1 - m, 0, upto=0)
                    parts.append(_nt(rnd, m))
                elif e == 0:
                    fill_to(rnd, parts, at, end - 1 - m, 3)
                    parts.append(b"@" + _HDR[:m - 1])
                else:
                    fill_to(rnd, parts, at, end - 1 - m, 2, L=m + 5, upto=2)
                    parts.append(b"I" * m)
                out.append((f"cut {S}{e:+d} {leave}", b"".join(parts), S, e, leave))
    return out


def seam_cases():
    return [Case(f"seams {s}", seam_text(s), 0) for s in (0, 1)] + [Case(n, t, 0) for n, t, _S, _e, _l in seam_cut_texts()]


def seam_census(data: bytes, tile: int):
    """(the (kind, d) pairs found at seams of `tile` bytes, sequence lines that start at a tile start)."""
    _a, nlpos, _ks, start, _stop = line_table(data)
    d = (nlpos + 2) % tile - 2
    at = (d <= 1) & (nlpos + 2 >= tile)
    pairs = set(zip((np.flatnonzero(at) % 4).tolist(), d[at].tolist()))
    return pairs, int(((start % tile == 0) & (start > 0)).sum())


# ---- 2. lines longer than a tile ------------------------------------------------------------------------------

LONG = 70000                  # bytes of a long line, its newline included: at least one whole 32-KiB tile inside
SINGLE = 100000
LONG_PLACES = ("middle", "first", "last", "open")


def _long_line(kind: int, n: int) -> bytes:
    if kind == 1:
        return (_nt_pool()[11:11 + 50000] * (n // 50000 + 1))[:n]
    return (b"@", b"", b"+", b"I")[kind] + (b"h", b"", b"p", b"I")[kind] * (n - 1)


def _plain(rnd, nrec: int):
    return [ln for _ in range(nrec) for ln in record_lines(rnd)]


@functools.lru_cache(maxsize=None)
def long_line_cases():
    """A line of 70 000 bytes of every kind in the middle of a text, as the first line of a chunk (line0 =
    its kind), as the last line with its newline and without one; and one line of 100 000 bytes without a
    newline at every line0."""
    rnd = random.Random(2000)
    out = []
    for kind in range(4):
        for place in LONG_PLACES:
            rec = record_lines(rnd)
            rec[kind] = _long_line(kind, LONG if place == "open" else LONG - 1)
            if place == "middle":
                lines, line0 = _plain(rnd, 20) + rec + _plain(rnd, 20), 0
            elif place == "first":
                lines, line0 = rec[kind:] + _plain(rnd, 20), kind
            else:
                lines, line0 = _plain(rnd, 20) + rec[:kind + 1], 0
            data = _join(lines)
            out.append(Case(f"long {KINDS[kind]} {place}", data[:-1] if place == "open" else data, line0))
    out += [Case(f"single line0 {l0}", b"A" * SINGLE, l0) for l0 in range(4)]
    return out


# ---- 3. one-pass density classes ------------------------------------------------------------------------------

COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2111, 2112, 2113, 4095, 4096,
          4097, 8192, 32768)
DENSITY_LAYOUTS = ("ascending", "shuffled", "paired")


def _segment(rng, count: int) -> bytes:
    """32 KiB with `count` newlines at random places: the last byte is a newline only by chance, so most
    lines cross the segment's edges."""
    seg = np.frombuffer(_nt_pool()[:TILE1], np.uint8).copy()
    seg[rng.choice(TILE1, count, replace=False)] = 10
    return seg.tobytes()


@functools.lru_cache(maxsize=None)
def density_text(layout: str) -> bytes:
    """Segment k of 32 KiB holds exactly the next value of COUNTS, with an ordinary segment (200 to 700
    newlines) before, between and after: COUNTS ascending; in a seeded order; or the ascending layout twice,
    64 tiles apart, so that equal dense tiles meet in one staging shard."""
    rng = np.random.default_rng(3000 + DENSITY_LAYOUTS.index(layout))
    order = list(COUNTS)
    if layout == "shuffled":
        order = [COUNTS[k] for k in rng.permutation(len(COUNTS))]
    segs = [_segment(rng, int(rng.integers(200, 701)))]
    for c in order:
        segs += [_segment(rng, c), _segment(rng, int(rng.integers(200, 701)))]
    if layout == "paired":
        segs += [_segment(rng, int(rng.integers(200, 701))) for _ in range(STAGE_SHARDS - len(segs))] + segs
    return b"".join(segs)


def density_cases():
    return [Case(f"density {lay}", density_text(lay), 0) for lay in DENSITY_LAYOUTS]


def shard_load(data: bytes):
    """Staging words each shard needs: the newlines of its tiles that hold more than kTileCap."""
    c = tile_counts(data, TILE1)
    return np.bincount(np.arange(c.size) % STAGE_SHARDS, np.where(c > TILE_CAP, c, 0), STAGE_SHARDS).astype(np.int64)


# ---- 4. NUL bytes ---------------------------------------------------------------------------------------------

NUL_EDGE_BYTES = (TILE2 - 1, TILE1, 3 * TILE2, 2 * TILE1 - 1)     # last / first byte of a 16-KiB, of a 32-KiB tile


@functools.lru_cache(maxsize=None)
def _nul_base() -> bytes:
    """No NUL yet: a sequence line of 100 nt over each seam of NUL_EDGE_BYTES, a sequence line of 70 000
    bytes, 200 records of 100 to 150 nt (many cross a 1-KiB edge) and an unterminated last sequence line."""
    rnd = random.Random(4000)
    parts, pos = [], 0
    for S in (TILE2, TILE1, 3 * TILE2, 2 * TILE1):
        pos = fill_to(rnd, parts, pos, S - 20, 0, L=100)
    rec = record_lines(rnd)
    rec[1] = _long_line(1, LONG - 1)
    parts.append(_join(_plain(rnd, 10) + rec))
    parts += [_join(record_lines(rnd, L=rnd.randint(100, 150))) for _ in range(200)]
    parts.append(b"@open\n" + _nt(rnd, 41))
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def nul_text(total: int):
    """(text with exactly `total` NUL bytes, {what: position}) -- see the list in nul_census."""
    base = _nul_base()
    offs, lens, _nl = np_index(base)
    offs, lens = offs.astype(np.int64), lens.astype(np.int64)
    _a, nlpos, _ks, _s, _e = line_table(base)
    starts = np.concatenate((np.zeros(1, np.int64), nlpos + 1))
    buf = bytearray(base)
    rnd = random.Random(4100 + total)
    used, put = set(), {}

    def nul(what, p, line=None):
        assert buf[p] not in (0, 10) and (line is None or (line not in used and offs[line] <= p < offs[line] + lens[line]))
        buf[p] = 0
        put[what] = int(p)
        if line is not None:
            used.add(line)

    def free(ok):
        return next(int(i) for i in rnd.sample(range(len(offs) - 1), len(offs) - 1) if i not in used and ok(i))

    for p in NUL_EDGE_BYTES:
        nul(f"byte {p}", p, int(np.searchsorted(offs, p, side="right")) - 1)
    long_i = int(np.argmax(lens))
    nul("long line, third tile", (offs[long_i] // TILE1 + 2) * TILE1 + 17, long_i)
    nul("open last line", int(offs[-1]) + 10, len(offs) - 1)
    i = free(lambda i: 2 <= lens[i] <= 150)
    nul("first byte", int(offs[i]), i)
    i = free(lambda i: 2 <= lens[i] <= 150)
    nul("last byte", int(offs[i] + lens[i] - 1), i)
    edge = (offs // NUL_SUB + 1) * NUL_SUB                       # the first 1-KiB edge after each line's start
    inside = lambda i: lens[i] <= 150 and edge[i] - offs[i] >= 4 and offs[i] + lens[i] - edge[i] >= 5      # noqa: E731
    i = free(inside)
    nul("twice, first", int(edge[i]) - 3, i)
    used.discard(i)
    nul("twice, second", int(edge[i]) + 3, i)
    i = free(inside)
    nul("offset 1023", int(edge[i]) - 1, i)
    i = free(inside)
    nul("offset 1024", int(edge[i]), i)
    recs = rnd.sample([r for r in range(20, len(offs) - 1) if 1 <= lens[r] <= 150], 3)
    for r, kind in zip(recs, (0, 2, 3)):
        nul(f"{KINDS[kind]} line", int(starts[4 * r + kind]) + (1 if kind == 0 else 0))
    k = 0
    while bytes(buf).count(b"\0") < total:                       # the rest: inside sequence lines and in headers
        if k % 2:
            i = free(lambda i: 3 <= lens[i] <= 150)
            nul(f"fill {k}", int(offs[i] + lens[i] // 2), i)
        else:
            p = int(starts[4 * rnd.randrange(20, len(offs) - 1)]) + 1
            if buf[p] != 0:
                nul(f"fill {k}", p)
        k += 1
    return bytes(buf), put


NUL_MANY = (NUL_CAP, NUL_CAP + 1)


@functools.lru_cache(maxsize=None)
def nul_many_text(n: int) -> bytes:
    """n records of 3 to 10 nt, every sequence line with exactly one NUL (at its first, an inner or its
    last byte), from 256 distinct records in a seeded order."""
    rng = np.random.default_rng(4200)
    rnd = random.Random(4200)
    recs = []
    for k in range(256):
        L = 3 + k % 8
        seq = bytearray(_nt(rnd, L))
        seq[(0, L // 2, L - 1, 1)[k % 4]] = 0
        recs.append(b"@" + _HDR[:k % 5] + b"\n" + bytes(seq) + b"\n+\n" + b"I" * L + b"\n")
    return b"".join(recs[k] for k in rng.integers(0, 256, n))


def nul_cases():
    return [Case(f"nul {t}", nul_text(t)[0], 0) for t in (NUL_LIST_SCAN, NUL_LIST_SCAN + 1)] + \
           [Case(f"nul lines {n}", nul_many_text(n), 0) for n in NUL_MANY]


# ---- 5. line phase ----------------------------------------------------------------------------------------------

def tiny_texts(alphabet: bytes, maxlen: int):
    """Every text over the alphabet of length 0..maxlen."""
    return [bytes(t) for n in range(maxlen + 1) for t in itertools.product(alphabet, repeat=n)]


PHASE_MAXLEN = 7


def phase_calls():
    """(text, line0, at_eof) of every text over {A, newline} up to 7 bytes at every line0; at_eof False as
    well where the text is a valid inner chunk (empty, or ending in a newline)."""
    out = []
    for t in tiny_texts(b"A\n", PHASE_MAXLEN):
        for l0 in range(4):
            out.append((t, l0, True))
            if not t or t.endswith(b"\n"):
                out.append((t, l0, False))
    return out


# ---- 6. tile groups ---------------------------------------------------------------------------------------------

GROUPS_BYTES = 1026 * TILE1 + 12345


@functools.lru_cache(maxsize=None)
def groups_text() -> bytes:
    """1026 one-pass tiles and 12 345 bytes: blocks of about 700 KB, each a unit of 200 records of the
    block's own shape (headers up to 2..60 bytes, reads up to 0..300 nt) repeated, so the newlines per
    tile and per group of 1024 tiles differ.  No final newline."""
    rnd = random.Random(6000)
    blocks, size = [], 0
    while size < GROUPS_BYTES:
        hmax, lmax = rnd.randint(2, 60), rnd.choice((0, 5, 20, 36, 75, 150, 300))
        unit = b"".join(_join(record_lines(rnd, hmax=hmax, lmax=lmax)) for _ in range(200))
        blocks.append(unit * (700_000 // len(unit) + 1))
        size += len(blocks[-1])
    data = b"".join(blocks)[:GROUPS_BYTES]
    return data[:-1] + b"A" if data.endswith(b"\n") else data


def groups_census(data: bytes, tile: int):
    """(tiles, groups, newlines per group)."""
    c = tile_counts(data, tile)
    tot = np.add.reduceat(c, np.arange(0, c.size, GROUP_TILES))
    return int(c.size), int(tot.size), [int(x) for x in tot]


def middle_cut(data: bytes):
    nl = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
    return int(nl[np.searchsorted(nl, len(data) // 2)]) + 1


# ---- the engine ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dense_file_text(size: int = 1 << 20) -> bytes:
    """About 1 MiB of very short valid records: headers '@' + 0..3 bytes, reads of 1..7 nt (4 bytes per
    line on average: 8 000 newlines per 32-KiB tile)."""
    rnd = random.Random(7000)
    recs = [_join(record_lines(rnd, rnd.randint(1, 4), rnd.randint(1, 7))) for _ in range(4096)]
    out, n = [], 0
    while n < size:
        out.append(recs[rnd.randrange(4096)])
        n += len(out[-1])
    return b"".join(out)
