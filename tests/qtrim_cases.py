"""The 3' quality trim sweep shared by test_qtrim.py (host rule against a Python restatement) and
test_qtrim_gpu.py (device against host): the rule and the quality-line locate restated in Python, and the
smallest shapes at which the kernel can still go wrong -- lengths around the 16-byte chunks, one round of
every lane group (16 * G for G = 2, 4, 8) and the 1024 limit, every cut position, sums that return to zero,
equal maxima, breaks and maxima at the first and last byte of a chunk and of a round, hostile bytes, and for
the FASTQ layout every start residue, '+' lines of several lengths, short, long and missing quality lines
and texts that end early.  Everything is seeded."""
import numpy as np

LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 255, 256, 257, 1023, 1024)
CUTOFFS = (1, 2, 20, 30, 93)
BASES = (33, 64)
HOSTILE = (0x00, 0x20, 0x7F, 0xFF)
PLUS_LENS = (1, 15, 16, 17, 300)
FAKE = ((1025, None), (0xFFFFFFFF, None))
GROUPS = (2, 4, 8)          # lane groups whose round edges the sweep plants breaks and maxima at


def ref_qtrim(q: bytes, L: int, cutoff: int, base: int) -> int:
    """The rule, restated over the running sums: the rightmost position of the greatest positive sum met
    before the first negative one, else L."""
    if L > 1024:
        return L
    sums = np.cumsum(cutoff + base - np.frombuffer(q[:L], np.uint8)[::-1].astype(np.int64))
    neg = np.nonzero(sums < 0)[0]
    sums = sums[:neg[0]] if neg.size else sums
    if sums.size == 0 or sums.max() <= 0:
        return L
    return L - 1 - int(np.argmax(sums))       # (argmax: the first maximum met from the right)


def ref_locate(blob: bytes, off: int, L: int):
    """(qoff, Q) of the quality line of the sequence line blob[off : off + L], or None."""
    e1 = blob.find(b"\n", off + L)
    if e1 < 0:
        return None
    e2 = blob.find(b"\n", e1 + 1)
    if e2 < 0:
        return None
    e3 = blob.find(b"\n", e2 + 1)
    return e2 + 1, (len(blob) if e3 < 0 else e3) - e2 - 1


def ref_fastq(blob: bytes, off: int, L: int, cutoff: int, base: int):
    """(new length, usable) of one read in the FASTQ layout form."""
    if L == 0 or L > 1024:
        return L, True
    loc = ref_locate(blob, off, L)
    if loc is None or loc[1] < L:
        return L, False
    return ref_qtrim(blob[loc[0]:loc[0] + L], L, cutoff, base), True


def score(cutoff: int, base: int, d: int) -> int:
    """The quality byte whose score c - (q - b) is d."""
    q = cutoff + base - d
    assert 0 <= q <= 255
    return q


def from_scores(cutoff: int, base: int, ds) -> bytes:
    return bytes(score(cutoff, base, d) for d in ds)


def edge_case(cutoff: int, base: int, L: int, p_break: int, p_max: int) -> bytes:
    """Scores 0 right of p_max, +1 at p_max (the only maximum: stop = p_max), 0 down to p_break, where -2
    ends the walk; left of it a low run (+1 each) that must stay."""
    assert 0 <= p_break < p_max < L
    ds = [1] * p_break + [-2] + [0] * (p_max - p_break - 1) + [1] + [0] * (L - 1 - p_max)
    return from_scores(cutoff, base, ds)


def sweep_quals(rng, cutoff: int, base: int, newline: bool):
    """The quality runs of one (cutoff, base); a (fake length, None) entry is a read that must not be read.
    newline: '\\n' may stand among the hostile bytes (the explicit form only)."""
    c, b = cutoff, base
    hi, lo = score(c, b, -min(10, 255 - c - b)), score(c, b, 1)
    out = []
    for L in LENGTHS:
        out.append(bytes([hi]) * L)                                     # all high: no trim
        out.append(bytes([lo]) * L)                                     # all low: trims to 0
        out.append(bytes([c + b]) * L)                                  # exactly at the cutoff: every score 0
        out.append(bytes(rng.integers(max(0, c + b - 3), c + b + 4, L, dtype=np.int64).astype(np.uint8)))
        if L >= 3:
            out.append(from_scores(c, b, [-1] * (L - 3) + [1, -1, 1]))  # 1, 0, 1 then break: the right maximum wins
    out += list(FAKE)
    good = [-2] * 40
    for k in range(1, 41):                                              # a low tail of every length: every cut position
        out.append(from_scores(c, b, good[:40 - k] + [1] * k))
    # a tail whose sum returns to exactly 0 and then rises: no break, the maximum lies further left
    out.append(from_scores(c, b, [-2] * 20 + [1, 1, 1, -1, 1]))         # sums 1 0 1 2 3 then -: stop 20
    out.append(from_scores(c, b, [-2] * 20 + [1, 1, -1, -1, 1, 1]))     # sums 1 2 1 0 1 2: equal maxima, the right one: 24
    # low tail, a high run that breaks the walk, a low run further left that must stay
    out.append(from_scores(c, b, [1] * 10 + [-2] * 5 + [1] * 3))
    out.append(from_scores(c, b, [1] * 30 + [-1] * 4 + [1] * 3))       # 1 2 3 2 1 0 -1: breaks after touching 0
    # two equal maxima with a dip between them: the right one wins
    out.append(from_scores(c, b, [-2] * 8 + [1, -1, 0, 1, 1]))          # sums 1 2 2 1 2 then -: stop 11
    # the break, and the maximum, at the first and last byte of a 16-B chunk and of a round (whatever the
    # run's alignment: every position next to a multiple of 16 from either end, on runs that span two rounds)
    for G in GROUPS:
        for L in (16 * G - 1, 16 * G + 1, 32 * G + 3):
            edges = sorted({p for p in range(L - 1) if p % 16 in (0, 1, 14, 15) or (L - p) % 16 in (0, 1, 2, 15)})
            for p in edges:
                out.append(edge_case(c, b, L, p, p + 1))
                if p + 17 < L:
                    out.append(edge_case(c, b, L, p, p + 17))
    # hostile bytes at and near the 3' end, in a run that is otherwise at the cutoff
    hostile = HOSTILE + ((0x0A,) if newline else ())
    for hb in hostile:
        for k in (0, 1, 15, 16, 29):
            q = bytearray([c + b] * 30)
            q[29 - k] = hb
            out.append(bytes(q))
            q = bytearray([lo] * 30)
            q[29 - k] = hb
            out.append(bytes(q))
    return out


def explicit_layout(rng, quals):
    """(blob, offsets, lens, qual, qoffsets) for the explicit form: read k's qualities start at residue
    k mod 16 of `qual`; the sequence bytes are junk that is never read.  A (length, None) entry gets offsets
    inside the buffers and takes no bytes."""
    parts, qoffs, lens = [], [], []
    pos = 0
    for k, q in enumerate(quals):
        if isinstance(q, tuple):
            qoffs.append(pos // 2)
            lens.append(q[0])
            continue
        pad = (k % 16 - pos) % 16
        parts += [b"\n" * pad, q]
        qoffs.append(pos + pad)
        lens.append(len(q))
        pos += pad + len(q)
    qual = np.frombuffer(b"".join(parts), np.uint8).copy() if pos else np.zeros(0, np.uint8)
    blob = np.full(max(pos, 1), ord("A"), np.uint8)
    qoffs = np.array(qoffs, np.uint64)
    return blob, qoffs.copy(), np.array(lens, np.uint32), qual, qoffs


def expected_explicit(quals, cutoff: int, base: int):
    out = [q[0] if isinstance(q, tuple) else ref_qtrim(q, len(q), cutoff, base) for q in quals]
    full = [q[0] if isinstance(q, tuple) else len(q) for q in quals]
    return (np.array(out, np.uint32),
            [sum(1 for a, f in zip(out, full) if a < f), sum(f - a for a, f in zip(out, full)), 0])


def fastq_layout(rng, quals, tail: bytes = b"\n"):
    """FASTQ text of one record per quality run (no '\\n' in it) and its index (offsets, lens): record k's
    sequence line starts at residue k mod 16, its '+' line has PLUS_LENS[k % 5] bytes; every eighth record's
    quality line is one byte longer than its read, every eighth (offset 4) one byte shorter, every 41st
    empty.  The text ends with `tail` after the last quality line.  A (length, None) entry gets an offset
    inside the text."""
    parts, offs, lens = [], [], []
    pos = 0
    for k, q in enumerate(quals):
        if isinstance(q, tuple):
            offs.append(pos // 2)
            lens.append(q[0])
            continue
        assert b"\n" not in q
        L = len(q)
        hdr = b"@" + b"h" * ((k % 16 - pos - 2) % 16) + b"\n"
        plus = b"+" + b"p" * (PLUS_LENS[k % 5] - 1) + b"\n"
        ql = q + b"J" if k % 8 == 1 else q[:-1] if k % 8 == 5 and L else b"" if k % 41 == 7 else q
        rec = hdr + b"A" * L + b"\n" + plus + ql + b"\n"
        offs.append(pos + len(hdr))
        lens.append(L)
        parts.append(rec)
        pos += len(rec)
    text = b"".join(parts)
    if text:
        text = text[:-1] + tail
    return text, np.array(offs, np.uint64), np.array(lens, np.uint32)


def expected_fastq(text: bytes, offs, lens, cutoff: int, base: int):
    out, noq = [], 0
    for o, L in zip(offs.tolist(), lens.tolist()):
        k, usable = ref_fastq(text, o, L, cutoff, base)
        out.append(k)
        noq += not usable
    full = lens.tolist()
    return (np.array(out, np.uint32),
            [sum(1 for a, f in zip(out, full) if a < f), sum(f - a for a, f in zip(out, full)), noq])


def as_blob(text: bytes) -> np.ndarray:
    return np.frombuffer(text, np.uint8).copy() if text else np.zeros(0, np.uint8)


def special_texts(cutoff: int, base: int):
    """(text, offsets, lens) of small FASTQ texts around the ends of the layout form: the text ending after
    the sequence's newline, after the '+' line and inside the quality line (every cut of a two-record text
    from the second sequence line on), a last quality line of exactly L bytes with no newline, and a
    sequence line shortened by a NUL (its length is strlen - 1)."""
    lo, hi = score(cutoff, base, 1), score(cutoff, base, -2)
    L = 20
    rec = b"@r\n" + b"A" * L + b"\n+\n" + bytes([hi]) * 12 + bytes([lo]) * 8 + b"\n"
    two = rec + rec
    offs = np.array([3, len(rec) + 3], np.uint64)
    lens = np.array([L, L], np.uint32)
    out = [(two[:cut], offs, lens) for cut in range(len(rec) + 3 + L, len(two) + 1)]
    nul = b"@r\nACGTACG\x00TTTT\n+\n" + bytes([hi]) * 3 + bytes([lo]) * 9 + b"\n"
    out.append((nul + rec, np.array([3, len(nul) + 3], np.uint64), np.array([6, L], np.uint32)))
    return out


def degraded_library(rng, n: int, adapter: bytes = b"TGGAATTCTCGGGTGCCAAGG", pool: int = 300, cutoff: int = 20, base: int = 33):
    """A library-like FASTQ file: n records of an insert from a pool, the adapter's start and a few more
    bases; about a third of the reads have a 3' tail of 1..12 bases that degrades (qualities below the
    cutoff, and bases that are sequencing noise).  -> (text, sequence lines, quality lines)."""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    inserts = [bytes(rng.choice(acgt, int(rng.integers(15, 41)))) for _ in range(pool)]
    picks = rng.integers(0, pool, n)
    bad = rng.random(n) < 0.35
    tails = rng.integers(1, 13, n)
    recs, seqs, quals = [], [], []
    for i in range(n):
        s = bytearray(inserts[picks[i]] + adapter[:int(rng.integers(8, 22))])
        q = bytearray(rng.integers(base + cutoff + 5, base + cutoff + 20, len(s), dtype=np.int64).astype(np.uint8))
        if bad[i]:
            k = int(tails[i])
            s[-k:] = bytes(rng.choice(acgt, k))
            q[-k:] = bytes(rng.integers(base + 2, base + cutoff, k, dtype=np.int64).astype(np.uint8))
        seqs.append(bytes(s))
        quals.append(bytes(q))
        recs.append(b"@read%d\n" % i + bytes(s) + b"\n+\n" + bytes(q) + b"\n")
    return b"".join(recs), seqs, quals
