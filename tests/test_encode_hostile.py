"""Encode kernels against the oracle on hostile bytes: every accepted byte value, every start
alignment x tail length, rejected bytes all around the reads.

The ragged encode kernels (k_encode_var_dense, and the drop-in engine's k_short_keys, k_encode_rows,
k_encode_classes, k_encode_class) load the whole 16-byte chunks a word touches, encode them where
they lie, shift by the start alignment, mask what lies past the read, and divert a word whose chunks
hold a rejected or bit-6-clear byte to an exact re-encode.  The corpus here is built so that a wrong
mask, shift, alias rule or diversion shows:

  * layout() puts the reads at explicit offsets: the start alignment (offset % 16) steps through
    0..15, and the 16 head bytes, every gap byte and the tail pad (>= 32 bytes, to the end of a
    16-byte chunk) are bytes the oracle rejects -- so every read has a rejected byte right before and
    right after it, and a batch of valid reads must still encode without raising;
  * a content is clean (a: random ACGT), accepted-hostile (b: the 16 accepted byte values -- c & 0x3F
    in {0x01, 0x03, 0x07, 0x14}, bits 6 and 7 free; bit 6 clear is an alias whose table-path code
    carries into the next nucleotide -- at the first / last / chunk-edge / word-edge positions) or
    rejected (c: one rejected byte at one of those positions);
  * a corpus lists an odd number of contents 16 times over, so each content lands at all 16
    alignments and its count is 16 x its multiplicity: a wrong encode at one alignment splits a key;
  * the encode_var and engine batches run a second and third time with the same reads between plain
    bases and between all 16 accepted values (GAPS): there a read's first and last word stay on the
    fast path, or have an alias right behind the read's end.

Expected values come from the oracle alone (oracle.encode_one / encode_batch / count).
"""
import ctypes as C
import functools

import numpy as np
import pytest

ACCEPTED = tuple(sorted(lo | hi for lo in (0x01, 0x03, 0x07, 0x14) for hi in (0x00, 0x40, 0x80, 0xC0)))
ALIASES = tuple(b for b in ACCEPTED if not b & 0x40)          # bit 6 clear: table-path carry
REJECTED = tuple(b for b in range(256) if b not in ACCEPTED)  # 240 values
# the gap alphabet: FASTQ neighbours, near-misses of the accepted values, the ends of both halves
FASTQ_BYTES = (0x0A, ord("@"), ord("+"), ord("!"), ord("#"), ord("5"), ord("I"), ord("~"), ord("N"), ord("a"),
               0x00, 0x7F, 0x80, 0xFF)
GAP_BYTES = FASTQ_BYTES + (0x02, 0x15, 0x42, 0x45, 0x55, 0x74, 0xC0, 0xC2, 0xBF)
NEAR_MISSES = tuple(sorted({a ^ (1 << k) for a in ACCEPTED for k in range(6)} - set(ACCEPTED)))
# friendly neighbours: with only plain bases around it a read's first and last word stay on the
# kernels' fast path (the mask and the shift decide alone); with all 16 accepted values around it an
# alias sits right behind the read's end, where a leaking mask would let it carry
GAPS = {"rejected": GAP_BYTES, "plain": tuple(b for b in ACCEPTED if b & 0x40), "accepted": ACCEPTED}
TOO_LONG = "Sequences longer than 1024 bases are not supported."
_PLAIN = np.frombuffer(b"ACTG", np.uint8)                     # code (c >> 1) & 3 -> the plain base


# ------------------------------------------------------------------------------------------------
# corpus builder (plain numpy)
# ------------------------------------------------------------------------------------------------
def positions(L):
    """{0, 1, 15, 16, 31, 32, 32k - 1, 32k, L - 2, L - 1} within [0, L): first, last, chunk edge, word edges."""
    p = {0, 1, 15, 16, 31, 32, L - 2, L - 1}
    for k in range(1, L // 32 + 2):
        p |= {32 * k - 1, 32 * k}
    return sorted(x for x in p if 0 <= x < L)


def clean(L, rng):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes()


class _Cycle:
    """The 16 accepted values, the 8 aliases and the 4 plain bases handed out in turn, so a corpus of a
    few dozen (b) reads uses every value and every alias -> next-base pair."""

    def __init__(self):
        self.acc = [0, 0]
        self.pair = 0

    def accepted(self, tail=False):
        """(one turn for the bytes of tail words, one for those of full 32-nt words)"""
        self.acc[tail] += 1
        return ACCEPTED[(self.acc[tail] * 7) % 16]  # 7: neighbours in a read are not neighbours in value

    def alias_pair(self):
        self.pair += 1
        return ALIASES[self.pair % 8], b"ACGT"[(self.pair // 8) % 4]


def hostile(L, rng, cyc):
    """(b): random ACGT with the position set overwritten by accepted values, an alias followed by a
    chosen plain base at two random places of the tail word, and one more accepted value anywhere."""
    r = bytearray(clean(L, rng))
    if L == 0:
        return bytes(r)
    pos = positions(L)
    t0 = 32 * ((L - 1) // 32)                      # the tail word's first byte
    table = L <= 32 or L % 32 != 0                 # ... which takes the table path
    for p in [int(rng.integers(0, L))] + pos:
        r[p] = cyc.accepted(table and p >= t0)
    for _ in range(2):
        free = [p for p in range(t0, L - 1) if not {p - 1, p, p + 1, p + 2} & set(pos)]
        if free:
            p = free[int(rng.integers(0, len(free)))]
            r[p], r[p + 1] = cyc.alias_pair()
            pos = pos + [p, p + 1]
    return bytes(r)


def rejected(read, pos, byte):
    """(c): `read` with exactly one rejected byte."""
    assert byte in REJECTED and 0 <= pos < len(read)
    r = bytearray(read)
    r[pos] = byte
    return bytes(r)


def plain_twin(read):
    """The read with every byte replaced by the plain base of its code bits."""
    a = np.frombuffer(read, np.uint8)
    return _PLAIN[(a >> 1) & 3].tobytes()


def twin_differs(read):
    """Whether the table path makes `read` encode differently from plain_twin(read), from the rule: in a
    table-path word (the only word of a read <= 32 nt, the partial tail word of a longer one) an alias
    is the value 4 at its place, ORed in: its own two bits stay clear and bit 2 lands on the next
    nucleotide's low bit (lost past bit 63).  Full 32-nt words of longer reads carry nothing."""
    L = len(read)
    for w in range((L + 31) // 32):
        nb = min(32, L - 32 * w)
        if L > 32 and nb == 32:
            continue
        word = twin = 0
        for j in range(nb):
            b = read[32 * w + j]
            word |= ((b >> 1) & 3 if b & 0x40 else 4) << 2 * j
            twin |= ((b >> 1) & 3) << 2 * j
        if word & (1 << 64) - 1 != twin:
            return True
    return False


def layout(reads, seed, gap_bytes=GAP_BYTES):
    """Place `reads` at explicit offsets -> (blob u8, offsets i64, lens i32).  Read i starts at
    alignment i % 16 behind a gap of 1..16 rejected bytes; 16 rejected head bytes; a tail pad of at
    least 32 rejected bytes that ends the blob on a 16-byte chunk (the kernels' contract: the blob is
    readable to the end of its last 16-byte chunk).  (gap_bytes: another alphabet for all of those.)"""
    rng = np.random.default_rng(seed)
    gap = np.array(gap_bytes, np.uint8)

    def fill(k):
        return gap[rng.integers(0, len(gap), k)].tobytes()

    parts, offs, pos = [fill(16)], [], 16
    for i, r in enumerate(reads):
        g = (i % 16 - pos) % 16 or 16
        parts.append(fill(g))
        pos += g
        offs.append(pos)
        parts.append(r)
        pos += len(r)
    tail = 32 + (-(pos + 32)) % 16
    parts.append(fill(tail))
    blob = np.frombuffer(b"".join(parts), np.uint8).copy()
    return blob, np.array(offs, np.int64), np.array([len(r) for r in reads], np.int32)


def corpus(lengths, seed, extra=()):
    """-> (contents, kinds, reads): for each length one (a) and one (b) content (+ `extra` contents,
    + two repeated contents: multiplicity 2), padded to an odd number, listed 16 times over."""
    rng = np.random.default_rng(seed)
    cyc = _Cycle()
    contents, kinds = [], []
    for L in lengths:
        contents += [clean(L, rng), hostile(L, rng, cyc)]
        kinds += ["a", "b"]
    for r in extra:
        contents.append(r)
        kinds.append("a" if set(r) <= set(b"ACGT") else "b")
    for k in (1, len(contents) // 2):               # a (b) content and another one, twice each
        contents.append(contents[k])
        kinds.append(kinds[k])
    if len(contents) % 2 == 0:
        L = [x for x in lengths if x][0]
        contents.append(clean(L, rng))
        kinds.append("a")
    return contents, kinds, contents * 16


def _tails(classes, per):
    """Lengths 32 c + t for every tail t = 1..32, `per` classes c each, taken in turn from `classes`."""
    out, k = [], 0
    for t in range(1, 33):
        for _ in range(per):
            out.append(32 * classes[k % len(classes)] + t)
            k += 1
    return out


VAR_LENGTHS = list(range(0, 201)) + [255, 256, 257, 480, 481, 511, 512, 513, 1000, 1023, 1024]


def _rows_lengths(S):
    """k_encode_rows at stride S: every length of the top class, a sample of the lower ones."""
    top = list(range(32 * (S - 2) + 1, 32 * (S - 1) + 1))
    low = [L for L in (33, 47, 48, 49, 64, 65, 80, 96, 97, 111, 128) if L < top[0]]
    return top + low


# name -> (lengths, extra contents); the dispatch these steer is ss_ingest.hip's process_chunk
CORPORA = {
    "var": (VAR_LENGTHS, ()),
    "var200": (list(range(0, 201)), ()),
    "short": (list(range(1, 32)) + [0, 32], ()),                            # k_short_keys (+ the 32-nt table)
    "rows3": (_rows_lengths(3), (b"",)),                                    # k_encode_rows, S = 3..6
    "rows4": (_rows_lengths(4), (b"",)),
    "rows5": (_rows_lengths(5), (b"",)),
    "rows6": (_rows_lengths(6), (b"",)),
    "classes_mixed": (_tails(list(range(0, 15)), 3), ()),                   # k_encode_classes, 1..480 nt
    "classes_wide": (_tails(list(range(6, 15)), 2), ()),                    # k_encode_classes, 193..480 nt
    "class_long": (_tails(list(range(15, 32)), 1) + [40, 200, 7], ()),      # k_encode_class, 481..1024 nt
}
INGEST = ["short", "rows3", "rows4", "rows5", "rows6", "classes_mixed", "classes_wide", "class_long"]


@functools.lru_cache(maxsize=None)
def get_corpus(name, gaps="rejected"):
    lengths, extra = CORPORA[name]
    seed = 1000 + sorted(CORPORA).index(name)
    contents, kinds, reads = corpus(lengths, seed, extra)
    blob, offs, lens = layout(reads, seed, GAPS[gaps])
    return {"contents": contents, "kinds": kinds, "reads": reads, "blob": blob, "offs": offs, "lens": lens}


def _tail_bytes(L):
    return (L - 1) % 32 + 1


def expected_rows(exp):
    """oracle.count rows -> the ss_ingest_results layout (ceil(L / 32) words a row, none for L = 0)."""
    return ([L for (_w, L, _c, _f) in exp], [c for (_w, _L, c, _f) in exp],
            [int(x) for (w, L, _c, _f) in exp for x in w[:(L + 31) // 32]])


def expected_error(oracle, reads):
    """What the reference raises for the first rejected read of `reads` -> (type, message, read index,
    whether the product attaches .read_index): the bytes oracle.count names, decoded as ASCII."""
    with pytest.raises(ValueError) as ei:
        oracle.count(reads)
    kind, idx, off, nb = ei.value.args[0]
    if kind == 2:
        return Exception, TOO_LONG, idx, False
    bad = reads[idx][off:off + nb]
    try:
        return Exception, "Unsupported base character: " + bad.decode("ascii"), idx, True
    except UnicodeDecodeError as u:
        return UnicodeDecodeError, str(u), idx, False


def check_raised(ei, want, *, index_required=True):
    typ, msg, idx, has_index = want
    assert type(ei.value) is typ and str(ei.value) == msg, (type(ei.value), str(ei.value), want)
    if has_index and index_required:
        assert ei.value.read_index == idx
    else:
        assert getattr(ei.value, "read_index", idx) == idx


# ------------------------------------------------------------------------------------------------
# CPU: the corpus has the coverage the GPU tests rely on, and the host paths agree with the oracle
# ------------------------------------------------------------------------------------------------
def test_byte_classes_match_oracle(oracle):
    """The oracle accepts exactly ACCEPTED (16 values) and rejects every gap, near-miss and FASTQ byte."""
    ok = tuple(b for b in range(256) if oracle.encode_one(bytes([b]))[1].kind == 0)
    assert ok == ACCEPTED and len(REJECTED) == 240
    assert set(GAP_BYTES) <= set(REJECTED) and set(NEAR_MISSES) <= set(REJECTED)
    assert len(NEAR_MISSES) >= 60
    # bit 7 is ignored, bit 6 picks plain base against alias with carry
    assert [int(oracle.encode_one(bytes([b]))[0][0]) for b in (0x41, 0xC1, 0x01, 0x81)] == [0, 0, 4, 4]


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_corpus_coverage(oracle, name):
    c = get_corpus(name)
    contents, kinds, reads, blob, offs, lens = (c[k] for k in ("contents", "kinds", "reads", "blob", "offs", "lens"))
    n = len(reads)
    assert len(contents) % 2 == 1 and n == 16 * len(contents) and n <= 7000
    assert name not in INGEST or n <= 4200
    # the layout: explicit offsets, hostile head / gaps / tail, the pad to the last chunk's end
    rej = np.zeros(256, bool)
    rej[list(REJECTED)] = True
    inside = np.zeros(len(blob), bool)
    for o, L, r in zip(offs, lens, reads):
        assert blob[o:o + L].tobytes() == r
        assert not inside[o:o + L].any()
        inside[o:o + L] = True
        assert rej[blob[o - 1]] and rej[blob[o + L]]
    assert rej[blob[~inside]].all() and not inside[:16].any()
    end = int(offs[-1] + lens[-1])
    assert len(blob) % 16 == 0 and len(blob) - end >= 32
    assert (offs % 16 == np.arange(n) % 16).all()
    # every content at every alignment; every (alignment, tail bytes) pair
    seen = {}
    for i, r in enumerate(reads):
        seen.setdefault(r, set()).add(int(offs[i] % 16))
    assert all(v == set(range(16)) for v in seen.values())
    pairs = {(int(o % 16), _tail_bytes(int(L))) for o, L in zip(offs, lens) if L}
    assert pairs >= {(a, t) for a in range(16) for t in range(1, 33)}
    assert {"a", "b"} <= set(kinds)
    # every accepted byte in a tail (table-path) word and -- where the corpus has reads past 32 nt -- in
    # a full 32-nt word; every alias followed by each plain base inside a tail word
    in_tail, in_full, alias_next = set(), set(), set()
    for r in contents:
        L = len(r)
        t0 = 32 * ((L - 1) // 32) if L else 0
        in_tail |= set(r[t0:]) if (L <= 32 or L % 32) else set()
        if L > 32:
            in_full |= set(r[:32 * (L // 32)])
        tail = r[t0:] if (L <= 32 or L % 32) else b""
        alias_next |= {(x, y) for x, y in zip(tail, tail[1:]) if x in ALIASES and y in b"ACGT"}
    assert in_tail >= set(ACCEPTED)
    assert max(len(r) for r in contents) <= 32 or in_full >= set(ACCEPTED)
    assert alias_next >= {(x, y) for x in ALIASES for y in b"ACGT"}
    # no (a) or (b) read is rejected; a (b) read differs from its plain twin exactly where the rule says
    differ = equal = 0
    for r, k in zip(contents, kinds):
        w, e = oracle.encode_one(r)
        assert e.kind == 0, r
        if k == "b":
            tw, te = oracle.encode_one(plain_twin(r))
            assert te.kind == 0
            d = not np.array_equal(w, tw)
            assert d == twin_differs(r), r
            differ += d
            equal += not d
    # (the equal ones are known equal by the rule above: no table-path word, or a carry onto a set bit)
    assert differ >= 16 and differ + equal == kinds.count("b"), (differ, equal)
    # the counts: a wrong encode at one alignment would split a key
    exp = oracle.count(reads)
    assert all(cnt % 16 == 0 for (_w, _L, cnt, _f) in exp) and sum(cnt for (_w, _L, cnt, _f) in exp) == n


@pytest.mark.parametrize("gaps", ["plain", "accepted"])
def test_friendly_layout(gaps):
    """The same reads between accepted bytes: placed and aligned alike, every gap byte of the alphabet."""
    for name in ("var200", "rows4", "classes_mixed"):
        c, h = get_corpus(name, gaps), get_corpus(name)
        assert c["reads"] == h["reads"] and (c["offs"] == h["offs"]).all() and len(c["blob"]) == len(h["blob"])
        inside = np.zeros(len(c["blob"]), bool)
        for o, L in zip(c["offs"], c["lens"]):
            assert c["blob"][o:o + L].tobytes() == h["blob"][o:o + L].tobytes()
            inside[o:o + L] = True
        assert set(c["blob"][~inside].tolist()) == set(GAPS[gaps])


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_host_paths_match_oracle(oracle, name):
    """ss_host_encode == oracle.encode_one and ShortSeqCounter(device="host") == oracle.count on the corpus."""
    from shortseq_amd import ShortSeqCounter, _native
    lib = _native.lib()
    c = get_corpus(name)
    for r in c["contents"]:
        L = len(r)
        wo, eo = oracle.encode_one(r, 32)
        wh = np.zeros(32, np.uint64)
        eh = _native.SsErr()
        buf = np.frombuffer(r, np.uint8) if L else np.zeros(1, np.uint8)
        assert lib.ss_host_encode(buf.ctypes.data, L, wh.ctypes.data, C.byref(eh)) == eo.kind == 0
        assert np.array_equal(wh, wo), r
    got = ShortSeqCounter(c["reads"], device="host")
    el, ec, ew = expected_rows(oracle.count(c["reads"]))
    assert [len(k) for k in got] == el
    assert list(got.values()) == ec
    assert [int(x) for k in got for x in k.packed[:(len(k) + 31) // 32]] == ew


def test_host_rejects_like_oracle(oracle):
    """(c) reads: the host codec names the bytes the oracle names, for every rejected value."""
    from shortseq_amd import _native
    lib = _native.lib()
    rng = np.random.default_rng(77)
    cyc = _Cycle()
    for k, byte in enumerate(REJECTED):
        L = (1, 16, 31, 32, 33, 48, 96, 100, 161)[k % 9]
        pos = positions(L)
        r = rejected(hostile(L, rng, cyc), pos[k % len(pos)], byte)
        _w, eo = oracle.encode_one(r, 32)
        wh = np.zeros(32, np.uint64)
        eh = _native.SsErr()
        assert lib.ss_host_encode(np.frombuffer(r, np.uint8).ctypes.data, L, wh.ctypes.data, C.byref(eh)) == eo.kind == 1
        assert (eh.byte_offset, eh.nbytes) == (eo.byte_offset, eo.nbytes)


# ------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------
def _dev(gpu, c):
    import torch
    return tuple(torch.from_numpy(c[k]).to(gpu) for k in ("blob", "offs", "lens"))


GAPS_ALL = ["rejected", "plain", "accepted"]


def _dev_reads(gpu, reads, seed):
    import torch
    return tuple(torch.from_numpy(a).to(gpu) for a in layout(reads, seed))


@functools.lru_cache(maxsize=None)
def _expected_words(name, wpr):
    """[n, wpr] oracle words of the corpus, one oracle.encode_one per content."""
    import oracle
    c = get_corpus(name)
    per = {}
    for r in c["contents"]:
        if r not in per:
            w, e = oracle.encode_one(r, wpr)
            assert e.kind == 0
            per[r] = w
    return np.stack([per[r] for r in c["reads"]])


def _assert_rows(got, exp):
    gl, gc, gw = got
    el, ec, ew = expected_rows(exp)
    assert gl.tolist() == el
    assert gc.tolist() == ec
    assert gw.tolist() == ew


# ------------------------------------------------------------------------------------------------
# GPU: encode_var (k_encode_var_dense)
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("gaps", GAPS_ALL)
@pytest.mark.parametrize("name,wpr", [("var", 32), ("var", None), ("var200", None)])
def test_encode_var_hostile(gpu, oracle, name, wpr, gaps):
    """Every length 0..200 and the class edges up to 1024, (a) and (b), at all 16 alignments between
    rejected neighbours: every row and every word (the zero padding included) == oracle.encode_one;
    the call does not raise.  var200's default wpr is 7 (no power of two).  (gaps: the same between
    plain bases and between all accepted values.)"""
    import shortseq_amd.batch as B
    c = get_corpus(name, gaps)
    blob, offs, lens = _dev(gpu, c)
    words = B.encode_var(blob, offs, lens, wpr=wpr)
    w = wpr if wpr is not None else max(1, (max(CORPORA[name][0]) + 31) // 32)
    assert tuple(words.shape) == (len(c["reads"]), w)
    got = words.cpu().numpy().view(np.uint64)
    exp = _expected_words(name, w)
    bad = np.nonzero((got != exp).any(1))[0]
    assert not len(bad), [(int(i), len(c["reads"][i]), int(c["offs"][i] % 16)) for i in bad[:8]]


# ------------------------------------------------------------------------------------------------
# GPU: the ingest kernels through DeviceIngest
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("gaps", GAPS_ALL)
@pytest.mark.parametrize("name", INGEST)
def test_ingest_hostile(gpu, oracle, name, gaps):
    """One batch per kernel (k_short_keys; k_encode_rows at S = 3..6; k_encode_classes with and without
    short reads; k_encode_class): lengths, counts, words and first-occurrence order == oracle.count.
    (gaps: the same reads between rejected bytes, between plain bases, between all accepted values.)"""
    import shortseq_amd.batch as B
    c = get_corpus(name, gaps)
    blob, offs, lens = _dev(gpu, c)
    eng = B.DeviceIngest(gpu)
    try:
        eng.count(blob, offs, lens)
        got = eng.results()
    finally:
        eng.close()
    _assert_rows(got, oracle.count(c["reads"]))


@pytest.mark.gpu
def test_ingest_hostile_speculative_rows(gpu, oracle):
    """The S = 4 corpus over four count() calls on one engine: the second call's row encode is queued
    gated behind the split, the third and fourth run it on the side stream; results() after each call
    == oracle.count of the reads so far."""
    import shortseq_amd.batch as B
    c = get_corpus("rows4")
    blob, offs, lens = _dev(gpu, c)
    n = len(c["reads"])
    cuts = [0, n // 4 + 3, n // 2 + 1, 3 * n // 4 + 2, n]
    eng = B.DeviceIngest(gpu)
    try:
        for a, b in zip(cuts, cuts[1:]):
            eng.count(blob, offs[a:b], lens[a:b])
            _assert_rows(eng.results(), oracle.count(c["reads"][:b]))
    finally:
        eng.close()


def _rows_of(counter):
    return ([len(k) for k in counter], list(counter.values()),
            [int(x) for k in counter for x in k.packed[:(len(k) + 31) // 32]])


def _one_length_reads(L, seed, n_contents=41):
    rng = np.random.default_rng(seed)
    cyc = _Cycle()
    contents = [hostile(L, rng, cyc) for _ in range(n_contents)]
    return contents, [contents[i] for i in rng.integers(0, n_contents, 16 * n_contents)] + contents


@pytest.mark.gpu
@pytest.mark.parametrize("L", [20, 40, 100, 500])
def test_counter_dense_list_hostile(gpu, oracle, L):
    """ShortSeqCounter(list, device="cuda") of one-length (b) reads (the engine's dense chunk) == oracle.count."""
    from shortseq_amd import ShortSeqCounter
    contents, reads = _one_length_reads(L, 300 + L)
    assert {b for r in contents for b in r} >= set(ACCEPTED)
    assert _rows_of(ShortSeqCounter(reads, device="cuda")) == expected_rows(oracle.count(reads))


# ------------------------------------------------------------------------------------------------
# GPU: the first rejected read
# ------------------------------------------------------------------------------------------------
def _bad_batch(lengths, L_bad, pos, byte, at, seed, n=48, bad_read=None):
    """n (b) reads of `lengths` in turn; read `at` is a (c) read (an L_bad-nt (b) read with `byte` at
    `pos`; or `bad_read`), and a second rejected read follows later as a decoy."""
    rng = np.random.default_rng(seed)
    cyc = _Cycle()
    reads = [hostile(lengths[i % len(lengths)], rng, cyc) for i in range(n)]
    reads[at] = bad_read if bad_read is not None else rejected(hostile(L_bad, rng, cyc), pos, byte)
    d = at + 1 + int(rng.integers(0, n - at - 1))
    Ld = len(reads[d]) or L_bad
    reads[d] = rejected(hostile(Ld, rng, cyc), int(rng.integers(0, Ld)), ord("N"))
    return reads


# path -> (the lengths around the bad read, the bad read's length)
BAD_PATHS = {
    "short": ([5, 17, 31, 1, 24], 29),
    "len32": ([32, 7, 32, 19], 32),
    "rows4": ([40, 64, 65, 96, 77], 83),
    "classes": ([12, 150, 333, 64, 480, 200], 301),
    "class_long": ([500, 90, 1024, 20, 700], 777),
}


def _position_cases(L):
    pos = positions(L)
    return [(p, GAP_BYTES[k % len(GAP_BYTES)]) for k, p in enumerate(pos)]


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(BAD_PATHS))
def test_ingest_first_bad_positions(gpu, oracle, path):
    """A (c) read among (b) reads, its byte at every position of the set (first, last, chunk and word
    edges), at read index 0 and further in, and a 1025-nt read; a later bad read as decoy.  One engine,
    reset() between the cases; the raised type, message and .read_index are the oracle's."""
    import shortseq_amd.batch as B
    lengths, L_bad = BAD_PATHS[path]
    cases = [(p, b, 0 if k == 0 else 1 + (5 * k) % 40, None) for k, (p, b) in enumerate(_position_cases(L_bad))]
    cases.append((0, 0, 9, hostile_long()))
    eng = B.DeviceIngest(gpu)
    try:
        for k, (pos, byte, at, bad_read) in enumerate(cases):
            reads = _bad_batch(lengths, L_bad, pos, byte, at, 500 + k, bad_read=bad_read)
            want = expected_error(oracle, reads)
            assert want[2] == at
            with pytest.raises(Exception) as ei:
                eng.count(*_dev_reads(gpu, reads, k))
            check_raised(ei, want)
            eng.reset()
        # and the engine still counts a clean batch of the same shape
        reads = [r for r in _bad_batch(lengths, L_bad, 0, ord("N"), 0, 1)[1:]
                 if oracle.encode_one(r)[1].kind == 0]
        eng.count(*_dev_reads(gpu, reads, 1))
        _assert_rows(eng.results(), oracle.count(reads))
    finally:
        eng.close()


def hostile_long():
    return hostile(1025, np.random.default_rng(1025), _Cycle())


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(BAD_PATHS))
def test_ingest_first_bad_values(gpu, oracle, path):
    """The near-misses (an accepted value with one of its low six bits flipped) and the FASTQ bytes as
    the rejected byte, the position cycling through the set."""
    import shortseq_amd.batch as B
    lengths, L_bad = BAD_PATHS[path]
    pos = positions(L_bad)
    eng = B.DeviceIngest(gpu)
    try:
        for k, byte in enumerate(NEAR_MISSES + FASTQ_BYTES):
            reads = _bad_batch(lengths, L_bad, pos[k % len(pos)], byte, 1 + k % 30, 900 + k)
            want = expected_error(oracle, reads)
            with pytest.raises(Exception) as ei:
                eng.count(*_dev_reads(gpu, reads, k))
            check_raised(ei, want)
            eng.reset()
    finally:
        eng.close()


@pytest.mark.gpu
def test_ingest_first_bad_across_groups(gpu, oracle):
    """One batch of short, 32-nt and class reads; the earlier bad read in one group and the later in
    another, every ordered pair: the earlier wins."""
    import shortseq_amd.batch as B
    groups = {"short": 23, "len32": 32, "class": 130}
    rng = np.random.default_rng(6)
    eng = B.DeviceIngest(gpu)
    try:
        k = 0
        for ga, La in groups.items():
            for gb, Lb in groups.items():
                if ga == gb:
                    continue
                cyc = _Cycle()
                reads = [hostile((23, 32, 130, 9, 70)[i % 5], rng, cyc) for i in range(60)]
                reads[14 + k] = rejected(hostile(La, rng, cyc), positions(La)[k % 4], ord("N"))
                reads[31 + k] = rejected(hostile(Lb, rng, cyc), Lb - 1, ord("@"))
                want = expected_error(oracle, reads)
                assert want[2] == 14 + k
                with pytest.raises(Exception) as ei:
                    eng.count(*_dev_reads(gpu, reads, k))
                check_raised(ei, want)
                eng.reset()
                k += 1
        # a rejected byte before a too-long read and behind one, in each group
        for k, (g, Lg) in enumerate(groups.items()):
            for first_long in (False, True):
                cyc = _Cycle()
                reads = [hostile((23, 32, 130, 9, 70)[i % 5], rng, cyc) for i in range(60)]
                bad = rejected(hostile(Lg, rng, cyc), positions(Lg)[k], ord("~"))
                reads[20 + k], reads[40 + k] = (hostile_long(), bad) if first_long else (bad, hostile_long())
                want = expected_error(oracle, reads)
                assert want[2] == 20 + k and (want[1] == TOO_LONG) == first_long
                with pytest.raises(Exception) as ei:
                    eng.count(*_dev_reads(gpu, reads, k))
                check_raised(ei, want)
                eng.reset()
    finally:
        eng.close()


@pytest.mark.gpu
def test_ingest_first_bad_speculative_rows(gpu, oracle):
    """The rejected read in a chunk whose row encode was queued ahead of its length split: in the
    second chunk at one stride (gated behind the split) and in the fourth (on the side stream).  The
    index is the global one, and after reset() the engine counts the clean chunks exactly."""
    import shortseq_amd.batch as B
    c = get_corpus("rows4")
    n = len(c["reads"])
    q = n // 4
    eng = B.DeviceIngest(gpu)
    try:
        for bad_chunk in (1, 3):
            reads = list(c["reads"])
            at = bad_chunk * q + 37
            reads[at] = rejected(reads[at], len(reads[at]) - 1, ord("I"))
            reads[at + 50] = rejected(reads[at + 50], 0, ord("N"))
            dev = _dev_reads(gpu, reads, bad_chunk)
            for k in range(bad_chunk):
                eng.count(dev[0], dev[1][k * q:(k + 1) * q], dev[2][k * q:(k + 1) * q])
            want = expected_error(oracle, reads[:(bad_chunk + 1) * q])
            assert want[2] == at
            with pytest.raises(Exception) as ei:
                eng.count(dev[0], dev[1][bad_chunk * q:(bad_chunk + 1) * q], dev[2][bad_chunk * q:(bad_chunk + 1) * q])
            check_raised(ei, want)
            eng.reset()
        dev = _dev(gpu, c)
        eng.count(dev[0], dev[1][:q], dev[2][:q])
        _assert_rows(eng.results(), oracle.count(c["reads"][:q]))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [20, 40, 100, 500])
def test_counter_dense_list_first_bad(gpu, oracle, L):
    """The dense list path: a (c) read at each position of the set, a decoy behind it."""
    from shortseq_amd import ShortSeqCounter
    for k, (pos, byte) in enumerate(_position_cases(L)):
        reads = _bad_batch([L], L, pos, byte, (2 + 3 * k) % 60, 700 + k, n=64)
        want = expected_error(oracle, reads)
        with pytest.raises(Exception) as ei:
            ShortSeqCounter(reads, device="cuda")
        check_raised(ei, want, index_required=False)


@pytest.mark.gpu
def test_encode_var_first_bad_positions(gpu, oracle):
    """encode_var: the (c) read's byte at every position of the set for a short, a rows-sized, a class
    and a long read, and a 1025-nt read."""
    import shortseq_amd.batch as B
    k = 0
    for L_bad in (29, 32, 83, 301, 777):
        for pos, byte in _position_cases(L_bad):
            reads = _bad_batch([5, 32, 150, 64, 480, 33, 700], L_bad, pos, byte, 0 if k % 7 == 0 else 1 + k % 40, 40 + k)
            want = expected_error(oracle, reads)
            with pytest.raises(Exception) as ei:
                B.encode_var(*_dev_reads(gpu, reads, k))
            check_raised(ei, want)
            k += 1
    reads = _bad_batch([5, 32, 150], 0, 0, 0, 11, 1, bad_read=hostile_long())
    want = expected_error(oracle, reads)
    assert want[:3] == (Exception, TOO_LONG, 11)
    with pytest.raises(Exception) as ei:
        B.encode_var(*_dev_reads(gpu, reads, 1))
    check_raised(ei, want)
    assert ei.value.read_index == 11


@pytest.mark.gpu
def test_encode_var_first_bad_all_values(gpu, oracle):
    """encode_var: each of the 240 rejected values, one launch each on a tiny batch."""
    import shortseq_amd.batch as B
    for k, byte in enumerate(REJECTED):
        L_bad = (29, 32, 83, 161)[k % 4]
        pos = positions(L_bad)
        reads = _bad_batch([5, 32, 150, 64], L_bad, pos[k % len(pos)], byte, k % 12, 2000 + k, n=16)
        want = expected_error(oracle, reads)
        with pytest.raises(Exception) as ei:
            B.encode_var(*_dev_reads(gpu, reads, k))
        check_raised(ei, want)


@pytest.mark.gpu
def test_encode_fixed_first_bad_all_values(gpu, oracle):
    """The fixed-length encode: each of the 240 rejected values, one launch each on a tiny batch
    (lengths on the 16-byte fast path and on the general one)."""
    import torch
    import shortseq_amd.batch as B
    for k, byte in enumerate(REJECTED):
        L = (1, 16, 31, 32, 33, 48, 96, 100)[k % 8]
        pos = positions(L)
        reads = _bad_batch([L], L, pos[k % len(pos)], byte, k % 12, 3000 + k, n=16)
        want = expected_error(oracle, reads)
        t = torch.frombuffer(bytearray(b"".join(reads)), dtype=torch.uint8).to(gpu).view(16, L)
        with pytest.raises(Exception) as ei:
            B.encode(t, L)
        check_raised(ei, want)


# ------------------------------------------------------------------------------------------------
# GPU: the fixed-length kernels on accepted bytes and hostile stride padding
# ------------------------------------------------------------------------------------------------
FIXED_L = (1, 16, 31, 32, 33, 48, 96, 100, 512)
FIXED_N = 777


@functools.lru_cache(maxsize=None)
def _fixed_rows(L):
    """FIXED_N (b) reads of length L (61 contents, drawn with repeats) -> (reads, [n, L] u8)."""
    rng = np.random.default_rng(4000 + L)
    cyc = _Cycle()
    contents = [hostile(L, rng, cyc) for _ in range(61)]
    if L == 1:
        contents = [bytes([b]) for b in ACCEPTED]
    reads = [contents[i] for i in rng.integers(0, len(contents), FIXED_N)]
    return reads, np.frombuffer(b"".join(reads), np.uint8).reshape(FIXED_N, L)


def _padded(rows, stride, seed):
    """[n, stride] u8: the rows with rejected bytes in the padding columns."""
    rng = np.random.default_rng(seed)
    n, L = rows.shape
    gap = np.array(GAP_BYTES, np.uint8)
    a = gap[rng.integers(0, len(gap), (n, stride))]
    a[:, :L] = rows
    return np.ascontiguousarray(a)


def _check_fixed(gpu, oracle, L, stride):
    import torch
    import shortseq_amd.batch as B
    reads, rows = _fixed_rows(L)
    n = FIXED_N
    assert L < 16 or {b for r in reads for b in r} >= set(ACCEPTED)
    a = rows if stride == L else _padded(rows, stride, L * 131 + stride)
    exp, rc, _e = oracle.encode_batch(np.ascontiguousarray(rows).reshape(-1), n, L)
    assert rc == 0
    t = torch.from_numpy(a.copy()).to(gpu)
    got = B.encode(t, L) if stride == L else B.encode(t.reshape(-1), L, stride=stride)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), exp)
    ref = exp[5]
    words, dist = B.encode_hamming_ref(t, L, torch.from_numpy(ref.view(np.int64).copy()))
    assert np.array_equal(words.cpu().numpy().view(np.uint64), exp)
    assert np.array_equal(dist.cpu().numpy().astype(np.uint32), oracle.hamming_ref_batch(exp, n, L, ref))
    cexp = oracle.count(reads)
    ctr = B.GpuCounter(1 << 10, device=gpu)
    try:
        ctr.insert(t, L)
        if L <= 32:
            k, cnt, first = ctr.items_sorted()
            assert [int(x) for x in k] == [w[0] for (w, _L, _c, _f) in cexp]
        else:
            k, cnt, first = ctr.items_sorted_words()
            assert [tuple(int(x) for x in row) for row in k] == [w for (w, _L, _c, _f) in cexp]
        assert [int(x) for x in cnt] == [c for (_w, _L, c, _f) in cexp]
        assert [int(x) for x in first] == [f for (_w, _L, _c, f) in cexp]
    finally:
        ctr.close()
    return a, exp


@pytest.mark.gpu
@pytest.mark.parametrize("L", FIXED_L)
def test_fixed_accepted_bytes(gpu, oracle, L):
    """B.encode, B.encode_hamming_ref and GpuCounter.insert on (b) reads holding all 16 accepted
    values: every row == the oracle's."""
    _check_fixed(gpu, oracle, L, L)


@pytest.mark.gpu
@pytest.mark.parametrize("L", FIXED_L)
def test_fixed_hostile_stride_padding(gpu, oracle, L):
    """The same calls, and HostStager.encode on a padded view, with stride L + 3 and L + 16 and the
    padding filled with rejected bytes: the results equal the oracle's and nothing raises."""
    import shortseq_amd.batch as B
    st = B.HostStager(gpu, chunk_bytes=1 << 16, nslots=3, copy_threads=2)
    try:
        for stride in (L + 3, L + 16):
            a, exp = _check_fixed(gpu, oracle, L, stride)
            assert np.array_equal(st.encode(a[:, :L]), exp), stride
    finally:
        st.close()
