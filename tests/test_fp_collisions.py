"""Distinct keys that share a 64-bit fingerprint, through every multi-word path of the counter.

Keys longer than 32 nt are counted under words_fp (csrc/ss_device.h); equality is decided on the words,
so every word comparison behind an equal fingerprint has to work: the aggregate's three phases, the
merge's find / claim, the verify kernels that raise the class flag, the folds that keep a new key apart
from a resident one, and the exact recount after a raised flag.  Random reads never collide in 64 bits;
fp_collide.py builds rows that do (same width, a partly used last word, two length classes, the clamp
of ~0) and these tests feed them as reads and rows.

The CPU tests check the constructions; the GPU tests compare counts and first indices exactly with a
dict over the same reads (or oracle.count), and pin the Python restatement of words_fp to the
fingerprints the device stored (extract_words' fps) -- without that pin a family that did not collide
on the device would pass everything.
"""
import collections
import functools
import random

import numpy as np
import pytest

import fp_collide as fc

REPS = (3, 5, 7, 11)          # occurrences of a family's four rows: any merge of two changes a count
K = len(REPS)
ASCII_L = (64, 96, 128, 160, 224, 256, 1024)      # W = 2 3 4 5 7 8 32
ENGINE_L = (64, 96, 128, 160)                     # one family per read-order row stride
MAX_DRAWS = 100_000


# ---- the rows under test (fixed seeds: the CPU tests check the very rows the GPU tests feed) ------

def _family(row, L, j, seed):
    W = (L + 31) // 32
    keep = fc.unused_bits(L) if (L % 32 and j + 1 == W - 1) else 0
    return fc.family(row, j, K, random.Random(seed), keep_zero=keep, max_draws=MAX_DRAWS)


@functools.lru_cache(maxsize=None)
def key_family(L):
    """K colliding GpuCounter keys of L nt (W words, seed(W)); the last two words differ -> (rows, draws)."""
    rng = random.Random(1000 + L)
    return _family(fc.rand_words(rng, L), L, (L + 31) // 32 - 2, 3000 + L)


@functools.lru_cache(maxsize=None)
def class_family(L):
    """K colliding class rows of L nt (W words and the length, seed(W + 1)); the first two words differ."""
    rng = random.Random(2000 + L)
    return _family(fc.class_row(fc.rand_words(rng, L), L), L, 0, 4000 + L)


@functools.lru_cache(maxsize=None)
def cross_pair():
    return fc.cross_class_pair(random.Random(77))


@functools.lru_cache(maxsize=None)
def clamp_keys():
    return fc.clamp_pair(random.Random(78))


@functools.lru_cache(maxsize=None)
def clamp_class_rows():
    return fc.clamp_pair(random.Random(79), (64,))


def _read_of_class_row(r):
    return fc.to_read(r[:-1], r[-1])


# ---- CPU: the algebra and the constructions ----------------------------------------------------

def test_fp_inverses():
    rng = random.Random(1)
    assert (fc.M1 * fc.M1_INV) & fc.MASK == 1 and (fc.M2 * fc.M2_INV) & fc.MASK == 1
    for x in [0, 1, fc.MASK, fc.CLAMPED, 1 << 63] + [fc.rand_word(rng) for _ in range(200)]:
        assert fc.f_inv(fc.f(x)) == x and fc.f(fc.f_inv(x)) == x
        assert fc.final_inv(fc.final_raw(x)) == x and fc.final_raw(fc.final_inv(x)) == x
    assert fc.fp_final(fc.final_inv(fc.EMPTY)) == fc.CLAMPED      # the clamp: never the free-slot value
    assert fc.fp((1, 2)) != fc.fp((1, 2, 0))                       # the width is in the seed


def _check_reads(oracle, rows, Ls, with_length):
    """The rows are pairwise different, and each decodes to a read of its length that encodes back to
    its words under the oracle and under the host codec."""
    import shortseq_amd as sq
    assert len(set(rows)) == len(rows)
    for r, L in zip(rows, Ls):
        W = (L + 31) // 32
        words = r[:-1] if with_length else r
        assert len(words) == W and (not with_length or r[-1] == L)
        read = fc.to_read(words, L)
        assert len(read) == L and set(read) <= set(b"ACGT")
        ow, err = oracle.encode_one(read, W)
        assert err.kind == 0 and tuple(int(x) for x in ow) == tuple(words)
        assert tuple(sq.pack(read).packed) == tuple(words)
    assert len({fc.to_read(r[:-1] if with_length else r, L) for r, L in zip(rows, Ls)}) == len(rows)


@pytest.mark.parametrize("L", ASCII_L)
def test_same_width_key_family(oracle, L):
    rows, _ = key_family(L)
    assert len(rows) == K and len({fc.fp(r) for r in rows}) == 1
    _check_reads(oracle, rows, [L] * K, False)


@pytest.mark.parametrize("L", ENGINE_L + (224,))
def test_same_width_class_family(oracle, L):
    rows, _ = class_family(L)
    assert len(rows) == K and len({fc.fp(r) for r in rows}) == 1
    assert fc.fp(rows[0]) != fc.fp(rows[0][:-1])      # the length word and the wider seed are hashed
    _check_reads(oracle, rows, [L] * K, True)


@pytest.mark.parametrize("with_length", [False, True])
def test_partial_last_word_family(oracle, with_length):
    """L = 60: the second word uses 56 bits (asked of the host codec), so the difference xored into it
    must be clear in the other 8 -- one draw in 256."""
    unused = fc.unused_bits(60)
    assert bin(unused).count("1") == 8
    rows, draws = (class_family if with_length else key_family)(60)
    assert draws < MAX_DRAWS
    assert len(rows) == K and len({fc.fp(r) for r in rows}) == 1
    assert all(r[1] & unused == 0 for r in rows)
    _check_reads(oracle, rows, [60] * K, with_length)


def test_cross_class_pair(oracle):
    a, b = cross_pair()
    assert len(a) == 3 and len(b) == 4 and a[-1] == 64 and b[-1] == 96
    assert fc.seed(3) != fc.seed(4) and fc.fp(a) == fc.fp(b)
    _check_reads(oracle, [a, b], [64, 96], True)


@pytest.mark.parametrize("with_length", [False, True])
def test_clamp_pair(oracle, with_length):
    p, q = clamp_class_rows() if with_length else clamp_keys()
    assert fc.final_raw(fc.state(p)) == fc.EMPTY and fc.final_raw(fc.state(q)) == fc.CLAMPED
    assert fc.fp(p) == fc.fp(q) == fc.CLAMPED
    _check_reads(oracle, [p, q], [64, 64], with_length)


# ---- GPU: GpuCounter ----------------------------------------------------------------------------

def _plan(n, cuts, fixed, extras, rng):
    """index -> family member: `fixed` as given, then extras = [(member, segment, count)] at free
    interior indices of cuts[segment] .. cuts[segment + 1]."""
    place = dict(fixed)
    for k, s, cnt in extras:
        lo, hi = cuts[s], cuts[s + 1]
        free = [i for i in rng.sample(range(lo + 1, hi - 1), cnt + len(place)) if i not in place][:cnt]
        for i in free:
            place[i] = k
    got = collections.Counter(place.values())
    assert [got[k] for k in range(K)] == list(REPS)
    return place


def _plan_one(n, rng):
    """The whole family in one insert: index 0, the last index, the rest inside."""
    return [0, n], _plan(n, [0, n], {0: 0, n - 1: 3}, [(0, 0, 2), (1, 0, 5), (2, 0, 7), (3, 0, 10)], rng)


def _plan_split(n, rng):
    """Three inserts: A; then B and C; then all four.  Members at index 0, at the last index and on
    both sides of both insert boundaries."""
    c1, c2 = n // 3 + 1, 2 * n // 3 + 3           # (odd segment sizes)
    fixed = {0: 0, c1 - 1: 0, c1: 1, c2 - 1: 2, c2: 3, n - 1: 0}
    extras = [(1, 1, 1), (2, 1, 2), (1, 2, 3), (2, 2, 4), (3, 2, 10)]
    return [0, c1, c2, n], _plan(n, [0, c1, c2, n], fixed, extras, rng)


def _reference(rows_u64):
    """bytes of a row's words -> (count, first index): the plain dict the table must equal."""
    ref = {}
    for i in range(rows_u64.shape[0]):
        kb = rows_u64[i].tobytes()
        c = ref.get(kb)
        ref[kb] = (1, i) if c is None else (c[0] + 1, c[1])
    return ref


def _row_bytes(r):
    return np.array(r, dtype=np.uint64).tobytes()


def _check_table(c, ref, families, n_parts=1):
    """The table's entries == ref exactly; every stored fingerprint == the Python fp of its words; each
    family's rows are separate entries under one fingerprint, in one owner part."""
    fps, _lens, words, counts, first, parts = c.extract_words(n_parts)
    assert not c.overflowed()
    pc = [int(x) for x in parts.cpu().tolist()]
    m = sum(pc)
    w = words[:m].cpu().numpy().view(np.uint64)
    f = fps[:m].cpu().numpy().view(np.uint64)
    cn, fi = counts[:m].cpu().tolist(), first[:m].cpu().tolist()
    got = {w[i].tobytes(): (int(cn[i]), int(fi[i])) for i in range(m)}
    assert len(got) == m                                   # no key twice
    assert got == ref
    assert c.size() == len(ref)
    for i in range(m):                                     # the pin: device fingerprints == fc.fp
        assert int(f[i]) == fc.fp(tuple(int(x) for x in w[i])), i
    at = {w[i].tobytes(): i for i in range(m)}
    bounds = np.cumsum([0] + pc)
    for fam in families:
        idx = [at[_row_bytes(r)] for r in fam]             # (KeyError: a member is missing)
        assert len(set(idx)) == len(fam)
        assert {int(f[i]) for i in idx} == {fc.fp(fam[0])}
        assert len({int(np.searchsorted(bounds, i, side="right")) for i in idx}) == 1


_ASCII_CAP = {64: 1 << 12, 96: 1 << 13, 128: 1 << 14, 160: 1 << 12, 224: 1 << 13, 256: 1 << 14, 1024: 1 << 12}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["one", "split", "reset"])
@pytest.mark.parametrize("L", ASCII_L)
def test_counter_ascii_colliders(gpu, oracle, L, mode):
    """GpuCounter.insert of L-nt reads holding four keys of one fingerprint among 20 000 pool reads:
    one insert (one region, one LDS table: phase 1 compares rows behind an equal tag, phase 2b claims
    two slots under one key); three inserts (phase 2a probes past a resident slot of the same
    fingerprint and other words); the same after a prefilled table's reset()."""
    import torch
    import shortseq_amd.batch as B
    n, U = 20_000, 2_000
    fam, _ = key_family(L)
    cuts, place = (_plan_one if mode == "one" else _plan_split)(n, random.Random(L))
    ascii = B.synth_pool_reads(n, L, 500 + L, 600 + L, U, device=gpu)
    idx = sorted(place)
    col = np.frombuffer(b"".join(fc.to_read(fam[place[i]], L) for i in idx), dtype=np.uint8).reshape(-1, L)
    ascii[torch.tensor(idx, device=gpu)] = torch.from_numpy(col.copy()).to(gpu)
    words, rc, _err = oracle.encode_batch(ascii.cpu().numpy().reshape(-1), n, L)
    assert rc == 0
    ref = _reference(words)
    assert [ref[_row_bytes(r)][0] for r in fam] == list(REPS)
    c = B.GpuCounter(_ASCII_CAP[L], device=gpu)
    try:
        if mode == "reset":
            c.insert(ascii[: n // 2], L)
            c.reset()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            c.insert(ascii[lo:hi], L, base_index=lo)
        assert c.words == (L + 31) // 32
        _check_table(c, ref, [fam])
    finally:
        c.close()


def _dev_rows(gpu, a, shift):
    """Rows on the device, 16-B aligned (shift 0) or 8 B off (shift 1)."""
    import torch
    buf = torch.zeros(a.size + 2, dtype=torch.int64, device=gpu)
    v = buf[shift:shift + a.size].view(-1, a.shape[1])
    v.copy_(torch.from_numpy(a.view(np.int64)))
    assert v.data_ptr() % 16 == 8 * shift
    return v


def _word_pool(W, U, n, seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 64, size=(U, W), dtype=np.uint64)
    return pool, pool[rng.integers(0, U, size=n)]


def _word_family(W, seed):
    rng = random.Random(seed)
    return fc.family([fc.rand_word(rng) for _ in range(W)], W - 2, K, rng)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("W,shift", [(2, 0), (2, 1), (3, 0), (4, 0), (4, 1), (6, 0), (6, 1), (7, 0), (8, 0)])
def test_counter_insert_words_colliders(gpu, W, shift):
    """insert_words over three inserts (A; B, C; all four): the dwordx4 row gathers of every width, the
    even widths both 16-B aligned (EVEN) and 8 B off (the realigning form), W = 8 the any-width form."""
    import shortseq_amd.batch as B
    n, U = 20_000, 2_000
    fam = _word_family(W, 50 + W)
    cuts, place = _plan_split(n, random.Random(W * 2 + shift))
    _pool, rows = _word_pool(W, U, n, 60 + W)
    for i, k in place.items():
        rows[i] = np.array(fam[k], dtype=np.uint64)
    ref = _reference(rows)
    assert [ref[_row_bytes(r)][0] for r in fam] == list(REPS)
    c = B.GpuCounter(1 << (12 + W % 3), device=gpu)
    try:
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            c.insert_words(_dev_rows(gpu, rows[lo:hi], shift), base_index=lo)
        assert c.words == W and c.length == -2
        _check_table(c, ref, [fam])
    finally:
        c.close()


@pytest.mark.gpu
def test_counter_merge_words_colliders(gpu):
    """One merge_words call with entries that collide with resident keys but are other keys, entries
    that are resident keys, and two new entries that collide with each other; extract_words by owner
    (1 and 3 parts: a family lands in one part); then the table's growth path -- every entry merged
    into a fresh table of another capacity, and once more onto itself (every entry now has to find its
    own slot among residents of its fingerprint)."""
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd._native import check, lib
    W, n, U = 3, 20_000, 2_000
    f1, f2, f3 = (_word_family(W, s) for s in (91, 92, 93))
    pool, rows = _word_pool(W, U, n, 94)
    for i, r in ((0, f1[0]), (1, f1[1]), (n - 1, f1[0]), (7, f2[0])):         # residents: f1 A B, f2 A
        rows[i] = np.array(r, dtype=np.uint64)
    ref = _reference(rows)
    t = B.GpuCounter(1 << 12, device=gpu)
    t2 = B.GpuCounter(1 << 14, device=gpu)
    try:
        t.insert_words(_dev_rows(gpu, rows, 0))
        fresh = np.random.default_rng(95).integers(0, 1 << 64, size=(50, W), dtype=np.uint64)
        ent = ([(f1[2], 7, 40), (f1[0], 11, 5), (f1[3], 13, 41),          # new; resident (first stays 0); new
                (f2[1], 17, 3), (f2[0], 19, 2),                           # new beside resident f2 A; resident
                (f3[0], 23, 9), (f3[1], 29, 8), (f3[2], 31, 6)]           # new, colliding with each other
               + [(tuple(int(x) for x in pool[i]), 2 + i, 100 + i) for i in range(0, 300, 3)]
               + [(tuple(int(x) for x in r), 37, 50_000 + i) for i, r in enumerate(fresh)])
        assert len({w for (w, _c, _f) in ent}) == len(ent)                # merge_words takes distinct keys
        random.Random(96).shuffle(ent)
        for (w, cnt, fi) in ent:
            oc, of = ref.get(_row_bytes(w), (0, fi))
            ref[_row_bytes(w)] = (oc + cnt, min(of, fi))

        def merge(dst, entries):
            ww = np.array([w for (w, _c, _f) in entries], dtype=np.uint64).view(np.int64).reshape(len(entries), W)
            dst.merge_words(torch.from_numpy(ww).to(gpu),
                            torch.tensor([cc for (_w, cc, _f) in entries], dtype=torch.int64, device=gpu),
                            torch.tensor([ff for (_w, _c, ff) in entries], dtype=torch.int64, device=gpu))

        merge(t, ent)
        fams = [f1, f2[:2], f3[:3]]
        for n_parts in (1, 3):
            _check_table(t, ref, fams, n_parts)
        # growth: the whole table as entries into an empty table of another capacity
        _fps, _lens, words, counts, first, parts = t.extract_words(1)
        m = int(parts.sum().item())
        check(lib().ss_counter_set_words(t2._h, W), "ss_counter_set_words")
        t2.merge_words(words[:m].contiguous(), counts[:m].contiguous(), first[:m].contiguous())
        for n_parts in (1, 3):
            _check_table(t2, ref, fams, n_parts)
        t2.merge_words(words[:m].contiguous(), counts[:m].contiguous(), first[:m].contiguous())
        _check_table(t2, {k: (2 * c, f) for k, (c, f) in ref.items()}, fams, 3)
    finally:
        t.close()
        t2.close()


@pytest.mark.gpu
def test_counter_clamp_pair(gpu, oracle):
    """Two 64-nt reads whose fingerprints before the clamp are ~0 (the free-slot value) and ~1: both are
    kept, both under ~1, and size() counts both."""
    import torch
    import shortseq_amd.batch as B
    L, n, U = 64, 20_000, 2_000
    p, q = clamp_keys()
    ascii = B.synth_pool_reads(n, L, 7, 8, U, device=gpu)
    place = {0: p, 5: q, 6: q, n // 2: p, n // 2 + 1: q, n - 1: p}
    idx = sorted(place)
    col = np.frombuffer(b"".join(fc.to_read(place[i], L) for i in idx), dtype=np.uint8).reshape(-1, L)
    ascii[torch.tensor(idx, device=gpu)] = torch.from_numpy(col.copy()).to(gpu)
    words, rc, _err = oracle.encode_batch(ascii.cpu().numpy().reshape(-1), n, L)
    assert rc == 0
    ref = _reference(words)
    assert ref[_row_bytes(p)] == (3, 0) and ref[_row_bytes(q)] == (3, 5)
    c = B.GpuCounter(1 << 12, device=gpu)
    try:
        c.insert(ascii[: n // 2 + 1], L)
        c.insert(ascii[n // 2 + 1:], L, base_index=n // 2 + 1)
        assert fc.fp(p) == fc.fp(q) == fc.CLAMPED
        _check_table(c, ref, [[p, q]])
    finally:
        c.close()


# ---- GPU: the drop-in engine ----------------------------------------------------------------------

PATHS = ("rows", "cls_rep", "cls_wide")
# rows:     every read 33-160 nt: read-order rows (k_flat_verify, k_flat_fold_find)
# cls_rep:  reads of <= 32 nt beside them: class-ordered rows of <= 6 words (k_cls_verify_rep, k_cls_fold_find)
# cls_wide: reads past 160 nt as well, a family at 224 nt: rows of 8 words (k_cls_verify)


def _engine_families(path):
    """[(rows, reps)]: a family per row stride, the 60-nt family (a partly used word), the clamp pair."""
    fams = [(class_family(L)[0], REPS) for L in ENGINE_L + (60,)]
    fams.append((list(clamp_class_rows()), (3, 5)))
    if path == "cls_wide":
        fams.append((class_family(224)[0], REPS))
    return fams


@pytest.fixture(scope="module")
def pinned(gpu):
    """The engine hashes a class row (words, length) with the same words_fp as insert_words does: every
    class row fed below goes through a packed-word table of its width once, and the stored fingerprints
    must equal fc.fp and be shared inside each family (and across the cross-class pair)."""
    import shortseq_amd.batch as B
    fams = [f for (f, _r) in _engine_families("cls_wide")]
    a, b = cross_pair()
    by_w = collections.defaultdict(list)
    for fam in fams + [[a], [b]]:
        by_w[len(fam[0])].append(fam)
    stored = {}
    for W1, group in sorted(by_w.items()):
        rows = np.concatenate([np.array([r for fam in group for r in fam], dtype=np.uint64),
                               _word_pool(W1, 500, 2_000, W1)[1]])
        ref = _reference(rows)
        c = B.GpuCounter(1 << 12, device=gpu)
        try:
            c.insert_words(_dev_rows(gpu, rows, 0))
            _check_table(c, ref, group)
            fps, _l, words, _c, _f, parts = c.extract_words(1)
            m = int(parts.sum().item())
            for w, f in zip(words[:m].cpu().numpy().view(np.uint64), fps[:m].cpu().numpy().view(np.uint64)):
                stored[tuple(int(x) for x in w)] = int(f)
        finally:
            c.close()
    assert stored[a] == stored[b] == fc.fp(a)
    return stored


def _background(rng, path, k=400):
    if path == "rows":
        lens = [rng.randint(33, 160) for _ in range(k)] + [33, 64, 65, 96, 97, 128, 129, 160]
    elif path == "cls_rep":
        lens = [rng.randint(1, 160) for _ in range(k)] + [1, 31, 32, 33, 64, 160]
    else:
        lens = [rng.randint(1, 300) for _ in range(k)] + [1, 32, 33, 160, 161, 224, 225, 300]
    return [bytes(rng.choice(b"ACGT") for _ in range(L)) for L in lens]


def _chunk(rng, pool, n, inject):
    """n reads drawn from the pool, with inject = [(read, times)] at index 0, at the last index and at
    random indices between."""
    reads = [pool[i] for i in rng.choices(range(len(pool)), k=n)]
    todo = [r for (r, t) in inject for _ in range(t)]
    rng.shuffle(todo)
    if todo:
        spots = [0, n - 1] + rng.sample(range(1, n - 1), max(0, len(todo) - 2))
        for i, r in zip(spots, todo):
            reads[i] = r
    return reads


def _device(gpu, reads):
    import torch
    lens = torch.tensor([len(r) for r in reads], dtype=torch.int32)
    offs = torch.zeros(len(reads), dtype=torch.int64)
    offs[1:] = torch.cumsum(lens.to(torch.int64), 0)[:-1]
    blob = torch.frombuffer(bytearray(b"".join(reads) + b"\0" * 16), dtype=torch.uint8)
    return blob.to(gpu), offs.to(gpu), lens.to(gpu)


def _assert_results(eng, oracle, reads, times=1):
    exp = oracle.count(reads)
    for _ in range(times):
        gl, gc, gw = eng.results()
        assert gl.tolist() == [L for (_w, L, _c, _f) in exp]
        assert gc.tolist() == [c for (_w, _L, c, _f) in exp]
        assert gw.tolist() == [int(x) for (w, L, _c, _f) in exp for x in w[:(L + 31) // 32]]
    return exp


def _members(fams, pick):
    """[(read, times)] of the members `pick(k)` lets through."""
    return [(_read_of_class_row(r), reps[k]) for (rows, reps) in fams for k, r in enumerate(rows) if pick(k)]


def _chunks_for(pattern, path, seed):
    """The chunks of a pattern, 24 000 reads in all.
    first:  one chunk holding every family whole.
    later:  a collision-free chunk (member A of every family, resident afterwards), then every family whole.
    across: A and never B; B and never A; then both with the rest -- no chunk of the first two holds a
            collision, so only the fold's word compare keeps B apart from the resident A."""
    rng = random.Random(seed)
    pool = _background(rng, path)
    fams = _engine_families(path)
    if pattern == "first":
        return [_chunk(rng, pool, 24_000, _members(fams, lambda k: True))]
    if pattern == "later":
        return [_chunk(rng, pool, 12_000, _members(fams, lambda k: k == 0)),
                _chunk(rng, pool, 12_000, _members(fams, lambda k: True))]
    return [_chunk(rng, pool, 8_000, _members(fams, lambda k: k == 0)),
            _chunk(rng, pool, 8_000, _members(fams, lambda k: k == 1)),
            _chunk(rng, pool, 8_000, _members(fams, lambda k: True))]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["first", "later", "across"])
@pytest.mark.parametrize("path", PATHS)
def test_ingest_colliders(gpu, oracle, pinned, path, pattern):
    """DeviceIngest (default sizing: the fingerprint path) over chunks holding colliding reads ==
    oracle.count of all reads so far, after every chunk (twice after the first: a first read-order chunk
    defers its fold and queues the speculative finish, which a raised flag must drop).  A chunk holding
    a whole family must raise the class flag in its verify kernel and recount exactly, into class tables
    that may already hold members; a chunk holding one member beside a resident one must keep them apart
    in the fold."""
    import shortseq_amd.batch as B
    chunks = _chunks_for(pattern, path, 10 * PATHS.index(path) + len(pattern))
    for (rows, _r) in _engine_families(path):
        assert all(pinned[r] == fc.fp(rows[0]) for r in rows)
    eng = B.DeviceIngest(gpu)
    try:
        done = []
        for i, ch in enumerate(chunks):
            eng.count(*_device(gpu, ch))
            done += ch
            exp = _assert_results(eng, oracle, done, times=2 if i == 0 else 1)
        got = {(L, w[:(L + 31) // 32]): c for (w, L, c, _f) in exp}
        for (rows, reps) in _engine_families(path):          # the plan itself: every member, apart
            per = [got[(r[-1], r[:-1])] for r in rows]
            assert per == [t * (2 if (pattern != "first" and k == 0) or (pattern == "across" and k == 1) else 1)
                           for k, t in enumerate(reps)]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_ingest_cross_class_pair(gpu, oracle, pinned, path):
    """A 64-nt and a 96-nt read with one fingerprint in one chunk: the representative of the fingerprint
    is a row of the other class -- the whole-row compare of the read-order rows (the length word and the
    zero tail differ), the class word of k_cls_verify_rep, the class range of k_cls_verify."""
    import shortseq_amd.batch as B
    a, b = cross_pair()
    assert pinned[a] == pinned[b]
    rng = random.Random(300 + PATHS.index(path))
    reads = _chunk(rng, _background(rng, path), 20_000, [(_read_of_class_row(a), 3), (_read_of_class_row(b), 5)])
    eng = B.DeviceIngest(gpu)
    try:
        eng.count(*_device(gpu, reads))
        exp = _assert_results(eng, oracle, reads, times=2)
    finally:
        eng.close()
    got = {(L, w): c for (w, L, c, _f) in exp}
    assert got[(64, a[:-1])] == 3 and got[(96, b[:-1])] == 5


@pytest.mark.gpu
def test_ingest_export_merge_colliders(gpu, oracle, pinned):
    """Engine 1 holds member A of every family and engine 2 member B (no engine sees a collision); after
    export() and merge() both survive with their own counts and first indices."""
    import shortseq_amd.batch as B
    rng = random.Random(400)
    pool = _background(rng, "rows")
    fams = _engine_families("rows")
    r1 = _chunk(rng, pool, 10_000, _members(fams, lambda k: k == 0))
    r2 = _chunk(rng, pool, 10_000, _members(fams, lambda k: k == 1))
    e1, e2 = B.DeviceIngest(gpu), B.DeviceIngest(gpu)
    try:
        e1.count(*_device(gpu, r1))
        e2.count(*_device(gpu, r2))
        assert e2.export() > 0
        e1.merge(e2, len(r1))
        exp = _assert_results(e1, oracle, r1 + r2)
    finally:
        e1.close()
        e2.close()
    got = {(L, w[:(L + 31) // 32]): c for (w, L, c, _f) in exp}
    for (rows, reps) in fams:
        assert [got[(r[-1], r[:-1])] for r in rows[:2]] == list(reps[:2])


def _items(c):
    return [(type(k).__name__, str(k), len(k), v) for k, v in c.items()]


@pytest.mark.gpu
def test_dropin_colliders(gpu, pinned, tmp_path):
    """ShortSeqCounter(list, device="cuda") and read_and_count_fastq (one chunk, and 64-KiB chunks) over
    a list that holds the 64-nt family, the 96-nt family and the cross-class pair == the host path:
    keys, counts, dict order."""
    import shortseq_amd as sq
    rng = random.Random(500)
    a, b = cross_pair()
    inject = _members([(class_family(64)[0], REPS), (class_family(96)[0], REPS)], lambda k: True)
    inject += [(_read_of_class_row(a), 3), (_read_of_class_row(b), 5)]
    reads = _chunk(rng, _background(rng, "rows"), sq._shortseq.GPU_MIN_READS, inject)
    assert len(reads) >= 65_536
    host = _items(sq.ShortSeqCounter(reads, device="host"))
    assert sum(v for (_t, _s, _l, v) in host) == len(reads)
    by_str = {s: v for (_t, s, _l, v) in host}
    assert [by_str[fc.to_read(r[:-1], r[-1]).decode()] for r in class_family(64)[0]] == list(REPS)
    assert _items(sq.ShortSeqCounter(reads, device="cuda")) == host
    p = tmp_path / "colliders.fq"
    with open(p, "wb") as fh:
        for i, r in enumerate(reads):
            fh.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    assert _items(sq.read_and_count_fastq(str(p), device="host")) == host
    for chunk in (0, 1 << 16):
        assert _items(sq.read_and_count_fastq(str(p), device="cuda", _chunk_bytes=chunk)) == host
