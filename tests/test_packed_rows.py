"""The operations that consume packed rows -- ss_decode_fixed / ss_decode_var, ss_slice_fixed /
ss_slice_var, ss_hamming_ref / ss_hamming_pair on padded rows, HostStager.decode -- on every row of
every batch, in every layout the C ABI promises, and past the 4096-block cap of the grid-stride
kernels (k_decode_gen, k_slice wrap at 1,048,576 lanes).

References are vectorised numpy restatements of the header's definitions (bit gather for the slice,
a character table for the decode, the whole-word popcount for the distance); the CPU tests at the
top pin each of them to the oracle (and the slice to the golden file), which is what lets the GPU
tests trust them on batches too large for per-row oracle calls.

Inputs: reads through the encoder (oracle.encode_batch / B.encode), then "dirty": random bits ORed
in above bit 2L of a row and random words in its padding (wpr > words), so a kernel that looks past
the read shows.  Source rows sit between random guard words, outputs between canary guards (0xEE
bytes, 0xFF words), and whole buffers are compared: a write outside a row's L bytes or outside a
slice's words fails.  All comparisons are exact.
"""
import functools

import numpy as np
import pytest

ACTG = np.frombuffer(b"ACTG", dtype=np.uint8)
M55 = np.uint64(0x5555555555555555)
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
CANARY = 0xEE
GW = 80          # guard words around packed buffers (640 B: keeps 16-B alignment)
GB = 256         # guard bytes around ASCII buffers (keeps 16-B alignment)
MAX_NT = 1024


def _words_for(L):
    return (L + 31) // 32


def _wpr_for(L):
    return max(1, _words_for(L))


def _ham_words(L):
    return 1 if L <= 32 else _words_for(L)


def _round16(L):
    return (L + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------------------------
def _u64_of(x, n):
    """starts / lens as the kernel sees them: u32 values, widened to u64 (no wrap in 2 * x)."""
    a = np.asarray(x)
    if a.dtype != np.uint32:
        assert a.dtype.kind in "iu" and a.min(initial=0) >= 0 and a.max(initial=0) < 2 ** 32
    return np.broadcast_to(a.astype(np.uint64), (n,))


def np_slice(rows, starts, lens, out_wpr, read_lens=None, block=2048):
    """include/shortseq_amd.h, batch slice: output bit p of row r is source bit 2 st + p, set only
    when p < 2 ln and 2 st + p < 64 wpr; with read lengths st = min(st, L_r), ln = min(ln, L_r - st)
    first.  rows uint64 [n, wpr] -> uint64 [n, out_wpr]."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    n, wpr = rows.shape
    st, ln = _u64_of(starts, n), _u64_of(lens, n)
    if read_lens is not None:
        rl = _u64_of(read_lens, n)
        st = np.minimum(st, rl)
        ln = np.minimum(ln, rl - st)
    two = np.uint64(2)
    out = np.zeros((n, out_wpr), dtype=np.uint64)
    p = np.arange(64 * out_wpr, dtype=np.uint64)[None, :]
    for a in range(0, n, block):
        b = min(n, a + block)
        bits = np.unpackbits(rows[a:b].view(np.uint8), axis=1, bitorder="little")     # [m, 64 wpr]
        idx = two * st[a:b, None] + p
        ok = (p < two * ln[a:b, None]) & (idx < np.uint64(64 * wpr))
        got = np.take_along_axis(bits, np.where(ok, idx, np.uint64(0)).astype(np.intp), axis=1)
        got = np.where(ok, got, np.uint8(0))
        out[a:b] = np.packbits(got, axis=1, bitorder="little").view(np.uint64)
    return out


def np_chars(rows):
    """uint64 [n, wpr] -> uint8 [n, 32 wpr]: character j of a row = b"ACTG"[(word j/32 >> 2 (j%32)) & 3]
    (byte k of a little-endian word holds nts 4k .. 4k + 3)."""
    b = np.ascontiguousarray(rows, dtype="<u8").view(np.uint8)
    codes = np.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], axis=-1)
    return ACTG[codes.reshape(b.shape[0], -1)]


def np_decode_fixed(rows, L, stride, base, total):
    """The whole output buffer of ss_decode_fixed at d_ascii = buffer + base: L bytes per read at
    row * stride, everything else the canary."""
    n = rows.shape[0]
    exp = np.full(total, CANARY, dtype=np.uint8)
    assert base + n * stride <= total
    if n and L:
        exp[base:base + n * stride].reshape(n, stride)[:, :L] = np_chars(rows)[:, :L]
    return exp


def np_decode_var(rows, lens, offs, total, block=4096):
    """The whole output buffer of ss_decode_var: lens[r] bytes at offs[r]; a read longer than 1024
    writes nothing."""
    exp = np.full(total, CANARY, dtype=np.uint8)
    chars = np_chars(rows)
    j = np.arange(chars.shape[1], dtype=np.int64)[None, :]
    for a in range(0, rows.shape[0], block):
        b = min(rows.shape[0], a + block)
        ln = lens[a:b].astype(np.int64)
        ln[ln > MAX_NT] = 0
        m = j < ln[:, None]
        pos = offs[a:b].astype(np.int64)[:, None] + j
        exp[pos[m]] = chars[a:b][m]
    return exp


def np_hamming(a, b, L):
    """Header formula: sum over W = (L <= 32 ? 1 : ceil(L/32)) whole words of
    popcount(((x >> 1) | x) & 0x5555...), x = a ^ b.  b: rows like a, or one reference row."""
    W = _ham_words(L)
    x = a[:, :W] ^ (b[:, :W] if b.ndim == 2 else b[None, :W])
    y = np.ascontiguousarray(((x >> np.uint64(1)) | x) & M55)
    return np.unpackbits(y.view(np.uint8), axis=1).sum(axis=1).astype(np.uint32)


# ---------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------
def _encoded(oracle, seed, n, L):
    """n generator reads of L nt through the oracle's encoder -> uint64 [n, wpr_for(L)], clean."""
    words, rc, _ = oracle.encode_batch(oracle.gen_reads(seed, 0, n, L), n, L)
    assert rc == 0
    return words


def _dirty(rng, words, lens, wpr):
    """Rows [n, wpr] holding the reads' words, with random bits above bit 2 * len of each row: the
    rest of the read's last word and all of its padding words.  lens: one length or one per row."""
    n, W = words.shape
    rows = np.zeros((n, wpr), dtype=np.uint64)
    rows[:, :W] = words
    ln = np.broadcast_to(np.asarray(lens, dtype=np.int64), (n,))
    sh = np.clip(2 * ln[:, None] - 64 * np.arange(wpr, dtype=np.int64)[None, :], 0, 64)
    mask = np.where(sh >= 64, np.uint64(0), FF << np.minimum(sh, 63).astype(np.uint64))
    assert not (rows & mask).any()
    return rows | (rng.integers(0, 2 ** 64, size=(n, wpr), dtype=np.uint64) & mask)


def _dirty_reads(oracle, rng, seed, n, L, wpr):
    return _dirty(rng, _encoded(oracle, seed, n, L), L, wpr)


@functools.lru_cache(maxsize=None)
def _big_words(oracle):
    """70,001 reads of 1024 nt through the encoder: 2,240,032 random words, shared (read-only) by
    the tests past the grid cap, which view them as [n, wpr] rows."""
    w = _encoded(oracle, 901, 70001, 1024).reshape(-1)
    w.setflags(write=False)
    return w


def _big_rows(oracle, n, wpr):
    return _big_words(oracle)[:n * wpr].reshape(n, wpr)


# ---------------------------------------------------------------------------------------------
# Pinning: the numpy references against the oracle (CPU only)
# ---------------------------------------------------------------------------------------------
def test_np_slice_pinned_to_golden(oracle, golden):
    checked = 0
    for case in golden["slices"]:
        seq = case["seq"]
        L = len(seq)
        src, err = oracle.encode_one(seq.encode(), _wpr_for(L))
        assert err.kind == 0
        items = []
        for it in case["slices"]:
            if "step" in it:
                continue
            st, sp, _ = slice(it["start"], it["stop"]).indices(L)
            ln = max(0, sp - st)
            assert ln == it["length"]
            items.append((st if ln else 0, ln, [int(h, 16) for h in it["words"]]))
        for it in case["indices"]:
            if "raises" not in it:
                items.append((it["index"] % L, 1, [int(h, 16) for h in it["words"]]))
        for st, ln, gold in items:
            ow = _wpr_for(ln)
            got = [int(x) for x in np_slice(src[None, :], np.uint32(st), np.uint32(ln), ow)[0]]
            assert got == oracle.slice_words(src, st, ln), (L, st, ln)
            m = max(len(got), len(gold))        # ShortSeq192 keeps 3 words, unused ones 0
            assert got + [0] * (m - len(got)) == gold + [0] * (m - len(gold)), (L, st, ln)
            checked += 1
    assert checked > 1500


def test_np_slice_pinned_to_oracle_random(oracle):
    rng = np.random.default_rng(5)
    checked = 0
    for L in (1, 31, 32, 33, 64, 97, 150, 512, 1000, 1024):
        n = 240
        wpr = _wpr_for(L) + (L % 3)                  # dense and padded rows
        if wpr > 32:
            wpr = 32
        rows = _dirty_reads(oracle, rng, 300 + L, n, L, wpr)
        starts = rng.integers(0, L + 6, size=n).astype(np.uint32)
        lens = rng.integers(0, L + 6, size=n).astype(np.uint32)
        starts[:4], lens[:4] = (0, L, L - 1, 0), (L, 0, 1, 0)
        got = np_slice(rows, starts, lens, wpr, read_lens=np.uint32(L))
        for r in range(n):
            st = min(int(starts[r]), L)
            ln = min(int(lens[r]), L - st)
            exp = oracle.slice_words(rows[r], st, ln)
            exp += [0] * (wpr - len(exp))
            assert [int(x) for x in got[r]] == exp, (L, r, st, ln)
            checked += 1
    assert checked >= 2000


def test_np_slice_unclamped_semantics():
    """Without read lengths: a start at or past 32 wpr gives a zero row, a huge len the row from
    start to the end of its wpr words, an out_wpr below the slice its first 32 out_wpr nts -- the
    arithmetic in 64 bits, no wrap at 2^31."""
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 2 ** 64, size=(4, 3), dtype=np.uint64)
    big = [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    for v in big + [96, 97]:
        assert not np_slice(rows, np.uint32(v), np.uint32(5), 3).any()
    for v in big + [96, 97, 200]:
        assert np.array_equal(np_slice(rows, np.uint32(0), np.uint32(v), 3), rows)
        got = np_slice(rows, np.uint32(32), np.uint32(v), 4)
        assert np.array_equal(got[:, :2], rows[:, 1:]) and not got[:, 2:].any()
    assert np.array_equal(np_slice(rows, np.uint32(32), np.uint32(64), 1), rows[:, 1:2])
    assert np.array_equal(np_slice(rows, np.uint32(1), np.uint32(3), 1)[:, 0],
                          (rows[:, 0] >> np.uint64(2)) & np.uint64(63))


def test_np_decode_pinned_to_oracle(oracle):
    rng = np.random.default_rng(7)
    for L in (1, 15, 16, 17, 31, 32, 33, 63, 64, 96, 100, 1000, 1024):
        n = 64
        for wpr in sorted({_wpr_for(L), min(32, _wpr_for(L) + 1), 32}):
            rows = _dirty_reads(oracle, rng, 400 + L, n, L, wpr)
            exp = oracle.decode_batch(rows, n, L, wpr).reshape(n, L)
            assert np.array_equal(np_chars(rows)[:, :L], exp), (L, wpr)
            assert np.array_equal(exp.reshape(-1), oracle.gen_reads(400 + L, 0, n, L)), (L, wpr)
            buf = np_decode_fixed(rows, L, L + 3, 5, 5 + n * (L + 3) + 2)
            body = buf[5:5 + n * (L + 3)].reshape(n, L + 3)
            assert np.array_equal(body[:, :L], exp) and (body[:, L:] == CANARY).all()
            assert (buf[:5] == CANARY).all() and (buf[-2:] == CANARY).all()
    # var: permuted offsets, a skipped (too long) read
    rows = _dirty_reads(oracle, rng, 77, 5, 128, 4)
    lens = np.array([0, 1, 33, 128, 1025], dtype=np.uint32)
    offs = np.array([200, 150, 10, 300, 500], dtype=np.uint64)
    buf = np_decode_var(rows, lens, offs, 600)
    chars = oracle.decode_batch(rows, 5, 128, 4).reshape(5, 128)
    want = np.full(600, CANARY, dtype=np.uint8)
    for r in range(4):
        want[int(offs[r]):int(offs[r]) + int(lens[r])] = chars[r, :lens[r]]
    assert np.array_equal(buf, want)


def test_np_hamming_pinned_to_oracle(oracle):
    rng = np.random.default_rng(8)
    for L in (1, 31, 32, 33, 64, 96, 97, 150, 1000, 1024):
        W = _ham_words(L)
        n = 200
        for wpr in sorted({W, min(32, W + 1), min(32, W + 5), 32}):
            a = _dirty_reads(oracle, rng, 500 + L, n, L, wpr)
            b = _dirty_reads(oracle, rng, 600 + L, n, L, wpr)
            b[::7] = a[::7]
            b[::7, wpr - 1] ^= np.uint64(1) if wpr > W else np.uint64(0)     # padding never counts
            pair = np_hamming(a, b, L)
            assert np.array_equal(pair, oracle.hamming_pair_batch(a, b, n, L, wpr=wpr)), (L, wpr)
            assert not pair[::7].any()
            ref = a[n // 3].copy()
            assert np.array_equal(np_hamming(a, ref, L), oracle.hamming_ref_batch(a, n, L, ref, wpr=wpr)), (L, wpr)


# ---------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------
def _api():
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd._native import lib
    return torch, B, lib()


def _stream(torch, gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


def _dev(torch, gpu, a):
    """numpy -> device tensor of the same bits (uint64 as int64, uint32 as int32)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(gpu)


class _Src:
    """Packed rows on the device between GW random guard words on either side: a kernel that reads
    past a row's wpr words, or past the batch, meets noise."""

    def __init__(self, torch, gpu, rows, rng):
        self.n, self.wpr = rows.shape
        buf = rng.integers(0, 2 ** 64, size=2 * GW + rows.size, dtype=np.uint64)
        buf[GW:GW + rows.size] = rows.reshape(-1)
        self.buf = _dev(torch, gpu, buf)
        self.flat = self.buf[GW:GW + rows.size]
        self.t = self.flat.view(self.n, self.wpr)
        self.ptr = self.flat.data_ptr() if rows.size else self.buf.data_ptr() + 8 * GW
        assert self.ptr % 16 == 0


class _WordsOut:
    """n x ow output words pre-filled with 0xFF.., between GW guard words of the same."""

    def __init__(self, torch, gpu, n, ow):
        self.n, self.ow = n, ow
        self.buf = torch.full((2 * GW + n * ow,), -1, dtype=torch.int64, device=gpu)
        self.t = self.buf[GW:GW + n * ow].view(n, ow)
        self.ptr = self.buf.data_ptr() + 8 * GW

    def check(self, want, what):
        got = self.buf.cpu().numpy().view(np.uint64)
        assert (got[:GW] == FF).all() and (got[GW + self.n * self.ow:] == FF).all(), ("guard words", what)
        body = got[GW:GW + self.n * self.ow].reshape(self.n, self.ow)
        if not np.array_equal(body, want):
            r = np.flatnonzero((body != want).any(axis=1))
            raise AssertionError((what, "rows differ", len(r), "first", int(r[0]),
                                  [hex(int(x)) for x in body[r[0]]], [hex(int(x)) for x in want[r[0]]]))


def _slice_var(torch, gpu, lib, src, starts, lens, read_lens, out_wpr, want, what):
    """One ss_slice_var launch into a canary-guarded buffer; every row and the guards compared."""
    out = _WordsOut(torch, gpu, src.n, out_wpr)
    d_st, d_ln = _dev(torch, gpu, starts), _dev(torch, gpu, lens)
    d_rl = None if read_lens is None else _dev(torch, gpu, read_lens)
    rc = lib.ss_slice_var(src.ptr, src.n, src.wpr, None if d_rl is None else d_rl.data_ptr(), d_st.data_ptr(),
                          d_ln.data_ptr(), out.ptr, out_wpr, _stream(torch, gpu))
    assert rc == 0, what
    out.check(want, what)


def _decode_fixed(torch, gpu, lib, src, L, stride, base, what):
    """One ss_decode_fixed launch at d_ascii = (16-B aligned) + base; the whole buffer compared."""
    total = GB + base + src.n * stride + GB
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=gpu)
    assert out.data_ptr() % 16 == 0
    rc = lib.ss_decode_fixed(src.ptr, src.n, L, src.wpr, out.data_ptr() + GB + base, stride, _stream(torch, gpu))
    assert rc == 0, what
    return out.cpu().numpy(), total


# ---------------------------------------------------------------------------------------------
# 1. ss_decode_fixed layouts
# ---------------------------------------------------------------------------------------------
DECODE_LS = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 80, 96, 100, 112, 1000, 1008, 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("L", DECODE_LS)
def test_decode_fixed_layouts(gpu, oracle, L):
    """wpr x stride x output offset: both sides of the fast predicate (L % 16, stride % 16, 16-B
    aligned d_ascii), k_decode_g16 with cpr 3 / 5 / 7 / 63, both alignment branches of store_chars.
    Exactly L bytes per read are written, wherever the rows lie."""
    torch, B, lib = _api()
    rng = np.random.default_rng(1000 + L)
    n, W = 257, _wpr_for(L)
    for wpr in sorted({W, min(32, W + 1), 32}):
        rows = _dirty_reads(oracle, rng, 10 + L, n, L, wpr)
        src = _Src(torch, gpu, rows, rng)
        chars = np_chars(rows)[:, :L]
        for stride in sorted({L, L + 1, L + 3, _round16(L) + 16}):
            for base in (0, 1, 8, 16):
                got, total = _decode_fixed(torch, gpu, lib, src, L, stride, base, (L, wpr, stride, base))
                want = np.full(total, CANARY, dtype=np.uint8)
                want[GB + base:GB + base + n * stride].reshape(n, stride)[:, :L] = chars
                assert np.array_equal(got, want), (L, wpr, stride, base)
        # 1-D words through B.decode(..., wpr=), and an empty batch
        out = torch.full((2 * GB + n * L,), CANARY, dtype=torch.uint8, device=gpu)
        back = B.decode(src.flat, L, wpr=wpr, out=out[GB:GB + n * L].view(n, L))
        assert back.shape == (n, L)
        assert np.array_equal(out.cpu().numpy(), np_decode_fixed(rows, L, L, GB, 2 * GB + n * L)), (L, wpr, "1-D")
        out.fill_(CANARY)
        assert lib.ss_decode_fixed(src.ptr, 0, L, wpr, out.data_ptr() + GB, L, _stream(torch, gpu)) == 0
        assert bool((out == CANARY).all()), (L, wpr, "n = 0")


# ---------------------------------------------------------------------------------------------
# 2. k_decode_gen past the grid cap (4096 blocks x 256 lanes = 1,048,576 lanes, one per word)
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,L,stride", [(33001, 1000, 1000), (33001, 1024, 1025), (70001, 1000, 1000)])
def test_decode_gen_past_grid_cap(gpu, oracle, n, L, stride):
    """32 words per row: 33,001 rows are 1,056,032 lanes (the last 7,456 wrap once), 70,001 rows
    wrap twice.  L = 1000 is off the 16-nt grid and the odd stride 1025 off the 16-B grid, so both
    take k_decode_gen.  Rows of 1024 random nts read as 1000 are dirty above bit 2L."""
    torch, B, lib = _api()
    rng = np.random.default_rng(n + L)
    rows = _big_rows(oracle, n, 32)
    src = _Src(torch, gpu, rows, rng)
    got, total = _decode_fixed(torch, gpu, lib, src, L, stride, 0, (n, L, stride))
    assert np.array_equal(got, np_decode_fixed(rows, L, stride, GB, total))


# ---------------------------------------------------------------------------------------------
# 3. ss_decode_var
# ---------------------------------------------------------------------------------------------
def _var_layout(rng, lens):
    """Offsets that place the reads in a random order with 0..5 canary bytes between neighbours
    (neither sorted nor aligned); a read that must be skipped (> 1024) still owns 64 bytes."""
    n = len(lens)
    room = np.where(lens > MAX_NT, 64, lens).astype(np.int64) + rng.integers(0, 6, size=n)
    order = rng.permutation(n)
    offs = np.zeros(n, dtype=np.uint64)
    offs[order] = GB + 3 + np.concatenate(([0], np.cumsum(room[order])[:-1]))
    return offs, int(GB + 3 + room.sum() + GB)


def _decode_var_case(gpu, rows, lens, rng, what):
    torch, B, lib = _api()
    offs, total = _var_layout(rng, lens)
    src = _Src(torch, gpu, rows, rng)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device=gpu)
    d_lens, d_offs = _dev(torch, gpu, lens), _dev(torch, gpu, offs)
    rc = lib.ss_decode_var(src.ptr, d_lens.data_ptr(), src.n, src.wpr, out.data_ptr(), d_offs.data_ptr(),
                           _stream(torch, gpu))
    assert rc == 0, what
    assert np.array_equal(out.cpu().numpy(), np_decode_var(rows, lens, offs, total)), what


@pytest.mark.gpu
def test_decode_var_past_grid_cap(gpu, oracle):
    rng = np.random.default_rng(33)
    n = 33001
    lens = rng.integers(0, MAX_NT + 1, size=n).astype(np.uint32)
    seeds = np.array([0, 1, 31, 32, 33, 1024, 1025, 0xFFFFFFFF], dtype=np.uint32)
    lens[:len(seeds)] = seeds
    lens[-len(seeds):] = seeds[::-1]             # in the wrapped lanes as well
    _decode_var_case(gpu, _big_rows(oracle, n, 32), lens, rng, "wpr 32")


@pytest.mark.gpu
def test_decode_var_small_rows(gpu, oracle):
    rng = np.random.default_rng(34)
    n = 3001
    rows = _dirty_reads(oracle, rng, 35, n, 128, 4)
    lens = rng.integers(0, 129, size=n).astype(np.uint32)
    lens[:8] = (0, 1, 31, 32, 33, 128, 1025, 0xFFFFFFFF)
    _decode_var_case(gpu, rows, lens, rng, "wpr 4")


# ---------------------------------------------------------------------------------------------
# 4. slice_var, exhaustive
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", (1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160))
def test_slice_var_exhaustive(gpu, oracle, L):
    """Every (start, len) with start + len <= L + 2 in one launch, each row another dirty read; with
    the read lengths (clamped to the read) and without (the dirty bits past L are then part of the
    slice, up to the end of the row's words)."""
    torch, B, lib = _api()
    rng = np.random.default_rng(2000 + L)
    pairs = np.array([(s, l) for s in range(L + 3) for l in range(L + 3 - s)], dtype=np.uint32)
    starts, lens = pairs[:, 0].copy(), pairs[:, 1].copy()
    n, wpr = len(pairs), _wpr_for(L)
    rows = _dirty_reads(oracle, rng, 20 + L, n, L, wpr)
    src = _Src(torch, gpu, rows, rng)
    rl = np.full(n, L, dtype=np.uint32)
    for read_lens in (rl, None):
        want = np_slice(rows, starts, lens, wpr, read_lens=read_lens)
        _slice_var(torch, gpu, lib, src, starts, lens, read_lens, wpr, want, (L, read_lens is not None))


@pytest.mark.gpu
@pytest.mark.parametrize("L", (512, 1000, 1024))
def test_slice_var_long_boundaries(gpu, oracle, L):
    torch, B, lib = _api()
    rng = np.random.default_rng(3000 + L)
    vals = sorted({0, 1, 31, 32, 33, 63, 64, 65, L - 65, L - 64, L - 33, L - 32, L - 31, L - 1, L})
    pairs = np.array([(s, l) for s in vals for l in vals if s <= L], dtype=np.uint32)
    starts, lens = pairs[:, 0].copy(), pairs[:, 1].copy()
    n, wpr = len(pairs), _wpr_for(L)
    rows = _dirty_reads(oracle, rng, 30 + L, n, L, wpr)
    src = _Src(torch, gpu, rows, rng)
    for read_lens in (np.full(n, L, dtype=np.uint32), None):
        want = np_slice(rows, starts, lens, wpr, read_lens=read_lens)
        _slice_var(torch, gpu, lib, src, starts, lens, read_lens, wpr, want, (L, read_lens is not None))


# ---------------------------------------------------------------------------------------------
# 5. slice_var shapes: out_wpr != wpr, lens past out_wpr, u32 extremes
# ---------------------------------------------------------------------------------------------
def _shape_cases(rng, wpr):
    """(starts, lens) u32: 400 random pairs in 0 .. 32 wpr + 2 (lens that fit an out_wpr and lens
    that exceed it), then the extremes 2^31 - 1, 2^31, 2^32 - 1 and 32 wpr with its neighbours
    against small values and against each other."""
    nt = 32 * wpr
    ext = [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, nt - 1, nt, nt + 1]
    small = [0, 1, 31, 32, 33]
    pairs = [(e, s) for e in ext for s in small] + [(s, e) for s in small for e in ext] + \
            [(a, b) for a in ext for b in ext]
    starts = np.concatenate((rng.integers(0, nt + 3, size=400), [p[0] for p in pairs])).astype(np.uint32)
    lens = np.concatenate((rng.integers(0, nt + 3, size=400), [p[1] for p in pairs])).astype(np.uint32)
    return starts, lens


@pytest.mark.gpu
@pytest.mark.parametrize("wpr", (1, 5, 32))
def test_slice_var_shapes_and_extremes(gpu, oracle, wpr):
    """out_wpr below, at and above wpr; a len past out_wpr leaves the first 32 out_wpr nts of the
    slice.  starts / lens are u32 (int32 bit patterns from batch.py's tensors): without read lengths
    a start at or past 32 wpr is a zero row and a huge len the read from start to the end of its
    words, 2^31 and 2^32 - 1 included; with read lengths both are clamped to the read."""
    torch, B, lib = _api()
    rng = np.random.default_rng(4000 + wpr)
    starts, lens = _shape_cases(rng, wpr)
    n = len(starts)
    rows = _dirty_reads(oracle, rng, 40 + wpr, n, 32 * wpr, wpr)      # every bit of a row random
    src = _Src(torch, gpu, rows, rng)
    rl = rng.integers(0, 32 * wpr + 1, size=n).astype(np.uint32)
    for out_wpr in sorted({1, 2, max(1, wpr - 1), wpr, min(32, wpr + 1), 32}):
        for read_lens in (rl, None):
            want = np_slice(rows, starts, lens, out_wpr, read_lens=read_lens)
            _slice_var(torch, gpu, lib, src, starts, lens, read_lens, out_wpr, want,
                       (wpr, out_wpr, read_lens is not None))
    # the same through batch.py's int32 tensors
    d = lambda a: _dev(torch, gpu, a)  # noqa: E731
    got = B.slice_var(src.t, d(starts), d(lens), read_lens=None, out_wpr=wpr).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, np_slice(rows, starts, lens, wpr))
    got = B.slice_var(src.t, d(starts), d(lens), read_lens=d(rl)).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, np_slice(rows, starts, lens, wpr, read_lens=rl))


# ---------------------------------------------------------------------------------------------
# 6. k_slice past the grid cap
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,wpr", [(33001, 32), (140001, 5)])
def test_slice_var_past_grid_cap(gpu, oracle, n, wpr):
    """33,001 rows x 32 lanes = 1,056,032 lanes; 140,001 rows x 8 lanes (5 live, 3 idle) =
    1,120,008 lanes: the grid-stride loop wraps.  Every row compared."""
    torch, B, lib = _api()
    rng = np.random.default_rng(n)
    rows = _big_rows(oracle, n, wpr)
    starts = rng.integers(0, 32 * wpr + 3, size=n).astype(np.uint32)
    lens = rng.integers(0, 32 * wpr + 3, size=n).astype(np.uint32)
    read_lens = None if wpr == 32 else rng.integers(0, 32 * wpr + 1, size=n).astype(np.uint32)
    src = _Src(torch, gpu, rows, rng)
    want = np_slice(rows, starts, lens, wpr, read_lens=read_lens)
    _slice_var(torch, gpu, lib, src, starts, lens, read_lens, wpr, want, (n, wpr))


@pytest.mark.gpu
def test_slice_fixed_past_grid_cap(gpu, oracle):
    torch, B, lib = _api()
    rng = np.random.default_rng(61)
    n, L = 33001, 1024
    rows = _big_rows(oracle, n, 32)
    src = _Src(torch, gpu, rows, rng)
    out = _WordsOut(torch, gpu, n, 32)
    res, ln = B.slice_fixed(src.t, L, 1, 1024, out=out.t)
    assert ln == 1023 and res.data_ptr() == out.ptr
    out.check(np_slice(rows, np.uint32(1), np.uint32(1023), 32), "slice_fixed (1, 1024)")


# ---------------------------------------------------------------------------------------------
# 7. slice_fixed layouts
# ---------------------------------------------------------------------------------------------
def _fixed_bounds(L):
    """About 40 (start, stop) pairs: whole read, ends, word boundaries with their neighbours,
    negative and open bounds, empty and reversed ranges."""
    b = {(None, None), (0, L), (0, 1), (L - 1, L), (0, 0), (L, L), (None, 1), (-1, None), (1, None),
         (None, -1), (-L, None), (-L - 2, L + 2), (L + 1, L + 5), (2, 1), (-1, -2), (-3, -1), (-2, None)}
    for s in (31, 32, 33, 64, 97):
        if s < L:
            b |= {(s, None), (None, s), (s, min(L, s + 32)), (s, min(L, s + 33))}
    for a, c in ((-33, -1), (-65, -32), (-64, None), (None, -33), (-97, -64), (7, -7), (33, -31)):
        b.add((a, c))
    return sorted(b, key=repr)


@pytest.mark.gpu
@pytest.mark.parametrize("L", (1, 32, 33, 64, 96, 97, 150, 1024))
def test_slice_fixed_layouts(gpu, oracle, L):
    """Python slice bounds on dense and padded (dirty) rows, every row compared; out= tensors of the
    width needed, one more, and 32, pre-filled with 0xFF: words past the slice come back zero."""
    torch, B, lib = _api()
    rng = np.random.default_rng(5000 + L)
    n = 1000
    for wpr in sorted({_wpr_for(L), min(32, _wpr_for(L) + 2)}):
        rows = _dirty_reads(oracle, rng, 50 + L, n, L, wpr)
        src = _Src(torch, gpu, rows, rng)
        for a, b in _fixed_bounds(L):
            st, sp, _ = slice(a, b).indices(L)
            ln = max(0, sp - st)
            need = _wpr_for(ln)
            core = np_slice(rows, np.uint32(st if ln else 0), np.uint32(ln), need)
            if ln:      # the slice lies inside the read: never a dirty bit
                assert np.array_equal(np_chars(core)[:, :ln], np_chars(rows)[:, st:st + ln])
            for ow in sorted({need, min(32, need + 1), 32}):
                out = _WordsOut(torch, gpu, n, ow)
                res, got_ln = B.slice_fixed(src.t, L, a, b, out=out.t)
                assert got_ln == ln and res.data_ptr() == out.ptr
                want = np.zeros((n, ow), dtype=np.uint64)
                want[:, :need] = core
                out.check(want, (L, wpr, a, b, ow))
        res, got_ln = B.slice_fixed(src.t, L, 0, min(L, 33))        # the tensor batch.py allocates
        assert tuple(res.shape) == (n, _wpr_for(min(L, 33)))
        assert np.array_equal(res.cpu().numpy().view(np.uint64),
                              np_slice(rows, np.uint32(0), np.uint32(got_ln), res.shape[1]))


# ---------------------------------------------------------------------------------------------
# 8. hamming on padded rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", (1, 32, 33, 64, 96, 97, 150, 1000))
def test_hamming_padded_rows(gpu, oracle, L):
    """wpr > W with random padding words and dirty bits above 2L: k_ham_group's padded-row branch.
    The whole-word distance counts the dirty bits of word W - 1 and never a padding word; the same
    rows packed densely (wpr == W, the streaming kernels) give the same distances."""
    torch, B, lib = _api()
    rng = np.random.default_rng(6000 + L)
    W = _ham_words(L)
    s = _stream(torch, gpu)
    for n in (1, 255, 4097):
        wb = _encoded(oracle, 70 + L, n, L)
        wb[::5] = _encoded(oracle, 60 + L, n, L)[::5]
        da = _dirty_reads(oracle, rng, 60 + L, n, L, W)         # dense rows: dirty above 2L only
        db = _dirty(rng, wb, L, W)
        ref_row = n // 3
        want_pair, want_ref = np_hamming(da, db, L), np_hamming(da, da[ref_row], L)
        # 1000 nt fill all 32 words a row may have: no padded layout exists, and a distance array
        # off the 8-B grid sends the dense rows to the lane-group kernel instead
        for wpr in sorted({min(32, W + 1), min(32, W + 5), 32}):
            a, b = (rng.integers(0, 2 ** 64, size=(n, wpr), dtype=np.uint64) for _ in range(2))
            a[:, :W], b[:, :W] = da, db                         # the same reads, random padding words
            sa, sb = _Src(torch, gpu, a, rng), _Src(torch, gpu, b, rng)
            assert np.array_equal(want_pair, oracle.hamming_pair_batch(a, b, n, L, wpr=wpr))
            assert np.array_equal(want_ref, oracle.hamming_ref_batch(a, n, L, a[ref_row], wpr=wpr))
            g = 8 if wpr > W else 9
            for which, want in (("pair", want_pair), ("ref", want_ref)):
                out = torch.full((n + 16,), -1, dtype=torch.int32, device=gpu)
                if which == "pair":
                    rc = lib.ss_hamming_pair(sa.ptr, sb.ptr, n, L, wpr, out.data_ptr() + 4 * g, s)
                else:
                    rc = lib.ss_hamming_ref(sa.ptr, n, L, wpr, sa.ptr + 8 * wpr * ref_row, out.data_ptr() + 4 * g, s)
                assert rc == 0, (L, n, wpr, which)
                got = out.cpu().numpy()
                assert (got[:g] == -1).all() and (got[g + n:] == -1).all(), (L, n, wpr, which, "guard")
                assert np.array_equal(got[g:g + n].view(np.uint32), want), (L, n, wpr, which)
        sa, sb = _Src(torch, gpu, da, rng), _Src(torch, gpu, db, rng)
        got = B.hamming_pair(sa.t, sb.t, L).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want_pair), (L, n, "dense pair")
        got = B.hamming_ref(sa.t, L, sa.t[ref_row].clone()).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want_ref), (L, n, "dense ref")


# ---------------------------------------------------------------------------------------------
# 9. HostStager.decode: many chunks, padded rows, strided out
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nslots", (2, 3))
def test_host_stager_decode_chunked_strided(gpu, oracle, nslots):
    """4096-byte chunks: 1000 reads take a dozen to well over a hundred chunks through 2 or 3
    slots (a chunk holds 4096 / max(8 wpr, stride) reads).  out is a view of a
    wider array (row stride L + 5, off the 16-B grid, and round16(L) + 16, on it); columns [:L] are
    the reads, the rest of a row is unspecified by the header."""
    torch, B, lib = _api()
    rng = np.random.default_rng(7000 + nslots)
    st = B.HostStager(gpu, chunk_bytes=4096, nslots=nslots, copy_threads=2)
    try:
        n = 1000
        for L in (31, 32, 100, 512):
            for wpr in sorted({_wpr_for(L), min(32, _wpr_for(L) + 1 + nslots)}):
                rows = _dirty_reads(oracle, rng, 80 + L, n, L, wpr)
                want = np_chars(rows)[:, :L]
                for stride in (L, L + 5, _round16(L) + 16):
                    buf = np.full((n, stride), CANARY, dtype=np.uint8)
                    out = buf[:, :L]
                    back = st.decode(rows, L, out=out)
                    assert back is out
                    assert np.array_equal(out, want), (L, wpr, stride)
    finally:
        st.close()
