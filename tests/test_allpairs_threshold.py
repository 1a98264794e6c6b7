"""All-pairs thresholded hamming at the threshold: batches in which, for every segment g of the
pigeonhole split, some pair lies at distance exactly max_dist and shares segment g alone, further
pairs lie at exactly max_dist + 1 (with and without a shared segment), and position L (the alias
position of the table-encoded tail, which the whole-word distance counts) decides some of both.
Every method must then get the compare, every segment's bounds and position L right on its own.

The pool restates the documented split (G = k + 1 segments, L // G + (g < L % G) read positions each,
position L in the last) only to aim its substitutions; every expectation is the oracle's brute force
over all pairs, and test_threshold_pool_is_sharp proves on the oracle's words that the pool has the
pairs it is meant to have."""
import functools

import numpy as np
import pytest

ALIAS = 0x01    # table code 4 as a read's last byte: 'A' at position L - 1 and a set bit at position L
M55 = np.uint64(0x5555555555555555)


def _brute(oracle, words, n, L, k):
    """Oracle distances of every pair (ora_hamming_ref_batch row by row) -> counts, sorted pairs."""
    cnt = np.zeros(n, dtype=np.int64)
    pairs = []
    for i in range(n - 1):
        d = oracle.hamming_ref_batch(words[i + 1:], n - i - 1, L, words[i])
        js = np.flatnonzero(d <= k) + i + 1
        cnt[i] += len(js)
        cnt[js] += 1
        pairs.extend((i, int(j)) for j in js)
    return cnt, pairs


def _split(L, k):
    """Bounds of the G = k + 1 segments over the L read positions: segment g = [b[g], b[g + 1])."""
    G = k + 1
    lens = [L // G + (1 if g < L % G else 0) for g in range(G)]
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def _tile_rows(L):
    """Rows per tile of the tiled form that serves L (launch_allpairs_mfma's RB by k-steps; Tile<>)."""
    if L > 128:
        return 256
    if L > 32:
        return 128
    P = min(L + 1, 32)
    return 1024 if P <= 16 else (512 if P <= 24 else 256)


def _threshold_pool(oracle, L, k, centres, seed):
    """ASCII rows (n, L), shuffled: `centres` random reads and around each, per non-empty segment g
    and per end (substitutions at each segment's first / last position):
      - one substitution in every non-empty segment but g: distance k, g the only shared segment;
      - that row with a second substitution in a segment of >= 2 positions: distance k + 1, shares g;
      - where L % 32 != 0 and g is not the last segment (centres end in 'A'): the first row without
        the last segment's substitution and with the last byte aliased (distance k, one mismatch at
        position L), and the first row with its last byte aliased (distance k + 1 through position L
        alone; its last-segment substitution then stays off the last byte, and where that segment is
        one position long the second substitution of the row above takes its place);
    and once per centre one substitution in every non-empty segment: distance k + 1, nothing shared."""
    rng = np.random.default_rng(seed)
    b = _split(L, k)
    G = k + 1
    segs = [g for g in range(G) if b[g + 1] > b[g]]
    alias = L % 32 != 0
    base = oracle.gen_reads(seed, 0, centres, L).reshape(centres, L).copy()
    if alias:
        base[:, L - 1] = ord("A")
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def sub(row, c, pos):
        row[pos] = rng.choice(acgt[acgt != c[pos]])

    def far_end(h, end):      # the second substitution of segment h: its other end
        return int(b[h + 1] - 1 if end == 0 else b[h])

    rows = []
    for c in base:
        rows.append(c.copy())
        for end in (0, 1):
            at = {h: int(b[h] if end == 0 else b[h + 1] - 1) for h in segs}
            for g in segs:
                others = [h for h in segs if h != g]
                wide = [h for h in others if b[h + 1] - b[h] >= 2]
                near = c.copy()
                for h in others:
                    sub(near, c, at[h])
                rows.append(near)
                if wide:
                    past = near.copy()
                    sub(past, c, far_end(wide[int(rng.integers(len(wide)))], end))
                    rows.append(past)
                if alias and g != segs[-1]:
                    last = segs[-1]
                    a1 = c.copy()
                    for h in others:
                        if h != last:
                            sub(a1, c, at[h])
                    a1[L - 1] = ALIAS
                    rows.append(a1)
                    a2 = a1.copy()
                    if b[last + 1] - b[last] >= 2:
                        sub(a2, c, at[last] if at[last] != L - 1 else L - 2)
                        rows.append(a2)
                    else:
                        inner = [h for h in wide if h != last]
                        if inner:
                            sub(a2, c, far_end(inner[int(rng.integers(len(inner)))], end))
                            rows.append(a2)
            if end == 0:
                every = c.copy()
                for h in segs:
                    sub(every, c, at[h])
                rows.append(every)
    rows = np.stack(rows)
    return rows[rng.permutation(len(rows))]


@functools.lru_cache(maxsize=None)
def _centres(L, k):
    """Centres for n > 2 tiles of the tiled form (at least 3, so that families meet strangers)."""
    import oracle
    family = len(_threshold_pool(oracle, L, k, 1, 0))
    return max(3, -(-(2 * _tile_rows(L) + 1) // family))


CASES = [
    # one word
    (12, 1),      # k_pig_pairs<2>
    (16, 3),      # k_pig_pairs<4>
    (31, 5),      # k_pig_pairs<8>, the alias position at bit 62 of the word
    (32, 7),      # k_pig_pairs<8>, P = 32, no alias position
    (30, 12),     # k_pig_pairs<16>
    (23, 2),      # KS = 3
    # W = 2..4
    (33, 2),
    (64, 3),
    (65, 4),
    (96, 5),
    (100, 7),     # KS rounded from 13 to 16: 27 padding positions folded into thr
    (127, 15),    # P = 128, G = 16
    (128, 5),
    # the long form
    (129, 3),
    (150, 6),
    (160, 31),    # G = 32, no alias position
    (256, 7),
    (257, 4),
    (500, 12),
    (993, 20),
    (1023, 9),
    (1024, 31),
    (64, 20),     # LG = 4
    (20, 16),     # W = 1, segments of 1-2 nt
]


@functools.lru_cache(maxsize=None)
def _case(L, k):
    """The pool's ASCII rows, packed words and brute-force counts / pairs; computed once per case
    and shared (callers do not modify them)."""
    import oracle
    ascii = _threshold_pool(oracle, L, k, _centres(L, k), 1000 * L + k)
    n = ascii.shape[0]
    words, rc, _ = oracle.encode_batch(np.ascontiguousarray(ascii).reshape(-1), n, L)
    assert rc == 0
    words = np.ascontiguousarray(words).reshape(n, -1)
    words.setflags(write=False)
    cnt, pairs = _brute(oracle, words, n, L, k)
    return words, cnt, pairs


def _mismatches(words, i):
    """Mismatch positions of row i against rows i + 1.. from the words: bool [n - i - 1, 32 W]."""
    x = words[i + 1:] ^ words[i]
    m = ((x >> np.uint64(1)) | x) & M55
    bits = np.unpackbits(np.ascontiguousarray(m).view(np.uint8), axis=1, bitorder="little")
    return bits[:, 0::2].astype(bool)


@pytest.mark.parametrize("L,k", CASES)
def test_threshold_pool_is_sharp(oracle, L, k):
    """On the oracle's words alone: per non-empty segment g at least `centres` pairs at distance
    exactly k whose only mismatch-free segment is g; at least `centres` pairs at exactly k + 1 that
    share a segment and one that shares none; for L % 32 != 0 a pair at k and one at k + 1 with
    position L among the mismatches; more than two tiles of rows."""
    words, _, _ = _case(L, k)
    n, W = words.shape
    centres = _centres(L, k)
    assert 2 * _tile_rows(L) < n <= 2600
    P = min(L + 1, 32 * W)
    b = _split(L, k)
    b[-1] = P                                    # position L belongs to the last segment
    G = k + 1
    only = np.zeros(G, dtype=np.int64)           # pairs at k whose one clean segment is g
    past_shared = past_none = at_L_k = at_L_k1 = 0
    for i in range(n - 1):
        d = oracle.hamming_ref_batch(words[i + 1:], n - i - 1, L, words[i])
        sel = np.flatnonzero((d == k) | (d == k + 1))
        if not len(sel):
            continue
        mm = _mismatches(words, i)[sel]
        assert not mm[:, P:].any()
        assert np.array_equal(mm.sum(axis=1), d[sel])
        cs = np.concatenate((np.zeros((len(sel), 1), np.int64), np.cumsum(mm, axis=1)), axis=1)
        clean = (cs[:, b[1:]] - cs[:, b[:-1]]) == 0             # [pair, segment]
        nclean = clean.sum(axis=1)
        near = d[sel] == k
        one = near & (nclean == 1)
        only += clean[one].sum(axis=0)
        past_shared += int((~near & (nclean >= 1)).sum())
        past_none += int((~near & (nclean == 0)).sum())
        if L % 32:
            at_L_k += int((near & mm[:, L]).sum())
            at_L_k1 += int((~near & mm[:, L]).sum())
    for g in range(G):
        if b[g + 1] > b[g]:
            assert only[g] >= centres, (g, only)
    assert past_shared >= centres
    assert past_none >= 1
    if L % 32:
        assert at_L_k >= 1 and at_L_k1 >= 1


def _methods(L, k):
    m = ["tiles", "auto"]
    if L <= 128 and k <= 15:
        m.append("pigeonhole")
    if k <= 31:
        m.append("bucketed")
    return m


def _check(B, torch, d, L, k, cnt_e, pairs_e, method):
    """Counts, sorted pairs, total, count-only and 3-pair truncation of one call."""
    cnt, pairs, total = B.hamming_all_pairs(d, L, k, max_pairs=len(pairs_e) + 10, method=method)
    assert total == len(pairs_e), method
    assert np.array_equal(cnt.cpu().numpy().astype(np.int64), cnt_e), method
    assert [tuple(int(x) for x in p) for p in pairs.cpu().numpy()] == pairs_e, method
    cnt2, _, total2 = B.hamming_all_pairs(d, L, k, method=method)
    assert total2 == total and torch.equal(cnt2, cnt), method
    if total > 4:    # truncated: the total still counts every pair, the kept ones are real
        _, p3, total3 = B.hamming_all_pairs(d, L, k, counts=False, max_pairs=3, method=method)
        assert total3 == total and p3.shape[0] == 3, method
        kept = {tuple(int(x) for x in q) for q in p3.cpu().numpy()}
        assert len(kept) == 3 and kept <= set(pairs_e), method


@pytest.mark.gpu
@pytest.mark.parametrize("L,k", CASES)
def test_threshold_every_method(gpu, oracle, L, k):
    import torch
    import shortseq_amd.batch as B
    words, cnt_e, pairs_e = _case(L, k)
    assert len(pairs_e) > 4
    d = torch.from_numpy(words.view(np.int64).copy()).to(gpu)
    for method in _methods(L, k):
        _check(B, torch, d, L, k, cnt_e, pairs_e, method)


@pytest.mark.gpu
@pytest.mark.parametrize("L,k,wpr", [(12, 1, 3), (100, 7, 6)])
def test_threshold_row_padding(gpu, oracle, L, k, wpr):
    """wpr > W up to 128 nt: the padding words hold a nonzero pattern per row and are neither
    compared nor bucketed by the tiles or the pigeonhole form."""
    import torch
    import shortseq_amd.batch as B
    words, cnt_e, pairs_e = _case(L, k)
    n, W = words.shape
    assert W < wpr
    wide = np.zeros((n, wpr), dtype=np.uint64)
    wide[:, :W] = words
    wide[:, W:] = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    d = torch.from_numpy(wide.view(np.int64)).to(gpu)
    for method in ("tiles", "pigeonhole"):
        _check(B, torch, d, L, k, cnt_e, pairs_e, method)


@functools.lru_cache(maxsize=None)
def _repeats(L):
    """~300 rows with identical pairs and pairs at every position differing: 30 distinct reads nine
    times each, the complements of six of them (distance L; with the last byte aliased, where
    L % 32 != 0, L + 1 = P: those six reads end in 'C', an aliased byte reads as 'A'), and a few
    threshold-pool rows.  -> packed words, read-only."""
    import oracle
    rng = np.random.default_rng(L)
    base = oracle.gen_reads(77 + L, 0, 30, L).reshape(30, L).copy()
    base[:6, L - 1] = ord("C")
    comp = np.zeros(256, np.uint8)
    comp[np.frombuffer(b"ACGT", np.uint8)] = np.frombuffer(b"CGTA", np.uint8)
    far = comp[base[:6]]
    rows = [np.repeat(base, 9, axis=0), far]
    if L % 32:
        aliased = far.copy()
        aliased[:, L - 1] = ALIAS
        rows.append(aliased)
    rows.append(_threshold_pool(oracle, L, 2, 1, L)[:24])
    ascii = np.concatenate(rows)
    ascii = ascii[rng.permutation(len(ascii))]
    n = ascii.shape[0]
    words, rc, _ = oracle.encode_batch(np.ascontiguousarray(ascii).reshape(-1), n, L)
    assert rc == 0
    words = np.ascontiguousarray(words).reshape(n, -1)
    words.setflags(write=False)
    return words


U32MAX = 2**32 - 1


@pytest.mark.gpu
@pytest.mark.parametrize("L,k", [(8, 8), (8, 9), (31, 31), (31, 32), (32, 32), (100, 100), (100, 101),
                                 (127, 127), (127, 128), (128, 127), (128, 128), (128, 1000), (150, 151),
                                 (1024, 1024), (12, U32MAX), (128, U32MAX), (150, U32MAX)])
def test_max_dist_at_and_past_P(gpu, oracle, L, k):
    """max_dist at P - 1 (only a pair differing at every one of the P = min(L + 1, 32 W) compared
    positions is out), at P and past it, up to 2^32 - 1 (every pair, identical rows included, is
    in); the forced bucketing methods refuse 2^32 - 1 like any max_dist past their range."""
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd._native import NativeError
    words = _repeats(L)
    n, W = words.shape
    P = min(L + 1, 32 * W)
    cnt_e, pairs_e = _brute(oracle, words, n, L, k)
    if k >= P:
        assert len(pairs_e) == n * (n - 1) // 2
    else:
        assert n * (n - 1) // 2 - len(pairs_e) >= 54         # six far rows against nine copies each
    d = torch.from_numpy(words.view(np.int64).copy()).to(gpu)
    if k == U32MAX:
        for method in ("pigeonhole", "bucketed"):
            with pytest.raises(NativeError):
                B.hamming_all_pairs(d, L, k, method=method)
    for method in ("tiles", "auto"):
        cnt, pairs, total = B.hamming_all_pairs(d, L, k, max_pairs=len(pairs_e) + 10, method=method)
        assert total == len(pairs_e), method
        assert np.array_equal(cnt.cpu().numpy().astype(np.int64), cnt_e), method
        assert [tuple(int(x) for x in p) for p in pairs.cpu().numpy()] == pairs_e, method
        if k >= P:
            assert total == n * (n - 1) // 2 and bool((cnt == n - 1).all()), method
        cnt2, _, total2 = B.hamming_all_pairs(d, L, k, method=method)
        assert total2 == total and torch.equal(cnt2, cnt), method
