"""All-pairs thresholded hamming through method "bucketed" (SS_ALLPAIRS_BUCKETED): the pigeonhole rule
past 128 nt and past max_dist 15, where rows are read through bucket-ordered indices by a group of
lanes per row.  Expectations are the oracle's brute force over every pair; only the two large
agreement tests compare against method="tiles" (brute force at 40k reads is 8e8 oracle distances)."""
import functools
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _umis(oracle, n, L, U, seed):
    """n reads drawn from U distinct L-mers plus 1-2 substitution variants (a UMI-like pool)."""
    rng = np.random.default_rng(seed)
    base = oracle.gen_reads(seed, 0, U, L).reshape(U, L)
    pick = base[rng.integers(0, U, size=n)].copy()
    mut = rng.random(n) < 0.4
    pos = rng.integers(0, L, size=n)
    pick[mut, pos[mut]] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(mut.sum()))]
    return pick.reshape(-1)


@functools.lru_cache(maxsize=None)
def _case(L, n, k):
    """Packed words of a UMI-like pool (U = max(2, n // 20), 40 % one-substitution variants) and the
    brute-force counts / pairs; computed once per shape and shared (callers do not modify them)."""
    import oracle
    ascii = _umis(oracle, n, L, max(2, n // 20), 7 * L + n + k)
    words, rc, _ = oracle.encode_batch(ascii, n, L)
    assert rc == 0
    words = np.ascontiguousarray(words).reshape(n, -1)
    words.setflags(write=False)
    cnt, pairs = _brute(oracle, words, n, L, k)
    return words, cnt, pairs


def _check(B, torch, d, L, k, cnt_e, pairs_e, method="bucketed"):
    """Counts, sorted pairs, total, count-only and 3-pair truncation of one forced call."""
    cnt, pairs, total = B.hamming_all_pairs(d, L, k, max_pairs=len(pairs_e) + 10, method=method)
    assert total == len(pairs_e)
    assert np.array_equal(cnt.cpu().numpy().astype(np.int64), cnt_e)
    assert [tuple(int(x) for x in p) for p in pairs.cpu().numpy()] == pairs_e
    cnt2, _, total2 = B.hamming_all_pairs(d, L, k, method=method)
    assert total2 == total and torch.equal(cnt2, cnt)
    if total > 4:    # truncated: the total still counts every pair, the kept ones are real
        _, p3, total3 = B.hamming_all_pairs(d, L, k, counts=False, max_pairs=3, method=method)
        assert total3 == total and p3.shape[0] == 3
        kept = {tuple(int(x) for x in q) for q in p3.cpu().numpy()}
        assert len(kept) == 3 and kept <= set(pairs_e)


LONG_CASES = [
    (129, 900, 1),     # W = 5, odd wpr, the alias position in the last word
    (130, 800, 0),     # one segment: every bucket an exact-duplicate group
    (150, 1000, 3),    # the common case: 37-38-nt hashed segments crossing word edges
    (160, 700, 31),    # G = 32, 5-nt exact-value buckets, L a multiple of 32 (no alias position)
    (256, 600, 7),     # W = 8, segments exactly one word
    (257, 600, 4),     # W = 9, a one-position last word
    (500, 500, 12),    # W = 16
    (993, 300, 20),    # W = 32, one position in the last word
    (1023, 300, 9),    # W = 32 with an alias position
    (1024, 300, 31),   # W = 32, every lane's word live, G = 32
    (64, 900, 20),     # W <= 4, k >= 16: the long form on short rows
    (20, 1000, 16),    # W = 1, 17 segments of 1-2 nt
    (20, 300, 21),     # G = 22 over P = 21 positions: an empty segment (bucket 0) reports every pair
    (96, 1000, 5),     # the delegated path (the existing pigeonhole form)
]


@pytest.mark.gpu
@pytest.mark.parametrize("L,n,k", LONG_CASES)
def test_bucketed_against_brute_force(gpu, oracle, L, n, k):
    import torch
    import shortseq_amd.batch as B
    words, cnt_e, pairs_e = _case(L, n, k)
    d = torch.from_numpy(words.view(np.int64).copy()).to(gpu)
    _check(B, torch, d, L, k, cnt_e, pairs_e)
    if (L, n, k) == (96, 1000, 5):
        cnt_b, p_b, tot_b = B.hamming_all_pairs(d, L, k, max_pairs=len(pairs_e) + 10, method="bucketed")
        cnt_p, p_p, tot_p = B.hamming_all_pairs(d, L, k, max_pairs=len(pairs_e) + 10, method="pigeonhole")
        assert tot_b == tot_p and torch.equal(cnt_b, cnt_p) and torch.equal(p_b, p_p)


@pytest.mark.gpu
@pytest.mark.parametrize("wpr", [6, 8])
def test_bucketed_ignores_row_padding(gpu, oracle, wpr):
    """wpr > W: the padding words hold a nonzero pattern and are neither compared nor bucketed."""
    import torch
    import shortseq_amd.batch as B
    L, n, k = 150, 1000, 3
    words, cnt_e, pairs_e = _case(L, n, k)
    assert words.shape[1] == 5
    wide = np.zeros((n, wpr), dtype=np.uint64)
    wide[:, :5] = words
    wide[:, 5:] = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    d = torch.from_numpy(wide.view(np.int64)).to(gpu)
    _check(B, torch, d, L, k, cnt_e, pairs_e)


@pytest.mark.gpu
def test_bucketed_one_repeated_read(gpu, oracle):
    """One bucket run of length n in every segment; only segment 0 reports."""
    import torch
    import shortseq_amd.batch as B
    n, L, k = 3000, 150, 2
    ascii = np.tile(oracle.gen_reads(8, 0, 1, L), n)
    words, _, _ = oracle.encode_batch(ascii, n, L)
    d = torch.from_numpy(words.view(np.int64).reshape(n, -1)).to(gpu)
    cnt, _, total = B.hamming_all_pairs(d, L, k, method="bucketed")
    assert total == n * (n - 1) // 2
    assert bool((cnt == n - 1).all())


@pytest.mark.gpu
def test_bucketed_limits(gpu, oracle):
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd._native import NativeError
    L = 150
    ascii = oracle.gen_reads(3, 0, 2, L)
    words, _, _ = oracle.encode_batch(ascii, 2, L)
    words = words.reshape(2, -1)
    d = torch.from_numpy(words.view(np.int64)).to(gpu)
    with pytest.raises(NativeError):
        B.hamming_all_pairs(d, L, 32, method="bucketed")
    with pytest.raises(NativeError):
        B.hamming_all_pairs(d[:, :1].contiguous(), 20, 32, method="bucketed")
    # n = 0, 1: zero; n = 2: the one pair's verdict either way
    for m in (0, 1):
        cnt, pairs, total = B.hamming_all_pairs(d[:m], L, 3, max_pairs=4, method="bucketed")
        assert total == 0 and cnt.shape[0] == m and pairs.shape[0] == 0 and not bool(cnt.any())
    dist = int(oracle.hamming_ref_batch(words[1:], 1, L, words[0])[0])
    assert dist > 3
    for k, near in ((3, False), (31, dist <= 31), (0, False)):
        cnt, pairs, total = B.hamming_all_pairs(d, L, k, max_pairs=4, method="bucketed")
        assert total == int(near) and cnt.tolist() == [int(near)] * 2
        assert pairs.cpu().tolist() == ([[0, 1]] if near else [])
    same = d[:1].repeat(2, 1)
    cnt, pairs, total = B.hamming_all_pairs(same, L, 0, max_pairs=4, method="bucketed")
    assert total == 1 and cnt.tolist() == [1, 1] and pairs.cpu().tolist() == [[0, 1]]
    # "pigeonhole" keeps refusing what it refused
    with pytest.raises(NativeError):
        B.hamming_all_pairs(torch.zeros((10, 5), dtype=torch.int64, device=gpu), 130, 1, method="pigeonhole")


def _pair_set(pairs):
    p = pairs.cpu().numpy().astype(np.int64)
    return p[:, 0] * (1 << 32) + p[:, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("L,k,U", [(150, 3, 12_000), (250, 5, 12_000), (1024, 16, 8_000)])
def test_bucketed_methods_agree_large(gpu, oracle, L, k, U):
    """n = 40k (>= 2^15, where auto runs the long form's histogram): tiles, bucketed and auto give
    the same counts, totals and pair sets."""
    import torch
    import shortseq_amd.batch as B
    n = 40_000
    ascii = _umis(oracle, n, L, U, L + k)
    words, _, _ = oracle.encode_batch(ascii, n, L)
    d = torch.from_numpy(words.view(np.int64).reshape(n, -1)).to(gpu)
    cnt_t, _, tot_t = B.hamming_all_pairs(d, L, k, method="tiles")
    for m in ("bucketed", "auto"):
        cnt, _, tot = B.hamming_all_pairs(d, L, k, method=m)
        assert tot == tot_t and torch.equal(cnt, cnt_t), m
    if tot_t <= 2_000_000:
        _, p_t, _ = B.hamming_all_pairs(d, L, k, max_pairs=tot_t, counts=False, method="tiles")
        _, p_g, _ = B.hamming_all_pairs(d, L, k, max_pairs=tot_t, counts=False, method="bucketed")
        assert np.array_equal(_pair_set(p_t), _pair_set(p_g))
    assert tot_t > 0
    assert int(cnt_t.sum().item()) == 2 * tot_t


@pytest.mark.gpu
def test_auto_one_repeated_long_read(gpu, oracle):
    """40k copies of one 150-nt read through auto: the closed form, whichever method it picks."""
    import torch
    import shortseq_amd.batch as B
    n, L, k = 40_000, 150, 3
    ascii = np.tile(oracle.gen_reads(8, 0, 1, L), n)
    words, _, _ = oracle.encode_batch(ascii, n, L)
    d = torch.from_numpy(words.view(np.int64).reshape(n, -1)).to(gpu)
    cnt, _, total = B.hamming_all_pairs(d, L, k, method="auto")
    assert total == n * (n - 1) // 2
    assert bool((cnt == n - 1).all())


@pytest.mark.gpu
def test_auto_long_reads_is_capturable(gpu, oracle):
    """AUTO at n = 2^15, L = 150 (where the eager call runs the long form's histogram) on a stream under
    hipGraph capture stays on the tiles: it captures, replays and equals the eager result."""
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd._native import lib, check
    n, L, k = 1 << 15, 150, 3
    ascii = _umis(oracle, n, L, 8000, 23)
    words, _, _ = oracle.encode_batch(ascii, n, L)
    d = torch.from_numpy(words.view(np.int64).reshape(n, -1)).to(gpu)
    cnt_e, _, tot_e = B.hamming_all_pairs(d, L, k, method="auto")
    assert tot_e > 0
    cnt = torch.empty(n, dtype=torch.int32, device=gpu)
    tot = torch.empty(1, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize(gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream(gpu).cuda_stream
        check(lib().ss_hamming_all_pairs_ex(d.data_ptr(), n, L, d.shape[1], k, cnt.data_ptr(), 0, 0, tot.data_ptr(),
                                            B.ALL_PAIRS_METHODS["auto"], s), "captured all pairs")
    cnt.fill_(-1)
    g.replay()
    torch.cuda.synchronize(gpu)
    assert int(tot.item()) == tot_e and torch.equal(cnt, cnt_e)


FORM_SEQUENCE = [
    (12, 1, "pigeonhole"),     # one-word form
    (150, 3, "bucketed"),      # long form, 8 lanes per entry
    (40, 2, "pigeonhole"),     # W = 2 with row copies
    (20, 20, "bucketed"),      # long form at W = 1, k >= 16: 21 one-position segments (20 nt + the alias position)
    (12, 1, "pigeonhole"),     # the one-word form again
]


@functools.lru_cache(maxsize=None)
def _form_case(L, n, k):
    """n rows drawn from a pool of 40 random reads, each copied with 0 .. k + 1 substitutions at random
    positions (fixed seed), and their brute-force counts / sorted pairs (int64 [m, 2]); shared, callers
    do not modify them.  One-word rows (L <= 32, the table path) draw their substitutions from all eight
    valid bytes: an aliased last byte (\x01 \x03 \x07 \x14) sets the bit at position L, which the
    distance counts, so two 20-nt rows can be 21 apart and (L 20, k 20) does not hit every pair."""
    import oracle
    rng = np.random.default_rng(1000 * L + k)
    pool = oracle.gen_reads(1000 * L + k, 0, 40, L).reshape(40, L)
    rows = pool[rng.integers(0, 40, size=n)].copy()
    alphabet = np.frombuffer(b"ACGT\x01\x03\x07\x14" if L <= 32 else b"ACGT", np.uint8)
    nsub = rng.integers(0, k + 2, size=n)
    for i in np.flatnonzero(nsub):
        pos = rng.integers(0, L, size=nsub[i])
        rows[i, pos] = alphabet[rng.integers(0, alphabet.size, size=nsub[i])]
    words, rc, _ = oracle.encode_batch(rows.reshape(-1), n, L)
    assert rc == 0
    words = np.ascontiguousarray(words).reshape(n, -1)
    words.setflags(write=False)
    cnt = np.zeros(n, dtype=np.int64)
    pairs = []
    for i in range(n - 1):                       # _brute, with the pairs kept as arrays (up to 12.5 M of them)
        d = oracle.hamming_ref_batch(words[i + 1:], n - i - 1, L, words[i])
        js = np.flatnonzero(d <= k) + i + 1
        cnt[i] += js.size
        cnt[js] += 1
        pairs.append(np.stack([np.full(js.size, i, dtype=np.int64), js.astype(np.int64)], axis=1))
    return words, cnt, np.concatenate(pairs)


@pytest.mark.gpu
def test_forms_share_the_scratch_back_to_back(gpu, oracle):
    """The three pigeonhole forms through one driver and one per-device grow-only scratch, back to back
    in one process: the sequence at n = 300 (more than one 256-thread block, a partial last wave), then
    at n = 5000 (the scratch freed and regrown between forms).  Every call: counts, total and sorted
    pairs equal brute force (then count-only and a 3-pair truncation, as _check), on inputs whose
    brute-force total is neither 0 nor every pair."""
    import torch
    import shortseq_amd.batch as B
    for n in (300, 5000):
        for L, k, method in FORM_SEQUENCE:
            words, cnt_e, pairs_e = _form_case(L, n, k)
            m = pairs_e.shape[0]
            print(f"n {n} L {L} k {k} {method}: brute-force total {m} of {n * (n - 1) // 2}")
            assert 0 < m < n * (n - 1) // 2
            d = torch.from_numpy(words.view(np.int64).copy()).to(gpu)
            cnt, pairs, total = B.hamming_all_pairs(d, L, k, max_pairs=m + 10, method=method)
            assert total == m
            assert np.array_equal(cnt.cpu().numpy().astype(np.int64), cnt_e)
            assert np.array_equal(pairs.cpu().numpy().astype(np.int64), pairs_e)
            cnt2, _, total2 = B.hamming_all_pairs(d, L, k, method=method)
            assert total2 == total and torch.equal(cnt2, cnt)
            _, p3, total3 = B.hamming_all_pairs(d, L, k, counts=False, max_pairs=3, method=method)
            assert total3 == total and p3.shape[0] == 3
            key = pairs_e[:, 0] * n + pairs_e[:, 1]             # sorted: the brute force runs in (i, j) order
            k3 = p3.cpu().numpy().astype(np.int64)
            assert bool(np.isin(k3[:, 0] * n + k3[:, 1], key).all())
            assert len(np.unique(k3[:, 0] * n + k3[:, 1])) == 3


def test_method_table_and_header_constant():
    """The Python method table has the four names and matches the ABI header's ids."""
    import shortseq_amd.batch as B
    assert B.ALL_PAIRS_METHODS == {"auto": 0, "tiles": 1, "pigeonhole": 2, "bucketed": 3}
    with open(os.path.join(REPO, "include", "shortseq_amd.h")) as f:
        ids = dict(re.findall(r"#define SS_ALLPAIRS_(\w+) (\d+)u", f.read()))
    assert {k.lower(): int(v) for k, v in ids.items()} == B.ALL_PAIRS_METHODS
