"""ss_hamming_all_pairs_ex where its other tests do not look: row counts at the edges of every tile,
block and LDS chunk (with real all-"A" rows next to the padding), the pigeonhole forms at their
block, lane-group, nbmax and scan-tile steps, dense batches whose full pair lists run through the
broadcast tile walk of k_pig_pairs and the waves' hit buffers past kPairBuf, the pair capacity at,
below and inside a flush run, and outputs pre-filled with garbage on every path that zeroes them.

Every device call goes through _raw: the outputs lie inside larger tensors, everything pre-filled with
-7, and the guards, the slots past the kept pairs, the total, the counts and the kept pairs are checked
there.  Expectations are the oracle's brute force over every pair (allpairs_shapes.brute); the two
n = 2^15 batches of one repeated read use the closed form.  The tests without the gpu mark build every
case and prove, on the oracle alone, that the inputs have what the device tests rely on."""
import numpy as np
import pytest

import allpairs_shapes as S

GUARD = 8
FILL = -7


def _raw(gpu, words, L, k, method, cap, ref, *, counts=True, dw=None):
    """One ss_hamming_all_pairs_ex call through ctypes.  d_counts (n), d_pairs (2 cap) and d_npairs
    (1) lie inside larger tensors, GUARD elements on both sides, everything pre-filled with FILL;
    d_pairs is null when cap = 0, d_counts when not counts.  ref = (counts, sorted keys | None, total)
    of the reference.  Asserts: the guards and every pair slot at or past min(total, cap) unchanged;
    total and counts equal the reference's; the kept pairs are distinct, expected, i < j < n, and
    the whole expected set when cap >= total.  -> (counts int64 [n] | None, sorted kept keys, total)."""
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd._native import lib, check
    cnt_e, keys_e, total_e = ref
    n, wpr = words.shape
    if dw is None:
        dw = torch.from_numpy(words.view(np.int64).copy()).to(gpu) if n else torch.zeros(1, dtype=torch.int64, device=gpu)
    cnt = torch.full((n + 2 * GUARD,), FILL, dtype=torch.int32, device=gpu)
    pairs = torch.full((2 * cap + 2 * GUARD,), FILL, dtype=torch.int32, device=gpu)
    tot = torch.full((1 + 2 * GUARD,), FILL, dtype=torch.int64, device=gpu)
    rc = lib().ss_hamming_all_pairs_ex(dw.data_ptr(), n, L, wpr, k, cnt[GUARD:].data_ptr() if counts else None,
                                       pairs[GUARD:].data_ptr() if cap else None, cap, tot[GUARD:].data_ptr(),
                                       B.ALL_PAIRS_METHODS[method], torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    check(rc, f"ss_hamming_all_pairs_ex {method}")
    what = (method, n, L, k, cap, counts)
    for t, m in ((cnt, n), (pairs, 2 * cap), (tot, 1)):
        assert bool((t[:GUARD] == FILL).all()) and bool((t[GUARD + m:] == FILL).all()), ("a guard element was written", what)
    total = int(tot[GUARD].item())
    assert total == total_e, what
    m = min(total, cap)
    assert bool((pairs[GUARD + 2 * m:] == FILL).all()), ("a pair slot past min(total, cap) was written", what)
    got_c = None
    if counts:
        got_c = cnt[GUARD:GUARD + n].cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(got_c, cnt_e), what
    else:
        assert bool((cnt == FILL).all()), what
    p = pairs[GUARD:GUARD + 2 * m].cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2)
    assert bool((p[:, 0] < p[:, 1]).all()) and bool((p[:, 1] < n).all()), ("a kept pair is not i < j < n", what)
    keys = np.sort((p[:, 0] << 32) | p[:, 1])
    assert bool((np.diff(keys) > 0).all()), ("a pair was kept twice", what)
    if cap:
        if cap >= total:
            assert np.array_equal(keys, keys_e), what
        else:
            at = np.minimum(np.searchsorted(keys_e, keys), len(keys_e) - 1)
            assert np.array_equal(keys_e[at], keys), ("a kept pair is not an expected pair", what)
    return got_c, keys, total


def _ref(cnt_keys):
    cnt, keys = cnt_keys
    return cnt, keys, len(keys)


# ---- without a device: the inputs have what the device tests rely on --------------------------------
def test_shapes_match_the_tile_table():
    """tile_rows / chunk_cols restate the launchers: the S of every family and the one family with
    two LDS chunks per tile."""
    want = {7: 1, 12: 2, 20: 3, 31: 4, 32: 4, 33: 6, 64: 8, 65: 12, 128: 16}
    for L, (family, rows) in S.TILE_FAMILIES.items():
        assert S.tile_rows(L) == rows, L
        if L in want:
            assert S.mfma_ks(S.shape(L)[1]) == want[L] and family == f"mfma-ks{want[L]}"
    assert [S.chunk_cols(L) for L in (129, 300, 1000)] == [256, 256, 128]
    assert [S.lane_group(L) for _, L, _, _ in S.PIG_FORMS[7:]] == [4, 8, 16, 32]
    assert max(n for _, n in S.TILE_CASES) == 2049 and len(set(S.TILE_CASES)) == len(S.TILE_CASES)


@pytest.mark.parametrize("L", list(S.TILE_FAMILIES))
def test_tile_edge_rows_are_paired(oracle, L):
    """Per n: row 0, row n - 1 and the rows on either side of a tile (and chunk) edge are all-"A"
    rows (packed word 0: at least two of them, row n - 1 among them), each in at least one expected
    pair at k = 0 and at the small k; at k = 2^32 - 1 every pair is expected."""
    rows = S.TILE_FAMILIES[L][1]
    for n in S.tile_ns(L):
        words, edges, ref = S.tile_case(L, n)
        assert words.shape[0] == n
        if n < 2:
            assert all(len(ref[k][1]) == 0 for k in ref)
            continue
        assert {0, n - 1} <= set(edges) and len(edges) >= 2
        assert set(edges) >= {x for x in (rows - 1, rows, 2 * rows - 1, 2 * rows) if x < n}
        assert not words[edges].any(), "an edge row is not all A"
        for k in (0, S.small_k(L)):
            assert bool((ref[k][0][edges] >= 1).all()), (n, k)
        assert len(ref[S.U32MAX][1]) == n * (n - 1) // 2 and bool((ref[S.U32MAX][0] == n - 1).all())
        if n > 300:         # the pool: some pairs, not every pair
            assert len(ref[0][1]) < len(ref[S.small_k(L)][1]) < n * (n - 1) // 2


@pytest.mark.parametrize("form,L,k,method", S.PIG_FORMS)
def test_pig_cases_build(oracle, form, L, k, method):
    """Every row count of the form builds, with pairs to find from 63 rows on; the forced method is the
    form the id names."""
    W = S.shape(L)[0]
    assert (method == "pigeonhole") == (W <= 4 and k <= 15)
    assert form.startswith("word") == S.is_word_form(L, k)
    ns = S.pig_ns(form, L)
    if form.startswith("long"):
        e = 256 // S.lane_group(L)
        assert {e - 1, e, e + 1} <= set(ns)
    assert S.nbmax(1024) == 10 and S.nbmax(1025) == 11
    for n in ns:
        words, (cnt, keys) = S.pig_case(L, k, n)
        assert words.shape[0] == n and cnt.sum() == 2 * len(keys)
        if n >= 63:
            assert len(keys) > 0
        if n >= 63 or (k >= L and n >= 3):      # not every pair: the compare decides
            assert len(keys) < n * (n - 1) // 2


@pytest.mark.parametrize("form,L,k,method", S.PIG_TWO_TILES)
def test_two_scan_tiles(oracle, form, L, k, method):
    """n = 4097: nbmax = 13, some segment has nb = 13 bits (two scan tiles of kPigTile buckets) and
    rows fall into buckets of both tiles."""
    words, (cnt, keys) = S.two_tile_case(L, k)
    n = words.shape[0]
    assert n == S.kPigTile + 1 and S.nbmax(n) == 13 and len(keys) > 0
    b = S.split(L, k)
    vals = S.segment_values(words, L, k)
    both = False
    for g in range(k + 1):
        length = b[g + 1] - b[g]
        nb = min(2 * length, 13)
        if nb < 13:
            continue
        tiles = {S.bucket(v, length, nb, 2 * length <= 13, form == "word") // S.kPigTile for v in vals[g]}
        assert tiles <= {0, 1}
        both = both or tiles == {0, 1}
    assert both


@pytest.mark.parametrize("kind,L,arg", sorted({(kind, L, arg) for kind, L, _, arg in S.DENSE_CASES}))
def test_dense_conditions(oracle, kind, L, arg):
    """On the generators alone.  (a) In the one-word cases some bucket run of some segment is >= 257
    rows (more rows than that share one segment value), which sends a wave into the broadcast tile
    walk; the 65-row batch of one read cannot and is the lane walk's dense case.  (b) Some aligned
    run of 64 bucket-ordered entries has more than kPairBuf expected hits: a duplicate group of c >= 64
    rows suffices, because its c (c - 1) / 2 pairs all belong to segment 0 (the first equal segment
    of identical rows), whose n entries are ceil(n / 64) aligned runs, so one run reports at least
    c (c - 1) / 2 / ceil(n / 64) of them."""
    ks = sorted({k for kd, LL, k, a in S.DENSE_CASES if (kd, LL, a) == (kind, L, arg)})
    words = S.encode(oracle, S.dense_ascii(kind, L, arg))
    n = words.shape[0]
    assert n <= 1500
    for k in ks:
        if S.is_word_form(L, k) and n > S.kPigTileWalk:
            assert S.longest_equal_segment_run(words, L, k) >= S.kPigTileWalk + 1, k
    c = S.largest_duplicate_group(words)
    assert c >= 64 and c * (c - 1) // 2 > S.kPairBuf * -(-n // 64)
    if kind == "heavy":
        assert sorted(np.unique(words, axis=0, return_counts=True)[1].tolist())[-3:] == [200, 300, 400]
        for k in ks:
            _, (cnt, keys) = S.dense_case(kind, L, k, arg)
            near = 400 * 399 // 2 + 300 * 299 // 2 + 200 * 199 // 2 + 400 * 300 + 400 * 200
            assert len(keys) >= near + (300 * 200 if k >= 2 else 0)
            assert len(keys) <= 1_200_000
    if kind == "ladder":
        sizes = sorted(np.unique(words, axis=0, return_counts=True)[1].tolist())
        assert sizes == S.LADDER


@pytest.mark.parametrize("batch,L,k", sorted({(b, L, k) for b, L, k, _ in S.CAP_CASES}))
def test_capacity_batches(oracle, batch, L, k):
    """The totals leave room for every capacity of the list, all distinct."""
    _, (cnt, keys) = S.dense_case(batch, L, k, 0)
    caps = _caps(len(keys))
    assert len(set(caps)) == len(caps) == 9 and len(keys) > 2 * S.kPairBuf + 100


def _caps(total):
    inside = (total - 1) // S.kPairBuf * S.kPairBuf + 100     # inside a wave's flush run
    if inside >= total:
        inside -= S.kPairBuf
    return [1, 2, S.kPairBuf - 1, S.kPairBuf, S.kPairBuf + 1, inside, total - 1, total, total + 1]


# ---- on the device --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L,n", S.TILE_CASES)
def test_tile_row_counts(gpu, oracle, L, n):
    """method="tiles" at the edges of the family's tile (S - 1, S, S + 1, 2 S + 1), of the 32-column
    blocks and of the WT 32 chunk, at k = 0, a small k and 2^32 - 1 (every pair a hit: only the index
    check keeps the padding out, and the all-"A" edge rows look like it)."""
    words, _, ref = S.tile_case(L, n)
    for k in (0, S.small_k(L), S.U32MAX):
        _raw(gpu, words, L, k, "tiles", len(ref[k][1]) + 10, _ref(ref[k]))
    _raw(gpu, words, L, S.small_k(L), "tiles", 0, _ref(ref[S.small_k(L)]))


@pytest.mark.gpu
@pytest.mark.parametrize("form,L,k,method,n", S.PIG_CASES)
def test_pig_row_counts(gpu, oracle, form, L, k, method, n):
    """The forced pigeonhole forms at wave, block, lane-group and nbmax steps, against brute force."""
    words, ck = S.pig_case(L, k, n)
    _raw(gpu, words, L, k, method, len(ck[1]) + 10, _ref(ck))
    _raw(gpu, words, L, k, method, 0, _ref(ck))


@pytest.mark.gpu
@pytest.mark.parametrize("form,L,k,method", S.PIG_TWO_TILES)
def test_pig_two_scan_tiles(gpu, oracle, form, L, k, method):
    """n = 4097: the second scan tile of k_pig_tile / k_pig_apply, against brute force."""
    words, ck = S.two_tile_case(L, k)
    _raw(gpu, words, L, k, method, len(ck[1]) + 10, _ref(ck))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,L,k,arg", S.DENSE_CASES)
def test_dense_pair_lists(gpu, oracle, kind, L, k, arg):
    """Dense batches with the full pair list compared, every forced method that serves (L, k) and the
    tiles."""
    words, ck = S.dense_case(kind, L, k, arg)
    for method in S.methods(L, k):
        _raw(gpu, words, L, k, method, len(ck[1]) + 10, _ref(ck))


@pytest.mark.gpu
@pytest.mark.parametrize("batch,L,k,method", S.CAP_CASES)
def test_capacity(gpu, oracle, batch, L, k, method):
    """Capacities 1, 2, around kPairBuf, inside a flush run and around the total: exactly min(total,
    cap) distinct expected pairs, nothing past them, total and counts unaffected; the same without
    d_counts; and count-only."""
    import torch
    words, ck = S.dense_case(batch, L, k, 0)
    dw = torch.from_numpy(words.view(np.int64).copy()).to(gpu)
    for cap in _caps(len(ck[1])):
        for counts in (True, False):
            _, keys, _ = _raw(gpu, words, L, k, method, cap, _ref(ck), counts=counts, dw=dw)
            assert len(keys) == min(cap, len(ck[1]))
    _raw(gpu, words, L, k, method, 0, _ref(ck), counts=False, dw=dw)
    _raw(gpu, words, L, k, method, 0, _ref(ck), dw=dw)


@pytest.mark.gpu
@pytest.mark.parametrize("L,k", [(12, 1), (150, 3)])
def test_auto_hands_over_after_histogram(gpu, oracle, L, k):
    """2^15 copies of one read: AUTO builds the histogram (whose kernel zeroes the outputs), then
    gives the batch to the tiles.  Outputs pre-filled; the closed form."""
    n = 1 << 15
    words = S.encode(oracle, np.tile(oracle.gen_reads(8, 0, 1, L).reshape(1, L), (n, 1)))
    ref = (np.full(n, n - 1, dtype=np.int64), None, n * (n - 1) // 2)
    _raw(gpu, words, L, k, "auto", 0, ref)
    _raw(gpu, words, L, k, "auto", 0, ref, counts=False)
