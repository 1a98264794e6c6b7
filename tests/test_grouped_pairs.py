"""Grouped all-pairs hamming (ss_hamming_all_pairs_grouped / _ex, ss_host_hamming_all_pairs_grouped,
batch.hamming_all_pairs_grouped, batch.umi_cluster_grouped, umi.dedup_groups): the pair step of a UMI
dedup restricted to groups of consecutive rows.

Expected values come from a brute force written here on the packed words with numpy: per group and all
i < j, popcount(((x >> 1) | x) & 0x5555...) of x = a ^ b summed over the W compared words.  The library
is not used for them.  Inputs are built so that hits exist inside groups AND across group boundaries (a
parent sequence is shared by adjacent groups), and every case asserts from the brute force that it
exercises what it claims.  Every comparison is exact: counts, total and the sorted pair set.
"""
import ctypes as C

import numpy as np
import pytest

SS_EARG = -1
FILL = 0xDEADBEEF
GUARD = 8
U32_MAX = (1 << 32) - 1
LOW = np.uint64(0x5555555555555555)


def _W(L):
    return 1 if L <= 32 else (L + 31) // 32


def _P(L):
    """Compared positions: min(L + 1, 32 W)."""
    return min(L + 1, 32 * _W(L))


def _pack(codes):
    """2-bit codes [n, L] -> packed words [n, W]: nt j in word j // 32 at bits 2 (j % 32)."""
    n, L = codes.shape
    W = _W(L)
    full = np.zeros((n, 32 * W), dtype=np.uint64)
    full[:, :L] = codes
    sh = (np.uint64(2) * np.arange(32, dtype=np.uint64))[None, None, :]
    return np.ascontiguousarray(np.bitwise_or.reduce(full.reshape(n, W, 32) << sh, axis=2))


def _make(rng, sizes, L):
    """-> (words [n, W], offsets [len(sizes) + 1]).  A group is a few random parents and copies of them
    with 0, 1 and 2 substitutions in turn; its first parent is the previous group's last one, so hits
    exist across every boundary between nonempty groups."""
    rows, carry = [], None
    for g in sizes:
        if g == 0:
            continue
        parents = rng.integers(0, 4, size=(1 + g // 12, L))
        if carry is not None:
            parents[0] = carry
        carry = parents[-1].copy()
        grp = parents[np.arange(g) % parents.shape[0]].copy()
        for r in range(g):
            for p in rng.choice(L, size=min((r // parents.shape[0]) % 3, L), replace=False):
                grp[r, p] = (grp[r, p] + rng.integers(1, 4)) % 4
        rows.append(grp)
    codes = np.concatenate(rows) if rows else np.zeros((0, L), dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return _pack(codes), off


def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1, dtype=np.int64)


def _brute(words, off, k):
    """-> (counts int64 [n], pairs int64 [m, 2] sorted, total) over the compared words `words` [n, W]."""
    n = words.shape[0]
    cnt = np.zeros(n, dtype=np.int64)
    out = []
    for b, e in zip(off[:-1], off[1:]):
        b, e = int(b), int(e)
        if e - b < 2:
            continue
        X = words[b:e]
        x = X[:, None, :] ^ X[None, :, :]
        d = _popcount(((x >> np.uint64(1)) | x) & LOW).sum(axis=2)
        i, j = np.nonzero(np.triu(d <= k, 1))
        cnt[b:e] += np.bincount(i, minlength=e - b) + np.bincount(j, minlength=e - b)
        out.append(np.stack([i + b, j + b], axis=1))
    pairs = np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    return cnt, pairs.astype(np.int64), pairs.shape[0]


def _one(n):
    return np.array([0, n], dtype=np.int64)


def _pad(rng, words, wpr):
    """The rows at stride wpr, the padding words random bits."""
    n, W = words.shape
    out = rng.integers(0, 1 << 63, size=(n, wpr), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, wpr), dtype=np.uint64)
    out[:, :W] = words
    return np.ascontiguousarray(out)


def _sorted_pairs(p):
    p = p.astype(np.int64).reshape(-1, 2)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def _same(got, exp, what):
    cnt, pairs, total = got
    assert total == exp[2], (what, "total", total, exp[2])
    if cnt is not None:
        assert np.array_equal(cnt, exp[0]), (what, "counts", np.flatnonzero(cnt != exp[0])[:8])
    if pairs is not None:
        assert np.array_equal(_sorted_pairs(pairs), exp[1]), (what, "pairs")


# --------------------------------------------------------------------------------------------------
# CPU: ss_host_hamming_all_pairs_grouped
def _host(words, L, k, off, *, counts=True, max_pairs=None, n=None, wpr=None, ngroups=None, null=()):
    """-> (rc, counts u32 [n], pairs u32 [cap, 2], total); the outputs pre-filled with FILL."""
    from shortseq_amd._native import lib
    nrows = words.shape[0]
    cap = nrows * (nrows - 1) // 2 + 1 if max_pairs is None else max_pairs
    cnt = np.full(max(1, nrows), FILL, dtype=np.uint32)
    pairs = np.full((max(1, cap), 2), FILL, dtype=np.uint32)
    tot = np.full(1, FILL, dtype=np.uint64)
    o32 = np.ascontiguousarray(off, dtype=np.uint32)
    p = lambda name, a: None if name in null else a.ctypes.data      # noqa: E731
    rc = lib().ss_host_hamming_all_pairs_grouped(
        p("words", words), nrows if n is None else n, L, words.shape[1] if wpr is None else wpr, k, p("off", o32),
        len(off) - 1 if ngroups is None else ngroups, cnt.ctypes.data if counts else None,
        p("pairs", pairs) if cap else None, cap, p("npairs", tot))
    return rc, cnt[:nrows], pairs, int(tot[0])


def _host_ok(words, L, k, off, **kw):
    rc, cnt, pairs, total = _host(words, L, k, off, **kw)
    assert rc == 0
    return cnt.astype(np.int64), pairs[:total], total


HOST_SIZES = [0, 1, 2, 3, 17, 60, 0, 0, 3, 17, 2, 1, 17, 3, 17, 1, 2, 17, 3, 17, 0, 17, 0]      # 200 rows
HOST_L = (1, 12, 31, 32, 33, 64, 128, 129, 1024)


@pytest.mark.parametrize("L", HOST_L)
def test_host_matches_brute_force(L):
    rng = np.random.default_rng(100 + L)
    assert sum(HOST_SIZES) == 200
    words, off = _make(rng, HOST_SIZES, L)
    W = _W(L)
    # stride W + 2 with random padding words, and a garbage row on either side of the n rows passed
    padded = _pad(rng, np.concatenate([words[:1], words, words[:1]]), W + 2)
    padded[0], padded[-1] = padded[0] ^ np.uint64(0x1234567), ~padded[-1]
    inner = padded[1:-1]
    assert inner.ctypes.data == padded.ctypes.data + 8 * (W + 2)
    for k in (0, 1, 3):
        exp = _brute(words, off, k)
        everything = _brute(words, _one(200), k)[2]
        assert everything > exp[2] > 0, (L, k)              # hits inside groups, more across them
        cnt, pairs, total = _host_ok(inner, L, k, off)
        _same((cnt, pairs, total), exp, (L, k))
        assert np.array_equal(pairs.astype(np.int64), exp[1]), "host pairs come in ascending (i, j) order"


def test_host_alias_bit():
    """Bit 2 L of a one-word row (the table-path alias bit) counts as a position."""
    rng = np.random.default_rng(7)
    for L in (7, 12, 31):
        words, off = _make(rng, HOST_SIZES, L)
        plain = _brute(words, off, 1)
        words[0::3, 0] |= np.uint64(1 << (2 * L))
        exp = _brute(words, off, 1)
        assert 0 < exp[2] < plain[2]                        # the bit is seen: it separates some pairs
        _same(_host_ok(words, L, 1, off), exp, ("alias", L))
        _same(_host_ok(words, L, 0, off), _brute(words, off, 0), ("alias k = 0", L))


def test_host_max_pairs_and_null_outputs():
    rng = np.random.default_rng(8)
    words, off = _make(rng, HOST_SIZES, 12)
    exp = _brute(words, off, 1)
    assert exp[2] >= 64
    cap = exp[2] // 2
    rc, cnt, pairs, total = _host(words, 12, 1, off, max_pairs=cap)
    assert rc == 0 and total == exp[2] and np.array_equal(cnt, exp[0])
    got = {tuple(p) for p in pairs.tolist()}
    assert len(got) == cap and got <= {tuple(p) for p in exp[1].tolist()}       # cap distinct valid pairs
    rc, cnt, pairs, total = _host(words, 12, 1, off, counts=False)              # h_counts = NULL
    assert rc == 0 and (cnt == FILL).all()
    _same((None, pairs[:total], total), exp, "no counts")
    rc, cnt, pairs, total = _host(words, 12, 1, off, max_pairs=0)               # h_pairs = NULL
    assert rc == 0 and (pairs == FILL).all()
    _same((cnt.astype(np.int64), None, total), exp, "no pairs")


def test_host_argument_errors():
    rng = np.random.default_rng(9)
    L = 40
    words, off = _make(rng, [3, 0, 5, 2], L)
    bad_first, bad_dec, bad_last = off.copy(), off.copy(), off.copy()
    bad_first[0] = 1
    bad_dec[2] = 9
    bad_last[-1] = 9
    assert bad_dec[2] > bad_dec[3]
    cases = {
        "null words": dict(null=("words",)), "null offsets": dict(null=("off",)), "null npairs": dict(null=("npairs",)),
        "L = 0": dict(L=0), "L = 1025": dict(L=1025), "wpr < W": dict(wpr=1), "n = 2^32": dict(n=1 << 32),
        "no group": dict(ngroups=0), "off[0] != 0": dict(off=bad_first), "a decrease": dict(off=bad_dec),
        "off[ngroups] != n": dict(off=bad_last),
    }
    for name, kw in cases.items():
        rc, cnt, pairs, total = _host(words, kw.pop("L", L), 1, kw.pop("off", off), **kw)
        assert rc == SS_EARG, name
        assert (cnt == FILL).all() and (pairs == FILL).all() and total == FILL, name
    rc, cnt, pairs, total = _host(words, L, 1, off)
    assert rc == 0 and not (cnt == FILL).any()
    from shortseq_amd._native import lib
    tot = C.c_uint64(7)
    assert lib().ss_host_hamming_all_pairs_grouped(None, 0, L, 2, 1, None, 0, None, None, 0, C.byref(tot)) == 0
    assert tot.value == 0                                                         # n = 0, no group: zeroed
    assert lib().ss_hamming_all_pairs_grouped_ws_bytes(10 ** 6, 10 ** 5, 12) == 0    # no workspace


# --------------------------------------------------------------------------------------------------
# CPU: umi.dedup_groups
def _dedup_case(seed, ngroups=12):
    """{label: {ShortSeq: count}}: groups of 12-nt UMIs near a few parents (some shared by adjacent
    groups) with 40-nt reads mixed in, an empty counter, a one-key counter, and count ties."""
    import shortseq_amd as ssa
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def seqs(parents, m):
        out = parents[rng.integers(0, parents.shape[0], size=m)].copy()
        for r in range(m):
            for p in rng.choice(out.shape[1], size=r % 3, replace=False):
                out[r, p] = (out[r, p] + rng.integers(1, 4)) % 4
        return [acgt[s].tobytes().decode() for s in out]

    groups, carry = {}, rng.integers(0, 4, size=(1, 12))
    for g in range(ngroups):
        parents = np.concatenate([carry, rng.integers(0, 4, size=(2, 12))])
        carry = parents[-1:]
        strs = seqs(parents, int(rng.integers(2, 40))) + seqs(rng.integers(0, 4, size=(2, 40)), int(rng.integers(0, 9)))
        order = rng.permutation(len(strs))
        counter = {}
        for i in order:
            counter.setdefault(ssa.from_str(strs[i]), int(rng.integers(1, 4)) if i % 2 else 2)     # ties
        groups[("cell%d" % (g // 3), "gene%d" % g)] = counter
    groups[("empty", 0)] = {}
    groups[("single", 0)] = {ssa.from_str("ACGTACGTACGT"): 5}
    return groups


def _check_dedup_groups(groups, device):
    import shortseq_amd.umi as U
    shared = 0
    for method in ("directional", "cluster"):
        got = U.dedup_groups(groups, 1, method, device=device)
        assert list(got) == list(groups)
        for lab, counter in groups.items():
            exp = U.dedup(counter, 1, method, device="host")
            assert list(got[lab][0].items()) == list(exp[0].items()), (method, lab)
            assert list(got[lab][1].items()) == list(exp[1].items()), (method, lab)
            shared += len(exp[0]) < len(counter)
    assert shared >= 8                                      # clusters of more than one key exist
    return got


def test_dedup_groups_host():
    import shortseq_amd.umi as U
    groups = _dedup_case(21)
    lens = {len(k) for c in groups.values() for k in c}
    assert lens == {12, 40}
    _check_dedup_groups(groups, "host")
    assert U.dedup_groups({}, device="host") == {}
    with pytest.raises(ValueError):
        U.dedup_groups(groups, method="adjacency")


# --------------------------------------------------------------------------------------------------
# GPU
def _dev(gpu, a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(gpu)


def _gpu_call(gpu, words, L, k, off, *, counts=True, max_pairs=None, tiles_per_launch=None, null=(), n=None,
              ngroups=None):
    """ss_hamming_all_pairs_grouped (tiles_per_launch None) or _ex through ctypes, the outputs inside larger
    tensors whose guard elements must stay unchanged -> the status when nonzero, else (counts int64 [n] |
    None, the written pairs int64 [min(total, cap), 2] | None, total)."""
    import torch
    from shortseq_amd._native import lib
    nrows, wpr = words.shape
    cap = nrows * (nrows - 1) // 2 + 1 if max_pairs is None else max_pairs
    dw = _dev(gpu, words.reshape(-1), np.int64) if nrows else torch.zeros(1, dtype=torch.int64, device=gpu)
    doff = _dev(gpu, np.asarray(off, dtype=np.uint32), np.int32)
    cnt = torch.full((nrows + 2 * GUARD,), -7, dtype=torch.int32, device=gpu)
    pairs = torch.full((2 * cap + 2 * GUARD,), -7, dtype=torch.int32, device=gpu)
    tot = torch.full((1 + 2 * GUARD,), -7, dtype=torch.int64, device=gpu)
    ng = len(off) - 1 if ngroups is None else ngroups
    ws_bytes = int(lib().ss_hamming_all_pairs_grouped_ws_bytes(nrows, ng, L))
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=gpu)
    p = lambda name, t: None if name in null else t      # noqa: E731
    args = (p("words", dw.data_ptr()), nrows if n is None else n, L, wpr, k, p("off", doff.data_ptr()), ng,
            cnt[GUARD:].data_ptr() if counts else None, pairs[GUARD:].data_ptr() if cap else None, cap,
            p("npairs", tot[GUARD:].data_ptr()), ws.data_ptr() if ws_bytes else None, ws_bytes)
    s = torch.cuda.current_stream(gpu).cuda_stream
    if tiles_per_launch is None:
        rc = lib().ss_hamming_all_pairs_grouped(*args, s)
    else:
        rc = lib().ss_hamming_all_pairs_grouped_ex(*args, tiles_per_launch, s)
    torch.cuda.synchronize(gpu)
    for t, m in ((cnt, nrows), (pairs, 2 * cap), (tot, 1)):
        assert bool((t[:GUARD] == -7).all()) and bool((t[GUARD + m:] == -7).all()), "a guard element was written"
    if rc:
        assert all(bool((t == -7).all()) for t in (cnt, pairs, tot)), "outputs written by a refused call"
        return rc
    total = int(tot[GUARD].item())
    if not counts:
        assert bool((cnt == -7).all())
    m = min(total, cap)
    assert bool((pairs[GUARD + 2 * m:] == -7).all()), "a pair slot past the total was written"
    got_c = cnt[GUARD:GUARD + nrows].cpu().numpy().view(np.uint32).astype(np.int64) if counts else None
    got_p = pairs[GUARD:GUARD + 2 * m].cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2) if cap else None
    return got_c, got_p, total


def _tile():
    import shortseq_amd.batch as B
    return B.GROUPED_ROW_TILE


def _layouts(T):
    """name -> (group sizes, whether in-group pairs exist)."""
    return {
        "no rows, no groups": ([], False),
        "no rows, empty groups": ([0, 0, 0], False),
        "one group of 1": ([1], False),
        "T groups of 1": ([1] * T, False),
        "T/2 groups of 2": ([2] * (T // 2), True),
        "a group of exactly T": ([T], True),
        "a group of T + 1": ([T + 1], True),
        "a group over the tile edge, T - 3 .. T + 5": ([T - 3, 8, 20], True),
        "a group of 2 T + 77 from mid-tile": ([100, 2 * T + 77, 30], True),
        "a final partial tile": ([40, T, 3, 5], True),
        "empty groups at the front, the middle and the end": ([0, 0, 50, 0, 0, 70, T, 0, 9, 0, 0], True),
    }


@pytest.fixture(scope="module")
def geometry():
    """layout name -> (words, offsets, brute force at k = 1, ungrouped total), computed once."""
    T = 256
    rng = np.random.default_rng(600)
    out = {}
    for name, (sizes, _hits) in _layouts(T).items():
        words, off = _make(rng, sizes, 12)
        out[name] = (words, off, _brute(words, off, 1), _brute(words, _one(words.shape[0]), 1)[2])
    return out


@pytest.mark.gpu
def test_gpu_tile_geometry(gpu, geometry):
    T = _tile()
    assert T == 256, "the layouts above are written for the kernel's row tile"
    for name, (sizes, hits) in _layouts(T).items():
        words, off, exp, everything = geometry[name]
        n = words.shape[0]
        assert n == sum(sizes)
        if hits:
            assert everything > exp[2] > 0 or len([g for g in sizes if g]) == 1 and everything == exp[2] > 0, name
        else:
            assert exp[2] == 0 and (n < 2 or everything > 0), name
        if name.startswith("a group of 2 T + 77"):
            assert off[1] % T and off[2] - off[1] == 2 * T + 77 and (off[2] - 1) // T - off[1] // T == 2    # three tiles
        if name.startswith("a group over"):
            assert off[1] == T - 3 and off[2] == T + 5
        _same(_gpu_call(gpu, words, 12, 1, off), exp, name)
        _same(_gpu_call(gpu, words, 12, 1, off, tiles_per_launch=1), exp, (name, "one tile per launch"))
        _same(_gpu_call(gpu, words, 12, 1, off, tiles_per_launch=2), exp, (name, "two tiles per launch"))


@pytest.mark.gpu
def test_gpu_no_pair_across_a_boundary(gpu):
    """Identical rows on both sides of every boundary, inside a tile and at tile edges."""
    T = _tile()
    rng = np.random.default_rng(601)
    sizes = [5, 7, T - 12, 3, T - 3, T, 2, 9]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert off[3] == T and off[5] == 2 * T and off[6] == 3 * T              # boundaries at tile edges
    n = int(off[-1])
    words = _pack(rng.integers(0, 4, size=(n, 12)))
    for b in off[1:-1]:
        words[b - 1] = words[b] = words[int(b) - 2]                          # b - 2, b - 1 | b alike
    exp = _brute(words, off, 0)
    one = _brute(words, _one(n), 0)
    cross = {(int(b) - 1, int(b)) for b in off[1:-1]}
    assert cross <= {tuple(p) for p in one[1].tolist()} and not cross & {tuple(p) for p in exp[1].tolist()}
    assert exp[2] >= len(sizes) - 1
    got = _gpu_call(gpu, words, 12, 0, off)
    _same(got, exp, "grouped")
    assert not cross & {tuple(p) for p in got[1].tolist()}
    got = _gpu_call(gpu, words, 12, 0, _one(n))
    _same(got, one, "the same rows as one group")
    assert cross <= {tuple(p) for p in got[1].tolist()}


GPU_SIZES = [0, 1, 2, 3, 17, 60, 0, 200, 3, 17, 2, 1, 130, 3, 17, 1, 2, 17, 3, 100, 17, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 31, 32, 33, 64, 96, 128, 129, 512, 1024])
def test_gpu_lengths_and_layouts(gpu, L):
    rng = np.random.default_rng(700 + L)
    words, off = _make(rng, GPU_SIZES, L)
    n, W = words.shape
    assert 550 <= n <= 650
    all_in_group = sum(g * (g - 1) // 2 for g in GPU_SIZES)
    for extra in (0, 1):
        padded = _pad(rng, words, W + extra)
        for k in (0, 1, _P(L), U32_MAX):
            exp = _brute(words, off, k)
            everything = _brute(words, _one(n), k)[2]
            assert everything > exp[2] > 0, (L, k)
            if k >= _P(L):
                assert exp[2] == all_in_group
            _same(_gpu_call(gpu, padded, L, k, off), exp, (L, extra, k))


@pytest.mark.gpu
def test_gpu_alias_bit(gpu):
    rng = np.random.default_rng(701)
    for L in (7, 12, 31):
        words, off = _make(rng, GPU_SIZES, L)
        plain = _brute(words, off, 1)
        words[0::3, 0] |= np.uint64(1 << (2 * L))
        exp = _brute(words, off, 1)
        assert 0 < exp[2] < plain[2]
        _same(_gpu_call(gpu, words, L, 1, off), exp, ("alias", L))


@pytest.mark.gpu
def test_gpu_one_group_equals_plain_call(gpu):
    import torch
    import shortseq_amd.batch as B
    rng = np.random.default_rng(702)
    words, _ = _make(rng, [250] * 4, 12)
    n = 1000
    exp = _brute(words, _one(n), 1)
    assert exp[2] > 0
    got = _gpu_call(gpu, words, 12, 1, _one(n))
    _same(got, exp, "one group")
    cnt, pairs, total = B.hamming_all_pairs(torch.from_numpy(words.view(np.int64)).to(gpu), 12, 1, max_pairs=exp[2] + 1,
                                            method="tiles")
    assert total == got[2] and np.array_equal(cnt.cpu().numpy().astype(np.int64), got[0])
    assert np.array_equal(pairs.cpu().numpy().astype(np.int64), _sorted_pairs(got[1]))


@pytest.mark.gpu
def test_gpu_max_pairs_null_outputs_and_arguments(gpu):
    rng = np.random.default_rng(703)
    L = 12
    words, off = _make(rng, GPU_SIZES, L)
    exp = _brute(words, off, 1)
    valid = {tuple(p) for p in exp[1].tolist()}
    assert exp[2] >= 64
    cap = exp[2] // 2
    cnt, pairs, total = _gpu_call(gpu, words, L, 1, off, max_pairs=cap)
    assert total == exp[2] and np.array_equal(cnt, exp[0]) and pairs.shape[0] == cap
    got = {tuple(p) for p in pairs.tolist()}
    assert len(got) == cap and got <= valid                  # distinct, valid, in-group, i < j
    cnt, pairs, total = _gpu_call(gpu, words, L, 1, off, max_pairs=0)                  # counts only
    assert pairs is None
    _same((cnt, None, total), exp, "counts only")
    cnt, pairs, total = _gpu_call(gpu, words, L, 1, off, counts=False)                 # d_counts = NULL
    assert cnt is None
    _same((None, pairs, total), exp, "pairs only")
    cnt, pairs, total = _gpu_call(gpu, words, L, 1, off, counts=False, max_pairs=0)    # the total alone
    assert total == exp[2]
    # no workspace is needed: 0 bytes asked for, so none is too small, and d_ws = NULL (passed above) is fine
    from shortseq_amd._native import lib
    assert lib().ss_hamming_all_pairs_grouped_ws_bytes(words.shape[0], len(off) - 1, L) == 0
    for name, kw in {"null words": dict(null=("words",)), "null offsets": dict(null=("off",)),
                     "null npairs": dict(null=("npairs",)), "no group": dict(ngroups=0), "n = 2^32": dict(n=1 << 32)}.items():
        assert _gpu_call(gpu, words, L, 1, off, **kw) == SS_EARG, name
    assert _gpu_call(gpu, words, 0, 1, off) == SS_EARG
    assert _gpu_call(gpu, words, 1025, 1, off) == SS_EARG
    assert _gpu_call(gpu, words, 33, 1, off) == SS_EARG                                # wpr 1 < W = 2
    _same(_gpu_call(gpu, words, L, 1, off), exp, "after the refused calls")


@pytest.mark.gpu
def test_gpu_malformed_offsets_stay_in_bounds(gpu):
    """A decreasing entry, and a last entry above n: not detected on the device, the outputs unspecified,
    but every end is clamped to n and an end <= i means no partners (k_gp_pairs / gp_row_end read
    off[1 .. ngroups] only and write row indices below n), so the call returns, the guards hold, every
    written index is below n, and the next well-formed call is right."""
    rng = np.random.default_rng(704)
    L = 12
    words, off = _make(rng, [100, 200, 150, 250, 120], L)
    n = words.shape[0]
    exp = _brute(words, off, 1)
    dec, high = off.copy(), off.copy()
    dec[2] = 50
    high[-1] = n + 1000
    assert dec[2] < dec[1] and high[-1] > n
    for bad in (dec, high):
        cnt, pairs, total = _gpu_call(gpu, words, L, 1, bad)
        assert pairs.size == 0 or (0 <= pairs.min() and pairs.max() < n)
        _same(_gpu_call(gpu, words, L, 1, off), exp, "the next well-formed call")


@pytest.mark.gpu
def test_gpu_graph_capture(gpu):
    """One call captured on a single stream and replayed equals the eager call."""
    import torch
    from shortseq_amd._native import check, lib
    rng = np.random.default_rng(705)
    L = 12
    words, off = _make(rng, GPU_SIZES * 3, L)
    n = words.shape[0]
    exp = _brute(words, off, 1)
    assert exp[2] > 0
    dw = _dev(gpu, words.reshape(-1), np.int64)
    doff = _dev(gpu, off.astype(np.uint32), np.int32)
    cap = exp[2] + 5
    cnt = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    pairs = torch.full((2 * cap,), -7, dtype=torch.int32, device=gpu)
    tot = torch.full((1,), -7, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize(gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream(gpu).cuda_stream
        check(lib().ss_hamming_all_pairs_grouped(dw.data_ptr(), n, L, 1, 1, doff.data_ptr(), len(off) - 1, cnt.data_ptr(),
                                                 pairs.data_ptr(), cap, tot.data_ptr(), None, 0, s), "captured grouped pairs")
    for t in (cnt, pairs, tot):
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize(gpu)
    total = int(tot.item())
    got = (cnt.cpu().numpy().astype(np.int64), pairs[:2 * min(total, cap)].cpu().numpy().astype(np.int64), total)
    _same(got, exp, "replay")
    _same(_gpu_call(gpu, words, L, 1, off), exp, "eager")


@pytest.mark.gpu
def test_batch_umi_cluster_grouped(gpu):
    import torch
    import shortseq_amd.batch as B
    rng = np.random.default_rng(706)
    L = 12
    sizes = [int(x) for x in rng.integers(1, 301, size=40)]
    sizes[3], sizes[17] = 1, 300
    words, off = _make(rng, sizes, L)
    n = words.shape[0]
    counts = rng.integers(1, 4, size=n).astype(np.int64)                                # ties everywhere
    exp = _brute(words, off, 1)
    assert _brute(words, _one(n), 1)[2] > exp[2] > 0
    dw = torch.from_numpy(words.view(np.int64)).to(gpu)
    dc = torch.from_numpy(counts).to(gpu)
    cnt, pairs, total = B.hamming_all_pairs_grouped(dw, L, 1, off.tolist(), max_pairs=exp[2] + 1)
    assert pairs.dtype == torch.int32 and cnt.dtype == torch.int32
    assert total == exp[2] and np.array_equal(cnt.cpu().numpy(), exp[0])
    assert np.array_equal(pairs.cpu().numpy().astype(np.int64), exp[1])                 # sorted
    doff = torch.from_numpy(off).to(gpu)
    for method in ("directional", "cluster"):
        rep, reps, csizes, sums, _rounds, tot = B.umi_cluster_grouped(dw, L, 1, doff, dc, method, max_pairs_hint=16)
        assert tot == exp[2]                                                            # (the buffer grew once)
        want = np.arange(n)
        for b, e in zip(off[:-1].tolist(), off[1:].tolist()):
            want[b:e] = B.umi_cluster(dw[b:e].contiguous(), L, 1, dc[b:e].contiguous(), method)[0].cpu().numpy() + b
        rep = rep.cpu().numpy()
        assert np.array_equal(rep, want), method
        assert (np.bincount(rep, minlength=n) > 1).any()
        reps = reps.cpu().numpy()
        assert sorted(reps.tolist()) == np.unique(rep).tolist()
        assert np.array_equal(csizes.cpu().numpy(), np.bincount(rep, minlength=n)[reps])
        assert np.array_equal(sums.cpu().numpy(), np.bincount(rep, weights=counts, minlength=n).astype(np.int64)[reps])
        grp = torch.bucketize(torch.from_numpy(reps).to(gpu), doff[1:], right=True).cpu().numpy()
        assert np.array_equal(grp, np.searchsorted(off[1:], reps, side="right"))
        # no cluster crosses a group: every row's representative lies in the row's own group
        assert np.array_equal(np.searchsorted(off[1:], rep, side="right"), np.searchsorted(off[1:], np.arange(n), side="right"))
    for bad in ([1] + off.tolist()[1:], off.tolist()[:-1] + [n + 1], off.tolist()[:2] + [0] + off.tolist()[3:], []):
        with pytest.raises(ValueError):
            B.hamming_all_pairs_grouped(dw, L, 1, bad)


@pytest.mark.gpu
def test_dedup_groups_gpu_equals_host(gpu):
    import shortseq_amd.umi as U
    groups = _dedup_case(21)
    dev = _check_dedup_groups(groups, "gpu")
    host = U.dedup_groups(groups, 1, "cluster", device="host")
    assert list(dev) == list(host)
    for lab in host:
        assert list(dev[lab][0].items()) == list(host[lab][0].items())
        assert list(dev[lab][1].items()) == list(host[lab][1].items())
