"""UMI clustering, the `adjacency` method (SS_CLUSTER_ADJACENCY through ss_cluster_pairs /
ss_host_cluster_pairs, batch.cluster_pairs / umi_cluster / umi_cluster_grouped, umi.dedup).

The reference here is a literal restatement of UMI-tools' `_get_best_min_account` and
`_group_adjacency`: adjacency sets, BFS components in count order, per component the shortest
count-ordered prefix whose nodes and their neighbours cover it (the covered set is kept incrementally,
which changes nothing but the time), then the walk over those leads with `observed`.  It knows nothing
of the cover / thr formulation the library uses.  Ties are broken by index (a stable sort over
ascending indices).  Every comparison is exact on rep, the representatives in rank order, sizes, sums
and the cluster count.
"""
import ctypes as C
from collections import deque

import numpy as np
import pytest

COUNT_POOL = (1, 1, 1, 2, 3, 4, 7, 8, 15, 100)
ADJACENCY = 3
SS_EARG = -1


# --------------------------------------------------------------------------------------------------
# the reference: UMI-tools, restated
def _components(n, adj, cnt):
    found, components = set(), []
    for node in sorted(range(n), key=lambda v: cnt[v], reverse=True):      # stable: ties by index
        if node in found:
            continue
        seen, queue = {node}, deque([node])
        while queue:
            for w in adj[queue.popleft()]:
                if w not in seen:
                    seen.add(w)
                    queue.append(w)
        found.update(seen)
        components.append(seen)
    return components


def _reference(n, pairs, counts):
    """-> (rep [n], reps, sizes, sums, number of clusters); counts None: all equal (order = identity)."""
    cnt = [1] * n if counts is None else [int(c) for c in counts]
    adj = [set() for _ in range(n)]
    for i, j in pairs:
        adj[int(i)].add(int(j))
        adj[int(j)].add(int(i))
    groups = []
    for comp in _components(n, adj, cnt):
        if len(comp) == 1:
            groups.append(list(comp))
            continue
        nodes = sorted(sorted(comp), key=lambda v: cnt[v], reverse=True)
        covered = set()
        for i, v in enumerate(nodes):               # the shortest prefix nodes[:i + 1] that covers comp
            covered.add(v)
            covered.update(adj[v])
            if len(covered) == len(comp):
                break
        leads = nodes[:i + 1]
        observed = set(leads)
        for lead in leads:
            connected = adj[lead]
            groups.append([lead] + sorted(connected - observed))
            observed.update(connected)
    groups.sort(key=lambda g: (-cnt[g[0]], g[0]))   # the representatives in rank order
    rep = [None] * n
    for g in groups:
        for v in g:
            assert rep[v] is None
            rep[v] = g[0]
    sums = None if counts is None else [sum(cnt[v] for v in g) for g in groups]
    return rep, [g[0] for g in groups], [len(g) for g in groups], sums, len(groups)


def _reference_network(n, pairs, counts, method):
    """The restated `cluster` / `directional` grouping (as tests/test_cluster.py states it) -> rep [n]."""
    cnt = [int(c) for c in counts]
    adj = [[] for _ in range(n)]
    for i, j in pairs:
        i, j = int(i), int(j)
        if method == "cluster" or cnt[i] >= 2 * cnt[j] - 1:
            adj[i].append(j)
        if method == "cluster" or cnt[j] >= 2 * cnt[i] - 1:
            adj[j].append(i)
    observed, rep = set(), [None] * n
    for comp in _components(n, adj, cnt):
        group = [v for v in sorted(sorted(comp), key=lambda v: cnt[v], reverse=True) if v not in observed]
        observed.update(group)
        for v in group:
            rep[v] = group[0]
    return rep


def _order(n, counts):
    if counts is None:
        return None
    return np.asarray(sorted(range(n), key=lambda v: int(counts[v]), reverse=True), dtype=np.uint32)


def _from_dense(n, order, rep, sizes, sums, ncl):
    """Dense outputs (values at the representatives, 0 elsewhere) -> the reference's tuple."""
    rep = [int(r) for r in rep]
    by_rank = range(n) if order is None else [int(v) for v in order]
    reps = [v for v in by_rank if rep[v] == v]
    others = [v for v in range(n) if rep[v] != v]
    assert all(int(sizes[v]) == 0 for v in others), "a size outside a representative"
    if sums is not None:
        assert all(int(sums[v]) == 0 for v in others), "a sum outside a representative"
    return (rep, reps, [int(sizes[v]) for v in reps], None if sums is None else [int(sums[v]) for v in reps], int(ncl))


def _host(n, pairs, counts, method=ADJACENCY):
    from shortseq_amd._native import lib
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 2))
    c = None if counts is None else np.asarray(counts, dtype=np.uint64)
    order = _order(n, counts)
    rep = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    sizes = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    sums = None if c is None else np.full(n, 0xDEADBEEF, dtype=np.uint64)
    ncl = C.c_uint64(1 << 40)
    rc = lib().ss_host_cluster_pairs(p.ctypes.data, p.shape[0], n, None if c is None else c.ctypes.data,
                                     None if order is None else order.ctypes.data, method, rep.ctypes.data,
                                     sizes.ctypes.data, None if sums is None else sums.ctypes.data, C.byref(ncl))
    if rc:
        return rc
    return _from_dense(n, order, rep, sizes, sums, ncl.value)


GUARD = 8


def _gpu_raw(gpu, n, pairs, counts, *, odd_offset=False, ws_bytes=None):
    """ss_cluster_pairs(SS_CLUSTER_ADJACENCY) through ctypes.  d_rep / d_sizes / d_sums / d_nclusters lie
    inside larger tensors whose guard elements must stay unchanged.  ws_bytes: the size passed (the
    allocation is always the full one).  -> the status when nonzero, else (reference-shaped tuple, rounds)."""
    import torch
    from shortseq_amd._native import lib
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).astype(np.uint32).view(np.int32)
    m = p.shape[0]
    lead = 1 if odd_offset else 0
    buf = torch.zeros((m + lead + 1, 2), dtype=torch.int32, device=gpu)
    buf[lead:lead + m] = torch.from_numpy(np.ascontiguousarray(p)).to(gpu)
    d_pairs = buf[lead:]
    assert d_pairs.data_ptr() % 16 == (8 if odd_offset else 0)
    d_counts = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.uint64).view(np.int64)).to(gpu)
    order = _order(n, counts)
    d_order = None if order is None else torch.from_numpy(order.view(np.int32)).to(gpu)
    full = int(lib().ss_cluster_ws_bytes_method(n, m, ADJACENCY))
    assert full >= int(lib().ss_cluster_ws_bytes(n, m)) + 8 * n
    ws = torch.empty(full // 8 + 2, dtype=torch.int64, device=gpu)
    rep = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device=gpu)
    sizes = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device=gpu)
    sums = None if counts is None else torch.full((n + 2 * GUARD,), -7, dtype=torch.int64, device=gpu)
    ncl = torch.full((3,), -7, dtype=torch.int64, device=gpu)
    rounds = C.c_uint32(99999)
    ptr = lambda t, off=0: None if t is None else t[off:].data_ptr()     # noqa: E731
    rc = lib().ss_cluster_pairs(d_pairs.data_ptr(), m, n, ptr(d_counts), ptr(d_order), ADJACENCY, ws.data_ptr(),
                                full if ws_bytes is None else ws_bytes, ptr(rep, GUARD), ptr(sizes, GUARD),
                                ptr(sums, GUARD), ncl[1:].data_ptr(), C.byref(rounds),
                                torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    for t in (rep, sizes, sums):
        if t is not None:
            assert bool((t[:GUARD] == -7).all()) and bool((t[GUARD + n:] == -7).all()), "a guard element was written"
    assert int(ncl[0]) == -7 and int(ncl[2]) == -7
    if rc:
        return rc
    got = _from_dense(n, order, rep[GUARD:GUARD + n].cpu().numpy().view(np.uint32),
                      sizes[GUARD:GUARD + n].cpu().numpy().view(np.uint32),
                      None if sums is None else sums[GUARD:GUARD + n].cpu().numpy().view(np.uint64), int(ncl[1]))
    return got, rounds.value


def _gpu_batch(gpu, n, pairs, counts):
    """batch.cluster_pairs(..., "adjacency") -> (reference-shaped tuple, rounds)."""
    import torch
    import shortseq_amd.batch as B
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).astype(np.uint32).view(np.int32)
    d_pairs = torch.from_numpy(np.ascontiguousarray(p)).to(gpu)
    d_counts = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.uint64).view(np.int64)).to(gpu)
    rep, reps, sizes, sums, rounds = B.cluster_pairs(d_pairs, n, d_counts, "adjacency")
    return ((rep.tolist(), reps.tolist(), sizes.tolist(),
             None if sums is None else [int(s) for s in sums.cpu().numpy().view(np.uint64)], len(reps)), rounds)


# --------------------------------------------------------------------------------------------------
# graphs (the generator, the count pool and the named graphs of tests/test_cluster.py)
def _random_graph(rng, n, m):
    counts = rng.choice(COUNT_POOL, size=n).astype(np.uint64)
    if n < 2 or m == 0:
        return counts, np.zeros((0, 2), dtype=np.int64)
    a = rng.integers(0, n, size=m)
    b = (a + rng.integers(1, n, size=m)) % n
    pairs = np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1)
    rng.shuffle(pairs)
    return counts, pairs


def _chain(n):
    return [(k, k + 1) for k in range(n - 2, -1, -1)]       # (n-2, n-1) first, (0, 1) last


def _star(leaves):
    return [(0, k) for k in range(1, leaves + 1)]


# name -> (n, pairs, counts, expected `adjacency` clusters as lists of nodes, representative first, in rank order)
NAMED = {
    # A = 10 covers B, B = 6 covers C: leads A and B; C goes to B
    "direction_matters": (3, [(0, 1), (1, 2)], [10, 6, 3], [[0], [1, 2]]),
    # node 1 (9) covers 2, node 0 (8) is still uncovered: both lead, 2 goes to the higher count
    "two_roots_higher_count": (3, [(0, 2), (1, 2)], [8, 9, 4], [[1, 2], [0]]),
    # node 1 (8, the lower index) covers 0, node 2 is uncovered until it leads itself
    "two_roots_lower_index": (3, [(0, 1), (0, 2)], [4, 8, 8], [[1, 0], [2]]),
    # counts and sums past 2^32; the count rule of `directional` plays no part
    "u64_threshold": (4, [(0, 1), (2, 3)], [1 << 33, (1 << 32) + 1, (1 << 33) + 1, (1 << 32) + 1], [[2, 3], [0, 1]]),
    "duplicate_pairs": (6, [(0, 1), (1, 2), (0, 1), (4, 5), (1, 2), (0, 1), (4, 5)], [3, 1, 1, 7, 2, 2], None),
    "counts_one_both_directions": (5, [(3, 4), (2, 3), (1, 2), (0, 1)], [1, 1, 1, 1, 1], [[0], [1], [2], [3, 4]]),
    "zero_counts": (4, [(0, 1), (1, 2), (2, 3)], [0, 0, 1, 0], None),
}


def _check_named(name, got):
    n, pairs, counts, expected = NAMED[name]
    assert got == _reference(n, pairs, counts), name
    if expected:
        rep = got[0]
        assert got[1] == [g[0] for g in expected], name
        for g in expected:
            assert all(rep[v] == g[0] for v in g), name
        assert got[4] == len(expected)
        assert got[3] == [sum(counts[v] for v in g) for g in expected]


# --------------------------------------------------------------------------------------------------
# CPU
def test_reference_on_the_hand_examples():
    """The restated UMI-tools procedure itself, on cases whose answer is known by hand."""
    chain = [(k, k + 1) for k in range(4)]
    assert _reference(3, [(0, 1), (1, 2)], [10, 6, 3]) == ([0, 1, 1], [0, 1], [1, 2], [10, 9], 2)
    # equal counts: 0, 1, 2 cover up to node 3; node 4 is reached only once 3 leads
    assert _reference(5, chain, [1] * 5) == ([0, 1, 2, 3, 3], [0, 1, 2, 3], [1, 1, 1, 2], [1, 1, 1, 2], 4)
    # the two ends (5) cover 1 and 3; node 2 is reached only once 1 leads, which takes it
    assert _reference(5, chain, [5, 1, 1, 1, 5]) == ([0, 1, 1, 4, 4], [0, 4, 1], [1, 2, 2], [5, 6, 2], 3)
    assert _reference(5, chain, None)[0] == [0, 1, 2, 3, 3]


def test_host_hand_examples():
    chain = [(k, k + 1) for k in range(4)]
    for n, pairs, counts in ((3, [(0, 1), (1, 2)], [10, 6, 3]), (5, chain, [1] * 5), (5, chain, [5, 1, 1, 1, 5]),
                             (5, chain, None)):
        assert _host(n, pairs, counts) == _reference(n, pairs, counts)


def test_host_random_graphs():
    """300 graphs; every third also without counts.  The method must not be an alias of an older one:
    on at least 100 of the graphs the reference grouping differs from the restated `cluster` grouping
    and from the restated `directional` grouping as well."""
    rng = np.random.default_rng(20250101)
    differs = 0
    for g in range(300):
        n = int(rng.integers(1, 41))
        m = int(rng.integers(0, 2 * n + 1))
        counts, pairs = _random_graph(rng, n, m)
        exp = _reference(n, pairs, counts)
        assert _host(n, pairs, counts) == exp, g
        differs += (exp[0] != _reference_network(n, pairs, counts, "cluster")
                    and exp[0] != _reference_network(n, pairs, counts, "directional"))
        if g % 3 == 0:      # no counts: order is the identity, no sums
            assert _host(n, pairs, None) == _reference(n, pairs, None), g
    print(f"adjacency differs from both other methods on {differs} of 300 graphs")
    assert differs >= 100, differs


def _chain_expected(n, rising):
    """Equal counts: leads 0 .. n-2, node n-1 joins n-2.  Counts rising with the index: leads n-1 .. 1,
    node 0 joins 1."""
    if rising:
        return [1] + list(range(1, n)), list(range(n - 1, 0, -1)), [1] * (n - 2) + [2]
    return list(range(n - 1)) + [n - 2], list(range(n - 1)), [1] * (n - 2) + [2]


def _star_expected(hub, leaf, isolated=0):
    """Hub 0 with 5000 leaves (and `isolated` further nodes of count 2, singletons).  A heavy hub: one
    cluster.  A light hub: every leaf leads, the hub joins leaf 1."""
    n = 5001 + isolated
    counts = np.array([hub] + [leaf] * 5000 + [2] * isolated, dtype=np.uint64)
    rep = ([0] * 5001 if hub > leaf else [1] + list(range(1, 5001))) + list(range(5001, n))
    return n, counts, rep, (1 if hub > leaf else 5000) + isolated


@pytest.fixture(scope="module")
def big_cases():
    """name -> (n, pairs, counts, the reference's tuple): the chain and star references, computed once."""
    out = {}
    n = 4097
    for rising in (False, True):
        counts = np.arange(1, n + 1, dtype=np.uint64) if rising else np.ones(n, dtype=np.uint64)
        exp = _reference(n, _chain(n), counts)
        rep, reps, sizes = _chain_expected(n, rising)
        assert exp[0] == rep and exp[1] == reps and exp[2] == sizes and exp[4] == n - 1
        out["chain_rising" if rising else "chain_equal"] = (n, _chain(n), counts, exp)
    for hub, leaf in ((10 ** 4, 1), (1, 3)):
        for isolated in (0, 1000):
            n, counts, rep, k = _star_expected(hub, leaf, isolated)
            exp = _reference(n, _star(5000), counts)
            assert exp[0] == rep and exp[4] == k
            out[f"star_{hub}_{leaf}_{isolated}"] = (n, _star(5000), counts, exp)
    return out


BIG = ["chain_equal", "chain_rising", "star_10000_1_0", "star_1_3_0", "star_10000_1_1000", "star_1_3_1000"]


@pytest.mark.parametrize("name", BIG)
def test_host_chain_and_star(big_cases, name):
    n, pairs, counts, exp = big_cases[name]
    assert _host(n, pairs, counts) == exp


@pytest.mark.parametrize("name", sorted(NAMED))
def test_host_named_graphs(name):
    n, pairs, counts, _ = NAMED[name]
    _check_named(name, _host(n, pairs, counts))


def test_host_argument_errors():
    assert _host(4, [(0, 4)], [1, 1, 1, 1]) == SS_EARG                       # a node >= n
    assert _host(4, [(4, 0)], None) == SS_EARG
    from shortseq_amd._native import lib
    rep = np.zeros(4, dtype=np.uint32)
    sums = np.zeros(4, dtype=np.uint64)
    ncl = C.c_uint64(0)
    host = lib().ss_host_cluster_pairs
    assert host(None, 0, 4, None, None, ADJACENCY, rep.ctypes.data, None, sums.ctypes.data, C.byref(ncl)) == SS_EARG
    assert host(None, 0, 1 << 32, None, None, ADJACENCY, rep.ctypes.data, None, None, C.byref(ncl)) == SS_EARG
    # 3 is a method where 2 still is none
    assert host(None, 0, 4, None, None, 2, rep.ctypes.data, None, None, C.byref(ncl)) == SS_EARG
    assert host(None, 0, 4, None, None, ADJACENCY, rep.ctypes.data, None, None, C.byref(ncl)) == 0
    assert rep.tolist() == [0, 1, 2, 3] and ncl.value == 4


def test_workspace_sizes():
    from shortseq_amd._native import lib
    L_ = lib()
    for n, m in ((0, 0), (1, 0), (100, 150), (1000, 1), (5001, 5000)):
        base = L_.ss_cluster_ws_bytes(n, m)
        assert L_.ss_cluster_ws_bytes_method(n, m, 0) == base and L_.ss_cluster_ws_bytes_method(n, m, 1) == base
        assert L_.ss_cluster_ws_bytes_method(n, m, ADJACENCY) >= base + 8 * n       # cover and thr at the least


def _pool_dict(seed, nkeys, lengths, U):
    """A mapping ShortSeq -> count of `nkeys` distinct keys: reads drawn from U random L-mers per length
    plus single-substitution variants, counted in order of first occurrence."""
    import shortseq_amd as ssa
    rng = np.random.default_rng(seed)
    base = {L: ["".join(rng.choice(list("ACGT"), size=L)) for _ in range(U)] for L in lengths}
    out = {}
    while True:
        L = lengths[int(rng.integers(0, len(lengths)))]
        s = list(base[L][int(rng.integers(0, U))])
        if rng.random() < 0.5:
            s[int(rng.integers(0, L))] = "ACGT"[int(rng.integers(0, 4))]
        s = "".join(s)
        if s not in out and len(out) == nkeys:
            break
        out[s] = out.get(s, 0) + 1
    return {ssa.from_str(s): c for s, c in out.items()}


def _dedup_reference(d, max_dist):
    """umi.dedup's contract from strings alone: per length, plain hamming pairs + _reference."""
    keys = list(d)
    strs = [str(k) for k in keys]
    cnts = [d[k] for k in keys]
    rep_of = list(range(len(keys)))
    for L in sorted({len(s) for s in strs}):
        mem = [i for i, s in enumerate(strs) if len(s) == L]
        pairs = [(a, b) for a in range(len(mem)) for b in range(a + 1, len(mem))
                 if sum(x != y for x, y in zip(strs[mem[a]], strs[mem[b]])) <= max_dist]
        rep = _reference(len(mem), pairs, [cnts[i] for i in mem])[0]
        for a, i in enumerate(mem):
            rep_of[i] = mem[rep[a]]
    sums = {}
    for i, r in enumerate(rep_of):
        sums[r] = sums.get(r, 0) + cnts[i]
    ranked = sorted(sums, key=lambda r: (-sums[r], r))
    return [(keys[r], sums[r]) for r in ranked], [(keys[i], keys[r]) for i, r in enumerate(rep_of)]


@pytest.mark.parametrize("lengths", [(12,), (12, 10)])
def test_dedup_host(lengths):
    import shortseq_amd.umi as U
    d = _pool_dict(5, 200, lengths, 12)
    assert len(d) == 200
    for k in (1, 2):
        clusters, assign = U.dedup(d, max_dist=k, method="adjacency", device="host")
        exp_clusters, exp_assign = _dedup_reference(d, k)
        assert list(clusters.items()) == exp_clusters and list(assign.items()) == exp_assign
        assert sum(clusters.values()) == sum(d.values())
        assert all(len(a) == len(b) for a, b in assign.items())       # lengths never mix
        assert 1 < len(clusters) < len(d)


# --------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_gpu_random_graphs(gpu, n):
    """m in {0, 1, 2, 3, odd, even} (the even one past one block of the pair passes), shuffled, counts with
    many ties; each graph from a 16-B aligned pointer, from an 8-B-only aligned one (the unaligned-head
    path, and with it the other parity of the tail) and through batch.cluster_pairs, with and without
    counts."""
    rng = np.random.default_rng(3000 + n)
    for m in (0, 1, 2, 3, (3 * n // 4) | 1, n // 2 * 2 + 1130):
        counts, pairs = _random_graph(rng, n, m)
        for c in (counts, None):
            exp = _reference(n, pairs, c)
            assert _gpu_raw(gpu, n, pairs, c)[0] == exp, (m, c is None)
            assert _gpu_raw(gpu, n, pairs, c, odd_offset=True)[0] == exp, (m, c is None, "odd offset")
            assert _gpu_batch(gpu, n, pairs, c)[0] == exp, (m, c is None, "batch")


@pytest.mark.gpu
@pytest.mark.parametrize("name", BIG)
def test_gpu_chain_and_star(gpu, big_cases, name):
    """The 4097-node chain (equal counts: the threshold is the chain's far end; rising counts: the order
    runs against the indices), the 5000-leaf star (every node's threshold atomic on one word), and the
    star beside 1000 singletons."""
    n, pairs, counts, exp = big_cases[name]
    for odd in (False, True):
        got, rounds = _gpu_raw(gpu, n, pairs, counts, odd_offset=odd)
        assert got == exp
        assert 1 <= rounds <= 64
    assert _gpu_batch(gpu, n, pairs, counts)[0] == exp


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NAMED))
def test_gpu_named_graphs(gpu, name):
    n, pairs, counts, _ = NAMED[name]
    _check_named(name, _gpu_raw(gpu, n, pairs, counts)[0])
    _check_named(name, _gpu_raw(gpu, n, pairs, counts, odd_offset=True)[0])
    _check_named(name, _gpu_batch(gpu, n, pairs, counts)[0])


@pytest.mark.gpu
def test_gpu_workspace_too_small(gpu):
    """One byte short of ss_cluster_ws_bytes_method(n, m, 3) is SS_EARG; so is the size of the other methods."""
    from shortseq_amd._native import lib
    rng = np.random.default_rng(78)
    n, m = 100, 150
    counts, pairs = _random_graph(rng, n, m)
    full = int(lib().ss_cluster_ws_bytes_method(n, m, ADJACENCY))
    assert _gpu_raw(gpu, n, pairs, counts, ws_bytes=full - 1) == SS_EARG
    assert _gpu_raw(gpu, n, pairs, counts, ws_bytes=int(lib().ss_cluster_ws_bytes(n, m))) == SS_EARG
    assert _gpu_raw(gpu, n, pairs, counts, ws_bytes=full)[0] == _reference(n, pairs, counts)


@pytest.mark.gpu
def test_gpu_duplicates_and_out_of_range(gpu):
    """Duplicate pairs change nothing.  A pair naming a node >= n is never dereferenced: SS_EARG, the
    guard elements unchanged (checked in _gpu_raw), and the next call on the device works."""
    rng = np.random.default_rng(77)
    n = 300
    counts, pairs = _random_graph(rng, n, 401)
    doubled = np.concatenate([pairs, pairs[::3], pairs[::-1]])
    exp = _reference(n, pairs, counts)
    assert _gpu_raw(gpu, n, doubled, counts)[0] == exp
    for bad in ((5, n), (n, n + 1), (0, 0xFFFFFFFF), (0x80000000, 0xFFFFFFFE)):
        for where in (0, 200, len(pairs)):          # head / body / tail of the stream
            broken = np.concatenate([pairs[:where], np.asarray([bad], dtype=np.int64), pairs[where:]])
            for odd in (False, True):
                assert _gpu_raw(gpu, n, broken, counts, odd_offset=odd) == SS_EARG, (bad, where, odd)
    assert _gpu_raw(gpu, n, pairs, counts)[0] == exp


def _brute_pairs(oracle, words, n, L, k):
    pairs = []
    for i in range(n - 1):
        d = oracle.hamming_ref_batch(words[i + 1:], n - i - 1, L, words[i])
        pairs.extend((i, int(j)) for j in np.flatnonzero(d <= k) + i + 1)
    return pairs


def _umi_pool(oracle, n, L, U, seed):
    """n reads drawn from U distinct L-mers plus substitution variants, then deduplicated and counted:
    distinct nodes that carry counts (the pools of tests/test_cluster.py)."""
    rng = np.random.default_rng(seed)
    base = oracle.gen_reads(seed, 0, U, L).reshape(U, L)
    pick = base[rng.integers(0, U, size=n)].copy()
    mut = rng.random(n) < 0.4
    pos = rng.integers(0, L, size=n)
    pick[mut, pos[mut]] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(mut.sum()))]
    rows, counts = np.unique(pick, axis=0, return_counts=True)
    return np.ascontiguousarray(rows), counts.astype(np.uint64)


@pytest.fixture(scope="module")
def pools(oracle):
    """L -> (words [g, W], counts, {k: (the oracle's brute-force pairs, the reference over them)}); computed once."""
    out = {}
    for L in (12, 40):
        rows, counts = _umi_pool(oracle, 2000, L, 100, 31 + L)
        g = rows.shape[0]
        words, rc, _ = oracle.encode_batch(rows.reshape(-1), g, L)
        assert rc == 0
        words = words.reshape(g, -1)
        brute = {}
        for k in (1, 2):
            p = _brute_pairs(oracle, words, g, L, k)
            brute[k] = (p, _reference(g, p, counts))
        out[L] = (words, counts, brute)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("L", [12, 40])
@pytest.mark.parametrize("k", [1, 2])
def test_umi_cluster_end_to_end(gpu, pools, L, k):
    """batch.umi_cluster (all-pairs, then clusters) against the restated UMI-tools procedure over the
    oracle's brute-force pairs; once more with a one-pair buffer, which runs the retry path."""
    import torch
    import shortseq_amd.batch as B
    words, counts, brute = pools[L]
    pairs, exp = brute[k]
    assert 1 < exp[4] < words.shape[0]
    d_words = torch.from_numpy(words.view(np.int64)).to(gpu)
    d_counts = torch.from_numpy(counts.view(np.int64)).to(gpu)
    for hint in (None, 1):
        rep, reps, sizes, sums, rounds, total = B.umi_cluster(d_words, L, k, d_counts, "adjacency", max_pairs_hint=hint)
        assert total == len(pairs)
        assert (rep.tolist(), reps.tolist(), sizes.tolist(), sums.tolist(), len(reps)) == exp, hint
        assert 1 <= rounds <= 64


@pytest.mark.gpu
def test_umi_cluster_grouped(gpu):
    """batch.umi_cluster_grouped: groups of 0, 1, 2 rows, a few small ones and one past the grouped
    kernel's 256-row tile; group by group equal to the reference run on that group alone."""
    import torch
    import shortseq_amd as ssa
    import shortseq_amd.batch as B
    rng = np.random.default_rng(707)
    L = 12
    assert B.GROUPED_ROW_TILE == 256
    strs, off = [], [0]
    for size in (0, 1, 2, 7, 0, 300, 33, 1, 2):
        parents = ["".join(rng.choice(list("ACGT"), size=L)) for _ in range(max(1, size // 6))]
        group = {}
        while len(group) < size:                    # distinct rows: parents and their 1- and 2-substitution variants
            s = list(parents[int(rng.integers(0, len(parents)))])
            for _ in range(int(rng.integers(0, 3))):
                s[int(rng.integers(0, L))] = "ACGT"[int(rng.integers(0, 4))]
            group["".join(s)] = True
        strs.extend(group)
        off.append(len(strs))
    n = len(strs)
    assert max(np.diff(off)) > B.GROUPED_ROW_TILE
    counts = rng.choice(COUNT_POOL, size=n).astype(np.int64)
    words = np.array([ssa.from_str(s).packed for s in strs], dtype=np.uint64).reshape(n, 1)
    chars = np.frombuffer("".join(strs).encode(), dtype=np.uint8).reshape(n, L)
    want, total, merged = list(range(n)), 0, 0
    for b, e in zip(off[:-1], off[1:]):
        dist = (chars[b:e, None, :] != chars[None, b:e, :]).sum(axis=2)
        local = [(i, j) for i in range(e - b) for j in range(i + 1, e - b) if dist[i, j] <= 1]
        total += len(local)
        rep = _reference(e - b, local, counts[b:e])[0]
        want[b:e] = [r + b for r in rep]
        merged += sum(r != i for i, r in enumerate(rep))
    assert merged > 0
    d_words = torch.from_numpy(words.view(np.int64)).to(gpu)
    d_counts = torch.from_numpy(counts).to(gpu)
    for hint in (None, 1):
        rep, reps, sizes, sums, _rounds, tot = B.umi_cluster_grouped(d_words, L, 1, off, d_counts, "adjacency",
                                                                     max_pairs_hint=hint)
        assert tot == total
        rep = rep.cpu().numpy()
        assert rep.tolist() == want
        reps = reps.cpu().numpy()
        assert np.array_equal(sizes.cpu().numpy(), np.bincount(rep, minlength=n)[reps])
        assert np.array_equal(sums.cpu().numpy(), np.bincount(rep, weights=counts, minlength=n).astype(np.int64)[reps])


@pytest.mark.gpu
def test_dedup_gpu_equals_host(gpu):
    import shortseq_amd.umi as U
    d = _pool_dict(5, 200, (12,), 12)
    host = U.dedup(d, max_dist=1, method="adjacency", device="host")
    dev = U.dedup(d, max_dist=1, method="adjacency", device="gpu")
    auto = U.dedup(d, max_dist=1, method="adjacency", device="auto")
    exp = _dedup_reference(d, 1)
    for got in (host, dev, auto):
        assert list(got[0].items()) == exp[0]
        assert list(got[1].items()) == exp[1]
