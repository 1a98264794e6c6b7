"""UMI clustering (ss_cluster_pairs / ss_host_cluster_pairs, batch.cluster_pairs / umi_cluster,
umi.dedup): the `cluster` and `directional` methods of UMI-tools over a pair list.

The reference here is a literal restatement of the UMI-tools procedure (adjacency lists from the count
rule, a BFS from every not-yet-found node in stable count-descending order, then every node kept in the
first group that observed it), written without the min-rank formulation the kernels use.  Every case
compares rep, reps, sizes, sums and the cluster count exactly.
"""
import ctypes as C
from collections import deque

import numpy as np
import pytest

COUNT_POOL = (1, 1, 1, 2, 3, 4, 7, 8, 15, 100)
METHODS = ("cluster", "directional")
METHOD_ID = {"cluster": 0, "directional": 1}
SS_EARG = -1


# --------------------------------------------------------------------------------------------------
# the reference: UMI-tools, restated
def _reference(n, pairs, counts, method):
    """-> (rep [n], reps, sizes, sums, number of clusters); counts None: all equal (order = identity)."""
    cnt = [1] * n if counts is None else [int(c) for c in counts]
    adj = [[] for _ in range(n)]
    for i, j in pairs:
        i, j = int(i), int(j)
        if method == "cluster":
            adj[i].append(j)
            adj[j].append(i)
        else:
            if cnt[i] >= 2 * cnt[j] - 1:
                adj[i].append(j)
            if cnt[j] >= 2 * cnt[i] - 1:
                adj[j].append(i)
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
    observed, groups = set(), []
    for comp in components:
        group = []
        for v in sorted(sorted(comp), key=lambda v: cnt[v], reverse=True):
            if v not in observed:                                            # first observation wins
                observed.add(v)
                group.append(v)
        groups.append(group)
    rep = [None] * n
    for g in groups:
        for v in g:
            rep[v] = g[0]
    sums = None if counts is None else [sum(cnt[v] for v in g) for g in groups]
    return rep, [g[0] for g in groups], [len(g) for g in groups], sums, len(groups)


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


def _host(n, pairs, counts, method):
    from shortseq_amd._native import lib
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 2))
    c = None if counts is None else np.asarray(counts, dtype=np.uint64)
    order = _order(n, counts)
    rep = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    sizes = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    sums = None if c is None else np.full(n, 0xDEADBEEF, dtype=np.uint64)
    ncl = C.c_uint64(1 << 40)
    rc = lib().ss_host_cluster_pairs(p.ctypes.data, p.shape[0], n, None if c is None else c.ctypes.data,
                                     None if order is None else order.ctypes.data, METHOD_ID[method], rep.ctypes.data,
                                     sizes.ctypes.data, None if sums is None else sums.ctypes.data, C.byref(ncl))
    if rc:
        return rc
    return _from_dense(n, order, rep, sizes, sums, ncl.value)


GUARD = 8


def _gpu_raw(gpu, n, pairs, counts, method, *, odd_offset=False, short_ws=0, with_counts=True):
    """ss_cluster_pairs through ctypes.  d_rep / d_sizes / d_sums lie inside larger tensors whose guard
    elements must stay unchanged.  -> the status when nonzero, else (reference-shaped tuple, rounds)."""
    import torch
    from shortseq_amd._native import lib
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).astype(np.uint32).view(np.int32)
    m = p.shape[0]
    lead = 1 if odd_offset else 0
    buf = torch.zeros((m + lead + 1, 2), dtype=torch.int32, device=gpu)
    buf[lead:lead + m] = torch.from_numpy(np.ascontiguousarray(p)).to(gpu)
    d_pairs = buf[lead:]
    assert d_pairs.data_ptr() % 16 == (8 if odd_offset else 0)
    use_counts = counts is not None and with_counts
    d_counts = torch.from_numpy(np.asarray(counts, dtype=np.uint64).view(np.int64)).to(gpu) if use_counts else None
    order = _order(n, counts)
    d_order = None if order is None else torch.from_numpy(order.view(np.int32)).to(gpu)
    ws_bytes = int(lib().ss_cluster_ws_bytes(n, m))
    ws = torch.empty(ws_bytes // 8 + 2, dtype=torch.int64, device=gpu)
    rep = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device=gpu)
    sizes = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device=gpu)
    sums = torch.full((n + 2 * GUARD,), -7, dtype=torch.int64, device=gpu) if use_counts else None
    ncl = torch.full((3,), -7, dtype=torch.int64, device=gpu)
    rounds = C.c_uint32(99999)
    ptr = lambda t, off=0: None if t is None else t[off:].data_ptr()     # noqa: E731
    rc = lib().ss_cluster_pairs(d_pairs.data_ptr(), m, n, ptr(d_counts), ptr(d_order), METHOD_ID[method], ws.data_ptr(),
                                ws_bytes - short_ws, ptr(rep, GUARD), ptr(sizes, GUARD), ptr(sums, GUARD),
                                ncl[1:].data_ptr(), C.byref(rounds), torch.cuda.current_stream(gpu).cuda_stream)
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


def _gpu_batch(gpu, n, pairs, counts, method):
    """batch.cluster_pairs -> (reference-shaped tuple, rounds)."""
    import torch
    import shortseq_amd.batch as B
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).astype(np.uint32).view(np.int32)
    d_pairs = torch.from_numpy(np.ascontiguousarray(p)).to(gpu)
    d_counts = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.uint64).view(np.int64)).to(gpu)
    rep, reps, sizes, sums, rounds = B.cluster_pairs(d_pairs, n, d_counts, method)
    return ((rep.tolist(), reps.tolist(), sizes.tolist(),
             None if sums is None else [int(s) for s in sums.cpu().numpy().view(np.uint64)], len(reps)), rounds)


# --------------------------------------------------------------------------------------------------
# graphs
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


# name -> (n, pairs, counts, {method: expected clusters as sets of nodes, representative first} or None)
NAMED = {
    # A = 10, B = 6, C = 3: A-B gives no edge (11 < 12), B-C gives B -> C
    "direction_matters": (3, [(0, 1), (1, 2)], [10, 6, 3],
                          {"directional": [[0], [1, 2]], "cluster": [[0, 1, 2]]}),
    # node 2 hangs under two roots: it goes to the higher count
    "two_roots_higher_count": (3, [(0, 2), (1, 2)], [8, 9, 4], {"directional": [[1, 2], [0]]}),
    # ... and with equal counts to the lower index (node 0 is the shared one here)
    "two_roots_lower_index": (3, [(0, 1), (0, 2)], [4, 8, 8], {"directional": [[1, 0], [2]]}),
    # (2^33, 2^32 + 1): 2^33 + 1 < 2^33 + 2, no edge; (2^33 + 1, 2^32 + 1): an edge; sums past 2^32 exact
    "u64_threshold": (4, [(0, 1), (2, 3)], [1 << 33, (1 << 32) + 1, (1 << 33) + 1, (1 << 32) + 1],
                      {"directional": [[2, 3], [0], [1]], "cluster": [[2, 3], [0, 1]]}),
    "duplicate_pairs": (6, [(0, 1), (1, 2), (0, 1), (4, 5), (1, 2), (0, 1), (4, 5)], [3, 1, 1, 7, 2, 2], None),
    "counts_one_both_directions": (5, [(3, 4), (2, 3), (1, 2), (0, 1)], [1, 1, 1, 1, 1],
                                   {"directional": [[0, 1, 2, 3, 4]]}),
    "zero_counts": (4, [(0, 1), (1, 2), (2, 3)], [0, 0, 1, 0], None),
}


def _check_named(name, method, got):
    n, pairs, counts, expected = NAMED[name]
    assert got == _reference(n, pairs, counts, method), (name, method)
    if expected and method in expected:
        rep = got[0]
        assert got[1] == [g[0] for g in expected[method]], (name, method)
        for g in expected[method]:
            assert all(rep[v] == g[0] for v in g), (name, method)
        assert got[4] == len(expected[method])


# --------------------------------------------------------------------------------------------------
# CPU
def test_reference_on_the_issue_examples():
    """The restated UMI-tools procedure itself, on cases whose answer is known by hand."""
    rep, reps, sizes, sums, k = _reference(3, [(0, 1), (1, 2)], [10, 6, 3], "directional")
    assert (rep, reps, sizes, sums, k) == ([0, 1, 1], [0, 1], [1, 2], [10, 9], 2)
    rep, reps, sizes, sums, k = _reference(3, [(0, 1), (1, 2)], [10, 6, 3], "cluster")
    assert (rep, reps, sizes, sums, k) == ([0, 0, 0], [0], [3], [19], 1)


def test_host_random_graphs():
    rng = np.random.default_rng(20240607)
    for g in range(300):
        n = int(rng.integers(1, 41))
        m = int(rng.integers(0, 2 * n + 1))
        counts, pairs = _random_graph(rng, n, m)
        for method in METHODS:
            assert _host(n, pairs, counts, method) == _reference(n, pairs, counts, method), (g, method)
        if g % 3 == 0:      # no counts: order is the identity, no sums
            assert _host(n, pairs, None, "cluster") == _reference(n, pairs, None, "cluster"), g


@pytest.mark.parametrize("name", sorted(NAMED))
def test_host_named_graphs(name):
    n, pairs, counts, _ = NAMED[name]
    for method in METHODS:
        _check_named(name, method, _host(n, pairs, counts, method))


def test_host_chain_and_star():
    n = 4097
    counts = np.arange(1, n + 1, dtype=np.uint64)
    got = _host(n, _chain(n), counts, "cluster")
    assert got == _reference(n, _chain(n), counts, "cluster") and got[1] == [n - 1] and got[2] == [n]
    ones = np.ones(n, dtype=np.uint64)
    got = _host(n, _chain(n), ones, "directional")
    assert got == _reference(n, _chain(n), ones, "directional") and got[1] == [0] and got[2] == [n]
    for hub, leaf in ((10 ** 4, 1), (1, 3)):
        counts = np.array([hub] + [leaf] * 5000, dtype=np.uint64)
        for method in METHODS:
            assert _host(5001, _star(5000), counts, method) == _reference(5001, _star(5000), counts, method)


def test_host_argument_errors():
    assert _host(4, [(0, 4)], [1, 1, 1, 1], "cluster") == SS_EARG            # a node >= n
    assert _host(4, [(0, 1)], None, "directional") == SS_EARG                # directional without counts
    from shortseq_amd._native import lib
    rep = np.zeros(4, dtype=np.uint32)
    sums = np.zeros(4, dtype=np.uint64)
    ncl = C.c_uint64(0)
    assert lib().ss_host_cluster_pairs(None, 0, 4, None, None, 0, rep.ctypes.data, None, sums.ctypes.data,
                                       C.byref(ncl)) == SS_EARG                # sums without counts
    assert lib().ss_host_cluster_pairs(None, 0, 4, None, None, 2, rep.ctypes.data, None, None, C.byref(ncl)) == SS_EARG
    assert lib().ss_host_cluster_pairs(None, 0, 1 << 32, None, None, 0, rep.ctypes.data, None, None,
                                       C.byref(ncl)) == SS_EARG


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


def _dedup_reference(d, max_dist, method):
    """umi.dedup's contract from strings alone: per length, plain hamming pairs + _reference."""
    keys = list(d)
    strs = [str(k) for k in keys]
    cnts = [d[k] for k in keys]
    rep_of = list(range(len(keys)))
    for L in sorted({len(s) for s in strs}):
        mem = [i for i, s in enumerate(strs) if len(s) == L]
        pairs = [(a, b) for a in range(len(mem)) for b in range(a + 1, len(mem))
                 if sum(x != y for x, y in zip(strs[mem[a]], strs[mem[b]])) <= max_dist]
        rep = _reference(len(mem), pairs, [cnts[i] for i in mem], method)[0]
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
    for method in METHODS:
        for k in (1, 2):
            clusters, assign = U.dedup(d, max_dist=k, method=method, device="host")
            exp_clusters, exp_assign = _dedup_reference(d, k, method)
            assert list(clusters.items()) == exp_clusters and list(assign.items()) == exp_assign
            assert sum(clusters.values()) == sum(d.values())
            assert all(len(a) == len(b) for a, b in assign.items())       # lengths never mix
            assert 1 < len(clusters) < len(d)


# --------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_gpu_random_graphs(gpu, n):
    """m in {0, 1, 2, 3, odd, even} (the even one past one block of the hook), shuffled, counts with
    many ties; each graph once more from an odd pair offset (an 8-B but not 16-B aligned pointer: the
    hook's unaligned-head path, and with it the other parity of the tail)."""
    rng = np.random.default_rng(1000 + n)
    for m in (0, 1, 2, 3, (3 * n // 4) | 1, n // 2 * 2 + 1130):
        counts, pairs = _random_graph(rng, n, m)
        for method in METHODS:
            exp = _reference(n, pairs, counts, method)
            assert _gpu_batch(gpu, n, pairs, counts, method)[0] == exp, (m, method)
            assert _gpu_raw(gpu, n, pairs, counts, method)[0] == exp, (m, method)
            assert _gpu_raw(gpu, n, pairs, counts, method, odd_offset=True)[0] == exp, (m, method, "odd offset")
        exp = _reference(n, pairs, None, "cluster")
        assert _gpu_batch(gpu, n, pairs, None, "cluster")[0] == exp, (m, "no counts")


def _jacobi_rounds(n, pairs, counts, method):
    """Rounds that lower a label when every hook pass, and every shortcut pass, reads the labels as they
    stood when the pass began -> (rounds, final labels, order).  The kernels only ever read fresher,
    hence lower, labels and both passes are monotone, so they never need more rounds than this (plus
    the idle round that confirms the fixpoint)."""
    cnt = np.asarray(counts, dtype=np.uint64)
    order = np.asarray(sorted(range(n), key=lambda v: int(cnt[v]), reverse=True), dtype=np.int64)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if method == "cluster":
        src, dst = np.concatenate([p[:, 0], p[:, 1]]), np.concatenate([p[:, 1], p[:, 0]])
    else:
        ci, cj = cnt[p[:, 0]].astype(object), cnt[p[:, 1]].astype(object)
        fwd = np.asarray(ci + 1 >= 2 * cj, dtype=bool)
        bwd = np.asarray(cj + 1 >= 2 * ci, dtype=bool)
        src, dst = np.concatenate([p[fwd, 0], p[bwd, 1]]), np.concatenate([p[fwd, 1], p[bwd, 0]])
    label = np.empty(n, dtype=np.int64)
    label[order] = np.arange(n)
    rounds = 0
    while True:
        hooked = label.copy()
        np.minimum.at(hooked, dst, label[src])
        short = np.minimum(hooked, hooked[order[hooked]])
        if np.array_equal(short, label):
            return rounds, label, order
        label = short
        rounds += 1


@pytest.mark.gpu
@pytest.mark.parametrize("method,rising", [("cluster", True), ("directional", False)])
def test_gpu_chain(gpu, method, rising):
    """4097 nodes, edges (k, k + 1) given last first.  `cluster` with counts rising towards node 4096
    (the minimum travels the whole chain, against the pair order); `directional` with all counts 1
    (both-direction edges).  One cluster, in no more rounds than the Jacobi simulation + 1: without a
    working shortcut pass that would be thousands."""
    n = 4097
    counts = np.arange(1, n + 1, dtype=np.uint64) if rising else np.ones(n, dtype=np.uint64)
    pairs = _chain(n)
    sim_rounds, sim_label, order = _jacobi_rounds(n, pairs, counts, method)
    assert 4 <= sim_rounds <= 32, sim_rounds
    exp = _reference(n, pairs, counts, method)
    assert exp[0] == [int(order[l]) for l in sim_label]
    assert exp[1] == [n - 1 if rising else 0] and exp[2] == [n]
    for odd in (False, True):
        got, rounds = _gpu_raw(gpu, n, pairs, counts, method, odd_offset=odd)
        print(f"chain {method}: rounds {rounds}, jacobi {sim_rounds}")
        assert got == exp
        assert rounds <= sim_rounds + 1, (rounds, sim_rounds)


@pytest.mark.gpu
@pytest.mark.parametrize("hub,leaf", [(10 ** 4, 1), (1, 3)])
def test_gpu_star(gpu, hub, leaf):
    """Hub 0 with 5000 leaves: every atomic of a pass lands on one label.
    Hub 10^4, leaves 1: the hub reaches every leaf, one cluster under both methods.
    Hub 1, leaves 3: no hub -> leaf edge (2 < 6), but every leaf -> hub edge holds (3 >= 2 * 1 - 1), so
    under `directional` the hub joins its highest-ranked ancestor, leaf 1, and the other 4999 leaves
    stay alone: 5000 clusters (the restated UMI-tools procedure gives the same; a 5001-singleton
    outcome would need no edge in either direction); `cluster` gives one, represented by leaf 1."""
    n = 5001
    counts = np.array([hub] + [leaf] * 5000, dtype=np.uint64)
    pairs = _star(5000)
    for method in METHODS:
        exp = _reference(n, pairs, counts, method)
        assert _gpu_raw(gpu, n, pairs, counts, method)[0] == exp
        assert _gpu_batch(gpu, n, pairs, counts, method)[0] == exp
        if hub > leaf:
            assert exp[1] == [0] and exp[2] == [n] and exp[3] == [hub + 5000 * leaf]
        elif method == "cluster":
            assert exp[1] == [1] and exp[2] == [n]
        else:
            assert exp[1] == list(range(1, n)) and exp[2] == [2] + [1] * 4999 and exp[0][0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NAMED))
def test_gpu_named_graphs(gpu, name):
    """Direction matters; a node under two roots; the u64 threshold and sums past 2^32; duplicate pairs."""
    n, pairs, counts, _ = NAMED[name]
    for method in METHODS:
        _check_named(name, method, _gpu_raw(gpu, n, pairs, counts, method)[0])
        _check_named(name, method, _gpu_raw(gpu, n, pairs, counts, method, odd_offset=True)[0])
        _check_named(name, method, _gpu_batch(gpu, n, pairs, counts, method)[0])


@pytest.mark.gpu
def test_gpu_duplicates_and_out_of_range(gpu):
    """Duplicate pairs change nothing.  A pair naming a node >= n is never dereferenced: SS_EARG, the
    guard elements around d_rep / d_sizes / d_sums unchanged (checked in _gpu_raw), and the next call
    on the device works."""
    rng = np.random.default_rng(77)
    n = 300
    counts, pairs = _random_graph(rng, n, 401)
    doubled = np.concatenate([pairs, pairs[::3], pairs[::-1]])
    for method in METHODS:
        exp = _reference(n, pairs, counts, method)
        assert _gpu_raw(gpu, n, doubled, counts, method)[0] == exp
        for bad in ((5, n), (n, n + 1), (0, 0xFFFFFFFF), (0x80000000, 0xFFFFFFFE)):
            for where in (0, 200, len(pairs)):          # head / body / tail of the stream
                broken = np.concatenate([pairs[:where], np.asarray([bad], dtype=np.int64), pairs[where:]])
                for odd in (False, True):
                    assert _gpu_raw(gpu, n, broken, counts, method, odd_offset=odd) == SS_EARG, (bad, where, odd)
        assert _gpu_raw(gpu, n, pairs, counts, method)[0] == exp


@pytest.mark.gpu
def test_gpu_argument_errors(gpu):
    from shortseq_amd._native import NativeError
    import shortseq_amd.batch as B
    import torch
    rng = np.random.default_rng(78)
    counts, pairs = _random_graph(rng, 100, 150)
    assert _gpu_raw(gpu, 100, pairs, counts, "cluster", short_ws=1) == SS_EARG           # one byte short
    assert _gpu_raw(gpu, 100, pairs, counts, "directional", short_ws=1) == SS_EARG
    assert _gpu_raw(gpu, 100, pairs, counts, "directional", with_counts=False) == SS_EARG
    with pytest.raises(NativeError):
        B.cluster_pairs(torch.zeros((3, 2), dtype=torch.int32, device=gpu), 10, None, "directional")


def _brute_pairs(oracle, words, n, L, k):
    pairs = []
    for i in range(n - 1):
        d = oracle.hamming_ref_batch(words[i + 1:], n - i - 1, L, words[i])
        pairs.extend((i, int(j)) for j in np.flatnonzero(d <= k) + i + 1)
    return pairs


def _umi_pool(oracle, n, L, U, seed):
    """n reads drawn from U distinct L-mers plus substitution variants (as test_allpairs.py), then
    deduplicated and counted: distinct nodes that carry counts."""
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
    """L -> (words [g, W], counts, {k: the oracle's brute-force pairs}); computed once."""
    out = {}
    for L in (12, 40):
        rows, counts = _umi_pool(oracle, 2000, L, 100, 31 + L)
        g = rows.shape[0]
        words, rc, _ = oracle.encode_batch(rows.reshape(-1), g, L)
        assert rc == 0
        words = words.reshape(g, -1)
        brute = {k: _brute_pairs(oracle, words, g, L, k) for k in (1, 2)}
        assert all(len(p) < (1 << 20) for p in brute.values())
        out[L] = (words, counts, brute)
    return out


def test_pool_pair_count_stays_small(pools):
    """The end-to-end pools keep the oracle side fast: brute-force pair counts far below 2^20, and
    enough pairs and count ties for the grouping to matter."""
    for L, (words, counts, brute) in pools.items():
        assert 300 < words.shape[0] <= 2000
        assert 100 < len(brute[1]) <= len(brute[2]) < (1 << 20)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [12, 40])
@pytest.mark.parametrize("k", [1, 2])
def test_umi_cluster_end_to_end(gpu, pools, L, k):
    """batch.umi_cluster (all-pairs, then clusters) against the restated UMI-tools procedure over the
    oracle's brute-force pairs; once more with a one-pair buffer, which runs the retry path."""
    import torch
    import shortseq_amd.batch as B
    words, counts, brute = pools[L]
    g = words.shape[0]
    d_words = torch.from_numpy(words.view(np.int64)).to(gpu)
    d_counts = torch.from_numpy(counts.view(np.int64)).to(gpu)
    for method in METHODS:
        exp = _reference(g, brute[k], counts, method)
        for hint in (None, 1):
            rep, reps, sizes, sums, rounds, total = B.umi_cluster(d_words, L, k, d_counts, method, max_pairs_hint=hint)
            assert total == len(brute[k])
            got = (rep.tolist(), reps.tolist(), sizes.tolist(), sums.tolist(), len(reps))
            assert got == exp, (method, hint)
            assert 1 <= rounds <= 64


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1])
def test_umi_cluster_without_pairs(gpu, n):
    """No read, and one read: no all-pairs run, every node its own cluster."""
    import torch
    import shortseq_amd.batch as B
    d_words = torch.full((n, 1), 0x1B, dtype=torch.int64, device=gpu)
    d_counts = torch.full((n,), 5, dtype=torch.int64, device=gpu)
    for method in METHODS:
        rep, reps, sizes, sums, rounds, total = B.umi_cluster(d_words, 12, 1, d_counts, method)
        assert (rep.tolist(), reps.tolist(), sizes.tolist(), sums.tolist()) == ([0] * n, [0] * n, [1] * n, [5] * n)
        assert rounds == 0 and total == 0


@pytest.mark.gpu
def test_dedup_gpu_equals_host(gpu):
    import shortseq_amd.umi as U
    d = _pool_dict(5, 200, (12,), 12)
    for method in METHODS:
        host = U.dedup(d, max_dist=1, method=method, device="host")
        dev = U.dedup(d, max_dist=1, method=method, device="gpu")
        assert list(dev[0].items()) == list(host[0].items())
        assert list(dev[1].items()) == list(host[1].items())
        assert list(dev[0].items()) == _dedup_reference(d, 1, method)[0]
