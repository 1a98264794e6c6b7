"""Every kernel chain of the counter insert (plan_insert in csrc/ss_counter.hip) on the inputs where it
differs from a plain scatter: skewed and crafted distributions, batch sizes at the tile and grid edges,
a region that runs full, and the first rejected read.  tests/counter_shapes.py builds the inputs and
the CPU reference and asserts each case's CPU-side conditions (load bound, "records spill", "a block
spans more than 64 coarse buckets", ...) when the case is built; the tests here that are not marked
`gpu` build every case without a device.

Every device case asserts last_route() first, then compares rows, counts and first indices
element-wise with the reference, and size() and overflow_word().  Distributions go in as two
batches with a continuing base index (the second meets slices the first wrote; first indices stay
global); then the table is reset and the second batch alone is inserted (the pending reset).

Key input has no Python binding: it is called through lib().ss_counter_insert_keys, whose ctypes
signature is set here.

Two things the code decides differently from what a 2^19-slot table can show, and so run on larger
tables here: k_pf_scatter's heavy-region dedup needs more than max(64, 2 * 8192 / nb) records of a
region in a tile, nb = regions per coarse bin, which at 2^19 slots (nb = 2) is the whole tile
(fine_heavy_case: 2^22 slots); and a slab of 2 * ceil(f / nb) + 256 slots cannot overrun with
nb = 2 (slab_overrun_case: 2^20 slots).  The reservation, not the batch, turns the slabs on, so
those cases reserve 2^19 / 2^20 reads and insert about 100 000; the 4 198 401-read batches reserve
past the threshold themselves and take the slab route as well.
"""
import ctypes as C

import numpy as np
import pytest

import counter_shapes as S

gpu_test = pytest.mark.gpu


# ---- without a device: the helper pinned to the oracle, every case's conditions ------------------

@pytest.mark.parametrize("L", [16, 20, 32, 40, 100])
def test_ref_table_is_oracle_count(oracle, L):
    """ref_table (numpy.unique over packed rows) against oracle.count on 4000 mixed rows: pool draws,
    runs of one read, "A" * L, "G" * L."""
    rng = np.random.default_rng(L)
    distinct = S.CODES[rng.integers(0, 4, size=(500, L))]
    rows = distinct[rng.integers(0, 500, size=4000)]
    rows[100:400] = rows[7]
    rows[1000:1010] = ord("A")
    rows[2000:2003] = ord("G")
    words = S.pack(rows)
    u, cnt, first = S.ref_table(words, base=0)
    exp = oracle.count([r.tobytes() for r in rows])
    assert [tuple(int(x) for x in r) for r in u] == [w for (w, _L, _c, _f) in exp]
    assert [int(x) for x in cnt] == [c for (_w, _L, c, _f) in exp]
    assert [int(x) for x in first] == [f for (_w, _L, _c, f) in exp]
    # the lexsort form is numpy.unique over the rows
    nu, nf, nc = np.unique(words, axis=0, return_index=True, return_counts=True)
    lu, lf, lc = S.unique_rows(words)
    assert np.array_equal(nu, lu) and np.array_equal(nf, lf) and np.array_equal(nc, lc)


def test_fp_np_is_fp_collide():
    import random

    import fp_collide
    rng = random.Random(4)
    for W in (2, 3, 4):
        rows = [[fp_collide.rand_word(rng) for _ in range(W)] for _ in range(50)]
        assert [int(x) for x in S.fp_np(np.array(rows, dtype=np.uint64))] == [fp_collide.fp(r) for r in rows]
    a, b = fp_collide.clamp_pair(rng)
    assert [int(x) for x in S.fp_np(np.array([a, b], dtype=np.uint64))] == [fp_collide.CLAMPED] * 2


def test_inverse_builder_lands_in_its_regions():
    rng = np.random.default_rng(1)
    for lg in (17, 19, 22):
        regs = [0, 5, S.regions(lg) - 1]
        keys = S.craft_keys_inverse(rng, lg, regs, 100)
        assert np.array_equal(S.region_of(keys, lg), np.repeat(regs, 100))
    assert (S.KSTAR * S.SLOT_MUL) & S.MASK == S.MASK


@pytest.mark.parametrize("route", list(S.ROUTES))
def test_cpu_conditions_distributions(route):
    for r, d in S.dist_ids():
        if r == route:
            case = S.dist_case(r, d)
            assert 60_000 <= sum(len(b) for b in case.batches) <= 100_000
    for r, n in S.size_ids():
        if r == route:
            S.size_case(r, n)
    if route in S.BIG_SIZES:
        S.assert_big_load(route)


def test_cpu_conditions_crafted():
    for route in S.OPTIMISTIC:
        S.fine_heavy_case(route)
    for d in ("one-region", "two-point"):
        assert S.slab_case(d).reserve >= 524_288
    S.slab_overrun_case()
    for route in S.SPARSE_ROUTES:
        assert min(S.sparse_case(route).notes[f"widest_span_{i}"] for i in range(2)) > 64
    for which in S.FULL_ROUTES:
        S.full_case(which)
    S.big_one_bin_keys()
    for kind in PLACED:
        _placed_set(kind)


def test_big_pools_are_the_generators(oracle):
    """A BIG_SIZES batch draws from gen_reads(seed)'s first U reads, the pool assert_big_load checks."""
    for L in (16, 40):
        U = 64
        drawn = oracle.gen_pool_reads(S.BIG_SEEDS[0], S.BIG_SEEDS[1], U, 0, 2000, L).reshape(-1, L)
        pool = oracle.gen_reads(S.BIG_SEEDS[0], 0, U, L).reshape(U, L)
        assert {r.tobytes() for r in drawn} <= {r.tobytes() for r in pool}


# ---- on the device -------------------------------------------------------------------------------

def _B():
    import shortseq_amd.batch as B
    f = B.lib().ss_counter_insert_keys
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    f.restype = C.c_int
    return B


def _counter(B, dev, lg, reserve=None):
    c = B.GpuCounter(1 << lg, device=dev)
    assert c.geometry() == (lg, S.slice_log_of(lg))   # the geometry the helper placed its keys by
    if reserve:
        assert c.reserve(reserve)
    return c


def _insert(B, dev, c, case, rows, base):
    """One batch (numpy rows / keys, or a device tensor of them) through the case's entry point."""
    import torch
    from shortseq_amd._native import check
    if case.kind == "keys":
        t = rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).to(dev)
        check(B.lib().ss_counter_insert_keys(c._h, t.data_ptr(), t.numel(), base, B._stream(dev)),
              "ss_counter_insert_keys")
    else:
        t = rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        if case.stride != case.L:
            wide = torch.zeros((t.shape[0], case.stride), dtype=torch.uint8, device=dev)
            wide[:, :case.L] = t
            t = wide
        c.insert(t.reshape(-1), case.L, stride=case.stride, base_index=base, partitioned=case.partitioned)
    assert c.last_route() == case.route_name
    return t


def _table(c, W):
    """Host copy of (rows uint64 [m, W], counts, first) sorted by first index, overflowed or not."""
    if W > 1:
        _fps, _lens, words, counts, first, parts = c.extract_words(1)
    else:
        words, _lens, counts, first, parts = c.extract(1)
    m = int(parts.sum().item())
    k = words[:m].cpu().numpy().view(np.uint64).reshape(m, W)
    cnt = counts[:m].cpu().numpy().astype(np.uint64)
    f = first[:m].cpu().numpy().astype(np.uint64)
    o = np.argsort(f, kind="stable")
    return k[o], cnt[o], f[o]


def _assert_table(c, ref):
    ek, ec, ef = ref
    k, cnt, f = _table(c, ek.shape[1])
    assert k.shape == ek.shape and np.array_equal(k, ek)
    assert np.array_equal(cnt, ec)
    assert np.array_equal(f, ef)
    assert c.size() == len(ek)
    assert int(c.overflow_word().item()) == 0


def _run_case(dev, case):
    B = _B()
    c = _counter(B, dev, case.lg, case.reserve)
    try:
        assert c.last_route() is None
        for i, rows in enumerate(case.batches):
            _insert(B, dev, c, case, rows, case.base(i))
        _assert_table(c, case.ref())
        c.reset()
        last = len(case.batches) - 1
        _insert(B, dev, c, case, case.batches[last], case.base(last))
        _assert_table(c, case.ref([last]))
    finally:
        c.close()


PLACED = (16, 20, 32, "keys", 40)     # key kinds; 40 nt: W = 2
PLACED_LG = 19
PLACED_REGIONS = (37, 38, 200)        # parts 9, 9 and 50 of 64


def _placed_set(kind):
    """300 keys in each of PLACED_REGIONS -> (rows to insert, their keys, their regions)."""
    if kind == "keys":
        keys = S.craft_keys_inverse(np.random.default_rng(2), PLACED_LG, PLACED_REGIONS, 300)
        rows = keys
    else:
        idx = np.concatenate([S.take(kind, PLACED_LG, lambda r, c, g=g: r == g, 300)
                              for g in PLACED_REGIONS])
        rows, keys = S.pool(kind).rows[idx], S.pool(kind).keys[idx]
    reg = S.region_of(keys, PLACED_LG)
    assert np.array_equal(reg, np.repeat(PLACED_REGIONS, 300))
    return rows, keys, reg


@gpu_test
@pytest.mark.parametrize("kind", PLACED, ids=str)
def test_crafted_sets_land_where_claimed(gpu, kind):
    """extract_ranges(64) of a table holding only a crafted set returns every key in the part of the
    region the helper computed for it (part = region * 64 / R), and nothing anywhere else."""
    B = _B()
    route = {16: "opt-plain", 20: "hist-2", 32: "opt-g16", "keys": "opt-keys", 40: "multi-2"}[kind]
    rows, keys, reg = _placed_set(kind)
    if kind == 40:
        # region-range extraction takes single-word keys.  A multi-word table places a row by
        # slot_top of its fingerprint, as a single-word table places a key: so (1) the multi-word
        # table's own fingerprints are the helper's, and its slot-order extract walks the claimed
        # regions in turn, and (2) below, those fingerprints as key input land in the claimed parts.
        case = S.Case(route, "placed", [rows])
        c = _counter(B, gpu, case.lg)
        try:
            _insert(B, gpu, c, case, rows, 0)
            fps, _lens, words, _counts, _first, parts = c.extract_words(1)
            m = int(parts.sum().item())
            assert m == len(keys)
            fps, words = fps[:m].cpu().numpy().view(np.uint64), words[:m].cpu().numpy().view(np.uint64)
            assert np.array_equal(fps, S.fp_np(words)) and np.array_equal(np.sort(fps), np.sort(keys))
            assert np.array_equal(S.region_of(fps, case.lg), np.repeat(PLACED_REGIONS, 300))   # slot order
        finally:
            c.close()
        route, rows = "opt-keys", keys
    case = S.Case(route, "placed", [rows])
    assert case.lg == PLACED_LG
    c = _counter(B, gpu, case.lg)
    try:
        _insert(B, gpu, c, case, rows, 0)
        k, _lens, counts, _first, parts = c.extract_ranges(64)
        parts = parts.cpu().numpy()
        assert int(parts.sum()) == len(keys) and int(c.overflow_word().item()) == 0
        got = k[:len(keys)].cpu().numpy().view(np.uint64)
        assert np.all(counts[:len(keys)].cpu().numpy() == 1)
        part_of_key = S.part_of_region(reg, case.lg)
        off = np.concatenate([[0], np.cumsum(parts)])
        for p in range(64):
            assert np.array_equal(np.sort(got[off[p]:off[p + 1]]), np.sort(keys[part_of_key == p])), p
    finally:
        c.close()


@gpu_test
@pytest.mark.parametrize("route,dist", S.dist_ids(), ids=lambda v: v)
def test_distribution(gpu, route, dist):
    _run_case(gpu, S.dist_case(route, dist))


@gpu_test
@pytest.mark.parametrize("route", S.OPTIMISTIC)
def test_fine_scatter_heavy_region(gpu, route):
    _run_case(gpu, S.fine_heavy_case(route))


@gpu_test
@pytest.mark.parametrize("dist", ["one-region", "two-point"])
def test_slab_route_under_skew(gpu, dist):
    _run_case(gpu, S.slab_case(dist))


@gpu_test
def test_slab_overrun(gpu):
    _run_case(gpu, S.slab_overrun_case())


@gpu_test
@pytest.mark.parametrize("route", S.SPARSE_ROUTES)
def test_sparse_buckets_unstaged(gpu, route):
    _run_case(gpu, S.sparse_case(route))


@gpu_test
@pytest.mark.parametrize("route,n", S.size_ids(), ids=lambda v: str(v))
def test_size(gpu, route, n):
    _run_case(gpu, S.size_case(route, n))


def _device_draws(dev, pool_rows, n, seed):
    """n rows drawn uniformly from pool_rows (numpy) on the device -> the device tensor."""
    import torch
    pool = torch.from_numpy(np.ascontiguousarray(pool_rows).view(np.int64 if pool_rows.dtype == np.uint64 else np.uint8))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    ids = torch.randint(0, len(pool_rows), (n,), device=dev, generator=g)
    return pool.to(dev)[ids]


def _host_words(case, t):
    h = t.cpu().numpy()
    return h.view(np.uint64)[:, None] if case.kind == "keys" else S.pack(h)


@gpu_test
@pytest.mark.parametrize("route", list(S.BIG_SIZES))
def test_big_size(gpu, route):
    """The multi-tile sizes, one batch each, generated on the device and copied back once for the
    reference.  The optimistic routes reserve 4 198 401 reads for it, which turns the slabs on."""
    B = _B()
    n, U = S.BIG_SIZES[route]
    S.assert_big_load(route)
    case = S.Case(route, f"n{n}", [])
    if route in S.OPTIMISTIC:
        assert n >= S.slab_reservation(case.lg)
        case.route_name = case.route_name.replace("counted cursors", "slabs")
    if case.kind == "keys":
        t = _device_draws(gpu, S.big_key_pool(route), n, 5)
    else:
        t = B.synth_pool_reads(n, case.L, S.BIG_SEEDS[0], S.BIG_SEEDS[1], U, device=gpu)
    c = _counter(B, gpu, case.lg)
    try:
        _insert(B, gpu, c, case, t, case.BASE)
        ref = S.ref_table(_host_words(case, t), base=case.BASE)
        assert len(ref[0]) <= U
        _assert_table(c, ref)
    finally:
        c.close()


@gpu_test
def test_big_one_bin_second_fine_tile(gpu):
    """4 198 401 reads of one coarse bin of a 2^21 table: the bin's sub-bins run full at
    pf_cap1 = 11 280 > 8192 records, so k_pf_scatter runs a second, partial tile on each; the other
    ~3.3 M records take the spill list."""
    B = _B()
    route, lg = S.BIG_ONE_BIN
    rows = S.big_one_bin_keys()
    case = S.Case(route, "big-one-bin", [], lg=lg)
    case.route_name = case.route_name.replace("counted cursors", "slabs")
    t = _device_draws(gpu, rows, S.BIG_OPT, 6)
    c = _counter(B, gpu, lg)
    try:
        _insert(B, gpu, c, case, t, case.BASE)
        _assert_table(c, S.ref_table(_host_words(case, t), base=case.BASE))
    finally:
        c.close()


@gpu_test
@pytest.mark.parametrize("which", S.FULL_ROUTES)
def test_region_runs_full(gpu, which):
    """2048 + 256 distinct keys, each twice, in one region of 2048 slots: the overflow word is the
    table-full bit alone; everything outside the region is exact; the region holds crafted keys only,
    each once -- on the single-word routes exactly 2048 of them with their exact counts and first
    indices (a claimed slot never changes and a full slice stays full), on the multi-word route with
    at most their true counts; after reset() the handle counts exactly again."""
    B = _B()
    case, _crowd, reg = S.full_case(which)
    W = _crowd.shape[1]
    c = _counter(B, gpu, case.lg)
    try:
        for i, rows in enumerate(case.batches):
            _insert(B, gpu, c, case, rows, case.base(i))
            if which == "opt-g16-spill" and i == 0:
                assert int(c.overflow_word().item()) == 0     # 2000 of the crowd: not full yet
        assert int(c.overflow_word().item()) == S.kOvfTable
        k, cnt, f = _table(c, W)
        ek, ec, ef = case.ref()
        inside, einside = S.region_of(S.keys_of(k), case.lg) == reg, S.region_of(S.keys_of(ek), case.lg) == reg
        assert int(einside.sum()) == S.CROWD
        assert np.array_equal(k[~inside], ek[~einside])
        assert np.array_equal(cnt[~inside], ec[~einside]) and np.array_equal(f[~inside], ef[~einside])
        # the crowded region: match every resident row to the reference's row of the same words
        rk, rc, rf = k[inside], cnt[inside], f[inside]
        both = np.concatenate([ek[einside], rk])
        u, first_at, counts = S.unique_rows(both)
        assert len(u) == S.CROWD                               # residents are crafted keys ...
        assert counts.max() <= 2 and int((counts == 2).sum()) == len(rk)   # ... each resident once
        o = np.lexsort(tuple(rk[:, j] for j in range(W - 1, -1, -1)))
        held = counts == 2
        tc, tf = ec[einside][first_at[held]], ef[einside][first_at[held]]  # (unique_rows: sorted by row, as o)
        if W == 1:
            assert len(rk) == S.SLOTS
            assert np.array_equal(rc[o], tc) and np.array_equal(rf[o], tf)
        else:
            assert 0 < len(rk) <= S.SLOTS
            assert np.all(rc[o] <= tc) and np.all(rc[o] >= 1)
        c.reset()
        plain = S.dist_case(case.route, "two-point")
        _insert(B, gpu, c, plain, plain.batches[0], plain.base(0))
        _assert_table(c, plain.ref([0]))
    finally:
        c.close()


@gpu_test
@pytest.mark.parametrize("route", S.ASCII_ROUTES)
def test_first_rejected_read(gpu, oracle, route):
    """A rejected byte in read n - 1 (in a partial last tile) and another in read n // 2: the insert
    raises what the reference raises for read n // 2 (first_bad is reset by k_prep on the optimistic
    route and by a stream write on the others, so a stale value of the insert before cannot win)."""
    import torch
    B = _B()
    n = S.kCoarseTile + 1000
    case = S.Case(route, "bad", [])
    rows = S.pool(S.pool_kind(route)).rows[:n].copy()
    c = _counter(B, gpu, case.lg)
    try:
        def reference_error(a):
            """(read index, message) of the oracle's first rejected read: the message names the
            byte, or for reads past 32 nt the 8-byte chunk, that the reference's encoder rejects."""
            with pytest.raises(ValueError) as ref:
                oracle.count([r.tobytes() for r in a])
            _kind, read_index, byte_offset, nbytes = ref.value.args[0]
            chunk = a[read_index].tobytes()[byte_offset:byte_offset + nbytes]
            return read_index, "Unsupported base character: " + chunk.decode("ascii")

        last = rows.copy()
        last[n - 1, case.L - 1] = ord("!")
        both = last.copy()
        both[n // 2, 3] = ord("N")
        assert reference_error(last)[0] == n - 1 and reference_error(both)[0] == n // 2
        assert "N" in reference_error(both)[1] and "!" in reference_error(last)[1]
        for a in (last, both):
            with pytest.raises(Exception) as ei:
                _insert(B, gpu, c, case, torch.from_numpy(a).to(gpu), 0)
            assert (ei.value.read_index, str(ei.value)) == reference_error(a)
            assert c.last_route() == case.route_name
        _insert(B, gpu, c, case, torch.from_numpy(rows).to(gpu), 0)     # and a clean batch raises nothing
    finally:
        c.close()
