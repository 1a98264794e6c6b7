"""u64 counts of the bare counter handle (ss_counter) through every insert route, merge and exit.

test_counter_u64.py reaches the u64 state (a slot's u32 low part plus the per-slot u64 array) through
the direct / exact-partition inserts and ss_counter_merge, and reads it back through items_sorted()
only.  Here: the optimistic partition's aggregate (and its overflow route), the multi-word aggregate,
merge_runs / merge_packed / merge_words carries, the sentinel key ~0 ("G" * 32) whose low part lands
on 0, reset of a handle whose u64 array is live -- read through extract(n_parts > 1),
extract_ranges, extract_words, pack_ranges and size.

Every expectation is oracle.count (pinned to the reference by test_oracle_golden.py) times the
repeats, or a dict of Python ints built here (count = sum, first = min); never another product path.
The tests pin results and the overflow word only, not whether the u64 array is allocated."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L32 = 32
SENT = (1 << 64) - 1            # the packed word of "G" * 32 (collides with the table's EMPTY)
M32 = 0xFFFFFFFF
OVF_FIELD = 4                   # overflow word: a count (or first index) did not fit its 32-bit field


def _reads_of(ascii, n, L):
    a = ascii.cpu().numpy().reshape(-1)
    return [a[i * L:(i + 1) * L].tobytes() for i in range(n)]


def _ref_dict(exp, reps=1, base=0):
    """oracle.count rows -> {key word: (count * reps, first + base)} (single-word keys)."""
    return {w[0]: (reps * c, f + base) for (w, _L, c, f) in exp}


def _as_dict(keys, counts, first):
    k = keys.cpu().numpy().view(np.uint64).tolist()
    d = dict(zip(k, zip(counts.cpu().numpy().tolist(), first.cpu().numpy().tolist())))
    assert len(d) == len(k), "a key extracted twice"
    return d


def _assert_order(keys, counts, first, exp, reps):
    """(keys, counts, first) device prefixes, in any order == the oracle's rows in first-occurrence order."""
    k = keys.cpu().numpy().view(np.uint64)
    c = counts.cpu().numpy()
    f = first.cpu().numpy()
    o = np.argsort(f, kind="stable")
    assert k[o].tolist() == [w[0] for (w, _L, _c, _f) in exp]
    assert c[o].tolist() == [reps * cc for (_w, _L, cc, _f) in exp]
    assert f[o].tolist() == [ff for (_w, _L, _c, ff) in exp]


def _i64(keys, gpu):
    """Python ints (u64 key words) -> an int64 device tensor of the same bits."""
    import torch
    return torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64)).to(gpu)


def _starts(parts):
    return [0] + np.cumsum(parts.cpu().numpy()).tolist()


def _unpack(rec):
    """packed records [m, 2] -> (keys u64, counts, first - first_base) numpy."""
    r = rec.cpu().numpy()
    v = r[:, 1].view(np.uint64)
    return r[:, 0].view(np.uint64), (v & np.uint64(M32)).astype(np.int64), (v >> np.uint64(32)).astype(np.int64)


def _assert_pack_clean(t, ref, n_parts=4):
    """pack_ranges of a table whose totals all fit u32: overflow word 0, part counts = those of
    extract_ranges, every record's low half = the key's total count, high half = its first index."""
    _k, _l, _c, _f, eparts = t.extract_ranges(n_parts)
    rec, parts = t.pack_ranges(n_parts, skip=-1, first_base=0)
    assert int(t.overflow_word().item()) == 0
    assert parts.cpu().tolist() == eparts.cpu().tolist()
    m = int(parts.sum().item())
    k, c, f = _unpack(rec[:m])
    got = dict(zip(k.tolist(), zip(c.tolist(), f.tolist())))
    assert len(got) == m
    assert got == ref


# ------------------------------------------------------------------------------------------------
# A. inserts that spill, read through every exit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,n,cap,partitioned", [
    (40_000, 300_000, 1 << 19, True),      # optimistic partition: k_pc_aggregate_slice on spilled slots
    (3, 300_000, 1 << 19, True),           # optimistic overflow: the aggregate, then the spill insert
    (5_000, 200_000, 1 << 17, True),       # <= 128 regions: the exact partition passes
    (900, 20_000, 1 << 16, False),         # direct insert
])
def test_counter_spilled_inserts_every_exit(gpu, oracle, U, n, cap, partitioned):
    """Three inserts of one batch with the spill limit at n / 2 (every insert first moves the slot
    counts, the sentinel's too, into the u64 array): 3 x oracle.count through items_sorted,
    extract(3), extract_ranges(4), extract_words(1), size and pack_ranges(4) -- whose records carry
    the whole count (every total is far below 2^32) and raise no overflow bit."""
    import shortseq_amd.batch as B
    from shortseq_amd.dist import owner_of_np, owner_of_region_np
    reps = 3
    ascii = B.synth_pool_reads(n, L32, 71, 72, U, device=gpu)
    ascii[7] = ord("G")
    ascii[n - 3] = ord("G")
    exp = oracle.count(_reads_of(ascii, n, L32))
    ref = _ref_dict(exp, reps)
    assert ref[SENT] == (2 * reps, 7)
    t = B.GpuCounter(cap, device=gpu)
    try:
        log2cap, slice_log = t.geometry()
        if cap >= 1 << 19:
            assert log2cap - slice_log > 7          # the optimistic partition's precondition
        elif partitioned:
            assert log2cap - slice_log <= 7         # the exact partition passes
        t.set_spill_limit(n // 2)
        for _ in range(reps):
            t.insert(ascii, L32, base_index=0, partitioned=partitioned)
        assert not t.overflowed()
        k, c, f = t.items_sorted()
        assert k.tolist() == [w[0] for (w, _L, _c, _f) in exp]
        assert c.tolist() == [reps * cc for (_w, _L, cc, _f) in exp]
        assert f.tolist() == [ff for (_w, _L, _c, ff) in exp]
        assert t.size() == len(exp)
        # extract by hash owner, 3 parts
        keys, lens, counts, first, parts = t.extract(n_parts=3)
        st = _starts(parts)
        assert st[-1] == len(exp)
        _assert_order(keys[:st[-1]], counts[:st[-1]], first[:st[-1]], exp, reps)
        assert (lens[:st[-1]] == L32).all()
        kh = keys[:st[-1]].cpu().numpy().view(np.uint64)
        for p in range(3):
            assert (owner_of_np(kh[st[p]:st[p + 1]], 3) == p).all()
        # extract by region range, 4 parts
        keys, lens, counts, first, parts = t.extract_ranges(4)
        st = _starts(parts)
        assert st[-1] == len(exp)
        _assert_order(keys[:st[-1]], counts[:st[-1]], first[:st[-1]], exp, reps)
        kh = keys[:st[-1]].cpu().numpy().view(np.uint64)
        for p in range(4):
            assert (owner_of_region_np(kh[st[p]:st[p + 1]], 4, log2cap, slice_log) == p).all()
        # extract_words of a single-word handle: the word column is the key
        fps, lens, words, counts, first, parts = t.extract_words(1)
        m = int(parts.sum().item())
        assert m == len(exp) and words.shape[1] == 1
        assert words[:m, 0].equal(fps[:m])
        _assert_order(words[:m, 0], counts[:m], first[:m], exp, reps)
        assert not t.overflowed()
        _assert_pack_clean(t, ref)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------
# B. multi-word handles
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,cap,U,n", [(33, 1 << 12, 500, 50_000), (100, 1 << 14, 3000, 100_000)])
def test_counter_multiword_spill_and_merge_words(gpu, oracle, L, cap, U, n):
    """L > 32: three spilling inserts == 3 x oracle.count; merge_words then adds a count past 2^32 to
    an existing key, the exact carry to another, a new key twice at 3e9 and a new key at 2^32 + 7 --
    counts exact, firsts the minima, no overflow; one more insert still counts exactly."""
    import torch
    import shortseq_amd.batch as B
    reps = 3
    pool = oracle.gen_pool_reads(81, 82, U, 0, n, L)
    exp = oracle.count([pool[i * L:(i + 1) * L].tobytes() for i in range(n)])
    d = torch.from_numpy(pool).to(gpu).view(n, L)
    W = (L + 31) // 32
    t = B.GpuCounter(cap, device=gpu)
    try:
        t.set_spill_limit(n // 2)
        for _ in range(reps):
            t.insert(d, L, base_index=0)
        assert t.words == W and not t.overflowed()
        words, cnt, f = t.items_sorted_words()
        assert [tuple(r) for r in words.tolist()] == [w for (w, _L, _c, _f) in exp]
        assert cnt.tolist() == [reps * cc for (_w, _L, cc, _f) in exp]
        assert f.tolist() == [ff for (_w, _L, _c, ff) in exp]
        ref = {w: (reps * c, ff) for (w, _L, c, ff) in exp}
        ka, kb = exp[5][0], exp[9][0]                 # existing keys (first index > 0)
        assert ref[ka][1] > 0 and ref[kb][1] > 0
        kc = (ka[0] ^ 0x5555, ) + ka[1:]              # new keys: an existing row, its first word changed
        kd = (kb[0] ^ 0x3333, ) + kb[1:]
        assert kc not in ref and kd not in ref and kc != kd
        rows = [(ka, (1 << 32) + 5, ref[ka][1] + 10),         # first stays
                (kb, (1 << 32) - ref[kb][0], 0),              # the exact carry; first drops to 0
                (kc, 3_000_000_000, 77),
                (kd, (1 << 32) + 7, 12)]
        rows2 = [(kc, 3_000_000_000, 55)]                     # kc again: 6e9, first 55
        for rr in (rows, rows2):
            for (w, c, ff) in rr:
                oc, of = ref.get(w, (0, ff))
                ref[w] = (oc + c, min(of, ff))
            as_i64 = np.array([w for (w, _c, _f) in rr], dtype=np.uint64).view(np.int64).reshape(len(rr), W)
            t.merge_words(torch.from_numpy(as_i64).to(gpu),
                          torch.tensor([c for (_w, c, _f) in rr], dtype=torch.int64, device=gpu),
                          torch.tensor([ff for (_w, _c, ff) in rr], dtype=torch.int64, device=gpu))
        assert ref[kb][0] == 1 << 32 and ref[kc] == (6_000_000_000, 55)

        def got():
            w_, c_, f_ = t.items_words()
            g = {tuple(r): (int(c), int(ff)) for r, c, ff in zip(w_.tolist(), c_.tolist(), f_.tolist())}
            assert len(g) == len(c_)
            return g

        assert got() == ref
        assert not t.overflowed()
        assert t.size() == len(ref)
        t.insert(d, L, base_index=0)
        for (w, _L, c, ff) in exp:
            ref[w] = (ref[w][0] + c, min(ref[w][1], ff))
        assert got() == ref
        assert not t.overflowed()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------
# C. merge_runs / merge_packed carries
# ------------------------------------------------------------------------------------------------
_RUN_CYCLE = [1, M32, 1 << 32, (1 << 32) + 5, 3_000_000_000]
_PACKED_CYCLE = [1, M32, 0x80000000]                 # fits the record's u32 count field


@pytest.fixture(scope="module")
def two_halves(gpu, oracle):
    """A 50 000-read pool batch (U = 300, "G" * 32 in both halves) and the oracle's count of each half
    (the second with global first indices); computed once, never modified."""
    import shortseq_amd.batch as B
    n, per = 50_000, 25_000
    ascii = B.synth_pool_reads(n, L32, 61, 62, 300, device=gpu)
    for r in (7, 9_000, per + 11, per + 500, n - 3):
        ascii[r] = ord("G")
    reads = _reads_of(ascii, n, L32)
    ref_a = _ref_dict(oracle.count(reads[:per]))
    ref_b = _ref_dict(oracle.count(reads[per:]), base=per)
    assert ref_a[SENT] == (2, 7) and ref_b[SENT] == (3, per + 11)
    return ascii, per, ref_a, ref_b


@pytest.mark.parametrize("state", ["u64", "inserts-ones", "inserts-carry"])
@pytest.mark.parametrize("sent_mode", ["exact", "3e9"])
@pytest.mark.parametrize("kind", ["runs", "packed"])
@pytest.mark.parametrize("p", [0, 1])
def test_counter_run_merges_carry(gpu, two_halves, p, kind, sent_mode, state):
    """Table B (second half) folds part p of table A's (first half) own extract_ranges / pack_ranges
    output, count fields overwritten by position (a cycle that carries past 32 bits; the sentinel's
    record lands B's sentinel exactly on 2^32, or adds 3e9).  u64: B first merged one key at 2^32, so
    its u64 part is live -- B's owned part is then exact (the dict of ints), the sentinel with a zero
    low word included, and no overflow bit.  Inserts only: counts of 1 merge exactly; the carrying
    cycle raises overflow value 4; an overflow word of 0 always means exact owned counts."""
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd.dist import owner_of_region_np
    ascii, per, ref_a, ref_b = two_halves
    world = 2
    ta, tb = B.GpuCounter(1 << 12, device=gpu), B.GpuCounter(1 << 12, device=gpu)
    try:
        ta.insert(ascii[:per], L32, base_index=0)
        tb.insert(ascii[per:], L32, base_index=per)
        geo = tb.geometry()
        assert geo == ta.geometry()

        def owner(k):
            return int(owner_of_region_np(np.array([k], dtype=np.uint64), world, *geo)[0])

        ref = dict(ref_b)                             # B's whole table, as Python ints
        if state == "u64":
            k0 = next(k for k in ref_b if k != SENT and owner(k) == p)
            tb.merge(_i64([k0], gpu),
                     torch.tensor([1 << 32], dtype=torch.int64, device=gpu),
                     torch.tensor([ref[k0][1] + 3], dtype=torch.int64, device=gpu), L32)
            ref[k0] = (ref[k0][0] + (1 << 32), ref[k0][1])
        # part p of A, straight from A's own output; only count fields change
        if kind == "runs":
            keys, _l, counts, first, parts = ta.extract_ranges(world)
            st = _starts(parts)
            a, b = st[p], st[p + 1]
            seg_keys = keys[a:b].cpu().numpy().view(np.uint64).tolist()
            seg_first = first[a:b].cpu().numpy().tolist()
        else:
            rec, parts = ta.pack_ranges(world, skip=-1, first_base=0)
            st = _starts(parts)
            a, b = st[p], st[p + 1]
            rk, _rc, rf = _unpack(rec[a:b])
            seg_keys, seg_first = rk.tolist(), rf.tolist()
        assert not ta.overflowed()
        m = b - a
        assert set(seg_keys) == {k for k in ref_a if owner(k) == p} and len(set(seg_keys)) == m
        assert all(ref_a[k][1] == f for k, f in zip(seg_keys, seg_first))
        cycle = [1] if state == "inserts-ones" else (_RUN_CYCLE if kind == "runs" else _PACKED_CYCLE)
        new = [cycle[i % len(cycle)] for i in range(m)]
        if SENT in seg_keys and state != "inserts-ones":
            assert seg_keys[-1] == SENT               # the sentinel goes last in its owner's segment
            v = (1 << 32) - ref_b[SENT][0] if sent_mode == "exact" else 3_000_000_000
            new[-1] = min(v, M32) if kind == "packed" else v
        for k, c, f in zip(seg_keys, new, seg_first):
            oc, of = ref.get(k, (0, f))
            ref[k] = (oc + c, min(of, f))
        if kind == "runs":
            tb.merge_runs(keys[a:b].contiguous(), torch.tensor(new, dtype=torch.int64, device=gpu),
                          first[a:b].contiguous(), [(0, m)], p, world, L32)
        else:
            seg = rec[a:b].clone()
            seg[:, 1] = (seg[:, 1] & ~M32) | torch.tensor(new, dtype=torch.int64, device=gpu)
            tb.merge_packed(seg, [(0, m, 0)], p, world, L32)
        ovf = int(tb.overflow_word().item())
        keys, _l, counts, first, parts = tb.extract_ranges(world)
        st = _starts(parts)
        got = _as_dict(keys[st[p]:st[p + 1]], counts[st[p]:st[p + 1]], first[st[p]:st[p + 1]])
        owned = {k: v for k, v in ref.items() if owner(k) == p}
        print(f"p={p} {kind} {sent_mode} {state}: overflow word {ovf}, owned {len(got)} / {len(owned)}, "
              f"sentinel owner {owner(SENT)}, sentinel {got.get(SENT)} ref {owned.get(SENT)}")
        carries = any(c >> 32 for (c, _f) in owned.values())
        if state == "u64":
            assert carries
            assert ovf == 0
            assert got == owned
            assert tb.size() == len(ref)
            if owner(SENT) == p and sent_mode == "exact":
                assert got[SENT] == (1 << 32, 7)
        elif state == "inserts-ones":
            assert not carries
            assert ovf == 0
            assert got == owned
            assert tb.size() == len(ref)
        else:
            assert carries                            # (from the reference: some owned total needs 33 bits)
            assert ovf & OVF_FIELD
        if ovf == 0:
            assert got == owned
    finally:
        ta.close()
        tb.close()


# ------------------------------------------------------------------------------------------------
# D. sentinel and reset edges, one table
# ------------------------------------------------------------------------------------------------
def _merge_sentinel(B, gpu, steps):
    import torch
    t = B.GpuCounter(1 << 12, device=gpu)
    first = 9
    for i, c in enumerate(steps):
        t.merge(torch.tensor([-1], dtype=torch.int64, device=gpu), torch.tensor([c], dtype=torch.int64, device=gpu),
                torch.tensor([first + 5 * i], dtype=torch.int64, device=gpu), L32)
    return t


def _assert_exits(t, ref, exp_order=None):
    """items_sorted, size and extract_ranges(2) of a single-word table == ref {key: (count, first)}."""
    k, c, f = t.items_sorted()
    assert dict(zip(k.tolist(), zip(c.tolist(), f.tolist()))) == ref and len(k) == len(ref)
    if exp_order is not None:
        assert k.tolist() == exp_order
    assert t.size() == len(ref)
    keys, _l, counts, first, parts = t.extract_ranges(2)
    m = int(parts.sum().item())
    assert m == len(ref)
    assert _as_dict(keys[:m], counts[:m], first[:m]) == ref
    assert not t.overflowed()


@pytest.mark.parametrize("steps", [[1 << 32], [(1 << 32) - 1, 1]], ids=["2^32", "2^32-1,+1"])
def test_counter_sentinel_zero_low_word(gpu, steps):
    """"G" * 32 merged to exactly 2^32 (its u32 low part is 0) is one entry, count 2^32, first 9,
    through items_sorted, size and extract_ranges; pack_ranges includes it and raises overflow value
    4, because the count does not fit a record."""
    import shortseq_amd.batch as B
    t = _merge_sentinel(B, gpu, steps)
    try:
        _assert_exits(t, {SENT: (1 << 32, 9)})
        rec, parts = t.pack_ranges(2, skip=-1, first_base=0)
        assert int(parts.sum().item()) == 1
        assert int(t.overflow_word().item()) == OVF_FIELD
        k, _c, f = _unpack(rec[:1])
        assert k.tolist() == [SENT] and f.tolist() == [9]
    finally:
        t.close()


@pytest.mark.parametrize("steps", [[1 << 32], [(1 << 32) - 1, 1]], ids=["2^32", "2^32-1,+1"])
def test_counter_sentinel_zero_low_word_then_insert(gpu, oracle, steps):
    """... and a 1 000-read batch with "G" * 32 twice on top: the sentinel is 2^32 + 2 (first = the
    batch's row), every other key equals oracle.count."""
    import shortseq_amd.batch as B
    n = 1000
    ascii = B.synth_pool_reads(n, L32, 63, 64, 100, device=gpu)
    ascii[4] = ord("G")
    ascii[700] = ord("G")
    ref = _ref_dict(oracle.count(_reads_of(ascii, n, L32)))
    assert ref[SENT] == (2, 4)
    ref[SENT] = ((1 << 32) + 2, 4)
    t = _merge_sentinel(B, gpu, steps)
    try:
        t.insert(ascii, L32, base_index=0)
        _assert_exits(t, ref)
    finally:
        t.close()


@pytest.mark.parametrize("partitioned", [False, True])
def test_counter_reset_drops_u64_counts(gpu, oracle, partitioned):
    """A handle holding counts past 2^32 (its u64 part live), reset, then counting a 20 000-read
    batch equals oracle.count of that batch alone -- the keys that were past 2^32 are in the batch,
    so a leak would show -- pack_ranges is clean; a spilling second insert doubles the counts."""
    import torch
    import shortseq_amd.batch as B
    n = 20_000
    ascii = B.synth_pool_reads(n, L32, 65, 66, 700, device=gpu)
    ascii[3] = ord("G")
    ascii[n - 1] = ord("G")
    exp = oracle.count(_reads_of(ascii, n, L32))
    big = [w[0] for (w, _L, _c, _f) in exp[:40]]
    assert SENT in big
    t = B.GpuCounter(1 << 12, device=gpu)
    try:
        t.merge(_i64(big, gpu),
                torch.tensor([(1 << 32) + 5 + i for i in range(len(big))], dtype=torch.int64, device=gpu),
                torch.zeros(len(big), dtype=torch.int64, device=gpu), L32)
        t.insert(ascii, L32, base_index=1, partitioned=partitioned)     # (spills: every count into the u64 part)
        k, c, _f = t.items_sorted()
        d0 = _ref_dict(exp)
        assert dict(zip(k.tolist(), c.tolist())) == {
            kk: cc + ((1 << 32) + 5 + big.index(kk) if kk in big else 0) for kk, (cc, _ff) in d0.items()}
        t.reset()
        t.insert(ascii, L32, base_index=0, partitioned=partitioned)
        _assert_exits(t, d0, [w[0] for (w, _L, _c, _f) in exp])
        _assert_pack_clean(t, d0)
        t.set_spill_limit(1)
        t.insert(ascii, L32, base_index=0, partitioned=partitioned)
        d2 = _ref_dict(exp, 2)
        _assert_exits(t, d2, [w[0] for (w, _L, _c, _f) in exp])
        _assert_pack_clean(t, d2)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------
# E. merge_words: the two exits of its claim phase (slice full, first index past the field)
# ------------------------------------------------------------------------------------------------
OVF_TABLE = 1                   # overflow word: a key found no free slot in its slice
OVF_INDEX = 8                   # overflow word: a first index was clamped to 0xFFFFFFFE


def _merge_rows(t, gpu, rows):
    """rows [(words tuple, count, first)] -> one merge_words call."""
    import torch
    W = len(rows[0][0])
    ww = np.array([w for (w, _c, _f) in rows], dtype=np.uint64).view(np.int64).reshape(len(rows), W)
    t.merge_words(torch.from_numpy(ww).to(gpu),
                  torch.tensor([c for (_w, c, _f) in rows], dtype=torch.int64, device=gpu),
                  torch.tensor([f for (_w, _c, f) in rows], dtype=torch.int64, device=gpu))


def _words_dict(t):
    """extract_words(1) -> {words tuple: (count, first)}; no look at the overflow word."""
    _fps, _lens, words, counts, first, parts = t.extract_words(1)
    m = int(parts.sum().item())
    w = words[:m].cpu().numpy().view(np.uint64).tolist()
    d = {tuple(r): (int(c), int(f)) for r, c, f in zip(w, counts[:m].tolist(), first[:m].tolist())}
    assert len(d) == m, "a key extracted twice"
    return d


@pytest.mark.parametrize("W", [2, 3, 7])
def test_counter_merge_words_slice_full(gpu, W):
    """96 distinct rows merged into a 64-slot table (one region, one slice): the overflow word is the
    table-full bit alone, exactly 64 of the rows are resident, each with its own count and first; the
    same 96 rows again double the 64 counts, keep the firsts, admit no other key, keep the bit."""
    import shortseq_amd.batch as B
    from shortseq_amd._native import check, lib
    rng = np.random.default_rng(200 + W)
    raw = rng.integers(0, 1 << 64, size=(96, W), dtype=np.uint64)
    rows = [(tuple(int(x) for x in r), 1 + i, i) for i, r in enumerate(raw)]
    src = {w: (c, f) for (w, c, f) in rows}
    assert len(src) == 96
    t = B.GpuCounter(64, device=gpu)
    try:
        assert t.capacity == 64
        check(lib().ss_counter_set_words(t._h, W), "ss_counter_set_words")
        _merge_rows(t, gpu, rows)
        assert int(t.overflow_word().item()) == OVF_TABLE
        got = _words_dict(t)
        assert len(got) == 64
        assert all(src[w] == v for w, v in got.items())
        _merge_rows(t, gpu, rows)
        got2 = _words_dict(t)
        assert got2 == {w: (2 * c, f) for w, (c, f) in got.items()}
        assert int(t.overflow_word().item()) == OVF_TABLE
    finally:
        t.close()


def test_counter_merge_words_first_past_field(gpu):
    """Firsts of 2^32 + 9 merged onto a resident key and with a new key: the overflow word is the
    index bit alone, the resident key keeps its first, the new key gets 0xFFFFFFFE; a resident key
    merged with a smaller first takes it; counts exact."""
    import torch
    import shortseq_amd.batch as B
    W = 2
    raw = np.random.default_rng(210).integers(0, 1 << 64, size=(3, W), dtype=np.uint64)
    ka, kb, kc = (tuple(int(x) for x in r) for r in raw)
    t = B.GpuCounter(1 << 12, device=gpu)
    try:
        t.insert_words(torch.from_numpy(raw[:2].view(np.int64).copy()).to(gpu), base_index=5)
        assert _words_dict(t) == {ka: (1, 5), kb: (1, 6)}
        _merge_rows(t, gpu, [(ka, 10, (1 << 32) + 9), (kb, 20, 2), (kc, 30, (1 << 32) + 9)])
        assert int(t.overflow_word().item()) == OVF_INDEX
        assert _words_dict(t) == {ka: (11, 5), kb: (21, 2), kc: (30, 0xFFFFFFFE)}
    finally:
        t.close()
