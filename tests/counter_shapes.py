"""Inputs for tests/test_counter_route_shapes.py: skewed, crafted and tile-edge batches for every
kernel chain of the counter insert (plan_insert in csrc/ss_counter.hip), with the reference table
and the table's placement rule restated on the CPU.

Reference: the reads are packed by oracle.encode_batch and counted by sorting -- (key or word row,
count, first index) as numpy.unique gives them (ref_table; test_ref_table_is_oracle_count pins it to
oracle.count).  Key input needs no packing: the u64 values are the keys.

Placement (csrc/ss_counter.hip slot_top / region_of / bin_of): h = key * 0x9E3779B97F4A7C15 mod 2^64,
top = h >> (64 - log2cap), region = top >> slice_log, coarse bin = region >> (rbits - 7) when
rbits = log2cap - slice_log > 7.  A multi-word key's `key` is its fingerprint (fp_collide.fp of its
packed words, restated on numpy arrays in fp_np).  The helper assumes slice_log = min(log2cap, 11);
every device test asserts ss_counter_geometry says the same.

Crafted key sets are filtered from random candidates (pool: random ASCII rows of length L, packed,
placed), which works for every L; key input also has a builder through the multiplier's inverse.
tests/test_counter_route_shapes.py::test_crafted_sets_land_where_claimed proves on the device
(extract_ranges) that a set lies in the regions it claims.

Every case asserts its CPU-side conditions when it is built, before anything goes to a device: no
region holds more than LOAD_BOUND distinct keys unless the case is about a region running full,
"records spill" and "a block spans more than 64 coarse buckets" where the case claims it.
Constants named k* restate csrc/ss_counter.hip; if one changes there, change it here.  Seeded.
"""
import functools

import numpy as np

import fp_collide

MASK = (1 << 64) - 1
SLOT_MUL = 0x9E3779B97F4A7C15
SLOT_INV = pow(SLOT_MUL, -1, 1 << 64)
KSTAR = (MASK * SLOT_INV) & MASK          # the key whose slot hash h is ~0
EMPTY = MASK                              # "G" * 32: the tables' free-slot value, kept in a slot of its own
CODES = np.frombuffer(b"ACTG", np.uint8)  # 2-bit code -> base

kSliceLogMax = 11       # 2048 slots per region
kCoarseBits = 7         # 128 coarse bins
kPartBlocks = 1024      # exact routes: fixed grid, contiguous read ranges
kTile = 4096            # k_pc_scatter_lds elements per tile
kKeysTile = 1024        # k_pc_keys reads per tile (kKeysT * kKeysU)
kMaxLocalBins = 1024    # k_pc_scatter_lds / k_pc_count: regions a block stages in LDS
kCoarseTile = 4096      # k_pf_coarse reads per tile (kPfT * kPfRPL)
kHeavy = 64             # reads of one bin in a coarse tile above which the bin is deduplicated
kFinePerBin = 8         # sub-bins per coarse bin
kNFill = 128 * kFinePerBin
kFineTile = 8192        # k_pf_scatter records per tile
kHeavyFine = 2
kSlabMinMean = 256
kSlabPad = 256
kOvfTable = 1
SLOTS = 1 << kSliceLogMax
LOAD_BOUND = 1536       # distinct keys per region a case without overflow may hold (3/4 of a slice)

# id: (kind: "ascii" or "keys", L, log2 capacity, GpuCounter.insert's `partitioned`, last_route())
# -- the geometry of CASES in test_counter_routes.py, and the two key-input routes
ROUTES = {
    "opt-g16": ("ascii", 32, 19, True, "optimistic g16 counted cursors"),
    "opt-plain": ("ascii", 16, 19, True, "optimistic plain counted cursors"),
    "opt-keys": ("keys", 32, 19, None, "optimistic keys counted cursors"),
    "exact-keys": ("ascii", 32, 17, True, "exact k_pc_keys one pass"),
    "hist-1": ("ascii", 20, 17, True, "exact k_pc_hist one pass"),
    "hist-2": ("ascii", 20, 19, True, "exact k_pc_hist two passes"),
    "keys-hist-1": ("keys", 32, 17, None, "exact k_pc_hist one pass"),
    "multi-1": ("ascii", 40, 17, None, "exact multi-word one pass"),
    "multi-2": ("ascii", 40, 19, None, "exact multi-word two passes"),
    "direct-g16": ("ascii", 32, 17, False, "direct g16"),
    "direct-gen": ("ascii", 20, 17, False, "direct generic"),
    "hist-2-s33": ("ascii", 32, 19, True, "exact k_pc_hist two passes"),    # rows 33 bytes apart (STRIDES)
}
STRIDES = {"hist-2-s33": 33}      # row stride where it is not L: a wider tensor's first L columns
OPTIMISTIC = ("opt-g16", "opt-plain", "opt-keys")
ASCII_ROUTES = tuple(r for r, v in ROUTES.items() if v[0] == "ascii")


def pool_kind(route):
    kind, L = ROUTES[route][:2]
    return "keys" if kind == "keys" else L


def _oracle():
    import oracle
    oracle.lib()
    return oracle


# ---- packing, fingerprints, placement --------------------------------------------------------------

def pack(rows):
    """ASCII rows uint8 [n, L] -> packed words uint64 [n, W] (oracle.encode_batch)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, L = rows.shape
    words, rc, _err = _oracle().encode_batch(rows.reshape(-1), n, L)
    assert rc == 0
    return words


def fp_np(words):
    """fp_collide.fp of every row of uint64 [n, W] (words_fp, csrc/ss_device.h)."""
    words = np.asarray(words, dtype=np.uint64)
    W = words.shape[1]
    with np.errstate(over="ignore"):
        h = np.full(words.shape[0], fp_collide.seed(W), dtype=np.uint64)
        for j in range(W):
            t = h ^ words[:, j]
            t ^= t >> np.uint64(29)
            h = t * np.uint64(fp_collide.M1)
        h ^= h >> np.uint64(32)
        h = h * np.uint64(fp_collide.M2)
        h ^= h >> np.uint64(29)
    h[h == np.uint64(fp_collide.EMPTY)] = np.uint64(fp_collide.CLAMPED)
    return h


def keys_of(words):
    """The value the table places: the packed word, or a multi-word row's fingerprint."""
    words = np.asarray(words, dtype=np.uint64)
    return words[:, 0].copy() if words.shape[1] == 1 else fp_np(words)


def slice_log_of(lg):
    return min(lg, kSliceLogMax)


def regions(lg):
    return 1 << (lg - slice_log_of(lg))


def region_of(keys, lg):
    with np.errstate(over="ignore"):
        h = np.asarray(keys, dtype=np.uint64) * np.uint64(SLOT_MUL)
    return ((h >> np.uint64(64 - lg)) >> np.uint64(slice_log_of(lg))).astype(np.int64)


def coarse_of(keys, lg):
    rbits = lg - slice_log_of(lg)
    r = region_of(keys, lg)
    return r >> (rbits - kCoarseBits) if rbits > kCoarseBits else r


def regions_per_bin(lg):
    return max(1, regions(lg) >> kCoarseBits)


def part_of_region(region, lg, nparts=64):
    """The extract_ranges part that holds a region."""
    return region * nparts // regions(lg)


def pf_cap1(n):
    """Sub-bin capacity of the optimistic partition for a reservation of n reads."""
    return ((5 * n // 2 + kNFill - 1) // kNFill + 1024 + 15) & ~15


def slab_reservation(lg):
    """The least reservation that turns the fine-pass slabs on (ss_counter_reserve)."""
    return kSlabMinMean * kNFill * (regions(lg) >> kCoarseBits)


# ---- the reference table ---------------------------------------------------------------------------

def unique_rows(words):
    """numpy.unique(words, axis=0, return_index=True, return_counts=True) by a lexsort (the same
    result, test_ref_table_is_oracle_count; the row-wise unique takes seconds on millions of rows)."""
    words = np.asarray(words, dtype=np.uint64)
    n, W = words.shape
    if W == 1:
        u, first, counts = np.unique(words[:, 0], return_index=True, return_counts=True)
        return u[:, None], first, counts
    order = np.lexsort(tuple(words[:, j] for j in range(W - 1, -1, -1)))   # stable: first index leads its run
    s = words[order]
    new = np.ones(n, dtype=bool)
    new[1:] = np.any(s[1:] != s[:-1], axis=1)
    starts = np.nonzero(new)[0]
    return s[starts], order[starts], np.diff(np.append(starts, n))


def ref_table(words, base=0):
    """(rows uint64 [m, W], counts uint64, first indices uint64) of the packed reads, in first-occurrence
    order; first indices are global (base + position)."""
    u, first, counts = unique_rows(words)
    o = np.argsort(first, kind="stable")
    return u[o], counts[o].astype(np.uint64), first[o].astype(np.uint64) + np.uint64(base)


# ---- candidate pools and crafted sets --------------------------------------------------------------

class Pool:
    """Distinct random candidates of one key kind: rows (ASCII uint8 [m, L], or the u64 keys), their
    packed words and the keys the table places.  The sentinel key is not among them."""

    def __init__(self, rows, words, keys):
        self.rows, self.words, self.keys = rows, words, keys


@functools.lru_cache(maxsize=None)
def pool(kind, m=1 << 20):
    rng = np.random.default_rng([20, 0 if kind == "keys" else kind, m])
    if kind == "keys":
        rows = rng.integers(0, 1 << 64, size=m, dtype=np.uint64)
        words = rows[:, None]
    else:
        rows = CODES[rng.integers(0, 4, size=(m, kind))]
        words = pack(rows)
    keys = keys_of(words)
    _, first = np.unique(keys, return_index=True)
    keep = np.sort(first)
    keep = keep[keys[keep] != np.uint64(EMPTY)]
    return Pool(rows[keep], words[keep], keys[keep])


def take(kind, lg, where, m, m_pool=1 << 20):
    """Indices into pool(kind, m_pool) of the first m candidates whose (region, coarse bin) satisfy
    `where(region, coarse)`; fails if the pool holds fewer."""
    p = pool(kind, m_pool)
    sel = np.nonzero(where(region_of(p.keys, lg), coarse_of(p.keys, lg)))[0]
    assert len(sel) >= m, f"pool of {len(p.keys)} holds {len(sel)} such candidates, {m} wanted"
    return sel[:m]


def craft_keys_inverse(rng, lg, region_ids, per_region):
    """Key input through the multiplier's inverse: per_region distinct u64 keys in each of region_ids."""
    rbits = lg - slice_log_of(lg)
    out = []
    for r in region_ids:
        low = rng.integers(0, 1 << (64 - rbits), size=per_region, dtype=np.uint64)
        low = np.unique(low)
        hs = (np.uint64(r) << np.uint64(64 - rbits)) | low
        with np.errstate(over="ignore"):
            out.append(hs * np.uint64(SLOT_INV))
    keys = np.concatenate(out)
    return keys[keys != np.uint64(EMPTY)]


# ---- cases -----------------------------------------------------------------------------------------

class Case:
    """Batches for one route.  batches: ASCII rows uint8 [n, L] or u64 keys [n], inserted in turn with
    a continuing base index from BASE into one table of 2^lg slots."""
    BASE = 11

    def __init__(self, route, name, batches, lg=None, reserve=None, notes=None):
        self.route, self.name, self.batches = route, name, batches
        self.kind, self.L, rlg, self.partitioned, self.route_name = ROUTES[route]
        self.lg = rlg if lg is None else lg
        self.stride = STRIDES.get(route, self.L)
        self.reserve = reserve          # reservation made before the first insert (None: the insert's own)
        self.notes = notes if notes is not None else {}   # figures the CPU conditions computed
        self._words = {}

    @property
    def id(self):
        return f"{self.route}-{self.name}"

    def words(self, i):
        """Packed words uint64 [n, W] of batch i (the keys themselves for key input)."""
        if i not in self._words:
            b = self.batches[i]
            self._words[i] = b[:, None] if self.kind == "keys" else pack(b)
        return self._words[i]

    def base(self, i):
        return self.BASE + sum(len(b) for b in self.batches[:i])

    def ref(self, which=None):
        """Reference table of the batches `which` (default all): rows, counts, global first indices,
        in first-occurrence order."""
        which = list(range(len(self.batches)) if which is None else which)
        pos = np.concatenate([np.arange(len(self.batches[i]), dtype=np.uint64) + np.uint64(self.base(i))
                              for i in which])
        u, f, c = unique_rows(np.concatenate([self.words(i) for i in which]))
        o = np.argsort(pos[f], kind="stable")
        return u[o], c[o].astype(np.uint64), pos[f][o]

    def reserved(self, i):
        """The reservation in force at batch i: `reserve`, or the largest batch so far."""
        return max([self.reserve or 0] + [len(b) for b in self.batches[:i + 1]])


def max_region_load(words, lg):
    """Most distinct keys in one region (the sentinel key of a single-word table lives outside them)."""
    u, _f, _c = unique_rows(words)
    k = keys_of(u)
    if u.shape[1] == 1:
        k = k[k != np.uint64(EMPTY)]
    return int(np.bincount(region_of(k, lg), minlength=1).max()) if len(k) else 0


def assert_load(case):
    load = max_region_load(np.concatenate([case.words(i) for i in range(len(case.batches))]), case.lg)
    assert load <= LOAD_BOUND, f"{case.id}: a region holds {load} distinct keys"
    case.notes["max_region_load"] = load
    return case


def spilled_lower_bound(keys, lg, cap1):
    """Records of one batch that must leave the sub-bins for the spill list, at the least: a coarse
    tile is kCoarseTile consecutive reads; a bin with more than kHeavy reads in a tile leaves one
    record per distinct key, any other bin one per read; a bin's kFinePerBin sub-bins hold cap1 each."""
    cb = coarse_of(keys, lg)
    nbins = 1 << kCoarseBits
    rec = np.zeros(nbins, dtype=np.int64)
    for t0 in range(0, len(keys), kCoarseTile):
        k, b = keys[t0:t0 + kCoarseTile], cb[t0:t0 + kCoarseTile]
        reads = np.bincount(b, minlength=nbins)
        uk = np.unique(k)
        distinct = np.bincount(coarse_of(uk, lg), minlength=nbins)
        rec += np.where(reads > kHeavy, distinct, reads)
    return int(np.maximum(rec - kFinePerBin * cap1, 0).sum())


def _split(rows, parts=2):
    n = len(rows)
    cut = [n * i // parts for i in range(parts + 1)]
    return [rows[cut[i]:cut[i + 1]] for i in range(parts)]


def _rows(kind, idx, m_pool=1 << 20):
    return pool(kind, m_pool).rows[idx]


def _seed(route, name):
    return [7, list(ROUTES).index(route), sum(map(ord, name))]


def sentinel_rows(route, n):
    kind, L = ROUTES[route][:2]
    return np.full(n, EMPTY, dtype=np.uint64) if kind == "keys" else np.full((n, L), ord("G"), dtype=np.uint8)


DISTS = ("one-key", "one-key-zero", "all-distinct", "one-bin", "one-region", "two-point", "two-point-sorted")


def dist_case(route, dist):
    """One of the distributions on one route, about 60 000 to 100 000 reads in two batches."""
    kind = pool_kind(route)
    L, lg = ROUTES[route][1], ROUTES[route][2]
    rng = np.random.default_rng(_seed(route, dist))
    R = regions(lg)
    notes = {}
    if dist == "one-key":
        rows = _rows(kind, np.full(60_000, 5))
    elif dist == "one-key-zero":       # "A" * L: key 0
        rows = np.zeros(60_000, np.uint64) if kind == "keys" else np.full((60_000, L), ord("A"), np.uint8)
    elif dist == "one-key-sentinel":   # "G" * 32: the key that equals the free-slot value
        assert L == 32
        rows = sentinel_rows(route, 60_000)
    elif dist == "one-key-kstar":      # h = ~0: the free-slot mark of the optimistic aggregate's LDS slice is h(~0)
        assert kind == "keys"
        rows = np.full(60_000, KSTAR, dtype=np.uint64)
    elif dist == "all-distinct":       # near the bound's mean load where 100 000 reads reach it
        n = min(100_000, R * 1400)
        rows = _rows(kind, rng.permutation(n))
    elif dist == "one-bin":
        b = 5 % (1 << min(kCoarseBits, lg - slice_log_of(lg)))
        if kind == "keys":
            rpb = regions_per_bin(lg)
            keys = craft_keys_inverse(rng, lg, range(b * rpb, (b + 1) * rpb), 1200)
            rows = keys[rng.integers(0, len(keys), size=100_000)]
        else:
            idx = take(kind, lg, lambda r, c: c == b, 1200 * regions_per_bin(lg))
            rows = _rows(kind, idx[rng.integers(0, len(idx), size=100_000)])
    elif dist == "one-region":         # about 1200 distinct keys of one region, about 60 reads each
        reg = 77 % R
        if kind == "keys":
            keys = craft_keys_inverse(rng, lg, [reg], 1200)
            rows = keys[rng.integers(0, len(keys), size=72_000)]
        else:
            idx = take(kind, lg, lambda r, c: r == reg, 1200)
            rows = _rows(kind, idx[rng.integers(0, len(idx), size=72_000)])
    elif dist in ("two-point", "two-point-sorted"):
        n = 80_000
        ids = rng.integers(1, 1 + n // 8, size=n)
        ids[rng.random(n) < 0.5] = 0           # the hot key
        if dist == "two-point-sorted":
            ids = np.sort(ids)                 # the hot key first: it fills whole tiles
        rows = _rows(kind, ids)
    else:
        raise KeyError(dist)
    case = Case(route, dist, _split(rows), notes=notes)
    assert_load(case)
    if dist == "one-bin" and route in OPTIMISTIC:
        # the sub-bins of the bin run full and records spill (k_spill_insert), in both batches
        for i in range(2):
            lb = spilled_lower_bound(keys_of(case.words(i)), lg, pf_cap1(case.reserved(i)))
            assert lb > 0, f"{case.id}: no spill expected in batch {i}"
            notes[f"spilled_lower_bound_{i}"] = lb
    return case


def dist_ids():
    """(route, distribution) of every distribution case."""
    out = []
    for route in ROUTES:
        kind, L = ROUTES[route][:2]
        for d in DISTS:
            out.append((route, d))
        if L == 32:
            out.append((route, "one-key-sentinel"))
        if kind == "keys":
            out.append((route, "one-key-kstar"))
    return out


# ---- optimistic route on larger tables: the fine scatter's heavy-region dedup, slab overrun ---------
# k_pf_scatter deduplicates a region holding more than max(64, kHeavyFine * kFineTile / nb) records of
# a tile, nb = regions per coarse bin.  At 2^19 slots nb = 2 and the threshold is the whole tile, so
# the branch needs a larger table: 2^22 slots give nb = 16 and a threshold of 1024.

def fine_heavy_at(lg):
    return max(64, kHeavyFine * (kFineTile // regions_per_bin(lg)))


def fine_heavy_case(route, lg=22):
    """A tenth of the reads fall on 480 keys of one region, the rest anywhere.  Per coarse tile
    the region's bin is heavy, so its keys leave the tile once each, most of them as plain records
    (one copy in the tile); a sub-bin collects several tiles' records of the region, more than the
    fine scatter's threshold, with plain records of one key among them: the dedup whose count
    k_pf_scatter takes from its LDS table."""
    assert route in OPTIMISTIC
    kind = pool_kind(route)
    rng = np.random.default_rng(_seed(route, "fine-heavy"))
    reg = 1234 % regions(lg)
    n = 400_000
    if kind == "keys":
        hot = craft_keys_inverse(rng, lg, [reg], 480)
    else:
        hot = _rows(kind, take(kind, lg, lambda r, c: r == reg, 480))
    rows = _rows(kind, rng.integers(0, 1 << 19, size=n))
    pick = rng.random(n) < 0.1
    rows[pick] = hot[rng.integers(0, len(hot), size=int(pick.sum()))]
    # (a reservation of 2^20 reads: sub-bins of 3584 records, so none of this spills in the coarse pass)
    case = Case(route, "fine-heavy", _split(rows), lg=lg, reserve=1 << 20)
    assert_load(case)
    for i in range(2):
        keys = keys_of(case.words(i))
        in_reg = region_of(keys, lg) == reg
        tiles = -(-len(keys) // kCoarseTile)
        assert tiles <= 128    # fewer tiles than any resident grid: tile t is block t, sub-bin t % 8
        recs = np.zeros(kFinePerBin, dtype=np.int64)
        singles = [[] for _ in range(kFinePerBin)]
        for t in range(tiles):
            sl = slice(t * kCoarseTile, (t + 1) * kCoarseTile)
            k = keys[sl][in_reg[sl]]
            assert len(k) > kHeavy
            u, c = np.unique(k, return_counts=True)
            recs[t % kFinePerBin] += len(u)
            singles[t % kFinePerBin].append(u[c == 1])
        assert recs.max() <= kFineTile and pf_cap1(case.reserved(i)) >= recs.max()   # one fine tile, nothing spills
        assert recs.min() > fine_heavy_at(lg), f"{case.id}: {recs.min()} records of the region in a sub-bin"
        folded = sum(int((np.unique(np.concatenate(s), return_counts=True)[1] > 1).sum()) for s in singles)
        assert folded > 100, f"{case.id}: {folded} keys folded by the fine dedup"
        case.notes[f"fine_dedup_keys_{i}"] = folded
    return case


def slab_case(dist, lg=19):
    """The slab route at 2^lg slots: a reservation of slab_reservation(lg) reads, then two batches of
    about 100 000 reads (the reservation decides the route, not the batch)."""
    route = "opt-g16"
    rng = np.random.default_rng(_seed(route, "slab" + dist))
    n = 200_000
    rows = _rows(32, rng.integers(0, n // 8, size=n))
    if dist == "one-region":      # a region's keys, about 60 reads each, mixed into uniform reads
        reg = 99 % regions(lg)
        hot = _rows(32, take(32, lg, lambda r, c: r == reg, 1200))
        pick = rng.random(n) < 0.36
        rows[pick] = hot[rng.integers(0, len(hot), size=int(pick.sum()))]
    elif dist == "two-point":
        rows[rng.random(n) < 0.5] = rows[0]
    else:
        raise KeyError(dist)
    rows[17] = ord("G")           # the sentinel key, once per batch
    rows[n // 2 + 3] = ord("G")
    case = Case(route, f"slab-{dist}-{lg}", _split(rows), lg=lg, reserve=slab_reservation(lg))
    case.route_name = "optimistic g16 slabs"
    return assert_load(case)


def slab_overrun_case(lg=20):
    """Slab overrun: every read in one region of a 2^20 table (4 regions per bin).  A sub-bin's f
    records all belong to one of its 4 slabs of 2 * ceil(f / 4) + kSlabPad slots, so the slab runs
    full once f passes about 512 and the rest goes to the spill list."""
    route = "opt-g16"
    rng = np.random.default_rng(_seed(route, "slab-overrun"))
    reg = 321 % regions(lg)
    hot = _rows(32, take(32, lg, lambda r, c: r == reg, 1200))
    rows = hot[rng.integers(0, len(hot), size=100_000)]
    case = Case(route, f"slab-overrun-{lg}", _split(rows), lg=lg, reserve=slab_reservation(lg))
    case.route_name = "optimistic g16 slabs"
    assert_load(case)
    nb = regions_per_bin(lg)
    for i in range(2):
        keys = keys_of(case.words(i))
        tiles = -(-len(keys) // kCoarseTile)
        assert tiles <= 128
        f = np.zeros(kFinePerBin, dtype=np.int64)      # records per sub-bin: one per distinct key and tile
        for t in range(tiles):
            f[t % kFinePerBin] += len(np.unique(keys[t * kCoarseTile:(t + 1) * kCoarseTile]))
        assert f.max() <= pf_cap1(case.reserved(i))    # nothing spills in the coarse pass
        slab = (2 * -(-f // nb) + kSlabPad + 15) & ~15
        # the fine scatter folds plain records of one key in a tile, never below the distinct keys
        over = np.minimum(f, 1200) - slab
        assert over.max() > 0, f"{case.id}: no slab overrun expected"
        case.notes[f"slab_overrun_lower_bound_{i}"] = int(np.maximum(over, 0).sum())
    return case


# ---- sparse coarse buckets on a large table: the exact two-pass routes' unstaged path -------------

SPARSE_ROUTES = ("hist-2", "multi-2")


def widest_block_span(keys, lg):
    """The most coarse buckets one partition block's range spans in the coarse-sorted order, first
    bucket to last: blocks take per = ceil(n / kPartBlocks) consecutive elements."""
    cb = np.sort(coarse_of(keys, lg))
    n = len(cb)
    per = -(-n // kPartBlocks)
    lo = np.arange(0, n, per)
    hi = np.minimum(lo + per, n) - 1
    return int((cb[hi] - cb[lo] + 1).max())


def sparse_case(route, lg=22):
    """Batches of about 100 000 reads into 2^22 slots (16 regions per coarse bin, 98 reads per partition block):
    one read, here and there two, in each of 120 coarse bins and the rest in one bin, so a block's
    range spans more than 64 buckets = more than kMaxLocalBins regions: k_pc_count counts into the
    global row and k_pc_scatter_lds<false, true> stores unstaged.  Two batches, no reset between."""
    assert route in SPARSE_ROUTES and regions_per_bin(lg) == 16
    kind = pool_kind(route)
    rng = np.random.default_rng(_seed(route, "sparse"))
    p = pool(kind)
    cb = coarse_of(p.keys, lg)
    full_bin = 127
    dense = take(kind, lg, lambda r, c: c == full_bin, 4800)
    batches = []
    for b in range(2):
        sparse = []
        for c in range(120):
            cand = np.nonzero(cb == c)[0]
            sparse += list(cand[2 * b: 2 * b + (2 if c % 6 == 0 else 1)])
        idx = np.concatenate([np.array(sparse), dense[rng.integers(0, len(dense), size=100_000)]])
        batches.append(_rows(kind, rng.permutation(idx)))
    case = Case(route, "sparse", batches, lg=lg)
    case.route_name = ROUTES[route][4]
    assert_load(case)
    for i in range(2):
        keys = keys_of(case.words(i))
        per_bin = np.bincount(coarse_of(keys, lg), minlength=128)
        assert int(((per_bin >= 1) & (per_bin <= 2)).sum()) >= 100
        span = widest_block_span(keys, lg)
        assert span > kMaxLocalBins // regions_per_bin(lg), f"{case.id}: widest block spans {span} buckets"
        case.notes[f"widest_span_{i}"] = span
    return case


# ---- sizes: uniform pools around the tile and grid edges -----------------------------------------

BIG_OPT = kCoarseTile * 1024 + kCoarseTile + 1     # a second tile for some block of any grid <= 1024, last tile of 1
SMALL_SIZES = (1, 2, 63, 64, 65, kPartBlocks - 1, kPartBlocks, kPartBlocks + 1)
ROUTE_SIZES = {
    "opt-g16": (kCoarseTile - 1, kCoarseTile, kCoarseTile + 1),
    "opt-plain": (kCoarseTile - 1, kCoarseTile, kCoarseTile + 1),
    "opt-keys": (kCoarseTile - 1, kCoarseTile, kCoarseTile + 1),
    "direct-g16": (511, 512, 513),      # k_count_g16: 2 lanes per read, 4 reads per lane pair and block of 256
}
# the multi-million sizes, one per route: (n, distinct keys of the pool)
BIG_SIZES = {
    "opt-g16": (BIG_OPT, 1 << 17),
    "opt-plain": (BIG_OPT, 1 << 17),
    "opt-keys": (BIG_OPT, 1 << 17),
    "exact-keys": (kPartBlocks * (kKeysTile + 1), 1 << 16),     # every block: a second tile of one read
    "hist-1": (kPartBlocks * (kTile + 1), 1 << 16),             # every block's scatter: a second tile of one
    "hist-2": (kPartBlocks * (kTile + 1), 1 << 17),
    "keys-hist-1": (kPartBlocks * (kTile + 1), 1 << 16),
    "multi-2": (kPartBlocks * (kTile + 1), 1 << 17),
    "direct-gen": (256 * 16 * 256 + 1, 1 << 16),                # just past the capped grid's first stride
}
BIG_SEEDS = (21, 22)     # synth_pool_reads (seed, pool_seed): pool item j is read j of gen_reads(seed)


def size_ids():
    out = []
    for route in ROUTES:
        for n in SMALL_SIZES + ROUTE_SIZES.get(route, ()):
            out.append((route, n))
    return out


def size_case(route, n):
    """n reads drawn from max(1, n // 8) pool keys, as one batch and the same batch again."""
    kind = pool_kind(route)
    rng = np.random.default_rng(_seed(route, f"size{n}"))
    rows = _rows(kind, rng.integers(0, max(1, n // 8), size=n))
    if ROUTES[route][1] == 32 and n > 2:
        rows[n // 2] = sentinel_rows(route, 1)[0]
    return assert_load(Case(route, f"n{n}", [rows, rows]))


def big_pool_words(route):
    """Packed words of every pool item a BIG_SIZES batch of an ASCII route can draw."""
    L = ROUTES[route][1]
    n, U = BIG_SIZES[route]
    o = _oracle()
    return pack(o.gen_reads(BIG_SEEDS[0], 0, U, L).reshape(U, L))


def big_key_pool(route):
    return pool("keys").keys[:BIG_SIZES[route][1]]


def assert_big_load(route):
    words = big_key_pool(route)[:, None] if ROUTES[route][0] == "keys" else big_pool_words(route)
    load = max_region_load(words, ROUTES[route][2])
    assert load <= LOAD_BOUND, f"{route}: a region of the pool holds {load} distinct keys"
    return load


BIG_ONE_BIN = ("opt-plain", 21)     # the one-bin distribution at BIG_OPT reads on a 2^21 table


@functools.lru_cache(maxsize=None)
def big_one_bin_keys():
    """The 8 x 1200 distinct rows of one coarse bin of a 2^21 table (L = 16): BIG_OPT reads drawn from
    them fill the bin's sub-bins to pf_cap1(BIG_OPT) > kFineTile records, so k_pf_scatter runs a
    second, partial tile; everything else spills."""
    route, lg = BIG_ONE_BIN
    kind = pool_kind(route)
    idx = take(kind, lg, lambda r, c: c == 9, 1200 * regions_per_bin(lg), m_pool=1 << 21)
    rows = _rows(kind, idx, m_pool=1 << 21)
    words = pack(rows)
    assert max_region_load(words, lg) <= LOAD_BOUND
    cap1 = pf_cap1(BIG_OPT)
    assert kFineTile < cap1 < 2 * kFineTile
    # a tile of kCoarseTile draws holds at least 2000 distinct keys of the 9600 (mean 3330): the
    # bin's 8 sub-bins run full after a few tiles each
    assert (BIG_OPT // kCoarseTile) * 2000 > kFinePerBin * cap1
    return rows


# ---- a region that runs full -----------------------------------------------------------------------

FULL_ROUTES = ("opt-g16", "hist-1", "multi-1", "direct-gen", "opt-g16-spill")
CROWD = SLOTS + 256


def full_case(which):
    """One region gets CROWD distinct crafted keys, each twice; every other region ordinary keys within
    the load bound.  -> (case, crowd words uint64 [CROWD, W], crowded region).
    "opt-g16-spill": the crowd's keys arrive through k_spill_insert.  Batch 0 leaves 2000 of them in
    the region (no overflow yet); batch 1 draws every read from the crowd region's coarse bin, whose
    sub-bins run full, so most records -- the 304 new crowd keys' among them -- take the spill list
    and meet the slice the aggregate has just filled, or fill it themselves."""
    route = "opt-g16" if which == "opt-g16-spill" else which
    kind = pool_kind(route)
    lg = ROUTES[route][2]
    rng = np.random.default_rng(_seed(route, "full" + which))
    reg = 41 % regions(lg)
    crowd = take(kind, lg, lambda r, c: r == reg, CROWD)
    p = pool(kind)
    notes = {}
    if which == "opt-g16-spill":
        bin_ = int(coarse_of(p.keys[crowd[:1]], lg)[0])
        others = take(kind, lg, lambda r, c: (c == bin_) & (r != reg), 1200 * (regions_per_bin(lg) - 1))
        b0 = np.concatenate([crowd[:2000], others])
        b1 = np.concatenate([crowd, crowd[2000:], others[rng.integers(0, len(others), size=60_000)],
                             crowd[rng.integers(0, 2000, size=35_000)]])
        batches = [_rows(kind, rng.permutation(b0)), _rows(kind, rng.permutation(b1))]
    else:
        ordinary = take(kind, lg, lambda r, c: r != reg, 40_000)
        idx = np.concatenate([crowd, crowd, ordinary[rng.integers(0, len(ordinary), size=60_000)]])
        batches = _split(_rows(kind, rng.permutation(idx)))
    case = Case(route, "full-" + which, batches, notes=notes)
    allw = np.concatenate([case.words(i) for i in range(2)])
    u, _f, _c = unique_rows(allw)
    k = keys_of(u)
    load = np.bincount(region_of(k, lg), minlength=regions(lg))
    assert load[reg] == CROWD
    load[reg] = 0
    assert load.max() <= LOAD_BOUND
    if which == "opt-g16-spill":
        lb = spilled_lower_bound(keys_of(case.words(1)), lg, pf_cap1(case.reserved(1)))
        assert lb > 20_000
        notes["spilled_lower_bound_1"] = lb
    return case, p.words[crowd], reg
