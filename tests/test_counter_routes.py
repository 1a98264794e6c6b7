"""The counter insert's dispatch: every kernel chain ss_counter_insert_fixed can take (plan_insert in
csrc/ss_counter.hip), pinned by GpuCounter.last_route() and checked against oracle.count.

Capacity 2^19 gives 256 regions (rbits 8: a coarse and a fine pass), 2^17 gives 64 (rbits 6: one
pass).  Each case inserts its reads in thirds into one table (global first indices; the later thirds
meet slices the first wrote), then resets the table and inserts the first third again: the second
round meets the pending reset (the single-word aggregate writes fresh slices, every other route
memsets first).  Every route gets one uniform pool here; test_counter_route_shapes.py runs the same
routes, and the two key-input routes (ss_counter_insert_keys through ctypes), on skewed, crafted and
tile-edge batches.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# id: (L, row stride, log2 capacity, n, partitioned, route)
CASES = {
    "optimistic-cursors": (32, 32, 19, 90_000, True, "optimistic g16 counted cursors"),
    # slabs need a reservation of >= kSlabMinMean * kNFill * (regions / 128) = 524 288 reads; the
    # first third's insert makes the reservation, so a third is at least that large
    "optimistic-slabs": (32, 32, 19, 1_800_000, True, "optimistic g16 slabs"),
    "optimistic-16": (16, 16, 19, 90_000, True, "optimistic plain counted cursors"),
    "exact-keys": (32, 32, 17, 90_000, True, "exact k_pc_keys one pass"),
    "exact-hist-1": (20, 20, 17, 90_000, True, "exact k_pc_hist one pass"),
    "exact-hist-2": (20, 20, 19, 90_000, True, "exact k_pc_hist two passes"),
    "exact-stride33": (32, 33, 19, 90_000, True, "exact k_pc_hist two passes"),
    "multi-1": (40, 40, 17, 60_000, None, "exact multi-word one pass"),
    "multi-2": (40, 40, 19, 60_000, None, "exact multi-word two passes"),
    "direct-g16": (32, 32, 17, 30_000, False, "direct g16"),
    "direct-generic": (20, 20, 17, 30_000, False, "direct generic"),
}


def case_reads(B, device, L, stride, n):
    """n pool reads of L nt over about n / 8 distinct ones, as a flat device buffer of rows `stride`
    bytes apart; "G" * 32 (the key that collides with the table's EMPTY) planted at two reads."""
    reads = B.synth_pool_reads(n, L, 21, 22, max(1, n // 8), device=device)
    if L == 32:
        reads[7] = ord("G")
        reads[n // 2 + 3] = ord("G")
    if stride == L:
        return reads.reshape(-1)
    import torch
    wide = torch.zeros((n, stride), dtype=torch.uint8, device=device)   # a wider tensor's first L columns
    wide[:, :L] = reads
    return wide.reshape(-1)


def thirds(n):
    t = n // 3
    return (0, t), (t, 2 * t), (2 * t, n)


def _assert_table(c, exp, L):
    ec = np.array([cc for (_w, _L, cc, _f) in exp], np.uint64)
    ef = np.array([ff for (_w, _L, _c, ff) in exp], np.uint64)
    if L > 32:
        k, cnt, f = c.items_sorted_words()
        ek = np.array([w for (w, _L, _c, _f) in exp], np.uint64)
    else:
        k, cnt, f = c.items_sorted()
        ek = np.array([w[0] for (w, _L, _c, _f) in exp], np.uint64)
    assert k.shape == ek.shape and np.array_equal(k, ek)
    assert np.array_equal(np.asarray(cnt).astype(np.uint64), ec)
    assert np.array_equal(np.asarray(f).astype(np.uint64), ef)
    assert c.size() == len(exp)
    assert not c.overflowed()


@pytest.mark.parametrize("case", list(CASES))
def test_insert_route(gpu, oracle, case):
    import shortseq_amd.batch as B
    L, stride, lg, n, partitioned, route = CASES[case]
    flat = case_reads(B, gpu, L, stride, n)
    host = flat.cpu().numpy()
    rows = [host[i * stride:i * stride + L].tobytes() for i in range(n)]
    c = B.GpuCounter(1 << lg, device=gpu)
    try:
        assert c.last_route() is None
        for lo, hi in thirds(n):
            c.insert(flat[lo * stride:hi * stride], L, stride=stride, base_index=lo, partitioned=partitioned)
            if lo == 0:
                assert c.last_route() == route
        assert c.last_route() == route
        _assert_table(c, oracle.count(rows), L)
        c.reset()
        lo, hi = thirds(n)[0]
        c.insert(flat[lo * stride:hi * stride], L, stride=stride, base_index=lo, partitioned=partitioned)
        assert c.last_route() == route
        _assert_table(c, oracle.count(rows[lo:hi]), L)
    finally:
        c.close()
