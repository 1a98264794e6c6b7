"""UMI dedup at the drop-in level: group a counter's distinct reads into UMI clusters.

``dedup(counter)`` takes a ShortSeqCounter (or any mapping ShortSeq -> count) and groups its keys as
UMI-tools' ``directional``, ``cluster`` or ``adjacency`` method does: keys of equal length within
``max_dist`` substitutions are neighbours, and a cluster is named by its highest-count key (ties: the
key that came first in the mapping).  ``adjacency``: in every connected component the leads are the
shortest count-ordered prefix whose keys and their neighbours cover the component; a lead names its own
cluster and every other key joins its highest-ranked neighbour.  In ranks (count descending, ties by
position): cover[v] = the lowest rank among v and its neighbours, thr = the highest cover in v's
component, v leads iff rank[v] <= thr, else it joins the key of rank cover[v].  UMI-tools leaves keys of
equal count to set iteration order; here they go by position in the mapping under every method.
The grouping itself is ss_cluster_pairs / ss_host_cluster_pairs (include/shortseq_amd.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._native import check, lib

__all__ = ["dedup", "dedup_groups", "AUTO_GPU_MIN_KEYS", "AUTO_GPU_MIN_GROUPED_KEYS"]

METHODS = {"cluster": 0, "directional": 1, "adjacency": 3}
GROUPED_METHODS = {"cluster": 0, "directional": 1}     # dedup_groups' own set
MAX_COUNT = 1 << 62

# device="auto": a length group of at least this many keys goes to the GPU (when there is one).  The
# host path checks every pair with one ss_host_hamming call each, so it grows with the square of the
# group; the GPU path costs its copies, launches and syncs, ~0.21 ms up to 512 keys.  Measured crossover
# on 12-nt pools: host 0.13 ms at 32 keys, 0.29 ms at 48 ("UMI clustering", the sweep).
AUTO_GPU_MIN_KEYS = 40


def _host_group(words: np.ndarray, L: int, counts: np.ndarray, max_dist: int, method: int) -> np.ndarray:
    """Brute-force pairs (ss_host_hamming) + ss_host_cluster_pairs -> rep [g] (group-local indices)."""
    L_ = lib()
    g, W = words.shape
    ham, base, step = L_.ss_host_hamming, words.ctypes.data, 8 * W
    pairs = [(i, j) for i in range(g - 1) for j in range(i + 1, g)
             if ham(base + i * step, base + j * step, L) <= max_dist]
    p = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    # count descending, ties by index: a stable ascending sort of (max - count), exact in u64
    order = np.ascontiguousarray(np.argsort(counts.max() - counts, kind="stable"), dtype=np.uint32)
    rep = np.empty(g, dtype=np.uint32)
    ncl = C.c_uint64(0)
    check(L_.ss_host_cluster_pairs(p.ctypes.data, p.shape[0], g, counts.ctypes.data, order.ctypes.data, method,
                                   rep.ctypes.data, None, None, C.byref(ncl)), "ss_host_cluster_pairs")
    return rep.astype(np.int64)


def _gpu_group(words: np.ndarray, L: int, counts: np.ndarray, max_dist: int, method: str) -> np.ndarray:
    import torch

    from . import batch as B
    dev = torch.device("cuda", torch.cuda.current_device())
    d_words = torch.from_numpy(words.view(np.int64)).to(dev)
    d_counts = torch.from_numpy(counts.view(np.int64)).to(dev)
    rep = B.umi_cluster(d_words, L, max_dist, d_counts, method)[0]
    return rep.cpu().numpy()


def _gpu_available() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def dedup(counter, max_dist: int = 1, method: str = "directional", device: str = "auto"):
    """-> (clusters, assignment): clusters maps each representative to its cluster's summed count,
    inserted by descending summed count, ties by the representative's first occurrence in `counter`;
    assignment maps every key of `counter` to its representative (in `counter`'s order).
    Keys are grouped by length first: reads of different lengths never share a cluster.
    device: "host" (every pair checked with ss_host_hamming, then ss_host_cluster_pairs), "gpu"
    (batch.umi_cluster), or "auto" (per length group: "gpu" from AUTO_GPU_MIN_KEYS keys on, when a GPU
    is present)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}")
    if device not in ("auto", "host", "gpu"):
        raise ValueError('device must be "auto", "host" or "gpu"')
    keys = list(counter.keys())
    cnts = [int(counter[k]) for k in keys]
    if any(c < 0 or c > MAX_COUNT for c in cnts):
        raise ValueError("counts must lie in 0 .. 2^62")
    groups: dict = {}
    for idx, k in enumerate(keys):
        groups.setdefault(len(k), []).append(idx)
    rep_of = list(range(len(keys)))
    have_gpu = None
    for L, members in groups.items():
        g = len(members)
        if g < 2:
            continue
        W = max(1, (L + 31) // 32)
        words = np.array([keys[i].packed for i in members], dtype=np.uint64).reshape(g, W)
        counts = np.array([cnts[i] for i in members], dtype=np.uint64)
        where = device
        if where == "auto":
            if have_gpu is None:
                have_gpu = _gpu_available()
            where = "gpu" if have_gpu and g >= AUTO_GPU_MIN_KEYS else "host"
        if where == "gpu":
            rep = _gpu_group(words, L, counts, max_dist, method)
        else:
            rep = _host_group(words, L, counts, max_dist, METHODS[method])
        for local, i in enumerate(members):
            rep_of[i] = members[int(rep[local])]
    sums: dict = {}
    for i, r in enumerate(rep_of):
        sums[r] = sums.get(r, 0) + cnts[i]
    ranked = sorted(sums, key=lambda r: (-sums[r], r))
    clusters = {keys[r]: sums[r] for r in ranked}
    assignment = {keys[i]: keys[r] for i, r in enumerate(rep_of)}
    return clusters, assignment


# dedup_groups, device="auto": the rows of one length from all groups go to the GPU from this many on
# (when there is one).  Both paths are linear in the rows for groups of a few keys: the host path is
# one C++ pass over the groups, the GPU path pays its copies, the offset check, the launches and the
# cluster rounds' syncs, ~0.4 ms up to 3·10^4 keys.  Measured on 12-nt keys in groups around 4: host
# 0.264 ms at 8192 keys, 0.489 ms at 16384; GPU 0.449 and 0.436 ms ("Grouped all-pairs", the sweep).
AUTO_GPU_MIN_GROUPED_KEYS = 16384


def _host_grouped(words: np.ndarray, L: int, counts: np.ndarray, offsets: np.ndarray, max_dist: int,
                  method: int) -> np.ndarray:
    """ss_host_hamming_all_pairs_grouped + ss_host_cluster_pairs -> rep [n] (global row indices)."""
    L_ = lib()
    n, W = words.shape
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    cap = max(1, 4 * n)
    tot = C.c_uint64(0)
    while True:      # a pair buffer of 4 n, one more run with exactly the total when that was too small
        p = np.empty((cap, 2), dtype=np.uint32)
        check(L_.ss_host_hamming_all_pairs_grouped(words.ctypes.data, n, L, W, max_dist, off.ctypes.data, off.size - 1,
                                                   None, p.ctypes.data, cap, C.byref(tot)),
              "ss_host_hamming_all_pairs_grouped")
        if tot.value <= cap:
            break
        cap = tot.value
    order = np.ascontiguousarray(np.argsort(counts.max() - counts, kind="stable"), dtype=np.uint32)
    rep = np.empty(n, dtype=np.uint32)
    ncl = C.c_uint64(0)
    check(L_.ss_host_cluster_pairs(p.ctypes.data, tot.value, n, counts.ctypes.data, order.ctypes.data, method,
                                   rep.ctypes.data, None, None, C.byref(ncl)), "ss_host_cluster_pairs")
    return rep.astype(np.int64)


def _gpu_grouped(words: np.ndarray, L: int, counts: np.ndarray, offsets: np.ndarray, max_dist: int,
                 method: str) -> np.ndarray:
    import torch

    from . import batch as B
    dev = torch.device("cuda", torch.cuda.current_device())
    d_words = torch.from_numpy(words.view(np.int64)).to(dev)
    d_counts = torch.from_numpy(counts.view(np.int64)).to(dev)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    return B.umi_cluster_grouped(d_words, L, max_dist, d_off, d_counts, method)[0].cpu().numpy()


def dedup_groups(groups, max_dist: int = 1, method: str = "directional", device: str = "auto"):
    """UMI dedup of many groups at once: `groups` maps a label (any hashable, e.g. (cell, gene)) to a
    ShortSeqCounter or any mapping ShortSeq -> count.  -> {label: (clusters, assignment)} in `groups`'
    order, each value equal to dedup(groups[label], max_dist, method), dict order included.
    UMIs are compared inside a group only, and keys of different lengths never cluster.  The rows of one
    length from all labels form one batch sorted by label with one offsets array: on the GPU one
    batch.umi_cluster_grouped call per distinct length, on the host ss_host_hamming_all_pairs_grouped +
    ss_host_cluster_pairs.  Clustering the batch on global row indices names the representatives a run
    per group would ("Grouped all-pairs").  device: "host", "gpu", or "auto" (per length:
    "gpu" from AUTO_GPU_MIN_GROUPED_KEYS rows on, when a GPU is present).
    method: "directional" or "cluster".  "adjacency" is refused here (ValueError); the grouped form of it
    is available through batch.umi_cluster_grouped."""
    if method not in GROUPED_METHODS:
        raise ValueError(f"method must be one of {sorted(GROUPED_METHODS)}")
    if device not in ("auto", "host", "gpu"):
        raise ValueError('device must be "auto", "host" or "gpu"')
    labels = list(groups.keys())
    keys_of, cnts_of = [], []
    for lab in labels:
        counter = groups[lab]
        keys = list(counter.keys())
        cnts = [int(counter[k]) for k in keys]
        if any(c < 0 or c > MAX_COUNT for c in cnts):
            raise ValueError("counts must lie in 0 .. 2^62")
        keys_of.append(keys)
        cnts_of.append(cnts)
    by_len: dict = {}                      # L -> rows (label index, key index), sorted by label
    for li, keys in enumerate(keys_of):
        for ki, k in enumerate(keys):
            by_len.setdefault(len(k), []).append((li, ki))
    rep_of = [list(range(len(keys))) for keys in keys_of]
    have_gpu = None
    for L, rows in by_len.items():
        n = len(rows)
        lab_idx = np.fromiter((li for li, _ in rows), dtype=np.int64, count=n)
        offsets = np.searchsorted(lab_idx, np.arange(len(labels) + 1))
        if np.diff(offsets).max() < 2:     # no group with a pair to look for
            continue
        W = max(1, (L + 31) // 32)
        words = np.array([keys_of[li][ki].packed for li, ki in rows], dtype=np.uint64).reshape(n, W)
        counts = np.array([cnts_of[li][ki] for li, ki in rows], dtype=np.uint64)
        where = device
        if where == "auto":
            if have_gpu is None:
                have_gpu = _gpu_available()
            where = "gpu" if have_gpu and n >= AUTO_GPU_MIN_GROUPED_KEYS else "host"
        if where == "gpu":
            rep = _gpu_grouped(words, L, counts, offsets, max_dist, method)
        else:
            rep = _host_grouped(words, L, counts, offsets, max_dist, GROUPED_METHODS[method])
        for (li, ki), r in zip(rows, rep):
            rep_of[li][ki] = rows[int(r)][1]
    out = {}
    for lab, keys, cnts, reps in zip(labels, keys_of, cnts_of, rep_of):
        sums: dict = {}
        for i, r in enumerate(reps):
            sums[r] = sums.get(r, 0) + cnts[i]
        ranked = sorted(sums, key=lambda r: (-sums[r], r))
        out[lab] = ({keys[r]: sums[r] for r in ranked}, {keys[i]: keys[r] for i, r in enumerate(reps)})
    return out
