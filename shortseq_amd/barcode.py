"""Barcode correction at the drop-in level: match a counter's reads against a whitelist.

``correct(counter, whitelist)`` takes a ShortSeqCounter (or any mapping ShortSeq -> count) and a list of
known barcodes (cell barcodes, sample indices, guide / feature barcodes) of one length, and assigns every
key to its nearest whitelist entry within ``max_dist`` substitutions.  The match itself is
ss_hamming_nearest / ss_host_hamming_nearest (include/shortseq_amd.h): per key the minimum distance,
the lowest whitelist index at it, and how many entries lie at it (an ambiguous key has more than one).
"""
from __future__ import annotations

import numpy as np

from ._native import check, lib

__all__ = ["correct", "AUTO_GPU_MIN_PAIRS"]

# device="auto": from this many (key, whitelist entry) pairs on the match goes to the GPU (when there
# is one).  Measured (tools/probe_nearest.py sweep, 16 nt; DESIGN.md, "Nearest-reference match", table
# (d)): the host loop costs 1.2 ns per one-word pair on one core, the GPU path (two copies in, the call,
# the copy back) 0.13 .. 0.40 ms whatever the size up to 10^8 pairs.  They cross between 10^5 pairs
# (host 0.125 ms, GPU 0.153 ms) and 3 * 10^5 (0.357 against 0.164 ms at 96 entries); at 1536 entries
# the GPU path costs 0.30 ms, which the host reaches at 2.5 * 10^5 pairs.
AUTO_GPU_MIN_PAIRS = 250_000


def _as_shortseq(x):
    from . import ShortSeq64, ShortSeq192, ShortSeqVar, pack
    return x if isinstance(x, (ShortSeq64, ShortSeq192, ShortSeqVar)) else pack(x)


def _words(seqs, W: int) -> np.ndarray:
    return np.array([s.packed for s in seqs], dtype=np.uint64).reshape(len(seqs), W)


def _host_match(q: np.ndarray, r: np.ndarray, L: int, max_dist: int):
    nq, nr = q.shape[0], r.shape[0]
    idx = np.empty(nq, dtype=np.uint32)
    dist = np.empty(nq, dtype=np.uint32)
    nbest = np.empty(nq, dtype=np.uint32)
    check(lib().ss_host_hamming_nearest(q.ctypes.data, nq, q.shape[1], r.ctypes.data, nr, r.shape[1], L, max_dist,
                                        idx.ctypes.data, dist.ctypes.data, nbest.ctypes.data), "ss_host_hamming_nearest")
    return np.where(idx == 0xFFFFFFFF, -1, idx.astype(np.int64)), nbest.astype(np.int64)


def _gpu_match(q: np.ndarray, r: np.ndarray, L: int, max_dist: int):
    import torch

    from . import batch as B
    dev = torch.device("cuda", torch.cuda.current_device())
    idx, _dist, nbest = B.hamming_nearest(torch.from_numpy(q.view(np.int64)).to(dev),
                                          torch.from_numpy(r.view(np.int64)).to(dev), L, max_dist)
    return idx.cpu().numpy(), nbest.cpu().numpy()


def _gpu_available() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def correct(counter, whitelist, max_dist: int = 1, *, ambiguous: str = "drop", device: str = "auto"):
    """-> (corrected, assignment).
    whitelist: a sequence of str / bytes / ShortSeq of one length; mixed lengths or a duplicated entry
    raise ValueError.
    assignment maps every key of `counter`, in its order, to a whitelist ShortSeq or None: None when the
    key has another length, when no entry lies within `max_dist` substitutions, or when more than one
    entry lies at the minimum distance and ambiguous="drop" (ambiguous="first" takes the lowest
    whitelist index instead).
    corrected maps the whitelist entries with a nonzero total to their summed counts, in whitelist order.
    device: "host" (ss_host_hamming_nearest), "gpu" (batch.hamming_nearest), or "auto" ("gpu" from
    AUTO_GPU_MIN_PAIRS key-entry pairs on, when a GPU is present)."""
    if ambiguous not in ("drop", "first"):
        raise ValueError('ambiguous must be "drop" or "first"')
    if device not in ("auto", "host", "gpu"):
        raise ValueError('device must be "auto", "host" or "gpu"')
    if max_dist < 0:
        raise ValueError("max_dist must be >= 0")
    wl = [_as_shortseq(x) for x in whitelist]
    if len({len(w) for w in wl}) > 1:
        raise ValueError("whitelist entries must all have one length")
    if len(set(wl)) != len(wl):
        raise ValueError("whitelist has a duplicated entry")
    keys = list(counter.keys())
    assignment = dict.fromkeys(keys)
    if not wl or not keys:
        return {}, assignment
    L = len(wl[0])
    members = [i for i, k in enumerate(keys) if len(k) == L]
    if not members or L == 0:
        return {}, assignment
    W = max(1, (L + 31) // 32)
    q = _words([keys[i] for i in members], W)
    r = _words(wl, W)
    where = device
    if where == "auto":
        where = "gpu" if len(members) * len(wl) >= AUTO_GPU_MIN_PAIRS and _gpu_available() else "host"
    idx, nbest = (_gpu_match if where == "gpu" else _host_match)(q, r, L, min(max_dist, 0xFFFFFFFF))
    totals = [0] * len(wl)
    for local, i in enumerate(members):
        j = int(idx[local])
        if j < 0 or (nbest[local] > 1 and ambiguous == "drop"):
            continue
        assignment[keys[i]] = wl[j]
        totals[j] += int(counter[keys[i]])
    corrected = {wl[j]: t for j, t in enumerate(totals) if t}
    return corrected, assignment
