#!/usr/bin/env python3
"""Two builds of the library over the same seeded inputs: hamming_all_pairs (every method that accepts
the case), hamming_nearest and hamming_all_pairs_grouped at the sizes tools/probe_f4.py,
tools/probe_nearest.py, tools/probe_grouped.py and the benchmark's F4 cases time.  Integer work: the
counts, totals, sorted pair lists and (idx, dist, nbest) must be equal, between the two builds and,
for all-pairs, between the methods.  The all-pairs inputs are the benchmark's (synth_reads /
synth_pool_reads, seed 7); the nearest and grouped inputs are this script's own, at the probes' sizes
(not their rows: the matched counts differ from the probes' logs).  A one-off A/B tool: the C ABI must
be the same in both builds, since this checkout's Python layer drives both by swapping the handle
that shortseq_amd._native.lib() returns.

python tools/ab_hamming_results.py OLD/libshortseq_amd.so [NEW/libshortseq_amd.so]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import shortseq_amd._native as N  # noqa: E402
import shortseq_amd.batch as B  # noqa: E402
from shortseq_amd.build import LIB  # noqa: E402

dev = torch.device("cuda", 0)
PAIR_CAP = 4_000_000      # pair lists are compared up to this many pairs; past it, counts and totals

# (n, L, k, pool): probe_f4.py's default, multiword and long cases and the benchmark's F4 entries
ALL_PAIRS = ((100_000, 12, 1, None), (200_000, 12, 1, None), (1_000_000, 12, 1, None), (100_000, 16, 2, None),
             (50_000, 32, 2, None), (200_000, 32, 3, None), (100_000, 8, 1, None), (20_000, 96, 4, None),
             (100_000, 64, 2, None), (100_000, 96, 3, None), (100_000, 128, 4, None), (200_000, 100, 1, None),
             (1_000_000, 96, 2, None), (100_000, 40, 5, None), (100_000, 96, 3, 1 << 16),
             (100_000, 150, 3, 1 << 16), (100_000, 250, 5, 1 << 16), (50_000, 1024, 16, 1 << 15),
             (100_000, 150, 3, None), (100_000, 150, 3, 64))


def load(path):
    L_ = C.CDLL(path)
    for name, res, args in N.SIGNATURES + N.INTERNAL_SIGNATURES:
        f = getattr(L_, name)
        f.restype = res
        f.argtypes = args
    return L_


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(torch.equal(a, b))


def main():
    libs = {"old": load(os.path.abspath(sys.argv[1])), "new": load(os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else LIB)}
    bad = 0

    def both(fn):
        out = {}
        for name, L_ in libs.items():
            N._lib = L_
            out[name] = fn()
        N._lib = libs["new"]
        return out["old"], out["new"]

    N._lib = libs["new"]
    for n, L, k, pool in ALL_PAIRS:
        a = B.synth_reads(n, L, seed=7, device=dev) if pool is None else B.synth_pool_reads(n, L, 7, 8, pool, device=dev)
        w = B.encode(a, L)
        W = w.shape[1]
        _, _, total = B.hamming_all_pairs(w, L, k, counts=False, method="tiles")
        cap = total if total <= PAIR_CAP else 0
        ref = None
        for m in ("tiles", "pigeonhole", "bucketed", "auto"):
            if m == "pigeonhole" and (W > 4 or k >= 16):
                continue
            o, nw = both(lambda: B.hamming_all_pairs(w, L, k, max_pairs=cap, method=m))
            ok = o[2] == nw[2] and same(o[0], nw[0]) and same(o[1], nw[1])
            if ref is None:
                ref = nw
            ok_m = nw[2] == ref[2] and same(nw[0], ref[0]) and same(nw[1], ref[1])
            bad += (not ok) + (not ok_m)
            print(f"all_pairs n={n} L={L} k={k} pool={pool} {m}: total {nw[2]} pairs compared {cap} "
                  f"old==new {ok} method==tiles {ok_m}", flush=True)
    # probe_nearest.py rate: 2^20 random queries x 2^17 random references, max_dist 1
    g = torch.Generator(device=dev)
    for L in (8, 12, 16, 32):
        g.manual_seed(100 + L)
        q = torch.randint(0, 1 << 62, (1 << 20, 1), generator=g, device=dev, dtype=torch.int64) & ((1 << (2 * L)) - 1 if L < 32 else -1)
        r = torch.randint(0, 1 << 62, (1 << 17, 1), generator=g, device=dev, dtype=torch.int64) & ((1 << (2 * L)) - 1 if L < 32 else -1)
        o, nw = both(lambda: B.hamming_nearest(q, r, L, 1))
        ok = all(same(x, y) for x, y in zip(o, nw))
        bad += not ok
        print(f"nearest nq=2^20 nr=2^17 L={L} k=1: matched {int((nw[0] >= 0).sum())} old==new {ok}", flush=True)
    # probe_grouped.py (a) and (c): 10^6 12-nt rows in groups around 4, with and without 20 groups of 10^4
    for heavy in (0, 20):
        rng = np.random.default_rng(1 + heavy)
        sizes = rng.geometric(0.25, size=400_000)
        sizes = sizes[:np.searchsorted(np.cumsum(sizes), 1_000_000 - heavy * 10_000)]
        if heavy:
            sizes = np.insert(sizes, np.sort(rng.choice(sizes.size, size=heavy, replace=False)), 10_000)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
        n = int(off[-1].item())
        g.manual_seed(5 + heavy)
        # 2^12 distinct UMIs: neighbours and duplicates inside the groups
        w = (torch.randint(0, 1 << 12, (n, 1), generator=g, device=dev, dtype=torch.int64) * 0x9E3779B1) & ((1 << 24) - 1)
        N._lib = libs["new"]
        _, _, total = B.hamming_all_pairs_grouped(w, 12, 1, off, counts=False)
        cap = total if total <= PAIR_CAP else 0
        o, nw = both(lambda: B.hamming_all_pairs_grouped(w, 12, 1, off, max_pairs=cap))
        ok = o[2] == nw[2] and same(o[0], nw[0]) and same(o[1], nw[1])
        bad += not ok
        print(f"grouped n={n} groups={sizes.size} heavy={heavy} L=12 k=1: total {nw[2]} pairs compared {cap} old==new {ok}",
              flush=True)
    print("RESULT", "equal" if not bad else f"{bad} MISMATCHES", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
