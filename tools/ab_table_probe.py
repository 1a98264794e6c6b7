#!/usr/bin/env python3
"""Two builds of the library over the same seeded inputs, for changes to the counter's slice probe
(ss_counter_merge_words, the drop-in engine's class-ordered and read-order folds and the extract):

  results  the drop-in engine (ss_ingest_add_device + finish) over the f2 workload at both pool
           sizes of bench.py (50M reads of 50-150 nt: read-order rows) and over 1-150 nt reads of
           the same size (class-ordered rows): lengths, counts and words of every distinct key, in
           first-occurrence order, must be equal to the last bit (integers: no tolerance);
  merge    ss_counter_merge_words of 2^22 distinct 3-word rows into a 2^23-slot table, twice (every
           key new, then every key found): the extracted (words, counts, first) sorted by first
           index must be equal, and the ms per call of both builds, alternating, are printed.

The C ABI must be the same in both builds: this checkout's Python layer drives both by swapping the
handle that shortseq_amd._native.lib() returns.

python tools/ab_table_probe.py OLD/libshortseq_amd.so [NEW/libshortseq_amd.so] [n reads]
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import shortseq_amd._native as N  # noqa: E402
import shortseq_amd.batch as B  # noqa: E402
from shortseq_amd.build import LIB  # noqa: E402

dev = torch.device("cuda", 0)


def load(path):
    L_ = C.CDLL(path)
    for name, res, args in N.SIGNATURES + N.INTERNAL_SIGNATURES:
        f = getattr(L_, name)
        f.restype = res
        f.argtypes = args
    return L_


def engine_rows(blob, offs, lens):
    eng = B.DeviceIngest(dev)
    try:
        eng.count(blob, offs, lens)
        return tuple(a.copy() for a in eng.results(copy=False))
    finally:
        eng.close()


def merge_twice(words, counts, first, reps=5):
    W = words.shape[1]
    ms, out = [], None
    for _ in range(reps):
        t = B.GpuCounter(1 << 23, device=dev)
        try:
            N.check(N.lib().ss_counter_set_words(t._h, W), "ss_counter_set_words")
            t.merge_words(words, counts, first)             # (the found scratch is allocated here)
            t.reset()
            N.check(N.lib().ss_counter_set_words(t._h, W), "ss_counter_set_words")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.merge_words(words, counts, first)             # every key new: find misses, claim + publish
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            t.merge_words(words, counts, first)             # every key found
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ms.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
            ovf = int(t.overflow_word().item())
            out = (ovf,) + t.items_sorted_words() if not ovf else (ovf,)
        finally:
            t.close()
    return ms, out


def main():
    libs = {"old": load(os.path.abspath(sys.argv[1])),
            "new": load(os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else LIB)}
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 50_000_000
    bad = 0

    def both(fn):
        out = {}
        for name, L_ in libs.items():
            N._lib = L_
            out[name] = fn()
        return out["old"], out["new"]

    for lo, hi, lu in ((50, 150, 20), (50, 150, 24), (1, 150, 20)):
        N._lib = libs["new"]
        blob, offs, lens = B.synth_ragged_pool_reads(n, 41, 42, 1 << lu, lo, hi, device=dev)
        o, nw = both(lambda: engine_rows(blob, offs, lens))
        ok = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(o, nw))
        bad += not ok
        print(f"engine n={n} L={lo}-{hi} pool=2^{lu}: rows {len(nw[0])} reads counted {int(nw[1].sum())} "
              f"old==new {ok}", flush=True)
        del blob, offs, lens
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    m, W = 1 << 22, 3
    words = torch.randint(-(1 << 62), 1 << 62, (m, W), generator=g, device=dev, dtype=torch.int64)
    counts = torch.arange(1, m + 1, dtype=torch.int64, device=dev)
    first = torch.randperm(m, generator=g, device=dev).to(torch.int64)
    res = {"old": [], "new": []}
    outs = {}
    for _ in range(3):
        for name, L_ in libs.items():
            N._lib = L_
            ms, outs[name] = merge_twice(words, counts, first)
            res[name] += ms
    ok = len(outs["old"]) == 4 and len(outs["new"]) == 4 and all(np.array_equal(a, b) for a, b in zip(outs["old"][1:], outs["new"][1:]))
    bad += not ok
    print(f"merge_words m=2^22 W={W} cap=2^23: overflow old {outs['old'][0]} new {outs['new'][0]} "
          f"entries {len(outs['new'][1]) if ok else '?'} old==new {ok}", flush=True)
    for name in ("old", "new"):
        for k, what in ((0, "new keys"), (1, "found keys")):
            v = sorted(x[k] for x in res[name])
            print(f"merge_words {what} {name}: median {v[len(v) // 2]:.4f} ms  min {v[0]:.4f}  max {v[-1]:.4f}  "
                  f"samples {len(v)}", flush=True)
    print("RESULT", "equal" if not bad else f"{bad} MISMATCHES", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
