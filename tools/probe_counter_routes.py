#!/usr/bin/env python3
"""Every insert route of the counter once (the case table of tests/test_counter_routes.py: three
inserts of thirds, a reset, one more insert), for a kernel trace of the dispatch:

    scripts/gpu.sh libprof counter_routes . "old new" -- python tools/probe_counter_routes.py
"""
import importlib.util
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import shortseq_amd.batch as B  # noqa: E402

spec = importlib.util.spec_from_file_location("routes", os.path.join(REPO, "tests", "test_counter_routes.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def main():
    dev = torch.device("cuda", 0)
    sizes = []
    for case, (L, stride, lg, n, partitioned, _route) in T.CASES.items():
        flat = T.case_reads(B, dev, L, stride, n)
        c = B.GpuCounter(1 << lg, device=dev)
        first = T.thirds(n)[0]
        for lo, hi in T.thirds(n) + ((None, None), first):
            if lo is None:
                c.reset()
                continue
            c.insert(flat[lo * stride:hi * stride], L, stride=stride, base_index=lo, partitioned=partitioned)
        sizes.append(f"{case} {c.size()}")
        c.close()
    print("table sizes after the last insert:", ", ".join(sizes), flush=True)


if __name__ == "__main__":
    main()
