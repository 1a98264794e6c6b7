#!/usr/bin/env python3
"""Nearest-reference match timings (DESIGN.md "Nearest-reference match"; the log is kept under
profiles/nearest/).  HIP events around the calls; random one-word rows made on the device.

python tools/probe_nearest.py rate              (a) rare hits: 2^20 random queries x 2^17 random references,
                                                L 8 / 12 / 16 / 32, max_dist 1: checked pairs/s = nq * nr / time;
                                                the first 512 queries are compared with ss_host_hamming_nearest
python tools/probe_nearest.py yardstick [LIB]   (b) ss_hamming_all_pairs_ex(..., SS_ALLPAIRS_TILES), count only,
                                                on one random batch of n = 2^19 rows (n (n - 1) / 2 = nq * nr of
                                                (a) less 0.0002 %) at the same L, through the library file LIB
                                                (default: this checkout's): run it on the parent commit's build
python tools/probe_nearest.py frequent          (c) every query an exact match, nr 96 / 1536 / 2^17, L 16:
                                                pairs/s and queries/s
python tools/probe_nearest.py splits            few queries (4096) against 2^20 references: ref_splits 1, auto, 8 .. 256
python tools/probe_nearest.py sweep             (d) barcode.correct's two match paths (host: ss_host_hamming_nearest on
                                                one core; gpu: batch.hamming_nearest with the copies both ways) over
                                                nq * nr from 10^4 to 10^8: where device="auto" should switch
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

dev = torch.device("cuda", 0)
REPS = 10
NQ, NR, N_YARD = 1 << 20, 1 << 17, 1 << 19
LENGTHS = (8, 12, 16, 32)


def event_ms(fn, reps=REPS, warm=2):
    """Median and minimum ms of fn() between two HIP events on the current stream."""
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def random_rows(n, L, seed):
    """n random one-word rows of L nt (2 L random bits, the rest zero) as int64 [n, 1] on the device."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lo = torch.randint(0, 1 << 32, (n,), generator=g, device=dev, dtype=torch.int64)
    hi = torch.randint(0, 1 << 32, (n,), generator=g, device=dev, dtype=torch.int64)
    w = lo | (hi << 32)
    if L < 32:
        w = w & ((1 << (2 * L)) - 1)
    return w.reshape(n, 1).contiguous()


def nearest_call(L_, q, r, L, k, splits=0):
    nq, nr = q.shape[0], r.shape[0]
    ws_bytes = int(L_.ss_hamming_nearest_ws_bytes(nq, nr, L, splits))
    ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.int32, device=dev)
    out = [torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(3)]
    s = torch.cuda.current_stream(dev).cuda_stream

    def fn():
        rc = L_.ss_hamming_nearest_ex(q.data_ptr(), nq, q.shape[1], r.data_ptr(), nr, r.shape[1], L, k, out[0].data_ptr(),
                                      out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws_bytes, splits, s)
        if rc:
            raise SystemExit(f"ss_hamming_nearest_ex failed: {rc}")
    return fn, out, ws_bytes


def host_check(L_, q, r, L, k, out, rows=512):
    hq = np.ascontiguousarray(q[:rows].cpu().numpy().view(np.uint64))
    hr = np.ascontiguousarray(r.cpu().numpy().view(np.uint64))
    h = [np.empty(rows, dtype=np.uint32) for _ in range(3)]
    rc = L_.ss_host_hamming_nearest(hq.ctypes.data, rows, hq.shape[1], hr.ctypes.data, hr.shape[0], hr.shape[1], L, k,
                                    h[0].ctypes.data, h[1].ctypes.data, h[2].ctypes.data)
    same = rc == 0 and all(np.array_equal(o[:rows].cpu().numpy().view(np.uint32), e) for o, e in zip(out, h))
    if not same:
        raise SystemExit("PARITY FAILURE: host and GPU nearest differ")
    return int((h[1] != 0xFFFFFFFF).sum())


def rate():
    from shortseq_amd._native import lib
    L_ = lib()
    for L in LENGTHS:
        q, r = random_rows(NQ, L, 100 + L), random_rows(NR, L, 200 + L)
        fn, out, _ = nearest_call(L_, q, r, L, 1)
        med, mn = event_ms(fn)
        matched = int((out[1] != -1).sum())
        hits512 = host_check(L_, q, r, L, 1, out)
        print(f"(a) rate L={L} nq={NQ} nr={NR} k=1: median {med:.3f} ms min {mn:.3f} ms  "
              f"{NQ * NR / med / 1e9:.2f} T pairs/s  queries matched {matched}  host==gpu on 512 rows True "
              f"({hits512} matched)", flush=True)


def yardstick(path):
    L_ = C.CDLL(path)
    fn_ap = L_.ss_hamming_all_pairs_ex
    fn_ap.restype = C.c_int
    fn_ap.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                      C.c_void_p, C.c_uint32, C.c_void_p]
    n = N_YARD
    pairs = n * (n - 1) // 2
    print(f"(b) yardstick library {os.path.relpath(path, REPO)}: n={n}, pairs {pairs} = nq*nr * {pairs / (NQ * NR):.6f}", flush=True)
    for L in LENGTHS:
        w = random_rows(n, L, 300 + L)
        tot = torch.empty(1, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream

        def fn():
            rc = fn_ap(w.data_ptr(), n, L, 1, 1, None, None, 0, tot.data_ptr(), 1, s)      # SS_ALLPAIRS_TILES, count only
            if rc:
                raise SystemExit(f"ss_hamming_all_pairs_ex failed: {rc}")
        med, mn = event_ms(fn)
        print(f"(b) yardstick L={L} n={n} k=1 tiles count-only: median {med:.3f} ms min {mn:.3f} ms  "
              f"{pairs / med / 1e9:.2f} T pairs/s  pairs within 1: {int(tot.item())}", flush=True)


def frequent():
    from shortseq_amd._native import lib
    L_, L = lib(), 16
    for nr in (96, 1536, 1 << 17):
        r = torch.unique(random_rows(2 * nr, L, 400 + nr))[:nr].reshape(nr, 1).contiguous()
        g = torch.Generator(device=dev)
        g.manual_seed(nr)
        q = r[torch.randint(0, nr, (NQ,), generator=g, device=dev)].contiguous()
        fn, out, _ = nearest_call(L_, q, r, L, 1)
        med, mn = event_ms(fn)
        exact = int((out[1] == 0).sum())
        host_check(L_, q, r, L, 1, out)
        print(f"(c) frequent L={L} nq={NQ} nr={nr} k=1, every query an exact match ({exact} at distance 0): "
              f"median {med:.3f} ms min {mn:.3f} ms  {NQ * nr / med / 1e9:.3f} T pairs/s  {NQ / med / 1e6:.2f} G queries/s",
              flush=True)


def splits():
    from shortseq_amd._native import lib
    L_, L, nq, nr = lib(), 16, 4096, 1 << 20
    q, r = random_rows(nq, L, 500), random_rows(nr, L, 501)
    base = None
    for sp in (1, 0, 8, 32, 64, 128, 256):
        fn, out, ws_bytes = nearest_call(L_, q, r, L, 1, sp)
        med, mn = event_ms(fn)
        got = [o.clone() for o in out]
        base = got if base is None else base
        same = all(torch.equal(a, b) for a, b in zip(got, base))
        print(f"splits L={L} nq={nq} nr={nr} ref_splits={sp or 'auto'}: workspace {ws_bytes} B  median {med:.3f} ms "
              f"min {mn:.3f} ms  {nq * nr / med / 1e9:.2f} T pairs/s  same as ref_splits=1 {same}", flush=True)
        if not same:
            raise SystemExit("PARITY FAILURE: split results differ")


def sweep():
    import shortseq_amd.barcode as BC
    L = 16
    rng = np.random.default_rng(1)
    for nq, nr in ((100, 96), (1000, 96), (3000, 96), (10_000, 96), (30_000, 96), (100_000, 96), (650, 1536), (2000, 1536),
                   (6500, 1536), (65_000, 1536), (1000, 10_000), (10_000, 10_000), (1000, 100_000)):
        r = rng.integers(0, 1 << (2 * L), size=(nr, 1), dtype=np.uint64)
        q = r[rng.integers(0, nr, size=nq)] ^ (np.uint64(1) << rng.integers(0, 2 * L, size=(nq, 1), dtype=np.uint64))
        BC._gpu_match(q, r, L, 1)
        t_gpu, t_host = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            g = BC._gpu_match(q, r, L, 1)
            t_gpu.append(time.perf_counter() - t0)
        for _ in range(3):
            t0 = time.perf_counter()
            h = BC._host_match(q, r, L, 1)
            t_host.append(time.perf_counter() - t0)
        if not (np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1])):
            raise SystemExit("PARITY FAILURE: host and GPU matches differ")
        print(f"(d) sweep L={L} nq={nq} nr={nr} pairs {nq * nr:.1e}: host {min(t_host) * 1e3:.3f} ms  "
              f"gpu incl. copies {min(t_gpu) * 1e3:.3f} ms", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rate"
    if mode == "yardstick":
        from shortseq_amd.build import LIB
        yardstick(os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else LIB)
    else:
        {"rate": rate, "frequent": frequent, "splits": splits, "sweep": sweep}[mode]()
