#!/usr/bin/env python3
"""UMI clustering timings (DESIGN.md "UMI clustering"; the log is kept under profiles/cluster/).

python tools/probe_cluster.py          ss_cluster_pairs alone and the whole batch.umi_cluster (HIP events),
                                       every method (cluster, directional, adjacency), against (a) ss_host_cluster_pairs on one core over
                                       the same pairs and (b) the ss_hamming_all_pairs_ex call that
                                       produced them: rounds, pairs/s, cluster step / (b)
python tools/probe_cluster.py sweep    umi.dedup's two paths per length group (host: one ss_host_hamming
                                       call per pair + ss_host_cluster_pairs; gpu: batch.umi_cluster incl.
                                       the copies) over 12-nt pools: where device="auto" should switch
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import shortseq_amd.batch as B  # noqa: E402
import shortseq_amd.umi as U  # noqa: E402
from shortseq_amd._native import check, lib  # noqa: E402

dev = torch.device("cuda", 0)
REPS = 10


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


def synth_counts(n, seed):
    """Heavy-tailed counts with many ties (most UMIs seen once or twice, a few often)."""
    rng = np.random.default_rng(seed)
    return np.minimum(np.floor(1.0 / rng.random(n)), 1 << 20).astype(np.uint64)


def case(n, L, k):
    words = B.encode(B.synth_reads(n, L, seed=7, device=dev), L)
    counts_np = synth_counts(n, 11)
    counts = torch.from_numpy(counts_np.view(np.int64)).to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    L_ = lib()
    tot = torch.empty(1, dtype=torch.int64, device=dev)
    check(L_.ss_hamming_all_pairs_ex(words.data_ptr(), n, L, words.shape[1], k, None, None, 0, tot.data_ptr(), 0, s), "count")
    m = int(tot.item())
    pairs = torch.empty((max(1, m), 2), dtype=torch.int32, device=dev)

    def all_pairs():
        check(L_.ss_hamming_all_pairs_ex(words.data_ptr(), n, L, words.shape[1], k, None, pairs.data_ptr(), m,
                                         tot.data_ptr(), 0, s), "all pairs")
    ap_med, ap_min = event_ms(all_pairs)
    order = torch.sort(counts, descending=True, stable=True).indices.to(torch.int32)
    ws_sizes = {code: int(L_.ss_cluster_ws_bytes_method(n, m, code)) for code in B.CLUSTER_METHODS.values()}
    ws = torch.empty(max(ws_sizes.values()) // 8 + 1, dtype=torch.int64, device=dev)
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.empty(n, dtype=torch.int64, device=dev)
    ncl = torch.empty(1, dtype=torch.int64, device=dev)
    rounds = C.c_uint32(0)
    h_pairs = pairs[:m].cpu().numpy().view(np.uint32)
    h_order = order.cpu().numpy().view(np.uint32)
    print(f"case n={n} L={L} k={k}: pairs={m}  all-pairs (b) median {ap_med:.3f} ms min {ap_min:.3f} ms", flush=True)
    for method, code in B.CLUSTER_METHODS.items():
        ws_bytes = ws_sizes[code]

        def cluster():
            check(L_.ss_cluster_pairs(pairs.data_ptr(), m, n, counts.data_ptr(), order.data_ptr(), code, ws.data_ptr(),
                                      ws_bytes, rep.data_ptr(), sizes.data_ptr(), sums.data_ptr(), ncl.data_ptr(),
                                      C.byref(rounds), s), "ss_cluster_pairs")
        cl_med, cl_min = event_ms(cluster)
        whole_med, whole_min = event_ms(lambda: B.umi_cluster(words, L, k, counts, method, max_pairs_hint=m), reps=5)
        h_rep = np.empty(n, dtype=np.uint32)
        h_sizes = np.empty(n, dtype=np.uint32)
        h_sums = np.empty(n, dtype=np.uint64)
        h_ncl = C.c_uint64(0)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            check(L_.ss_host_cluster_pairs(h_pairs.ctypes.data, m, n, counts_np.ctypes.data, h_order.ctypes.data, code,
                                           h_rep.ctypes.data, h_sizes.ctypes.data, h_sums.ctypes.data, C.byref(h_ncl)),
                  "ss_host_cluster_pairs")
            host.append((time.perf_counter() - t0) * 1e3)
        same = np.array_equal(rep.cpu().numpy().view(np.uint32), h_rep) and int(ncl.item()) == h_ncl.value
        print(f"  {method:11s} rounds {rounds.value}  clusters {int(ncl.item())}  host==gpu {same}  "
              f"ss_cluster_pairs median {cl_med:.3f} ms min {cl_min:.3f} ms ({m / cl_med / 1e3:.1f} M pairs/s)  "
              f"cluster/(b) {cl_med / ap_med:.3f}  umi_cluster median {whole_med:.3f} ms min {whole_min:.3f} ms  "
              f"(a) host one core min {min(host):.3f} ms", flush=True)
        if not same:
            raise SystemExit("PARITY FAILURE: host and GPU clusters differ")


def sweep():
    """Per length group, as umi.dedup runs it (the key unpacking before it is common to both paths)."""
    host_limit_s = 60.0
    host_rate = None
    for g in (8, 16, 24, 32, 48, 64, 128, 256, 512, 1000, 3000, 10_000, 100_000, 1_000_000):
        rng = np.random.default_rng(g)
        codes = np.unique(rng.integers(0, 1 << 24, size=2 * g, dtype=np.uint64))   # distinct 12-nt keys
        words = np.ascontiguousarray(rng.permutation(codes)[:g].reshape(g, 1))
        counts = synth_counts(g, 3)
        U._gpu_group(words, 12, counts, 1, "directional")
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            r_gpu = U._gpu_group(words, 12, counts, 1, "directional")
            t.append(time.perf_counter() - t0)
        gpu_ms = min(t) * 1e3
        if host_rate is None or g * g / 2 / host_rate < host_limit_s:
            t0 = time.perf_counter()
            r_host = U._host_group(words, 12, counts, 1, 1)
            host_s = time.perf_counter() - t0
            host_rate = g * g / 2 / host_s
            if not np.array_equal(r_host, r_gpu):
                raise SystemExit("PARITY FAILURE: host and GPU groups differ")
            host = f"{host_s * 1e3:.3f} ms"
        else:
            host = f"not run (quadratic: ~{g * g / 2 / host_rate:.0f} s at the last measured pair rate)"
        print(f"sweep keys {g}: gpu {gpu_ms:.3f} ms  host {host}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "sweep":
        sweep()
    else:
        for n, L, k in ((100_000, 12, 1), (1_000_000, 12, 1), (100_000, 12, 2)):
            case(n, L, k)
