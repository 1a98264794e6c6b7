#!/usr/bin/env python3
"""Grouped all-pairs hamming timings (DESIGN.md "Grouped all-pairs"; the log is kept under profiles/grouped/).

python tools/probe_grouped.py          12-nt UMIs, counts ~1/u, k = 1 (HIP events, medians):
                                       (a) 10^6 rows in groups of geometric sizes around 4, (b) 10^7 rows, same
                                       sizes, (c) 10^6 rows with a heavy tail (20 groups of 10^4 rows):
                                       ss_hamming_all_pairs_grouped, pairs checked per second, the whole
                                       batch.umi_cluster_grouped; then the first 2000 groups of (a) as a loop of
                                       batch.umi_cluster (the only way before the grouped call) against one
                                       umi_cluster_grouped over the same rows; then (d) ONE group of 10^3 .. 10^5
                                       rows against ss_hamming_all_pairs_ex TILES and AUTO on the same rows
python tools/probe_grouped.py sweep    umi.dedup_groups' two paths per length (host: ss_host_hamming_all_pairs_grouped
                                       + ss_host_cluster_pairs; gpu: batch.umi_cluster_grouped incl. the copies)
                                       over 2^8 .. 2^20 keys in groups around 4: where device="auto" should switch
"""
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
L, K = 12, 1


def event_ms(fn, reps=10, warm=2):
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


def group_sizes(n, seed, heavy=0, heavy_rows=10_000):
    """Geometric sizes of mean 4 (>= 1) summing to n, `heavy` groups of heavy_rows rows spread among them."""
    rng = np.random.default_rng(seed)
    sizes = rng.geometric(0.25, size=n // 3 + 16)
    sizes = sizes[:np.searchsorted(np.cumsum(sizes), n - heavy * heavy_rows)]
    if heavy:
        at = np.sort(rng.choice(sizes.size, size=heavy, replace=False))
        sizes = np.insert(sizes, at, heavy_rows)
    rest = n - int(sizes.sum())
    return np.append(sizes, rest) if rest else sizes


def synth(sizes, seed):
    """-> (words int64 [n, 1], counts int64 [n], offsets int64 [g + 1]) on the device: random 12-nt UMIs, three
    rows in ten a copy of an earlier row of their group with one substitution (sequencing errors), counts ~1/u."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
    n = int(off[-1].item())
    words = torch.randint(0, 1 << (2 * L), (n,), generator=g, device=dev, dtype=torch.int64)
    first = off[:-1].repeat_interleave(torch.from_numpy(np.asarray(sizes, dtype=np.int64)).to(dev))
    row = torch.arange(n, device=dev)
    err = (torch.rand(n, generator=g, device=dev) < 0.3) & (first != row)
    src = first + (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * (row - first)).to(torch.int64)
    flip = torch.randint(1, 4, (n,), generator=g, device=dev) << (2 * torch.randint(0, L, (n,), generator=g, device=dev))
    words = torch.where(err, words[src] ^ flip, words)
    counts = torch.clamp(torch.floor(1.0 / torch.rand(n, generator=g, device=dev, dtype=torch.float64)), max=1 << 20).to(torch.int64)
    return words.reshape(n, 1).contiguous(), counts, off


def grouped_call(words, off32, cnt, pairs, cap, tot):
    n = words.shape[0]
    check(lib().ss_hamming_all_pairs_grouped(words.data_ptr(), n, L, 1, K, off32.data_ptr(), off32.numel() - 1,
                                             None if cnt is None else cnt.data_ptr(), None if pairs is None else pairs.data_ptr(),
                                             cap, tot.data_ptr(), None, 0, torch.cuda.current_stream(dev).cuda_stream),
          "ss_hamming_all_pairs_grouped")


def workload(name, sizes, seed, reps):
    words, counts, off = synth(sizes, seed)
    n = words.shape[0]
    off32 = off.to(torch.int32)
    checked = int((sizes.astype(np.int64) * (sizes.astype(np.int64) - 1) // 2).sum())
    tot = torch.empty(1, dtype=torch.int64, device=dev)
    grouped_call(words, off32, None, None, 0, tot)
    m = int(tot.item())
    pairs = torch.empty((max(1, m), 2), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    med, lo = event_ms(lambda: grouped_call(words, off32, None, pairs, m, tot), reps)
    med_c, lo_c = event_ms(lambda: grouped_call(words, off32, cnt, None, 0, tot), reps)
    whole, whole_lo = event_ms(lambda: B.umi_cluster_grouped(words, L, K, off, counts, "directional", max_pairs_hint=m),
                               max(3, reps // 2), warm=1)
    print(f"{name}: rows {n}  groups {sizes.size}  largest {int(sizes.max())}  pairs checked {checked}  hits {m}\n"
          f"  ss_hamming_all_pairs_grouped (pair list) median {med:.3f} ms min {lo:.3f} ms  "
          f"{checked / med / 1e6:.2f} G pairs checked/s  {n / med / 1e3:.1f} M rows/s\n"
          f"  ss_hamming_all_pairs_grouped (counts only) median {med_c:.3f} ms min {lo_c:.3f} ms\n"
          f"  batch.umi_cluster_grouped (offset check, pairs, sort, cluster; directional) median {whole:.3f} ms min {whole_lo:.3f} ms",
          flush=True)
    return words, counts, off


def baseline_loop(words, counts, off, ngroups=2000):
    """The first `ngroups` groups: one batch.umi_cluster per group against one umi_cluster_grouped."""
    h_off = off[:ngroups + 1].cpu().numpy()
    n = int(h_off[-1])
    w, c, o = words[:n].contiguous(), counts[:n].contiguous(), off[:ngroups + 1].contiguous()

    def loop():
        rep = torch.empty(n, dtype=torch.int64, device=dev)
        for b, e in zip(h_off[:-1].tolist(), h_off[1:].tolist()):
            rep[b:e] = B.umi_cluster(w[b:e], L, K, c[b:e], "directional")[0] + b
        torch.cuda.synchronize(dev)
        return rep

    def grouped():
        rep = B.umi_cluster_grouped(w, L, K, o, c, "directional")[0]
        torch.cuda.synchronize(dev)
        return rep

    if not torch.equal(loop(), grouped()):
        raise SystemExit("PARITY FAILURE: the per-group loop and the grouped call name different representatives")
    t_loop, t_grp = [], []
    for _ in range(3):                                     # alternating, host clock around work that ends in a sync
        t0 = time.perf_counter()
        loop()
        t_loop.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        grouped()
        t_grp.append((time.perf_counter() - t0) * 1e3)
    lp, gp = sorted(t_loop)[1], sorted(t_grp)[1]
    print(f"baseline, first {ngroups} groups of (a) ({n} rows): loop of batch.umi_cluster median {lp:.1f} ms "
          f"({lp / ngroups * 1e3:.1f} us per group)  one batch.umi_cluster_grouped median {gp:.3f} ms  ratio {lp / gp:.0f}x", flush=True)
    total_groups = off.numel() - 1
    print(f"  EXTRAPOLATION (not measured): the loop over all {total_groups} groups of (a) at that per-group cost: "
          f"{lp / ngroups * total_groups / 1e3:.1f} s", flush=True)
    if not gp < lp:
        raise SystemExit("the grouped call is not faster than the loop over the same groups: something is wrong")


def one_group(n, reps):
    words, _counts, off = synth(np.array([n]), 40 + n)
    off32 = off.to(torch.int32)
    tot = torch.empty(1, dtype=torch.int64, device=dev)
    grouped_call(words, off32, None, None, 0, tot)
    m = int(tot.item())
    pairs = torch.empty((max(1, m), 2), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    out = [f"{event_ms(lambda: grouped_call(words, off32, None, pairs, m, tot), reps)[0]:.3f}"]
    for method in (B.ALL_PAIRS_METHODS["tiles"], B.ALL_PAIRS_METHODS["auto"]):
        def plain():
            check(lib().ss_hamming_all_pairs_ex(words.data_ptr(), n, L, 1, K, None, pairs.data_ptr(), m, tot.data_ptr(),
                                                method, s), "ss_hamming_all_pairs_ex")
        out.append(f"{event_ms(plain, reps)[0]:.3f}")
        if int(tot.item()) != m:
            raise SystemExit("PARITY FAILURE: one group and the plain call count different pairs")
    print(f"(d) one group of {n} rows ({n * (n - 1) // 2} pairs, {m} hits): grouped {out[0]} ms  "
          f"ss_hamming_all_pairs_ex TILES {out[1]} ms  AUTO {out[2]} ms (medians)", flush=True)


def sweep():
    for n in (1 << 8, 1 << 10, 1 << 12, 1 << 13, 1 << 14, 1 << 15, 1 << 16, 1 << 18, 1 << 20):
        sizes = group_sizes(n, n)
        words, counts, off = synth(sizes, n)
        h_words = np.ascontiguousarray(words.cpu().numpy().view(np.uint64))
        h_counts = np.ascontiguousarray(counts.cpu().numpy().view(np.uint64))
        h_off = off.cpu().numpy()
        r_gpu = U._gpu_grouped(h_words, L, h_counts, h_off, K, "directional")
        t_gpu, t_host = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            r_gpu = U._gpu_grouped(h_words, L, h_counts, h_off, K, "directional")
            t_gpu.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            r_host = U._host_grouped(h_words, L, h_counts, h_off, K, 1)
            t_host.append(time.perf_counter() - t0)
        if not np.array_equal(r_host, r_gpu):
            raise SystemExit("PARITY FAILURE: host and GPU representatives differ")
        print(f"sweep keys {n} (groups {sizes.size}): gpu median {sorted(t_gpu)[2] * 1e3:.3f} ms  "
              f"host median {sorted(t_host)[2] * 1e3:.3f} ms", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "sweep":
        sweep()
    else:
        a = workload("(a) 10^6 rows, groups ~4", group_sizes(1_000_000, 1), 1, 10)
        workload("(b) 10^7 rows, groups ~4", group_sizes(10_000_000, 2), 2, 6)
        workload("(c) 10^6 rows, heavy tail", group_sizes(1_000_000, 3, heavy=20), 3, 10)
        baseline_loop(*a)
        for n in (1_000, 10_000, 100_000):
            one_group(n, 6)
