#!/usr/bin/env python3
"""3' adapter trim timings (DESIGN.md "3' adapter trim"; the log is kept under profiles/trim/).

python tools/probe_trim.py [reads]     FASTQ-like ragged batches made on the device (a header, the read, '+', the
                                       qualities per record; reads = records per batch, default 4 000 000):
                                       (a) 50-byte small-RNA reads: a 15-40 nt insert from a pool, then the adapter
                                           and filler to the read's end, 1 % substitutions;
                                       (b) 150-byte reads without the adapter (every position is looked at);
                                       ss_trim_adapter3 (HIP events, warm-up, alternating variants, median and
                                       range) for every kernel shape -- lane group 2 / 4 / 8 / 16 / 32, chunks staged in
                                       LDS or aligned dwords straight from global memory -- with the bytes the
                                       kernel cannot avoid (the reads' 16-B chunks + 12 B per read in + 4 B out),
                                       that floor's rate, and the same with stats.  Every shape's lengths are
                                       compared with the library's, and the first 20 000 with the host function.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import shortseq_amd.batch as B  # noqa: E402
from shortseq_amd._native import check, lib  # noqa: E402

dev = torch.device("cuda", 0)
ADAPTER = b"TGGAATTCTCGGGTGCCAAGG"
HEADER = 24          # bytes of '@...\n' before a read


def make_batch(n, R, with_adapter, seed):
    """-> (blob u8, offsets i64 [n], lens i32 [n]): records of HEADER + R + 3 + R + 1 bytes."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    stride = HEADER + R + 3 + R + 1
    rec = torch.full((n, stride), ord("I"), dtype=torch.uint8, device=dev)
    rec[:, 0] = ord("@")
    rec[:, HEADER - 1] = ord("\n")
    rec[:, HEADER + R] = ord("\n")
    rec[:, HEADER + R + 1] = ord("+")
    rec[:, HEADER + R + 2] = ord("\n")
    rec[:, stride - 1] = ord("\n")
    if with_adapter:
        pool = acgt[torch.randint(0, 4, (500, R), generator=g, device=dev)]
        seq = pool[torch.randint(0, 500, (n,), generator=g, device=dev)]
        ins = torch.randint(15, 41, (n, 1), generator=g, device=dev)
        tail = torch.cat([torch.tensor(list(ADAPTER), dtype=torch.uint8, device=dev),
                          acgt[torch.randint(0, 4, (R,), generator=g, device=dev)]])[:R]
        rel = torch.arange(R, device=dev)[None, :] - ins
        seq = torch.where(rel >= 0, tail[rel.clamp(min=0)], seq)
        err = torch.rand((n, R), generator=g, device=dev) < 0.01
        seq = torch.where(err, acgt[torch.randint(0, 4, (n, R), generator=g, device=dev)], seq)
    else:
        seq = acgt[torch.randint(0, 4, (n, R), generator=g, device=dev)]
    rec[:, HEADER:HEADER + R] = seq
    offs = torch.arange(n, device=dev, dtype=torch.int64) * stride + HEADER
    lens = torch.full((n,), R, dtype=torch.int32, device=dev)
    return rec.reshape(-1), offs, lens


def floor_bytes(offs, lens):
    chunks = ((offs + lens - 1) >> 4) - (offs >> 4) + 1
    return int(chunks.sum().item()) * 16 + 16 * offs.numel()


def run(name, blob, offs, lens, reps=15, warm=3):
    n = lens.numel()
    ad = (C.c_uint8 * len(ADAPTER)).from_buffer_copy(ADAPTER)
    s = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty_like(lens)
    st = torch.zeros(2, dtype=torch.int64, device=dev)

    def call(group, staged, stats=False):
        check(lib().ss_trim_adapter3_shape(blob.data_ptr(), blob.numel(), offs.data_ptr(), lens.data_ptr(), n, ad,
                                           len(ADAPTER), 3, 10, out.data_ptr(), st.data_ptr() if stats else None, 0, group,
                                           staged, s), "ss_trim_adapter3_shape")

    call(0, -1, True)
    ref = out.clone()
    shortened, removed = (int(x) for x in st.cpu())
    h = B.host_trim_adapter(blob[:int(offs[min(n, 20000) - 1].item()) + 2048].cpu().numpy(), offs[:20000].cpu().numpy(),
                            lens[:20000].cpu().numpy(), ADAPTER)
    if not np.array_equal(h.view(np.int32), ref[:20000].cpu().numpy()):
        raise SystemExit("PARITY FAILURE: device and host lengths differ")
    shapes = [(g_, s_) for g_ in (2, 4, 8, 16, 32) for s_ in (1, 0)]
    times = {k: [] for k in shapes + ["lib+stats"]}
    for k in shapes:
        for _ in range(warm):
            call(*k)
        if not torch.equal(out, ref):
            raise SystemExit(f"PARITY FAILURE: shape {k} gives other lengths than the library's")
    for _ in range(reps):                       # the variants alternate inside every repetition
        for k in shapes + ["lib+stats"]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if k == "lib+stats":
                call(0, -1, True)
            else:
                call(*k)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    fb = floor_bytes(offs, lens)
    print(f"{name}: reads {n}  blob {blob.numel() / 1e6:.0f} MB  shortened {shortened}  bytes removed {removed}  "
          f"floor traffic {fb / 1e6:.1f} MB ({fb / n:.1f} B/read)", flush=True)
    for k in shapes + ["lib+stats"]:
        t = sorted(times[k])
        med = t[len(t) // 2]
        label = k if isinstance(k, str) else f"group {k[0]:2d} {'LDS-staged' if k[1] else 'direct    '}"
        print(f"  {label}: median {med:.3f} ms  range {t[0]:.3f} .. {t[-1]:.3f} ms  {n / med / 1e6:.2f} G reads/s  "
              f"floor bytes at {fb / med / 1e9:.3f} TB/s", flush=True)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    run("(a) 50-byte reads, insert + adapter", *make_batch(n, 50, True, 1))
    run("(b) 150-byte reads, no adapter", *make_batch(n // 2, 150, False, 2))
