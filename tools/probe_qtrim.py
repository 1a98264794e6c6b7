#!/usr/bin/env python3
"""3' quality trim timings (DESIGN.md "3' quality trim"; the log is kept under profiles/qtrim/).

python tools/probe_qtrim.py [reads]    FASTQ-layout batches made on the device (the records of tools/probe_trim.py:
                                       a 24-byte header, the read, '+', the qualities; reads = records per batch,
                                       default 4 000 000):
                                       (a) 50-byte reads: 90 % end in a base above the cutoff (the walk ends at
                                           its first byte), 10 % have a low tail of 1..20 bytes;
                                       (b) 150-byte reads, every one with a low tail of 50..150 bytes (every read
                                           walks far);
                                       ss_trim_quality3 in the layout form (HIP events, 3 warm-ups, 15 repetitions
                                       with the variants alternating inside each, median and range) for every lane
                                       group 1 / 2 / 4 / 8 / 16, the library's group with stats, and as the
                                       yardstick the library's k_trim_adapter3 on the same batch; with the bytes
                                       the kernel cannot avoid (offsets and lengths in, lengths out, one locate
                                       chunk and the quality chunks the walk needs) and that floor's rate.  Every
                                       group's lengths are compared with the library's, and the first 20 000 with
                                       the host function.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import shortseq_amd.batch as B  # noqa: E402
from shortseq_amd._native import check, lib  # noqa: E402
from probe_trim import ADAPTER, HEADER, make_batch  # noqa: E402

dev = torch.device("cuda", 0)
CUTOFF, BASE = 20, 33
GROUPS = (1, 2, 4, 8, 16)


def degrade(blob, n, R, lo, hi, share, seed):
    """Qualities 'I' everywhere; a `share` of the reads gets a tail of lo..hi bytes of quality 2..19."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    stride = HEADER + R + 3 + R + 1
    rec = blob.view(n, stride)
    tail = torch.randint(lo, hi + 1, (n, 1), generator=g, device=dev)
    tail = torch.where(torch.rand((n, 1), generator=g, device=dev) < share, tail, torch.zeros_like(tail))
    low = torch.randint(BASE + 2, BASE + CUTOFF, (n, R), generator=g, device=dev, dtype=torch.uint8)
    q = rec[:, HEADER + R + 3:HEADER + R + 3 + R]
    q.copy_(torch.where(torch.arange(R, device=dev)[None, :] >= R - tail, low, q))


def floor_bytes(offs, lens, out):
    """offsets 8 + lengths 4 in, lengths 4 out, one locate chunk, and the 16-B chunks of the quality line from
    the byte left of the new length (the one that ends the walk) to its end."""
    R = int(lens[0].item())
    qoff = offs + R + 3                                   # '\n' '+' '\n' behind the read
    first = qoff + (out.to(torch.int64) - 1).clamp(min=0)
    chunks = ((qoff + R - 1) >> 4) - (first >> 4) + 1
    return int(chunks.sum().item()) * 16 + (16 + 16) * offs.numel()


def run(name, blob, offs, lens, reps=15, warm=3):
    n = lens.numel()
    ad = (C.c_uint8 * len(ADAPTER)).from_buffer_copy(ADAPTER)
    s = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty_like(lens)
    st = torch.zeros(3, dtype=torch.int64, device=dev)

    def quality(group, stats=False):
        check(lib().ss_trim_quality3_shape(blob.data_ptr(), blob.numel(), offs.data_ptr(), lens.data_ptr(), n, None, None,
                                           CUTOFF, BASE, out.data_ptr(), st.data_ptr() if stats else None, 0, group, s),
              "ss_trim_quality3_shape")

    def adapter():
        check(lib().ss_trim_adapter3(blob.data_ptr(), blob.numel(), offs.data_ptr(), lens.data_ptr(), n, ad, len(ADAPTER), 3,
                                     10, out.data_ptr(), None, s), "ss_trim_adapter3")

    quality(0, True)
    ref = out.clone()
    shortened, removed, noqual = (int(x) for x in st.cpu())
    k = min(n, 20000)
    h = B.host_trim_quality(blob[:int(offs[k - 1].item()) + 2048].cpu().numpy(), offs[:k].cpu().numpy(), lens[:k].cpu().numpy(),
                            CUTOFF, base=BASE)
    if not np.array_equal(h.view(np.int32), ref[:k].cpu().numpy()):
        raise SystemExit("PARITY FAILURE: device and host lengths differ")
    variants = [("group %2d" % g_, lambda g_=g_: quality(g_)) for g_ in GROUPS]
    variants += [("lib+stats", lambda: quality(0, True)), ("k_trim_adapter3", adapter)]
    for label, f in variants[:len(GROUPS)]:
        for _ in range(warm):
            f()
        if not torch.equal(out, ref):
            raise SystemExit(f"PARITY FAILURE: {label} gives other lengths than the library's")
    for _ in range(warm):
        adapter()
    times = {label: [] for label, _ in variants}
    for _ in range(reps):                       # the variants alternate inside every repetition
        for label, f in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[label].append(e0.elapsed_time(e1))
    fb = floor_bytes(offs, lens, ref)
    print(f"{name}: reads {n}  blob {blob.numel() / 1e6:.0f} MB  shortened {shortened}  bytes removed {removed}  "
          f"no quality line {noqual}  floor traffic {fb / 1e6:.1f} MB ({fb / n:.1f} B/read)", flush=True)
    for label, _ in variants:
        t = sorted(times[label])
        med = t[len(t) // 2]
        print(f"  {label:16s}: median {med:.3f} ms  range {t[0]:.3f} .. {t[-1]:.3f} ms  {n / med / 1e6:.2f} G reads/s"
              + ("" if label == "k_trim_adapter3" else f"  floor bytes at {fb / med / 1e9:.3f} TB/s"), flush=True)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    blob, offs, lens = make_batch(n, 50, True, 1)
    degrade(blob, n, 50, 1, 20, 0.10, 3)
    run("(a) 50-byte reads, 10 % with a low tail of 1..20", blob, offs, lens)
    del blob, offs, lens
    blob, offs, lens = make_batch(n // 2, 150, False, 2)
    degrade(blob, n // 2, 150, 50, 150, 1.0, 4)
    run("(b) 150-byte reads, all with a low tail of 50..150", blob, offs, lens)
