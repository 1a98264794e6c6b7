#!/usr/bin/env python3
"""The engine's FASTQ stages with and without a 3' adapter, for one build per process (profiles/trim/README.md).

python tools/probe_trim_stage.py make FILE N                       write a small-RNA-like FASTQ of N 50-byte reads
                                                                   (seeded; the batch (a) of tools/probe_trim.py)
python tools/probe_trim_stage.py run ROOT FILE ADAPTER|none REPS LABEL
                                       import shortseq_amd from the built tree ROOT (this checkout, or one of the
                                       parent commit), count FILE once to warm up and REPS times, print the medians
                                       and ranges of fastq_stage_times()'s stages under LABEL.  Run the builds in
                                       separate processes, alternating, and compare the index stage."""
import contextlib
import io
import sys

import numpy as np

ADAPTER = b"TGGAATTCTCGGGTGCCAAGG"


def make(path, n, R=50):
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    hdr = 24
    stride = hdr + R + 3 + R + 1
    rec = np.full((n, stride), ord("I"), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1:hdr - 1] = ord("r")
    rec[:, hdr - 1] = ord("\n")
    rec[:, hdr + R] = ord("\n")
    rec[:, hdr + R + 1] = ord("+")
    rec[:, hdr + R + 2] = ord("\n")
    rec[:, stride - 1] = ord("\n")
    pool = acgt[rng.integers(0, 4, (500, R))]
    seq = pool[rng.integers(0, 500, n)]
    ins = rng.integers(15, 41, (n, 1))
    tail = np.concatenate([np.frombuffer(ADAPTER, np.uint8), acgt[rng.integers(0, 4, R)]])[:R]
    rel = np.arange(R)[None, :] - ins
    seq = np.where(rel >= 0, tail[np.clip(rel, 0, None)], seq)
    err = rng.random((n, R)) < 0.01
    seq = np.where(err, acgt[rng.integers(0, 4, (n, R))], seq)
    rec[:, hdr:hdr + R] = seq
    rec.tofile(path)


def run(root, path, adapter, reps, label):
    sys.path.insert(0, root)
    import shortseq_amd as sq
    from shortseq_amd import _shortseq
    kw = {} if adapter == "none" else {"adapter": adapter}
    rows = []
    nkeys = 0
    for _ in range(reps + 1):                      # (the first call warms up: code objects, engine buffers)
        with contextlib.redirect_stdout(io.StringIO()):
            c = sq.read_and_count_fastq(path, device="cuda", **kw)
        nkeys = len(c)
        rows.append(_shortseq.fastq_stage_times()[0])
    rows = rows[1:]
    out = [f"build={label} adapter={adapter} reps={reps} distinct={nkeys}"]
    for k in ("read_ms", "h2d_dev_ms", "index_ms", "count_ms", "finish_ms", "reduce_and_dict_ms", "total_ms"):
        v = sorted(r[k] for r in rows)
        out.append(f"  {k}: median {v[len(v) // 2]:.3f}  range {v[0]:.3f} .. {v[-1]:.3f}")
    print("\n".join(out), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "make":
        make(sys.argv[2], int(sys.argv[3]))
    else:
        run(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), sys.argv[6] if len(sys.argv) > 6 else "this")
