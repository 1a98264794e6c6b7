#!/usr/bin/env python3
"""The engine's FASTQ stages with and without a 3' quality cutoff, for one build per process
(profiles/qtrim/README.md; the method of tools/probe_trim_stage.py).

python tools/probe_qtrim_stage.py make FILE N                  write the FASTQ of tools/probe_trim_stage.py (N 50-byte
                                                               small-RNA-like reads, seeded) with 10 % of the quality
                                                               lines ending in a low tail of 1..20 bytes
python tools/probe_qtrim_stage.py run ROOT FILE CUTOFF|none REPS LABEL
                                       import shortseq_amd from the built tree ROOT (this checkout, or one of the
                                       parent commit, which only takes `none`), count FILE once to warm up and REPS
                                       times, print the medians and ranges of fastq_stage_times()'s stages under
                                       LABEL.  Run the builds in separate processes, alternating, and compare the
                                       index stage."""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_trim_stage as P  # noqa: E402


def make(path, n, R=50):
    P.make(path, n, R)
    rng = np.random.default_rng(8)
    stride = 24 + R + 3 + R + 1
    rec = np.memmap(path, np.uint8, "r+").reshape(n, stride)
    tail = np.where(rng.random(n) < 0.10, rng.integers(1, 21, n), 0)[:, None]
    low = rng.integers(33 + 2, 33 + 20, (n, R), dtype=np.int64).astype(np.uint8)
    q = rec[:, 24 + R + 3:24 + R + 3 + R]
    q[:] = np.where(np.arange(R)[None, :] >= R - tail, low, q)
    rec.flush()


def run(root, path, cutoff, reps, label):
    sys.path.insert(0, root)
    import shortseq_amd as sq
    from shortseq_amd import _shortseq
    kw = {} if cutoff == "none" else {"quality_cutoff": int(cutoff)}
    rows = []
    nkeys = 0
    for _ in range(reps + 1):                      # (the first call warms up: code objects, engine buffers)
        with contextlib.redirect_stdout(io.StringIO()):
            c = sq.read_and_count_fastq(path, device="cuda", **kw)
        nkeys = len(c)
        rows.append(_shortseq.fastq_stage_times()[0])
    rows = rows[1:]
    out = [f"build={label} quality_cutoff={cutoff} reps={reps} distinct={nkeys}"]
    for k in ("read_ms", "h2d_dev_ms", "index_ms", "count_ms", "finish_ms", "reduce_and_dict_ms", "total_ms"):
        v = sorted(r[k] for r in rows)
        out.append(f"  {k}: median {v[len(v) // 2]:.3f}  range {v[0]:.3f} .. {v[-1]:.3f}")
    print("\n".join(out), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "make":
        make(sys.argv[2], int(sys.argv[3]))
    else:
        run(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), sys.argv[6] if len(sys.argv) > 6 else "this")
