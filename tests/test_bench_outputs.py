"""bench.py's plain run on the GPU: `--steps` timed steps, one JSON line without the `--full` legs,
and `--dump-outputs DIR` holding what the last timed step computed -- checked here against the CPU
oracle's encode of the same generator reads (so two runs with the same arguments write the same files).
The batch is just past 2^20 reads: the dump keeps a seeded sample of the rows, and the last checksum
block is a partial one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L = (1 << 20) + 4099, 32

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_last_step_outputs(oracle, gpu, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--reads-per-gpu", str(N), "--dump-outputs", str(out)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["value"] > 0 and r["unit"] == "nt/s"
    assert abs(r["value"] - N * L / (r["ms_per_step"] * 1e-3)) <= 2e-3 * r["value"]   # 4 significant digits each
    assert "extra" not in r and r["cpu_baseline"] is None

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["first_bad", "words_hi", "words_lo", "words_rows", "words_sum_hi", "words_sum_lo"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    exp, rc, _ = oracle.encode_batch(oracle.gen_reads(1, 0, N, L), N, L)
    assert rc == 0 and got["first_bad"].tolist() == [-1.0]
    rows = got["words_rows"].astype(np.int64)
    assert rows.shape == (1 << 20,) and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < N
    lo, hi = exp & np.uint64(0xFFFFFFFF), exp >> np.uint64(32)
    assert np.array_equal(got["words_lo"], lo[rows].astype(np.float64))
    assert np.array_equal(got["words_hi"], hi[rows].astype(np.float64))
    fold = 1 << 16
    for name, half in (("words_sum_lo", lo), ("words_sum_hi", hi)):
        padded = np.zeros((-(-N // fold) * fold, 1), np.uint64)
        padded[:N] = half
        assert np.array_equal(got[name], padded.reshape(-1, fold, 1).sum(1).astype(np.float64)), name
