"""Sharded counter on the GPU with 2 ranks sharing one device (gloo exchange staged through host
memory; on a multi-GPU node the same code runs over RCCL).  Real HBM tables, real kernels; result
checked against the oracle over the whole read stream."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, n, L, U, q):
    sys.path[:0] = [REPO]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import shortseq_amd.batch as B
        from shortseq_amd.dist import ShardedCounter, owner_of_region_np
        dev = torch.device("cuda", 0)
        per = n // world
        ascii = B.synth_pool_reads(per, L, 5, 6, U, i0=rank * per, device=dev)
        sc = ShardedCounter(1 << 16, device=dev)
        sc.count(ascii, L, base_index=rank * per)
        keys, _c, _f = sc.owned_items()
        own = owner_of_region_np(keys.cpu().numpy().view(np.uint64), world, *sc.local.geometry())
        assert (own == rank).all()
        res = sc.gather_items(dst=0)
        sc.close()
        if rank == 0:
            q.put([np.asarray(x).tolist() for x in res])
    finally:
        dist.destroy_process_group()


def test_sharded_counter_two_ranks_one_gpu(oracle):
    n, L, U = 200_000, 32, 3000
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, L, U, q)) for r in range(world)]
    for p in procs:
        p.start()
    keys, counts, first = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    a = oracle.gen_pool_reads(5, 6, U, 0, n, L)
    exp = oracle.count([a[i * L:(i + 1) * L].tobytes() for i in range(n)])
    assert [int(k) for k in keys] == [w[0] for (w, _L, _c, _f) in exp]
    assert counts == [c for (_w, _L, c, _f) in exp]
    assert first == [f for (_w, _L, _c, f) in exp]


def _worker_words(rank, world, port, n, L, U, q):
    sys.path[:0] = [REPO]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import shortseq_amd.batch as B
        from shortseq_amd.dist import ShardedCounter
        dev = torch.device("cuda", 0)
        per = n // world
        ascii = B.synth_pool_reads(per, L, 5, 6, U, i0=rank * per, device=dev)
        sc = ShardedCounter(1 << 16, device=dev)
        sc.count(ascii, L, base_index=rank * per)
        res = sc.gather_items(dst=0)
        sc.close()
        if rank == 0:
            q.put([np.asarray(x).tolist() for x in res])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("L", [64, 100])
def test_sharded_counter_two_ranks_multiword(oracle, L):
    """VERDICT r3 missing item 2: keys longer than 32 nt through the sharded counter on real HBM tables
    (extract_words by owner, one all-to-all of (words, count, first) rows, merge_words), two ranks on
    one GPU; the gathered rows in first-occurrence order == oracle.count over the whole stream."""
    n, U = 120_000, 2500
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_words, args=(r, world, port, n, L, U, q)) for r in range(world)]
    for p in procs:
        p.start()
    words, counts, first = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    a = oracle.gen_pool_reads(5, 6, U, 0, n, L)
    exp = oracle.count([a[i * L:(i + 1) * L].tobytes() for i in range(n)])
    assert [[int(x) for x in w] for w in words] == [[int(x) for x in w] for (w, _L, _c, _f) in exp]
    assert counts == [c for (_w, _L, c, _f) in exp]
    assert first == [f for (_w, _L, _c, f) in exp]


def _worker_c5(rank, world, port, n, U, q):
    sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import shortseq_amd.batch as B
        from shortseq_amd.dist import ShardedCounter
        dev = torch.device("cuda", 0)
        ascii = B.synth_pool_reads(n, 32, 5, 77, U, i0=rank * n, device=dev)
        sc = ShardedCounter(2 * U, device=dev)
        sc.local.reserve(n)
        sc.count(ascii, 32, base_index=rank * n, check_errors=False)
        del ascii
        torch.cuda.empty_cache()
        res = sc.gather_items(dst=0)
        sc.close()
        if rank == 0:
            import oracle
            k, c, f = res
            q.put((len(k), int(c.sum()), oracle.table_digest(k, c, f)))
    except Exception as e:  # noqa: BLE001
        q.put(("error", rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_sharded_counter_8_ranks_c5_shards():
    """SURVEY §8(e) C5 rehearsal without an 8-GPU node: 8 ranks (one process each, all on this GPU,
    gloo staging the exchange through host memory where the node uses RCCL) each count a full
    125M-read shard of the 1B-read job in its own HBM table, exchange the other owners' regions and
    fold them in; the union gathered on rank 0 equals the generator-derived digest of the whole job
    (tests/golden/c5_digests.json uniform_U24_job8: content, not just the total)."""
    import json
    d = json.load(open(os.path.join(REPO, "tests", "golden", "c5_digests.json")))["uniform_U24_job8"]
    world, n = d["shards"], d["n"] // d["shards"]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_c5, args=(r, world, port, n, d["U"], q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=800)
    for p in procs:
        p.join(timeout=120)
    assert got[0] != "error", got
    assert all(p.exitcode == 0 for p in procs)
    assert got == (d["unique"], d["n"], d["digest"])


@pytest.mark.timeout(600)
def test_bench_two_ranks_rehearsal():
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one process per rank),
    rehearsed with 2 gloo ranks on this GPU: the ranks agree on every settle step (a C5 step holds the
    exchange), rank 0 prints ONE JSON line with the whole-job value, and the C5 line's table equals
    the 2-shard job digest (tests/golden/c5_digests.json uniform_U24_job2)."""
    import json
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2",
                        "--steps", "3", "--warmup", "1", "--dist-backend", "gloo", "--same-device", "--full"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=540)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["config"]["global_batch"] == 2 * r["config"]["reads_per_gpu"]
    assert r["extra"]["C5_counter_32"]["parity"] == "digest uniform_U24_job2"
    for k, v in r["extra"].items():
        assert "error" not in v, (k, v)


def _rccl_worker(port, q):
    """One rank on the nccl backend (RCCL): the exchange helpers with device tensors, as the
    multi-GPU bench calls them (a 1-rank all-to-all is a copy to itself)."""
    sys.path[:0] = [REPO]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from shortseq_amd.dist import exchange, exchange_packed
        assert dist.get_backend() == "nccl"
        g = torch.Generator().manual_seed(3)
        m = 100_003
        rec = torch.randint(-2 ** 62, 2 ** 62, (m + 17, 2), generator=g, dtype=torch.int64).to(dev)
        recv, sizes, bases, ex = exchange_packed(rec, torch.tensor([m], device=dev), 12345,
                                                 extra=torch.tensor([0], dtype=torch.int32, device=dev))
        ok = torch.equal(recv, rec[:m]) and sizes == [m] and bases == [12345] and ex == [0]
        # a raised overflow word: no record exchange, the word comes back (every rank raises alike)
        recv, sizes, bases, ex = exchange_packed(rec, torch.tensor([m], device=dev), 12345,
                                                 extra=torch.tensor([7], dtype=torch.int32, device=dev))
        ok = ok and recv.shape[0] == 0 and sizes == [0] and ex == [7]
        k = rec[:, 0].contiguous()
        kk, cc, ff, rs = exchange(k, k + 1, k + 2, torch.tensor([m], device=dev), with_sizes=True)
        ok = ok and torch.equal(kk, k[:m]) and torch.equal(cc, k[:m] + 1) and torch.equal(ff, k[:m] + 2) and rs == [m]
        f = torch.tensor([1], dtype=torch.int32, device=dev)
        dist.all_reduce(f, op=dist.ReduceOp.MAX)
        dist.barrier()
        q.put(bool(ok) and int(f.item()) == 1)
    finally:
        dist.destroy_process_group()


def test_rccl_exchange_helpers_world1():
    """The RCCL path of the exchange (backend nccl, device tensors, uneven split sizes passed from
    the host) at world size 1: the only RCCL configuration a 1-GPU box can form."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(port, q))
    p.start()
    ok = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert ok


@pytest.mark.timeout(300)
def test_bench_two_ranks_without_launcher():
    """`python bench.py --gpus 2` with no launcher: bench.py starts the two ranks
    itself (gloo rehearsal on this GPU, small C2 batch, no extras) and its ONE JSON line says
    n_gpus 2 with the whole-job batch; unmeasured across real devices."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONUNBUFFERED"] = "1"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--dist-backend", "gloo", "--same-device", "--reads-per-gpu", "4000000", "--no-extras"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["config"]["global_batch"] == 8_000_000 and r["value"] > 0
