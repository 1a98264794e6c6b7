"""3' adapter trim on the device: batch.trim_adapter (k_trim_adapter3) against the host function on the
whole sweep of tests/trim_cases.py, in place and not, with and without stats, across launch splits and
through a captured graph; DeviceIngest(adapter=...) and read_and_count_fastq(adapter=...) against the
Python-trimmed reads and the host path, error paths included; and the pooled engine's setting cleared."""
import numpy as np
import pytest

import shortseq_amd as sq

import trim_cases as T

pytestmark = pytest.mark.gpu

ADAPTER = b"TGGAATTCTCGGGTGCCAAGG"
LAYOUTS = ("back", "junk", "residue")


@pytest.fixture(scope="module")
def sweep():
    """Every case of the sweep with the host function's answer: (adapter, mo, ed, blob, offs, lens, out, stats)."""
    import shortseq_amd.batch as B
    cases = []
    rng = np.random.default_rng(4242)
    for ci, (A, mo, ed) in enumerate(T.combos()):
        adapter = T.rand_seq(rng, A)
        blob, offs, lens = T.layout(rng, T.sweep_reads(rng, adapter, mo, ed), LAYOUTS[ci % 3])
        cases.append((adapter, mo, ed, blob, offs, lens))
    for A in (3, 8, 17, 64):
        for adapter in T.wildcard_adapters(rng, A):
            for k, (mo, ed) in enumerate(((1, 0), (3, 10), (A, 4))):
                blob, offs, lens = T.layout(rng, T.wildcard_reads(rng, adapter), LAYOUTS[k])
                cases.append((adapter, mo, ed, blob, offs, lens))
    for n in (0, 1, 63, 64, 65):
        blob, offs, lens = T.layout(rng, T.library_reads(rng, n, ADAPTER), LAYOUTS[n % 3])
        cases.append((ADAPTER, 3, 10, blob, offs, lens))
    out = []
    for adapter, mo, ed, blob, offs, lens in cases:
        h, st = B.host_trim_adapter(blob, offs, lens, adapter, min_overlap=mo, err_div=ed, stats=True)
        out.append((adapter, mo, ed, blob, offs, lens, h, st))
    return out


@pytest.fixture(scope="module")
def big():
    """20 000 library-like reads, FASTQ-like layout, with the host's answer."""
    import shortseq_amd.batch as B
    rng = np.random.default_rng(20000)
    blob, offs, lens = T.layout(rng, T.library_reads(rng, 20000, ADAPTER), "junk")
    h, st = B.host_trim_adapter(blob, offs, lens, ADAPTER, stats=True)
    assert 0 < int(st[0]) <= 20000
    return blob, offs, lens, h, st


def _dev(gpu, blob, offs, lens):
    import torch
    # (an empty blob still needs a pointer the entry point accepts)
    b = torch.from_numpy(blob if blob.size else np.zeros(16, np.uint8)).to(gpu)
    return b, torch.from_numpy(offs.view(np.int64)).to(gpu), torch.from_numpy(lens.view(np.int32)).to(gpu)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("stats", (False, True))
@pytest.mark.parametrize("inplace", (False, True))
def test_trim_gpu_matches_host_on_the_sweep(gpu, sweep, inplace, stats):
    import torch
    import shortseq_amd.batch as B
    for ci, (adapter, mo, ed, blob, offs, lens, h, hst) in enumerate(sweep):
        b, o, ln = _dev(gpu, blob, offs, lens)
        out = ln if inplace else torch.full_like(ln, 0x5A5A5A5A)
        r = B.trim_adapter(b, o, ln, adapter, min_overlap=mo, err_div=ed, out=out, stats=stats)
        got, st = r if stats else (r, None)
        assert got is out
        g = _u32(got)
        bad = np.nonzero(g != h)[0]
        assert bad.size == 0, (ci, adapter, mo, ed, int(bad[0]), int(lens[bad[0]]), int(g[bad[0]]), int(h[bad[0]]))
        if stats:
            assert [int(x) for x in st.cpu()] == [int(x) for x in hst], (ci, adapter, mo, ed)
        if not inplace:
            assert np.array_equal(_u32(ln), lens)          # the input lengths are not written


@pytest.mark.parametrize("per", (1, 64, 0))
def test_trim_gpu_reads_per_launch(gpu, big, per):
    import shortseq_amd.batch as B
    blob, offs, lens, h, hst = big
    b, o, ln = _dev(gpu, blob, offs, lens)
    got, st = B.trim_adapter(b, o, ln, ADAPTER, stats=True, _reads_per_launch=per)
    assert np.array_equal(_u32(got), h)
    assert [int(x) for x in st.cpu()] == [int(x) for x in hst]
    # an adapter given as str, and no stats: one launch, the same lengths
    assert np.array_equal(_u32(B.trim_adapter(b, o, ln, ADAPTER.decode())), h)


def test_trim_gpu_earg(gpu, big):
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd._native import SS_EARG, lib
    blob, offs, lens, _h, _st = big
    b, o, ln = _dev(gpu, blob[:4096], offs[:8], lens[:8])
    out = torch.full_like(ln, 0x5A5A5A5A)
    ad = (B.C.c_uint8 * 64)(*ADAPTER)
    s = torch.cuda.current_stream(gpu).cuda_stream
    f = lib().ss_trim_adapter3
    for args in ((None, 4096, o.data_ptr(), ln.data_ptr(), 8, ad, 21, 3, 10, out.data_ptr(), None, s),
                 (b.data_ptr(), 4096, None, ln.data_ptr(), 8, ad, 21, 3, 10, out.data_ptr(), None, s),
                 (b.data_ptr(), 4096, o.data_ptr(), None, 8, ad, 21, 3, 10, out.data_ptr(), None, s),
                 (b.data_ptr(), 4096, o.data_ptr(), ln.data_ptr(), 8, None, 21, 3, 10, out.data_ptr(), None, s),
                 (b.data_ptr(), 4096, o.data_ptr(), ln.data_ptr(), 8, ad, 21, 3, 10, None, None, s),
                 (b.data_ptr(), 4096, o.data_ptr(), ln.data_ptr(), 8, ad, 0, 3, 10, out.data_ptr(), None, s),
                 (b.data_ptr(), 4096, o.data_ptr(), ln.data_ptr(), 8, ad, 65, 3, 10, out.data_ptr(), None, s),
                 (b.data_ptr(), 4096, o.data_ptr(), ln.data_ptr(), 8, ad, 21, 0, 10, out.data_ptr(), None, s),
                 (b.data_ptr(), 4096, o.data_ptr(), ln.data_ptr(), 1 << 32, ad, 21, 3, 10, out.data_ptr(), None, s)):
        assert f(*args) == SS_EARG
    torch.cuda.synchronize(gpu)
    assert (out.cpu() == 0x5A5A5A5A).all()


def test_trim_gpu_captured_graph(gpu, big):
    import torch
    import shortseq_amd.batch as B
    blob, offs, lens, h, _st = big
    b, o, ln = _dev(gpu, blob, offs, lens)
    out = torch.empty_like(ln)
    B.trim_adapter(b, o, ln, ADAPTER, out=out)             # (the code object is loaded before the capture)
    torch.cuda.synchronize(gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # one kernel node: no stats, one launch
        B.trim_adapter(b, o, ln, ADAPTER, out=out)
    out.fill_(-1)
    g.replay()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(_u32(out), h)


def _rows_of(counter):
    """A ShortSeqCounter's dict as the ss_ingest_results layout (lens, counts, words)."""
    lens, cnts, words = [], [], []
    for k, v in counter.items():
        lens.append(len(k))
        cnts.append(v)
        words.extend(int(w) for w in k.packed[:max(0, (len(k) + 31) // 32)])
    return np.array(lens, np.uint32), np.array(cnts, np.uint64), np.array(words, np.uint64)


def test_device_ingest_adapter(gpu):
    import shortseq_amd.batch as B
    rng = np.random.default_rng(70000)
    memo, trimmed = {}, []
    eng = B.DeviceIngest(gpu, adapter=ADAPTER)
    try:
        for batch in range(2):
            reads = T.library_reads(rng, 70_000, ADAPTER, pool=500, err_rate=0.002)
            blob, offs, lens = T.layout(rng, reads, "back" if batch else "junk")
            exp, _ = T.expected(reads, ADAPTER, 3, 10, memo)
            trimmed += [r[:k] for r, k in zip(reads, exp)]
            b, o, ln = _dev(gpu, blob, offs, lens)
            eng.count(b, o, ln)
            assert np.array_equal(_u32(ln), lens)          # the caller's lengths are not written
        gl, gc, gw = eng.results()
    finally:
        eng.close()
    el, ec, ew = _rows_of(sq.ShortSeqCounter(trimmed, device="host"))
    assert gl.tolist() == el.tolist()
    assert gc.tolist() == ec.tolist()
    assert np.array_equal(gw, ew)
    assert len(el) < 20_000 and int(ec.sum()) == 140_000


def _items(c):
    return [(type(k).__name__, str(k), len(k), v) for k, v in c.items()]


@pytest.fixture(scope="module")
def fastq_file(tmp_path_factory):
    """About 100 000 library-like records (some reads trimming to nothing, some with junk past the
    adapter), the untrimmed and the trimmed host counts."""
    rng = np.random.default_rng(100000)
    reads = T.library_reads(rng, 100_000, ADAPTER, pool=500, err_rate=0.002)
    for i in range(0, len(reads), 997):
        reads[i] = ADAPTER + T.rand_seq(rng, 9)                        # trims to b""
    for i in range(5, len(reads), 1013):
        reads[i] = T.rand_seq(rng, 45) + ADAPTER + b"NNN#"             # invalid bytes only in the removed tail
    recs = [b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)]
    p = tmp_path_factory.mktemp("trim") / "lib.fq"
    p.write_bytes(b"".join(recs))
    host = sq.read_and_count_fastq(str(p), device="host", adapter=ADAPTER)
    return str(p), p.stat().st_size, _items(host)


@pytest.mark.parametrize("chunks", (1, 3))
def test_fastq_gpu_adapter(gpu, fastq_file, chunks):
    path, size, host = fastq_file
    chunk = 0 if chunks == 1 else size // 3 - 1000      # (a chunk ends after a newline: at least three of them)
    got = sq.read_and_count_fastq(path, device="cuda", adapter=ADAPTER, _chunk_bytes=chunk)
    assert _items(got) == host


def test_fastq_gpu_adapter_all_devices(gpu, fastq_file):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    path, _size, host = fastq_file
    assert _items(sq.read_and_count_fastq(path, device="all", adapter=ADAPTER.decode())) == host


def test_fastq_gpu_adapter_errors(gpu, tmp_path):
    rng = np.random.default_rng(11)

    def write(name, lines):
        p = tmp_path / name
        p.write_bytes(b"".join(b"@r\n" + ln + b"\n+\n" + b"I" * len(ln) + b"\n" for ln in lines))
        return str(p)

    good = [T.rand_seq(rng, 24) + ADAPTER[:16] for _ in range(50)]
    for bad in (b"N", b"#", b"\xff"):
        # an invalid byte in the kept prefix: the host's message, i.e. that of sq.pack(trimmed)
        line = T.rand_seq(rng, 10) + bad + T.rand_seq(rng, 9) + ADAPTER[:14]
        path = write("kept.fq", good + [line] + good)
        with pytest.raises(Exception) as e_pack:
            sq.pack(line[:20])
        with pytest.raises(Exception) as e_host:
            sq.read_and_count_fastq(path, device="host", adapter=ADAPTER)
        with pytest.raises(Exception) as e_gpu:
            sq.read_and_count_fastq(path, device="cuda", adapter=ADAPTER)
        assert type(e_gpu.value) is type(e_host.value) is type(e_pack.value)
        assert str(e_gpu.value) == str(e_host.value) == str(e_pack.value)
        # the same byte only in the removed tail: no error, the host's counts
        path = write("tail.fq", good + [T.rand_seq(rng, 20) + ADAPTER + bad * 3] + good)
        assert _items(sq.read_and_count_fastq(path, device="cuda", adapter=ADAPTER)) == _items(
            sq.read_and_count_fastq(path, device="host", adapter=ADAPTER))
    # a 1100-byte line with the adapter at byte 50 is still the too-long error
    line = T.rand_seq(rng, 50) + ADAPTER + T.rand_seq(rng, 1100 - 50 - len(ADAPTER))
    path = write("long.fq", good + [line])
    for dev in ("host", "cuda"):
        with pytest.raises(Exception, match="Sequences longer than 1024 bases are not supported."):
            sq.read_and_count_fastq(path, device=dev, adapter=ADAPTER)


def test_fastq_gpu_adapter_setting_is_cleared(gpu, tmp_path):
    """The engines are pooled per device: a call without an adapter after one with an adapter reuses the
    engine and must count the untrimmed reads."""
    rng = np.random.default_rng(12)
    reads = T.library_reads(rng, 3000, ADAPTER, pool=50, err_rate=0.0)
    p = tmp_path / "c.fq"
    p.write_bytes(b"".join(b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for r in reads))
    plain_host = _items(sq.read_and_count_fastq(str(p), device="host"))
    trimmed_host = _items(sq.read_and_count_fastq(str(p), device="host", adapter=ADAPTER))
    assert plain_host != trimmed_host
    assert _items(sq.read_and_count_fastq(str(p), device="cuda", adapter=ADAPTER)) == trimmed_host
    assert _items(sq.read_and_count_fastq(str(p), device="cuda")) == plain_host
    assert _items(sq.ShortSeqCounter(reads, device="cuda")) == plain_host
    # also after a call that raised with the adapter set
    q = tmp_path / "d.fq"
    q.write_bytes(b"@r\nACGTNACGTACGTACGTACGTACGT" + ADAPTER + b"\n+\nI\n")
    with pytest.raises(Exception, match="Unsupported base character"):
        sq.read_and_count_fastq(str(q), device="cuda", adapter=ADAPTER)
    assert _items(sq.read_and_count_fastq(str(p), device="cuda")) == plain_host
