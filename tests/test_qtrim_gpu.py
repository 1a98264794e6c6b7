"""3' quality trim on the device: batch.trim_quality (k_trim_quality3) against the host function on the
whole sweep of tests/qtrim_cases.py in both forms, in place and not, with and without stats, across launch
splits and through a captured graph; read_and_count_fastq(quality_cutoff=...) on the device against the host
path -- alone, with adapter=, in one chunk and in several, with a chunk seam after each of a record's four
lines and at the ends of multi-GPU ranges, error paths included -- and the pooled engine's setting cleared."""
import numpy as np
import pytest

import shortseq_amd as sq

import qtrim_cases as Q

pytestmark = pytest.mark.gpu

ADAPTER = b"TGGAATTCTCGGGTGCCAAGG"


@pytest.fixture(scope="module")
def sweep():
    """Every case of the sweep with the host function's answer:
    (cutoff, base, blob, offs, lens, qual or None, qoffs or None, out, stats)."""
    import shortseq_amd.batch as B
    cases = []
    for cutoff in Q.CUTOFFS:
        for base in Q.BASES:
            rng = np.random.default_rng(7000 + 100 * cutoff + base)
            cases.append((cutoff, base) + Q.explicit_layout(rng, Q.sweep_quals(rng, cutoff, base, newline=True)))
            quals = Q.sweep_quals(rng, cutoff, base, newline=False)
            for tail in (b"\n", b""):
                text, offs, lens = Q.fastq_layout(rng, quals, tail)
                cases.append((cutoff, base, Q.as_blob(text), offs, lens, None, None))
            for text, offs, lens in Q.special_texts(cutoff, base):
                cases.append((cutoff, base, Q.as_blob(text), offs, lens, None, None))
    rng = np.random.default_rng(7)
    for n in (0, 1, 63, 64, 65):
        quals = [bytes(rng.integers(33, 75, int(rng.integers(1, 60)), dtype=np.int64).astype(np.uint8)) for _ in range(n)]
        text, offs, lens = Q.fastq_layout(rng, quals)
        cases.append((20, 33, Q.as_blob(text), offs, lens, None, None))
        cases.append((20, 33) + Q.explicit_layout(rng, quals))
    out = []
    for cutoff, base, blob, offs, lens, qual, qoffs in cases:
        h, st = B.host_trim_quality(blob, offs, lens, cutoff, base=base, qual=qual, qoffsets=qoffs, stats=True)
        out.append((cutoff, base, blob, offs, lens, qual, qoffs, h, st))
    return out


@pytest.fixture(scope="module")
def big():
    """20 000 library-like records whose tails degrade, as FASTQ text with its index and the host's answer."""
    import shortseq_amd.batch as B
    rng = np.random.default_rng(20000)
    text, seqs, _quals = Q.degraded_library(rng, 20000)
    offs, pos = [], 0
    for i, s in enumerate(seqs):
        offs.append(pos + len(b"@read%d\n" % i))
        pos = offs[-1] + 2 * len(s) + 4
    offs = np.array(offs, np.uint64)
    lens = np.array([len(s) for s in seqs], np.uint32)
    blob = Q.as_blob(text)
    h, st = B.host_trim_quality(blob, offs, lens, 20, stats=True)
    assert 0 < int(st[0]) < 20000 and int(st[2]) == 0
    return blob, offs, lens, h, st


def _t(gpu, a, dtype=None):
    import torch
    if a is None:
        return None
    if a.size == 0 and a.dtype == np.uint8:
        a = np.zeros(16, np.uint8)          # (an empty blob still needs a pointer the entry point accepts)
    return torch.from_numpy(a if dtype is None else a.view(dtype)).to(gpu)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("stats", (False, True))
@pytest.mark.parametrize("inplace", (False, True))
def test_qtrim_gpu_matches_host_on_the_sweep(gpu, sweep, inplace, stats):
    import torch
    import shortseq_amd.batch as B
    for ci, (cutoff, base, blob, offs, lens, qual, qoffs, h, hst) in enumerate(sweep):
        b, o, ln = _t(gpu, blob)[:blob.size], _t(gpu, offs, np.int64), _t(gpu, lens, np.int32)
        out = ln if inplace else torch.full_like(ln, 0x5A5A5A5A)
        r = B.trim_quality(b, o, ln, cutoff, base=base, qual=_t(gpu, qual), qoffsets=_t(gpu, qoffs, np.int64), out=out,
                           stats=stats)
        got, st = r if stats else (r, None)
        assert got is out
        g = _u32(got)
        bad = np.nonzero(g != h)[0]
        assert bad.size == 0, (ci, cutoff, base, qual is None, int(bad[0]), int(lens[bad[0]]), int(g[bad[0]]), int(h[bad[0]]))
        if stats:
            assert [int(x) for x in st.cpu()] == [int(x) for x in hst], (ci, cutoff, base, qual is None)
        if not inplace:
            assert np.array_equal(_u32(ln), lens)          # the input lengths are not written


@pytest.mark.parametrize("per", (1, 64, 0))
def test_qtrim_gpu_reads_per_launch(gpu, big, per):
    import shortseq_amd.batch as B
    blob, offs, lens, h, hst = big
    b, o, ln = _t(gpu, blob), _t(gpu, offs, np.int64), _t(gpu, lens, np.int32)
    got, st = B.trim_quality(b, o, ln, 20, stats=True, _reads_per_launch=per)
    assert np.array_equal(_u32(got), h)
    assert [int(x) for x in st.cpu()] == [int(x) for x in hst]
    assert np.array_equal(_u32(B.trim_quality(b, o, ln, 20)), h)      # no stats: one launch, the same lengths


def test_qtrim_gpu_every_lane_group(gpu, big, sweep):
    """The library's lane group is a measured choice: every compiled one gives the same lengths."""
    import torch
    from shortseq_amd._native import SS_EARG, SS_OK, lib
    s = torch.cuda.current_stream(gpu).cuda_stream
    blob, offs, lens, h, hst = big
    picked = [(20, 33, blob, offs, lens, None, None, h, hst)] + [c for c in sweep if c[0] == 20 and c[1] == 33][:3]
    for cutoff, base, blob, offs, lens, qual, qoffs, h, hst in picked:
        b, o, ln = _t(gpu, blob), _t(gpu, offs, np.int64), _t(gpu, lens, np.int32)
        qd, qo = _t(gpu, qual), _t(gpu, qoffs, np.int64)
        for group in (1, 2, 4, 8, 16):
            out = torch.full_like(ln, 0x5A5A5A5A)
            st = torch.zeros(3, dtype=torch.int64, device=gpu)
            assert lib().ss_trim_quality3_shape(b.data_ptr(), blob.size, o.data_ptr(), ln.data_ptr(), lens.size,
                                                None if qd is None else qd.data_ptr(), None if qo is None else qo.data_ptr(),
                                                cutoff, base, out.data_ptr(), st.data_ptr(), 0, group, s) == SS_OK
            assert np.array_equal(_u32(out), h), group
            assert [int(x) for x in st.cpu()] == [int(x) for x in hst], group
    assert lib().ss_trim_quality3_shape(b.data_ptr(), blob.size, o.data_ptr(), ln.data_ptr(), lens.size, None, None, 20, 33,
                                        out.data_ptr(), None, 0, 3, s) == SS_EARG


def test_qtrim_gpu_earg(gpu, big):
    import torch
    from shortseq_amd._native import SS_EARG, lib
    blob, offs, lens, _h, _st = big
    b, o, ln = _t(gpu, blob[:4096]), _t(gpu, offs[:8], np.int64), _t(gpu, lens[:8], np.int32)
    out = torch.full_like(ln, 0x5A5A5A5A)
    s = torch.cuda.current_stream(gpu).cuda_stream
    B_, O, LN, OUT = b.data_ptr(), o.data_ptr(), ln.data_ptr(), out.data_ptr()
    f = lib().ss_trim_quality3
    for args in ((None, 4096, O, LN, 8, None, None, 20, 33, OUT, None, s),       # the layout form needs the blob
                 (B_, 4096, None, LN, 8, None, None, 20, 33, OUT, None, s),
                 (B_, 4096, O, None, 8, None, None, 20, 33, OUT, None, s),
                 (B_, 4096, O, LN, 8, None, None, 20, 33, None, None, s),
                 (B_, 4096, O, LN, 8, None, O, 20, 33, OUT, None, s),           # quality offsets without quality bytes
                 (B_, 4096, O, LN, 8, None, None, 0, 33, OUT, None, s),
                 (B_, 4096, O, LN, 8, None, None, 94, 33, OUT, None, s),
                 (B_, 4096, O, LN, 8, B_, O, 94, 33, OUT, None, s),
                 (B_, 4096, O, LN, 8, None, None, 20, 0, OUT, None, s),
                 (B_, 4096, O, LN, 8, None, None, 20, 34, OUT, None, s),
                 (B_, 4096, O, LN, 8, B_, O, 20, 63, OUT, None, s),
                 (B_, 4096, O, LN, 1 << 32, None, None, 20, 33, OUT, None, s)):
        assert f(*args) == SS_EARG
    torch.cuda.synchronize(gpu)
    assert (out.cpu() == 0x5A5A5A5A).all()


def test_qtrim_gpu_captured_graph(gpu, big):
    import torch
    import shortseq_amd.batch as B
    blob, offs, lens, h, _st = big
    b, o, ln = _t(gpu, blob), _t(gpu, offs, np.int64), _t(gpu, lens, np.int32)
    out = torch.empty_like(ln)
    B.trim_quality(b, o, ln, 20, out=out)                  # (the code object is loaded before the capture)
    torch.cuda.synchronize(gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # one kernel node: no stats, one launch
        B.trim_quality(b, o, ln, 20, out=out)
    out.fill_(-1)
    g.replay()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(_u32(out), h)


def _items(c):
    return [(type(k).__name__, str(k), len(k), v) for k, v in c.items()]


@pytest.fixture(scope="module")
def fastq_file(tmp_path_factory):
    """About 100 000 library-like records whose tails degrade; the host path's counts with the cutoff alone
    and with the adapter too."""
    rng = np.random.default_rng(100000)
    text, _seqs, _quals = Q.degraded_library(rng, 100_000, pool=500)
    p = tmp_path_factory.mktemp("qtrim") / "lib.fq"
    p.write_bytes(text)
    host = _items(sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20))
    both = _items(sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20, adapter=ADAPTER))
    assert host != both
    return str(p), p.stat().st_size, host, both


@pytest.mark.parametrize("adapter", (None, ADAPTER))
@pytest.mark.parametrize("chunks", (1, 3))
def test_fastq_gpu_quality(gpu, fastq_file, chunks, adapter):
    path, size, host, both = fastq_file
    chunk = 0 if chunks == 1 else size // 3 - 1000      # (a chunk ends after a newline: at least three of them)
    kw = {} if adapter is None else {"adapter": adapter}
    got = sq.read_and_count_fastq(path, device="cuda", quality_cutoff=20, _chunk_bytes=chunk, **kw)
    assert _items(got) == (host if adapter is None else both)


def test_fastq_gpu_quality_all_devices(gpu, fastq_file):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    path, _size, host, both = fastq_file
    assert _items(sq.read_and_count_fastq(path, device="all", quality_cutoff=20)) == host
    assert _items(sq.read_and_count_fastq(path, device="all", quality_cutoff=20, adapter=ADAPTER)) == both


REC = 72          # '@' + 6 + '\n', 30 bases + '\n', '+' + '\n', 30 qualities + '\n'


@pytest.fixture(scope="module")
def seam_files(tmp_path_factory):
    """400 records of 72 bytes; read i has a low tail of 1 + i % 15 bases and is its own key up to there, so
    a read trimmed wrongly (or not at all) changes the dict.  -> {name: (path, host items)} for the whole
    file, the file without its final newline, and the file cut after the last record's '+' line."""
    rng = np.random.default_rng(400)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = []
    for i in range(400):
        k = 1 + i % 15
        seq = bytes(rng.choice(acgt, 30))
        qual = b"I" * (30 - k) + b"#" * k
        recs.append(b"@%06d\n" % i + seq + b"\n+\n" + qual + b"\n")
        assert len(recs[-1]) == REC
    text = b"".join(recs)
    d = tmp_path_factory.mktemp("seam")
    out = {}
    for name, data in (("whole", text), ("no_newline", text[:-1]), ("cut", text[:-31])):
        p = d / (name + ".fq")
        p.write_bytes(data)
        out[name] = (str(p), _items(sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20)))
    plain = _items(sq.read_and_count_fastq(out["whole"][0], device="host"))
    assert out["whole"][1] != plain and len(out["whole"][1]) == 400
    assert out["cut"][1][-1][2] == 30 and out["whole"][1][-1][2] == 30 - (1 + 399 % 15)     # the last read kept whole
    return out


# a chunk of 72 * 5 + d bytes ends after the d bytes of a sixth record: its header, sequence, '+' and quality line
@pytest.mark.parametrize("chunk", (REC * 5 + 8, REC * 5 + 39, REC * 5 + 41, REC * 5 + 72, 997, 4099))
@pytest.mark.parametrize("name", ("whole", "no_newline", "cut"))
def test_fastq_gpu_quality_chunk_seam(gpu, seam_files, name, chunk):
    path, host = seam_files[name]
    assert _items(sq.read_and_count_fastq(path, device="cuda", quality_cutoff=20, _chunk_bytes=chunk)) == host


@pytest.mark.parametrize("name", ("whole", "no_newline", "cut"))
def test_fastq_gpu_quality_range_seam(gpu, seam_files, name):
    """The end of a multi-GPU range is a seam too, and there the range's end says nothing about the file's:
    seven engines on device 0 take the ranges of ss_fastq_split, which for these files end after a sequence
    line (whole: ranges 1-3; cut: 2-6) and after a '+' line (no_newline: range 4)."""
    path, host = seam_files[name]
    size = {"whole": 400 * REC, "no_newline": 400 * REC - 1, "cut": 400 * REC - 31}[name]
    ends = [(size * p // 7) % REC for p in range(1, 7)]         # a range ends after the line this byte lies in
    assert any(8 <= o <= 38 for o in ends) and (name != "no_newline" or any(o in (39, 40) for o in ends))
    assert _items(sq.read_and_count_fastq(path, device=[0] * 7, quality_cutoff=20)) == host
    assert _items(sq.read_and_count_fastq(path, device=[0] * 3, quality_cutoff=20, _chunk_bytes=997)) == host


def test_fastq_gpu_quality_seam_behind_a_long_plus_line(gpu, tmp_path):
    """The '+' line repeats a 6000-byte header: the seam read's quality line lies past several reads of the file."""
    rng = np.random.default_rng(6000)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = []
    for i in range(40):
        name = b"%04d" % i + b"x" * 6000
        recs.append(b"@" + name + b"\n" + bytes(rng.choice(acgt, 30)) + b"\n+" + name + b"\n" +
                    b"I" * (29 - i % 20) + b"#" * (1 + i % 20) + b"\n")
    p = tmp_path / "plus.fq"
    p.write_bytes(b"".join(recs))
    host = _items(sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20))
    for chunk in (len(recs[0]) * 3 + 6006 + 31, len(recs[0]) * 3 + 6006 + 31 + 6006, 20000):
        assert _items(sq.read_and_count_fastq(str(p), device="cuda", quality_cutoff=20, _chunk_bytes=chunk)) == host


def test_fastq_gpu_quality_errors(gpu, tmp_path):
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def write(name, recs):
        p = tmp_path / name
        p.write_bytes(b"".join(b"@r\n" + s + b"\n+\n" + q + b"\n" for s, q in recs))
        return str(p)

    good = [(bytes(rng.choice(acgt, 30)), b"I" * 24 + b"#" * 6) for _ in range(50)]
    for bad in (b"N", b"#", b"\xff"):
        # an invalid byte only in the quality-trimmed tail: no error, the host's counts
        seq = bytes(rng.choice(acgt, 24)) + bad * 3 + b"ACG"
        path = write("tail.fq", good + [(seq, b"I" * 24 + b"#" * 6)] + good)
        assert _items(sq.read_and_count_fastq(path, device="cuda", quality_cutoff=20)) == _items(
            sq.read_and_count_fastq(path, device="host", quality_cutoff=20))
        # the same byte in the kept prefix: the host's exception, i.e. that of sq.pack(kept prefix)
        seq = bytes(rng.choice(acgt, 10)) + bad + bytes(rng.choice(acgt, 19))
        path = write("kept.fq", good + [(seq, b"I" * 24 + b"#" * 6)] + good)
        with pytest.raises(Exception) as e_pack:
            sq.pack(seq[:24])
        with pytest.raises(Exception) as e_host:
            sq.read_and_count_fastq(path, device="host", quality_cutoff=20)
        with pytest.raises(Exception) as e_gpu:
            sq.read_and_count_fastq(path, device="cuda", quality_cutoff=20)
        assert type(e_gpu.value) is type(e_host.value) is type(e_pack.value)
        assert str(e_gpu.value) == str(e_host.value) == str(e_pack.value)
    # an 1100-byte line is still the too-long error
    path = write("long.fq", good + [(bytes(rng.choice(acgt, 1100)), b"#" * 1100)])
    for dev in ("host", "cuda"):
        with pytest.raises(Exception, match="Sequences longer than 1024 bases are not supported."):
            sq.read_and_count_fastq(path, device=dev, quality_cutoff=20)
    with pytest.raises(ValueError):
        sq.read_and_count_fastq(path, device="cuda", quality_cutoff=94)
    with pytest.raises(ValueError):
        sq.read_and_count_fastq(path, device="cuda", quality_cutoff=20, quality_base=35)


def test_fastq_gpu_quality_setting_is_cleared(gpu, tmp_path):
    """The engines are pooled per device: a call without a cutoff after one with a cutoff reuses the engine
    and must count the untrimmed reads."""
    rng = np.random.default_rng(12)
    text, seqs, _quals = Q.degraded_library(rng, 3000, pool=50)
    p = tmp_path / "c.fq"
    p.write_bytes(text)
    plain_host = _items(sq.read_and_count_fastq(str(p), device="host"))
    trimmed_host = _items(sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20))
    assert plain_host != trimmed_host
    assert _items(sq.read_and_count_fastq(str(p), device="cuda", quality_cutoff=20)) == trimmed_host
    assert _items(sq.read_and_count_fastq(str(p), device="cuda")) == plain_host
    assert _items(sq.ShortSeqCounter(seqs, device="cuda")) == plain_host
    # also after a call that raised with the cutoff set
    q = tmp_path / "d.fq"
    q.write_bytes(b"@r\nACGTNACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIII###\n")
    with pytest.raises(Exception, match="Unsupported base character"):
        sq.read_and_count_fastq(str(q), device="cuda", quality_cutoff=20)
    assert _items(sq.read_and_count_fastq(str(p), device="cuda")) == plain_host
