"""3' adapter trim on the host (no GPU): ss_host_trim_adapter3 and csrc/host_trim.h against the rule
restated in Python (tests/trim_cases.py: slicing and a sum over the zipped bytes), the SS_EARG cases,
read_and_count_fastq(device="host", adapter=...) against ShortSeqCounter of the Python-trimmed lines,
and tools/trim_selftest.cpp -- the header against a naive loop with every read in an exactly-sized heap
block -- built with ASan + UBSan as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shortseq_amd as sq
import shortseq_amd.batch as B
from shortseq_amd._native import SS_EARG, SS_OK, lib

import trim_cases as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("back", "junk", "residue")


@pytest.mark.parametrize("A", T.ADAPTER_LENS)
def test_host_trim_matches_python_rule(A):
    rng = np.random.default_rng(1000 + A)
    for ci, (a_len, mo, ed) in enumerate(c for c in T.combos() if c[0] == A):
        adapter = T.rand_seq(rng, a_len)
        reads = T.sweep_reads(rng, adapter, mo, ed)
        blob, offs, lens = T.layout(rng, reads, LAYOUTS[ci % 3])
        exp, exp_stats = T.expected(reads, adapter, mo, ed)
        got, stats = B.host_trim_adapter(blob, offs, lens, adapter, min_overlap=mo, err_div=ed, stats=True)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (A, mo, ed, int(bad[0]), reads[int(bad[0])], int(got[bad[0]]), int(exp[bad[0]]))
        assert [int(x) for x in stats] == exp_stats
        # in place, and without stats
        lens2 = lens.copy()
        assert B.host_trim_adapter(blob, offs, lens2, adapter, min_overlap=mo, err_div=ed, out=lens2) is lens2
        assert np.array_equal(lens2, exp)


@pytest.mark.parametrize("A", (3, 8, 17, 64))
def test_host_trim_wildcards(A):
    rng = np.random.default_rng(2000 + A)
    for adapter in T.wildcard_adapters(rng, A):
        reads = T.wildcard_reads(rng, adapter)
        for mo, ed in ((1, 0), (3, 10), (A, 4)):
            blob, offs, lens = T.layout(rng, reads, "back")
            exp, exp_stats = T.expected(reads, adapter, mo, ed)
            got, stats = B.host_trim_adapter(blob, offs, lens, adapter, min_overlap=mo, err_div=ed, stats=True)
            assert np.array_equal(got, exp), (adapter, mo, ed)
            assert [int(x) for x in stats] == exp_stats
            if mo <= max(1, A - 2):      # the occurrence at 13 is found whatever lies under the wildcards
                assert all(int(g) <= 13 for g in got[:-1]), (adapter, got)      # (or a chance match before it)


def test_host_trim_consequences_of_the_rule():
    """err_div = 1 trims every read with enough overlap to 0; a 3-byte chance match at the end trims."""
    blob = np.frombuffer(b"GGGGGGGGGG" + b"CC" + b"ACACACATGG", np.uint8)
    offs = np.array([0, 10, 12], np.uint64)
    lens = np.array([10, 2, 10], np.uint32)
    assert list(B.host_trim_adapter(blob, offs, lens, b"TTTT", min_overlap=3, err_div=1)) == [0, 2, 0]
    assert list(B.host_trim_adapter(blob, offs, lens, b"TGGAATTC", min_overlap=3, err_div=10)) == [10, 2, 7]
    # case-sensitive, and an N in the read is a mismatch
    blob = np.frombuffer(b"ACGTtggaattcACGTNGGAATTC", np.uint8)
    assert list(B.host_trim_adapter(blob, np.array([0, 12], np.uint64), np.array([12, 12], np.uint32), b"TGGAATTC",
                                    min_overlap=3, err_div=0)) == [12, 12]


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 20000))
def test_host_trim_layouts_and_counts(kind, n):
    rng = np.random.default_rng(3000 + n)
    adapter = b"TGGAATTCTCGGGTGCCAAGG"
    reads = T.library_reads(rng, n, adapter)
    blob, offs, lens = T.layout(rng, reads, kind)
    if n and kind == "back":
        assert offs[0] == 0 and offs[-1] + lens[-1] == blob.size
    exp, exp_stats = T.expected(reads, adapter, 3, 10)
    got, stats = B.host_trim_adapter(blob, offs, lens, adapter, stats=True)
    assert np.array_equal(got, exp)
    assert [int(x) for x in stats] == exp_stats


def _raw_host_trim(blob, offs, lens, adapter, A, mo, ed, out, stats=None):
    return lib().ss_host_trim_adapter3(blob.ctypes.data if blob is not None else None, 0 if blob is None else blob.size,
                                       offs.ctypes.data if offs is not None else None,
                                       lens.ctypes.data if lens is not None else None, lens.size if lens is not None else 1,
                                       adapter, A, mo, ed, out.ctypes.data if out is not None else None,
                                       stats.ctypes.data if stats is not None else None)


def test_host_trim_earg_leaves_output_untouched():
    blob = np.frombuffer(b"ACGTACGTACGTTGGAATTC", np.uint8)
    offs = np.array([0, 8], np.uint64)
    lens = np.array([8, 12], np.uint32)
    ad = (C.c_uint8 * 64).from_buffer_copy(b"TGGAATTC" + bytes(56))
    mark = np.array([0xDEADBEEF, 0xDEADBEEF], np.uint32)
    stats = np.array([7, 7], np.uint64)

    def refused(*args, **kw):
        out = mark.copy()
        rc = _raw_host_trim(*args, out=out, stats=stats, **kw)
        assert rc == SS_EARG
        assert np.array_equal(out, mark) and list(stats) == [7, 7]

    refused(None, offs, lens, ad, 8, 3, 10)
    refused(blob, None, lens, ad, 8, 3, 10)
    refused(blob, offs, None, ad, 8, 3, 10)
    refused(blob, offs, lens, None, 8, 3, 10)
    refused(blob, offs, lens, ad, 0, 3, 10)
    refused(blob, offs, lens, ad, 65, 3, 10)
    refused(blob, offs, lens, ad, 8, 0, 10)
    assert _raw_host_trim(blob, offs, lens, ad, 8, 3, 10, out=None) == SS_EARG
    # n >= 2^32 (nothing is dereferenced)
    assert lib().ss_host_trim_adapter3(blob.ctypes.data, blob.size, offs.ctypes.data, lens.ctypes.data, 1 << 32, ad, 8, 3,
                                       10, mark.ctypes.data, None) == SS_EARG
    # a read ending past the blob, and an offset past it: refused before anything is written ...
    refused(blob, np.array([0, 9], np.uint64), lens, ad, 8, 3, 10)
    refused(blob, np.array([0, 21], np.uint64), np.array([8, 0], np.uint32), ad, 8, 3, 10)
    refused(blob, np.array([2 ** 64 - 1, 0], np.uint64), np.array([2, 8], np.uint32), ad, 8, 3, 10)
    # ... but not for a read that is too long anyway: it is never read
    out = mark.copy()
    assert _raw_host_trim(blob, np.array([0, 2 ** 40], np.uint64), np.array([8, 0xFFFFFFFF], np.uint32), ad, 8, 3, 10,
                          out=out) == SS_OK
    assert list(out) == [8, 0xFFFFFFFF]
    # n == 0 needs no buffers; the stats are zeroed
    st = np.array([5, 5], np.uint64)
    assert lib().ss_host_trim_adapter3(None, 0, None, None, 0, ad, 8, 3, 10, None, st.ctypes.data) == SS_OK
    assert list(st) == [0, 0]


def test_python_argument_checks():
    blob = np.frombuffer(b"ACGT", np.uint8)
    offs, lens = np.array([0], np.uint64), np.array([4], np.uint32)
    for bad in (b"", b"A" * 65):
        with pytest.raises(ValueError):
            B.host_trim_adapter(blob, offs, lens, bad)
    with pytest.raises(ValueError):
        B.host_trim_adapter(blob, offs, lens, b"ACG", min_overlap=0)
    with pytest.raises(ValueError):
        sq.read_and_count_fastq("nowhere.fq", device="host", adapter="")
    with pytest.raises(TypeError):
        sq.read_and_count_fastq("nowhere.fq", device="host", adapter=5)
    assert list(B.host_trim_adapter(blob, offs, lens, "GT", min_overlap=2)) == [2]      # a str adapter


ADAPTER = b"TGGAATTCTCGGGTGCCAAGG"


def _fastq_lines():
    """Sequence lines (as the file holds them, before the strlen - 1 cut) and the whole file."""
    rng = np.random.default_rng(77)
    seqs = [T.rand_seq(rng, 22) + ADAPTER[:15],            # trimmed to its insert
            T.rand_seq(rng, 30),                           # no adapter
            ADAPTER + T.rand_seq(rng, 5),                  # trims to b""
            T.rand_seq(rng, 18) + ADAPTER + b"NN#",        # its only invalid bytes lie in the removed tail
            T.rand_seq(rng, 22) + ADAPTER[:15],
            T.rand_seq(rng, 40) + ADAPTER,                 # a two-word key after the trim
            T.rand_seq(rng, 25) + ADAPTER[:4]]
    seqs[4] = seqs[0]                                      # a repeated key
    recs = []
    for i, s in enumerate(seqs):
        recs.append(b"@read%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n")
    # the last record's quality line has no newline; one more record whose SEQUENCE line is the file's
    # last line would lose its last character: keep that rule in view with a second file below
    data = b"".join(recs)[:-1]
    return seqs, data


def _py_trimmed(lines):
    return [ln[:T.ref_trim(ln, ADAPTER, 3, 10)] for ln in lines]


def _items(c):
    return [(str(k), len(k), v) for k, v in c.items()]


def test_fastq_host_adapter(tmp_path, capsys):
    seqs, data = _fastq_lines()
    p = tmp_path / "a.fq"
    p.write_bytes(data)
    got = sq.read_and_count_fastq(str(p), device="host", adapter=ADAPTER)
    exp = sq.ShortSeqCounter(_py_trimmed(seqs), device="host")
    assert _items(got) == _items(exp)
    assert any(len(k) == 0 for k in got) and got[sq.pack(b"")] == 1
    # str adapter, explicit parameters; and without an adapter the invalid tail is an error again
    assert _items(sq.read_and_count_fastq(str(p), "host", adapter=ADAPTER.decode(), min_overlap=3, err_div=10)) == _items(exp)
    with pytest.raises(Exception, match="Unsupported base character"):
        sq.read_and_count_fastq(str(p), device="host")
    # a file ending inside a sequence line: the line loses its last character first (strlen - 1), then is trimmed
    q = tmp_path / "b.fq"
    last = T.rand_seq(np.random.default_rng(5), 20) + ADAPTER[:10]
    q.write_bytes(data + b"\n@last\n" + last)
    got = sq.read_and_count_fastq(str(q), device="host", adapter=ADAPTER)
    exp = sq.ShortSeqCounter(_py_trimmed(seqs + [last[:-1]]), device="host")
    assert _items(got) == _items(exp)
    assert "total seqs" in capsys.readouterr().out


def test_fastq_host_adapter_bad_byte_in_kept_prefix(tmp_path):
    rng = np.random.default_rng(9)
    for bad in (b"N", b"#", b"\xff"):
        line = T.rand_seq(rng, 10) + bad + T.rand_seq(rng, 9) + ADAPTER[:14]
        trimmed = line[:T.ref_trim(line, ADAPTER, 3, 10)]
        assert trimmed == line[:20]
        p = tmp_path / "bad.fq"
        p.write_bytes(b"@r\n" + line + b"\n+\n" + b"I" * len(line) + b"\n")
        with pytest.raises(Exception) as e_pack:
            sq.pack(trimmed)
        with pytest.raises(Exception) as e_fq:
            sq.read_and_count_fastq(str(p), device="host", adapter=ADAPTER)
        assert type(e_fq.value) is type(e_pack.value) and str(e_fq.value) == str(e_pack.value)
    # a line past 1024 bytes stays the too-long error, adapter or not
    line = T.rand_seq(rng, 50) + ADAPTER + T.rand_seq(rng, 1100 - 50 - len(ADAPTER))
    p = tmp_path / "long.fq"
    p.write_bytes(b"@r\n" + line + b"\n+\n" + b"I" * len(line) + b"\n")
    with pytest.raises(Exception, match="longer than 1024"):
        sq.read_and_count_fastq(str(p), device="host", adapter=ADAPTER)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer runs belong on the CPU host")
def test_trim_selftest_sanitized(tmp_path):
    # a stand-alone program with its own sanitizer runtime; nothing is loaded into this process
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    exe = str(tmp_path / "trim_selftest")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tools", "trim_selftest.cpp"), "-o", exe], check=True, env=env)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    for mark in ("Sanitizer", "runtime error", "FAILED"):
        assert mark not in r.stderr, r.stderr[-4000:]
    assert "all checks held" in r.stdout
