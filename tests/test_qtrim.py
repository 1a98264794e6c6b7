"""3' quality trim on the host (no GPU): ss_host_trim_quality3 and csrc/host_qtrim.h against the rule and
the quality-line locate restated in Python (tests/qtrim_cases.py), in both forms; the SS_EARG cases;
read_and_count_fastq(device="host", quality_cutoff=...) against ShortSeqCounter of the Python-trimmed lines,
alone and with adapter=; and tools/qtrim_selftest.cpp -- the header against naive loops with every buffer in
an exactly-sized heap block -- built with ASan + UBSan as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shortseq_amd as sq
import shortseq_amd.batch as B
from shortseq_amd._native import SS_EARG, SS_OK, lib

import qtrim_cases as Q
import trim_cases as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTER = b"TGGAATTCTCGGGTGCCAAGG"


def test_python_rule_on_known_reads():
    """The restated rule itself, on reads worked out by hand (cutoff 20, base 33: 'I' = 40, '#' = 2, '5' = 20)."""
    assert Q.ref_qtrim(b"IIIIIIII", 8, 20, 33) == 8
    assert Q.ref_qtrim(b"########", 8, 20, 33) == 0
    assert Q.ref_qtrim(b"IIII####", 8, 20, 33) == 4
    assert Q.ref_qtrim(b"55555555", 8, 20, 33) == 8              # every score 0: the walk goes on, nothing moves
    assert Q.ref_qtrim(b"II#I", 4, 20, 33) == 4                  # the last base is good: s < 0 at once
    assert Q.ref_qtrim(b"#I##", 4, 20, 33) == 2                  # sums 18 36 16 34: the greatest one at 2
    assert Q.ref_qtrim(b"#II##", 5, 20, 33) == 3                 # sums 18 36 16 -4: the walk ends, the left # stays
    assert Q.ref_qtrim(b"4564", 4, 20, 33) == 3                  # sums 1 0 0 1: the right one of two equal maxima
    assert Q.ref_qtrim(b"", 0, 20, 33) == 0
    assert Q.ref_locate(b"@h\nACGT\n+h\nIIII\n@", 3, 4) == (11, 4)
    assert Q.ref_locate(b"@h\nACGT\n+h\nIII", 3, 4) == (11, 3)
    assert Q.ref_locate(b"@h\nACGT\n+h", 3, 4) is None


@pytest.mark.parametrize("base", Q.BASES)
@pytest.mark.parametrize("cutoff", Q.CUTOFFS)
def test_host_explicit_form_matches_python_rule(cutoff, base):
    rng = np.random.default_rng(100 * cutoff + base)
    quals = Q.sweep_quals(rng, cutoff, base, newline=True)
    blob, offs, lens, qual, qoffs = Q.explicit_layout(rng, quals)
    exp, exp_stats = Q.expected_explicit(quals, cutoff, base)
    assert 0 < exp_stats[0] < len(quals)
    got, stats = B.host_trim_quality(blob, offs, lens, cutoff, base=base, qual=qual, qoffsets=qoffs, stats=True)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (cutoff, base, int(bad[0]), quals[int(bad[0])], int(got[bad[0]]), int(exp[bad[0]]))
    assert [int(x) for x in stats] == exp_stats
    lens2 = lens.copy()      # in place, and without stats
    assert B.host_trim_quality(blob, offs, lens2, cutoff, base=base, qual=qual, qoffsets=qoffs, out=lens2) is lens2
    assert np.array_equal(lens2, exp)


@pytest.mark.parametrize("base", Q.BASES)
@pytest.mark.parametrize("cutoff", Q.CUTOFFS)
def test_host_fastq_form_matches_python_rule(cutoff, base):
    rng = np.random.default_rng(200 * cutoff + base)
    quals = Q.sweep_quals(rng, cutoff, base, newline=False)
    for tail in (b"\n", b""):
        text, offs, lens = Q.fastq_layout(rng, quals, tail)
        exp, exp_stats = Q.expected_fastq(text, offs, lens, cutoff, base)
        assert exp_stats[0] > 0 and exp_stats[2] > 0
        got, stats = B.host_trim_quality(Q.as_blob(text), offs, lens, cutoff, base=base, stats=True)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (cutoff, base, int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
        assert [int(x) for x in stats] == exp_stats
    seen = set()
    for text, offs, lens in Q.special_texts(cutoff, base):
        exp, exp_stats = Q.expected_fastq(text, offs, lens, cutoff, base)
        got, stats = B.host_trim_quality(Q.as_blob(text), offs, lens, cutoff, base=base, stats=True)
        assert np.array_equal(got, exp), (text, got, exp)
        assert [int(x) for x in stats] == exp_stats
        seen.add((int(exp[1]), exp_stats[2]))
    assert (20, 1) in seen and (12, 0) in seen       # the second read without its quality line, and with it


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65))
def test_host_counts(n):
    rng = np.random.default_rng(300 + n)
    quals = [bytes(rng.integers(33, 75, int(rng.integers(1, 60)), dtype=np.int64).astype(np.uint8)) for _ in range(n)]
    text, offs, lens = Q.fastq_layout(rng, quals)
    exp, exp_stats = Q.expected_fastq(text, offs, lens, 20, 33)
    got, stats = B.host_trim_quality(Q.as_blob(text), offs, lens, 20, stats=True)
    assert np.array_equal(got, exp) and [int(x) for x in stats] == exp_stats
    blob, offs, lens, qual, qoffs = Q.explicit_layout(rng, quals)
    exp, exp_stats = Q.expected_explicit(quals, 20, 33)
    got, stats = B.host_trim_quality(blob, offs, lens, 20, qual=qual, qoffsets=qoffs, stats=True)
    assert np.array_equal(got, exp) and [int(x) for x in stats] == exp_stats


def _raw_host(blob, offs, lens, qual, qoffs, cutoff, base, out, stats=None, n=None):
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    return lib().ss_host_trim_quality3(p(blob), 0 if blob is None else blob.size, p(offs), p(lens),
                                       (lens.size if lens is not None else 1) if n is None else n, p(qual),
                                       0 if qual is None else qual.size, p(qoffs), cutoff, base, p(out), p(stats))


def test_host_earg_leaves_output_untouched():
    text = b"@h\nACGTACGT\n+\nIIII####\n@h\nACGT\n+\nII##\n"
    blob = Q.as_blob(text)
    offs = np.array([3, 26], np.uint64)
    lens = np.array([8, 4], np.uint32)
    qual = Q.as_blob(b"IIII####II##")
    qoffs = np.array([0, 8], np.uint64)
    mark = np.array([0xDEADBEEF, 0xDEADBEEF], np.uint32)
    stats = np.array([7, 7, 7], np.uint64)

    def refused(*args, **kw):
        out = mark.copy()
        assert _raw_host(*args, out=out, stats=stats, **kw) == SS_EARG
        assert np.array_equal(out, mark) and list(stats) == [7, 7, 7]

    refused(None, offs, lens, None, None, 20, 33)           # the layout form needs the blob
    refused(blob, None, lens, None, None, 20, 33)
    refused(blob, offs, None, None, None, 20, 33)
    refused(blob, offs, lens, None, qoffs, 20, 33)          # quality offsets without quality bytes
    for cutoff, base in ((0, 33), (94, 33), (20, 0), (20, 32), (20, 34), (20, 63), (20, 65)):
        refused(blob, offs, lens, None, None, cutoff, base)
        refused(blob, offs, lens, qual, qoffs, cutoff, base)
    assert _raw_host(blob, offs, lens, None, None, 20, 33, out=None) == SS_EARG
    refused(blob, offs, lens, None, None, 20, 33, n=1 << 32)                 # (nothing is dereferenced)
    # a read or a quality run ending past its buffer: refused before anything is written ...
    refused(blob, np.array([3, len(text) - 3], np.uint64), lens, None, None, 20, 33)
    refused(blob, np.array([2 ** 64 - 1, 26], np.uint64), lens, None, None, 20, 33)
    refused(blob, offs, lens, qual, np.array([0, 9], np.uint64), 20, 33)
    refused(blob, offs, lens, qual, np.array([13, 8], np.uint64), 20, 33)
    # ... but not for a read that is too long anyway: it is never read
    out = mark.copy()
    assert _raw_host(blob, np.array([3, 2 ** 40], np.uint64), np.array([8, 0xFFFFFFFF], np.uint32), None, None, 20, 33,
                     out=out) == SS_OK
    assert list(out) == [4, 0xFFFFFFFF]
    out = mark.copy()
    assert _raw_host(blob, offs, np.array([8, 1025], np.uint32), qual, np.array([0, 2 ** 40], np.uint64), 20, 33, out=out) == SS_OK
    assert list(out) == [4, 1025]
    # the two forms agree here; n == 0 needs no buffers and zeroes the stats
    assert list(B.host_trim_quality(blob, offs, lens, 20)) == [4, 2]
    assert list(B.host_trim_quality(blob, offs, lens, 20, qual=qual, qoffsets=qoffs)) == [4, 2]
    st = np.array([5, 5, 5], np.uint64)
    assert lib().ss_host_trim_quality3(None, 0, None, None, 0, None, 0, None, 20, 33, None, st.ctypes.data) == SS_OK
    assert list(st) == [0, 0, 0]


def test_python_argument_checks():
    blob = Q.as_blob(b"@h\nACGT\n+\nII##\n")
    offs, lens = np.array([3], np.uint64), np.array([4], np.uint32)
    for cutoff, base in ((0, 33), (94, 33), (-1, 33), (20, 0), (20, 32), (20, 65)):
        with pytest.raises(ValueError):
            B.host_trim_quality(blob, offs, lens, cutoff, base=base)
        with pytest.raises(ValueError):
            sq.read_and_count_fastq("nowhere.fq", device="host", quality_cutoff=cutoff, quality_base=base)
    with pytest.raises(ValueError):
        B.host_trim_quality(blob, offs, lens, 20, qual=blob)
    assert list(B.host_trim_quality(blob, offs, lens, 20)) == [2]
    assert list(B.host_trim_quality(blob, offs, lens, 20, base=64)) == [0]       # 'I' is 9 above base 64


def _items(c):
    return [(str(k), len(k), v) for k, v in c.items()]


def _py_quality(seqs, quals, cutoff=20, base=33):
    return [s[:Q.ref_qtrim(q, len(s), cutoff, base)] if len(q) >= len(s) else s for s, q in zip(seqs, quals)]


def test_fastq_host_quality_library(tmp_path, capsys):
    rng = np.random.default_rng(4242)
    n = 20000
    text, seqs, quals = Q.degraded_library(rng, n)
    p = tmp_path / "lib.fq"
    p.write_bytes(text)
    cut = _py_quality(seqs, quals)
    shortened = sum(1 for a, b in zip(cut, seqs) if len(a) < len(b))
    assert 0 < shortened < n
    got = sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20)
    assert _items(got) == _items(sq.ShortSeqCounter(cut, device="host"))
    assert _items(sq.read_and_count_fastq(str(p), "host", quality_cutoff=20, quality_base=33)) == _items(got)
    # quality, then the adapter on the kept prefix
    both = [s[:T.ref_trim(s, ADAPTER, 3, 10)] for s in cut]
    got_both = sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20, adapter=ADAPTER)
    assert _items(got_both) == _items(sq.ShortSeqCounter(both, device="host"))
    alone = sq.read_and_count_fastq(str(p), device="host", adapter=ADAPTER)
    assert _items(alone) == _items(sq.ShortSeqCounter([s[:T.ref_trim(s, ADAPTER, 3, 10)] for s in seqs], device="host"))
    assert _items(got_both) != _items(alone) and len(got_both) < len(alone)
    # without a cutoff nothing changed
    assert _items(sq.read_and_count_fastq(str(p), device="host")) == _items(sq.ShortSeqCounter(seqs, device="host"))
    assert "total seqs" in capsys.readouterr().out


def test_fastq_host_quality_odd_records(tmp_path):
    """A short and a missing quality line keep the read; a longer one uses its first bytes; the last
    quality line needs no newline; a bad byte in the removed tail is no error, one in the kept prefix is."""
    recs = [(b"ACGTACGTAC", b"IIIIII####"),        # -> ACGTAC
            (b"ACGTACGTAC", b"IIIIII###"),         # short: kept whole
            (b"ACGTACGTAC", b"IIIIIIII##J"),       # long: the first 10 bytes count -> ACGTACGT
            (b"ACGTACNN", b"IIIIII##"),            # the invalid bytes lie in the removed tail
            (b"GGGG", b"####"),                    # -> the empty read
            (b"TTTTTT", b"IIII##")]                # the file's last line, without a newline -> TTTT
    text = b"".join(b"@r%d\n" % i + s + b"\n+r%d\n" % i + q + b"\n" for i, (s, q) in enumerate(recs))[:-1]
    p = tmp_path / "odd.fq"
    p.write_bytes(text)
    exp = [b"ACGTAC", b"ACGTACGTAC", b"ACGTACGT", b"ACGTAC", b"", b"TTTT"]
    assert _py_quality([s for s, _ in recs], [q for _, q in recs]) == exp
    got = sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20)
    assert _items(got) == _items(sq.ShortSeqCounter(exp, device="host"))
    assert got[sq.pack(b"")] == 1
    with pytest.raises(Exception, match="Unsupported base character"):
        sq.read_and_count_fastq(str(p), device="host")
    # the file cut after the last record's '+' line: that read keeps its length
    cut = text[:text.rindex(b"\n") + 1]
    p.write_bytes(cut)
    got = sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20)
    assert _items(got) == _items(sq.ShortSeqCounter(exp[:-1] + [b"TTTTTT"], device="host"))
    # a bad byte in the kept prefix: the packer's own exception
    p.write_bytes(b"@r\nACNTACGT\n+\nIIIIII##\n")
    with pytest.raises(Exception) as e_pack:
        sq.pack(b"ACNTAC")
    with pytest.raises(Exception) as e_fq:
        sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20)
    assert type(e_fq.value) is type(e_pack.value) and str(e_fq.value) == str(e_pack.value)
    # a line past 1024 bytes stays the too-long error
    p.write_bytes(b"@r\n" + b"A" * 1100 + b"\n+\n" + b"#" * 1100 + b"\n")
    with pytest.raises(Exception, match="longer than 1024"):
        sq.read_and_count_fastq(str(p), device="host", quality_cutoff=20)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer runs belong on the CPU host")
def test_qtrim_selftest_sanitized(tmp_path):
    # a stand-alone program with its own sanitizer runtime; nothing is loaded into this process
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    exe = str(tmp_path / "qtrim_selftest")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(REPO, "tools", "qtrim_selftest.cpp"), "-o", exe], check=True, env=env)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    for mark in ("Sanitizer", "runtime error", "FAILED"):
        assert mark not in r.stderr, r.stderr[-4000:]
    assert "all checks held" in r.stdout
