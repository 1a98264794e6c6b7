"""ss_fastq_index_onepass and ss_fastq_scan + ss_fastq_index where the texts of test_fastq.py do not reach
(inputs: tests/fastq_shapes.py): newlines of every kind of line two bytes around the tile seams of both
paths and texts that end there; lines longer than a tile (start_before's walk); one-pass tiles with 0 to
32 768 newlines, at and next to 512, 1024, 2048 (kTileCap), 2112 and 4096 (kLdsPos); NUL bytes at 64 / 65
(kNulListScan) and 65 536 / 65 537 NUL-holding lines (kNulCap), next to sub-block and tile edges, in a long
and in an unterminated line; every line phase on all tiny texts; and 1027 / 2053 tiles (two and three
tile groups, two tickets).  The expectation is a NumPy statement of the rule, pinned here to the C oracle.
Without a device the file proves that reference, the restated constants against the source, and a census
per family: that each text reaches what it is there for."""
import os

import numpy as np
import pytest

import fastq_shapes as S

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shortseq_amd", "csrc", "ss_fastq.hip")

FAMILIES = {"seams": S.seam_cases, "long": S.long_line_cases, "density": S.density_cases, "nul": S.nul_cases}
EDGE_TILE = {"seams": S.TILE2, "long": S.TILE1, "density": S.TILE1, "nul": S.TILE2}


# ---- without a device --------------------------------------------------------------------------------------

def _ora(oracle, data: bytes, line0: int = 0):
    """The C oracle on a chunk whose first line has the number line0: line0 empty lines in front, the
    entries that start inside them dropped."""
    offs, lens = oracle.fastq_index(b"\n" * line0 + data)
    keep = offs >= line0
    return offs[keep] - np.uint64(line0), lens[keep], data.count(b"\n")


def _first_diff(got, exp):
    """None, or a description of the first sequence line that differs."""
    (go, gl, gn), (eo, el, en) = got, exp
    n = min(go.size, eo.size)
    bad = np.flatnonzero((go[:n] != eo[:n]) | (gl[:n] != el[:n]))
    if bad.size:
        i = int(bad[0])
        return (f"{bad.size} of {n} sequence lines differ; line {i}: offset {int(go[i])} length {int(gl[i])}, expected "
                f"offset {int(eo[i])} length {int(el[i])}; expected offset mod 16384 = {int(eo[i]) % S.TILE2}, mod 32768 = "
                f"{int(eo[i]) % S.TILE1}, tile {int(eo[i]) // S.TILE1}")
    if go.size != eo.size:
        return f"{go.size} sequence lines, expected {eo.size} (the first {n} agree)"
    if gn != en:
        return f"{gn} newlines, expected {en}"
    return None


def _same(got, exp, what):
    assert got[0].dtype == exp[0].dtype == np.uint64 and got[1].dtype == exp[1].dtype == np.uint32, what
    msg = _first_diff(got, exp)
    assert msg is None, (what, msg)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[2] == exp[2], what


def test_reference_is_the_oracle_on_every_tiny_text(oracle):
    texts = S.tiny_texts(b"A\n\0", 7)
    assert len(texts) == 3280
    for t in texts:
        for l0 in range(4):
            _same(S.np_index(t, l0), _ora(oracle, t, l0), (t, l0))


@pytest.mark.parametrize("family", list(FAMILIES) + ["groups", "dense file"])
def test_reference_is_the_oracle(oracle, family):
    cases = {"groups": lambda: [S.Case("groups", S.groups_text(), 0)],
             "dense file": lambda: [S.Case("dense file", S.dense_file_text(), 0)]}.get(family, FAMILIES.get(family))()
    for c in cases:
        for l0 in range(4):
            _same(S.np_index(c.data, l0), _ora(oracle, c.data, l0), (c.name, l0))
        assert len(c.data) > S.TILE1, c.name


def test_reference_speed():
    """np_index has no loop per line: the 33.6-MB text in well under a second (the C oracle: 0.06 s)."""
    import time
    data = S.groups_text()
    t0 = time.perf_counter()
    S.np_index(data)
    dt = time.perf_counter() - t0
    print(f"np_index on {len(data)} bytes: {dt:.3f} s")
    assert dt < 2.0


def test_restated_constants_match_the_source():
    with open(SRC) as f:
        src = S.source_constants(f.read())
    for name, value in S.KERNEL_CONSTANTS.items():
        assert src.get(name) == value, (name, src.get(name), value)
    assert src["kFqTile"] == S.TILE2 and src["kFqTile1"] == S.TILE1
    assert src["kSubPerTile"] * S.NUL_SUB == S.TILE1
    assert sorted(S.KERNEL_CONSTANTS) == sorted(["kFqT", "kFqU", "kFqU1", "kTileCap", "kLdsPos", "kNulListScan", "kNulCap"])


def test_seam_census():
    for seed in (0, 1):
        data = S.seam_text(seed)
        for tile in (S.TILE2, S.TILE1):
            pairs, starts = S.seam_census(data, tile)
            print(f"seams {seed}: {len(data)} bytes, tile {tile}: {len(pairs)} (kind, d) pairs, {starts} sequence lines "
                  f"start at a tile start")
            assert pairs == set(S.SEAM_COMBOS), (seed, tile, sorted(set(S.SEAM_COMBOS) - pairs))
            assert starts >= 1
        assert len(data) > S.SEAM_COUNT * S.TILE2
    assert S.seam_text(0).endswith(b"\n") and not S.seam_text(1).endswith(b"\n")
    assert S.np_index(S.seam_text(1))[2] % 4 == 1                    # ... inside a sequence line
    seen = set()
    for name, text, seam, e, leave in S.seam_cut_texts():
        nl = text.count(b"\n")
        got = "complete" if text.endswith(b"\n") else ("sequence" if nl % 4 == 1 else "other")
        assert len(text) == seam + e and got == leave, (name, len(text), got)
        assert text[:80_000] == S.seam_text(0)[:80_000]
        seen.add((seam % S.TILE1 == 0, e, leave))
    print(f"seam cuts: {len(seen)} (tile size, end - S, leave) combinations")
    assert len(seen) == 18


def test_long_line_census():
    cases = S.long_line_cases()
    assert len(cases) == 20
    for c in cases:
        counts = S.tile_counts(c.data, S.TILE1)
        whole = counts[:len(c.data) // S.TILE1]                      # (a last partial tile is not a whole tile)
        empty, empty2 = int((whole == 0).sum()), int((S.tile_counts(c.data, S.TILE2)[:len(c.data) // S.TILE2] == 0).sum())
        offs, lens, nl = S.np_index(c.data, c.line0)
        print(f"{c.name}: {len(c.data)} bytes, line0 {c.line0}, {nl} newlines, newline-free tiles: {empty} of 32 KiB, "
              f"{empty2} of 16 KiB, longest sequence line {int(lens.max()) if lens.size else None}")
        assert empty >= 1 and empty2 >= 3, c.name
        if "sequence" in c.name:
            assert int(lens.max()) == S.LONG - 1, c.name             # reported exactly, not capped at 1024
        if c.name == "long sequence first":
            assert c.line0 == 1 and offs[0] == 0 and lens[0] == S.LONG - 1
        if c.name.startswith("single"):
            assert nl == 0 and (lens.tolist() == [S.SINGLE - 1]) == (c.line0 == 1)
    assert sorted({c.line0 for c in cases}) == [0, 1, 2, 3]
    assert sum(1 for c in cases if not c.data.endswith(b"\n")) == 8


def test_density_census():
    for lay in S.DENSITY_LAYOUTS:
        data = S.density_text(lay)
        c1, c2 = S.tile_counts(data, S.TILE1), S.tile_counts(data, S.TILE2)
        print(f"density {lay}: {len(data)} bytes, newlines per 32-KiB tile {c1.tolist()}")
        print(f"density {lay}: newlines per 16-KiB tile {c2.tolist()}")
        assert set(S.COUNTS) <= set(c1.tolist()), (lay, sorted(set(S.COUNTS) - set(c1.tolist())))
        assert len(data) % S.TILE1 == 0
        if lay != "paired":                                          # an ordinary segment around every dense one
            assert (c1[0::2] <= 700).all() and (c1[0::2] >= 200).all()
        classes = [int((c1 <= S.TILE_CAP).sum()), int(((c1 > S.TILE_CAP) & (c1 <= S.LDS_POS)).sum()), int((c1 > S.LDS_POS).sum())]
        print(f"density {lay}: tiles per class (fixed, staged, direct) {classes}")
        assert min(classes) >= 3
        # lines cross the segment edges: most segments do not end in a newline
        ends = np.frombuffer(data, np.uint8)[S.TILE1 - 1::S.TILE1]
        assert (ends != 10).sum() >= len(ends) // 2
    asc = S.tile_counts(S.density_text("ascending"), S.TILE1)[1::2].tolist()
    shuf = S.tile_counts(S.density_text("shuffled"), S.TILE1)[1::2].tolist()
    assert asc == list(S.COUNTS) and shuf != asc and sorted(shuf) == asc
    # the counts next to the round sizes and the class limits are all there
    for edge in (S.STAGED_ROUND, S.FIXED_ROUND, 2 * S.FIXED_ROUND, S.TILE_CAP, S.TILE_CAP + S.STAGED_ROUND, S.LDS_POS):
        assert {edge - 1, edge, edge + 1} <= set(S.COUNTS), edge
    # max_reads = 1 leaves every shard one tile of single-byte lines (32 768 words): the paired layout needs
    # twice that in one shard, so the call runs full and doubles; the other layouts only repeat with the count
    load = {lay: int(S.shard_load(S.density_text(lay)).max()) for lay in S.DENSITY_LAYOUTS}
    print(f"largest staging need of one shard: {load}")
    assert load["paired"] >= 2 * S.TILE1 and load["ascending"] <= S.TILE1 and load["shuffled"] <= S.TILE1


def test_nul_census():
    clean = S.np_index(S.nul_text(S.NUL_LIST_SCAN)[0].replace(b"\0", b"A"))
    for total in (S.NUL_LIST_SCAN, S.NUL_LIST_SCAN + 1):
        data, put = S.nul_text(total)
        offs, lens, _nl = S.np_index(data)
        nul = np.flatnonzero(np.frombuffer(data, np.uint8) == 0)
        changed = int((lens != clean[1]).sum())
        print(f"nul {total}: {len(data)} bytes, {nul.size} NUL bytes, {S.nul_lines(data)} sequence lines hold one, "
              f"{changed} lengths changed; placed: {put}")
        assert nul.size == total and np.array_equal(offs, clean[0])
        assert set(S.NUL_EDGE_BYTES) <= set(nul.tolist())
        assert {int(p) % S.TILE2 for p in S.NUL_EDGE_BYTES} == {S.TILE2 - 1, 0}
        assert {int(p) % S.TILE1 for p in S.NUL_EDGE_BYTES} >= {S.TILE1 - 1, 0}
        i = int(np.searchsorted(offs, put["first byte"]))
        assert offs[i] == put["first byte"] and lens[i] == S.NONE32 and (lens == S.NONE32).sum() == 1
        i = int(np.searchsorted(offs, put["last byte"], side="right")) - 1
        assert lens[i] == clean[1][i] - 2 == put["last byte"] - offs[i] - 1     # strlen stops there; less one
        i = int(np.searchsorted(offs, put["twice, first"], side="right")) - 1
        assert lens[i] == put["twice, first"] - offs[i] - 1 and put["twice, second"] < offs[i] + clean[1][i]
        assert put["twice, first"] // S.NUL_SUB + 1 == put["twice, second"] // S.NUL_SUB
        assert put["offset 1023"] % S.NUL_SUB == S.NUL_SUB - 1 and put["offset 1024"] % S.NUL_SUB == 0
        for what in ("offset 1023", "offset 1024", "long line, third tile", "open last line"):
            i = int(np.searchsorted(offs, put[what], side="right")) - 1
            assert lens[i] == put[what] - offs[i] - 1 < clean[1][i], what
        i = int(np.argmax(clean[1]))
        assert clean[1][i] == S.LONG - 1 and put["long line, third tile"] // S.TILE1 == offs[i] // S.TILE1 + 2
        assert put["open last line"] >= offs[-1] and not data.endswith(b"\n")
        for kind in (0, 2, 3):                                     # a NUL outside the sequence lines changes no length
            p = put[f"{S.KINDS[kind]} line"]
            assert data[:p].count(b"\n") % 4 == kind
        assert changed == S.nul_lines(data) >= 25
    for n in S.NUL_MANY:
        data = S.nul_many_text(n)
        offs, lens, _nl = S.np_index(data)
        print(f"nul lines {n}: {len(data)} bytes, {data.count(bytes(1))} NUL bytes in {S.nul_lines(data)} of {offs.size} "
              f"sequence lines, {int((lens == S.NONE32).sum())} at the first byte")
        assert data.count(b"\0") == n == S.nul_lines(data) == offs.size
        assert 1_000_000 < len(data) < 2_000_000 and (lens == S.NONE32).sum() > n // 8
    assert S.NUL_MANY == (S.NUL_CAP, S.NUL_CAP + 1)


def test_phase_census():
    calls = S.phase_calls()
    texts = {t for t, _l0, _e in calls}
    print(f"phase: {len(texts)} texts, {len(calls)} calls, {sum(1 for c in calls if not c[2])} of them not at the end")
    assert len(texts) == 255 and len(calls) == 255 * 4 + 128 * 4
    assert {(l0, e) for _t, l0, e in calls} == {(l0, e) for l0 in range(4) for e in (True, False)}


def test_groups_census():
    data = S.groups_text()
    assert len(data) == S.GROUPS_BYTES and not data.endswith(b"\n")
    t1, g1, tot1 = S.groups_census(data, S.TILE1)
    t2, g2, tot2 = S.groups_census(data, S.TILE2)
    c1 = S.tile_counts(data, S.TILE1)
    print(f"groups: {len(data)} bytes; one-pass {t1} tiles in {g1} groups with {tot1} newlines; two-pass {t2} tiles in "
          f"{g2} groups with {tot2}; newlines per one-pass tile {int(c1.min())}..{int(c1.max())}, {np.unique(c1).size} "
          f"distinct values; group_base[1] = {tot1[0]} / {tot2[0]}")
    assert t1 == 1027 >= S.GROUP_TILES + 1 and t2 == 2053 >= 2 * S.GROUP_TILES + 1 and (g1, g2) == (2, 3)
    assert tot1[0] > 0 and tot2[0] > 0 and min(tot1 + tot2) > 0          # group_base[g] for g >= 1 is not zero
    assert len(set(tot2)) == 3 and tot1[0] != tot1[1]
    assert np.unique(c1).size > 100 and c1.max() > S.LDS_POS and c1.min() <= S.TILE_CAP
    cut = S.middle_cut(data)
    assert data[cut - 1:cut] == b"\n" and cut // S.TILE1 in range(400, 600)


def test_dense_file_census():
    data = S.dense_file_text()
    c1 = S.tile_counts(data, S.TILE1)[:len(data) // S.TILE1]
    print(f"dense file: {len(data)} bytes, newlines per whole 32-KiB tile {int(c1.min())}..{int(c1.max())}")
    assert (c1 > S.TILE_CAP).all() and len(data) >= 1 << 20 and data.endswith(b"\n")
    assert set(data) <= set(b"@+ACGTI\n" + S._HDR[:3])


# ---- on the device -------------------------------------------------------------------------------------------

def _gpu_index(B, torch, dev, data, cuts=(), line0=0, at_eof=True, **kw):
    """test_fastq._gpu_index with the first chunk's line number, the newline total and the kernel's own
    types: `data` indexed on the device in chunks ending right after the newlines at `cuts - 1`."""
    bounds = [0] + sorted(cuts) + [len(data)]
    offs_all, lens_all = [], []
    first = line0
    for a, b in zip(bounds[:-1], bounds[1:]):
        chunk = data[a:b]
        buf = torch.tensor(np.frombuffer(chunk, np.uint8) if chunk else np.zeros(0, np.uint8), dtype=torch.uint8, device=dev)
        offs, lens, nl = B.fastq_index(buf, len(chunk), line0=line0, at_eof=(at_eof and b == len(data)), **kw)
        offs_all.append(offs.cpu().numpy().astype(np.uint64) + np.uint64(a))
        lens_all.append(lens.cpu().numpy().astype(np.uint32))
        line0 += nl
    return np.concatenate(offs_all), np.concatenate(lens_all), line0 - first


@pytest.fixture(scope="module")
def dev(gpu):
    import torch
    import shortseq_amd.batch as B
    return B, torch, gpu


@pytest.mark.gpu
@pytest.mark.parametrize("onepass", [True, False])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_whole(dev, family, onepass):
    for c in FAMILIES[family]():
        _same(_gpu_index(*dev, c.data, line0=c.line0, onepass=onepass), S.np_index(c.data, c.line0), (c.name, onepass))


@pytest.mark.gpu
@pytest.mark.parametrize("onepass", [True, False])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_chunked(dev, family, onepass):
    """Cuts right after the last newline before every seam or segment edge; after the first one at or past
    it; and after each of the first eight lines (every line0 at a chunk start)."""
    ran = 0
    for c in FAMILIES[family]():
        if family == "seams" and c.name.startswith("cut"):
            continue
        exp = S.np_index(c.data, c.line0)
        before, after = S.edge_cuts(c.data, S.edges_of(c.data, EDGE_TILE[family]))
        for what, cuts in (("before", before), ("after", after), ("first lines", S.first_line_cuts(c.data))):
            if cuts:
                ran += 1
                _same(_gpu_index(*dev, c.data, cuts, line0=c.line0, onepass=onepass), exp, (c.name, onepass, what, cuts[:4]))
    assert ran >= 6


@pytest.mark.gpu
@pytest.mark.parametrize("onepass", [True, False])
def test_phase(dev, onepass):
    """Every text over {A, newline} of 0 to 7 bytes, every line0, at the end of the file and (where the text
    allows it) not: about 1 500 calls."""
    ref = {}
    for t, l0, at_eof in S.phase_calls():
        exp = ref.get((t, l0)) or ref.setdefault((t, l0), S.np_index(t, l0))
        _same(_gpu_index(*dev, t, line0=l0, at_eof=at_eof, onepass=onepass), exp, (t, l0, at_eof, onepass))


@pytest.mark.gpu
@pytest.mark.parametrize("onepass,chunks", [(True, False), (False, False), (True, True)])
def test_tile_groups(dev, onepass, chunks):
    data = S.groups_text()
    cuts = [S.middle_cut(data)] if chunks else []
    _same(_gpu_index(*dev, data, cuts, onepass=onepass), S.np_index(data), ("groups", onepass, chunks))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", S.DENSITY_LAYOUTS)
def test_density_capacity_retry(dev, layout):
    """A bound of one read (the call is repeated with the count; in the paired layout a shard's staging
    region runs full first and the bound doubles) and the exact count: the same arrays."""
    data = S.density_text(layout)
    exp = S.np_index(data)
    for cap in (1, int(exp[0].size)):
        _same(_gpu_index(*dev, data, max_reads=cap), exp, (layout, cap))


def _items(c):
    return [(type(k).__name__, str(k), len(k), v) for k, v in c.items()]


@pytest.mark.gpu
@pytest.mark.parametrize("text", ["dense file", "seams"])
def test_engine_counts_equal_the_host(gpu, tmp_path, text):
    import shortseq_amd as sq
    data = S.dense_file_text() if text == "dense file" else S.seam_text(0)
    offs, lens, _nl = S.np_index(data)
    buf = np.frombuffer(data, np.uint8).copy()
    for o, n in zip(offs.tolist(), lens.tolist()):                   # (both texts are valid as they are)
        row = buf[o:o + n]
        row[~np.isin(row, np.frombuffer(b"ACGT", np.uint8))] = ord("A")
    assert buf.tobytes() == data
    p = tmp_path / "t.fq"
    p.write_bytes(buf.tobytes())
    h = _items(sq.read_and_count_fastq(str(p), device="host"))
    assert sum(it[3] for it in h) == offs.size
    for chunk in (0, 40_000):
        assert _items(sq.read_and_count_fastq(str(p), device="cuda", _chunk_bytes=chunk)) == h, (text, chunk)
