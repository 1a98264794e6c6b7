"""k_trim_adapter3 where the sweep of trim_cases.py does not reach (inputs: tests/trim_shapes.py): matches
at, across and past the seams of the 256-position windows at every start residue, in waves that mix long,
short and skipped reads; the second and later trips of the grid-stride loop; every compiled (lane group,
staged) shape; the budget multiply at every err_div up to 66 and past it; and the engine with reads of
more than one window.  The expectation is a NumPy statement of the rule (pinned here to the Python one),
for the two 131 k batches the host function with a sample against the rule.  Without a device the file
proves the reference, the generators' non-vacuity conditions and the trip arithmetic."""
import ctypes as C

import numpy as np
import pytest

import trim_cases as T
import trim_shapes as S

REF_COMBOS = ((1, 1, 0), (8, 3, 10), (9, 9, 1), (17, 17, 4), (33, 3, 8), (64, 3, 10), (64, 64, 0))


# ---- without a device --------------------------------------------------------------------------------------

@pytest.mark.parametrize("A,mo,ed", REF_COMBOS)
def test_reference_is_the_python_rule(A, mo, ed):
    rng = np.random.default_rng(100 * A + mo + ed)
    adapter = T.rand_seq(rng, A)
    reads = T.sweep_reads(rng, adapter, mo, ed)
    exp, exp_stats = T.expected(reads, adapter, mo, ed)
    got, stats = S.np_expected(reads, adapter, mo, ed)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (A, mo, ed, reads[int(bad[0])], int(got[bad[0]]), int(exp[bad[0]]))
    assert stats == exp_stats


def test_reference_wildcards_and_large_err_div():
    rng = np.random.default_rng(77)
    for A in (3, 17, 64):
        for adapter in T.wildcard_adapters(rng, A):
            reads = T.wildcard_reads(rng, adapter)
            for mo, ed in ((1, 0), (3, 10), (A, 4), (1, 65), (1, 0xFFFFFFFF)):
                assert np.array_equal(S.np_expected(reads, adapter, mo, ed)[0], T.expected(reads, adapter, mo, ed)[0])


def test_layout_at_places_every_read():
    rng = np.random.default_rng(5)
    reads = [T.rand_seq(rng, int(n)) for n in rng.integers(0, 70, 200)]
    reads[17] = (1025, None)
    residues = rng.integers(0, 16, len(reads))
    blob, offs, lens = S.layout_at(reads, residues)
    for r, res, o, n in zip(reads, residues, offs, lens):
        if isinstance(r, tuple):
            assert int(n) == r[0] and int(o) < blob.size
        else:
            assert int(o) % 16 == res and blob[int(o):int(o) + int(n)].tobytes() == r
    assert S.blob_reads(blob, offs, lens) == reads


@pytest.mark.parametrize("A,which", S.SEAM_BATCHES)
def test_seam_batches_reach_the_seams(A, which):
    b = S.seam_batch(A, which)
    planted = [(ci, p) for ci, (_r, kind, p) in enumerate(b.cases) if kind != "plain"]
    found = sum(1 for ci, p in planted if b.case_answer[ci] == p)
    print(f"{b.name}: cases {len(b.cases)} reads {len(b.reads)} blob {b.blob.size} planted {len(planted)} found {found}")
    assert found >= 0.95 * len(planted)
    answers = {b.case_answer[ci] for ci, _p in planted}
    for s in S.SEAMS:
        # the window's last position, the next one's first, a match that straddles the seam from as far
        # left as the adapter reaches, and one only the next window holds
        assert {s - A + 1, s - 1, s, s + 1} <= answers, (s, sorted(answers))
    for w in (1, 2, 3):
        assert any(w * S.KWIN <= a < (w + 1) * S.KWIN for a in answers)
    if b.err_div == 0:
        for ci, (r, kind, p) in enumerate(b.cases):
            if kind == "plain":
                assert b.case_answer[ci] == len(r)
            if kind == "nearmiss":          # not the near miss at the window's last position: the next window's
                assert b.case_answer[ci] == p and p // S.KWIN == (p - A - 3) // S.KWIN + 1
        assert sum(1 for c in b.cases if c[1] == "nearmiss") >= 6
    # a last window of one position: pmax = L - min_overlap at 256, 512 and 768
    assert {s + b.min_overlap for s in S.SEAMS} <= {len(c[0]) for c in b.cases}
    # every case at every residue, and no wave of the library shape (16 reads) with long reads only
    assert all(int(o) % 16 == res for o, res, ci in zip(b.offs, b.residues, b.case_of) if ci >= 0)
    seen = {(int(ci), int(res)) for ci, res in zip(b.case_of, b.residues) if ci >= 0}
    assert len(seen) == 16 * len(b.cases)
    per_wave = 64 // S.LIB_GROUP
    assert len(b.reads) % per_wave == 0
    kinds = set()
    for w0 in range(0, len(b.reads), per_wave):
        fill = [b.filler_kind[k] for k in range(w0, w0 + per_wave) if b.case_of[k] < 0]
        assert fill and len(fill) < per_wave
        kinds |= set(fill)
    assert kinds == {1025, 0xFFFFFFFF, "short", "library"}


def test_trip_arithmetic():
    assert S.trips(131072, S.LIB_GROUP) == (131072, 1)
    assert S.trips(S.LIB_TRIP_N, S.LIB_GROUP) == (131072, 2)
    assert [S.trips(n, 32) for n in S.G32_TRIP_NS] == [(16384, 1), (16384, 2), (16384, 4)]
    # the largest batch of test_trim_gpu.py stays inside one trip
    assert S.trips(100_000, S.LIB_GROUP)[1] == 1


def test_trip_batches_differ_between_trips():
    import shortseq_amd.batch as B
    for n, group in ((S.LIB_TRIP_N, S.LIB_GROUP),) + tuple((n, 32) for n in S.G32_TRIP_NS[1:]):
        per_trip, iters = S.trips(n, group)
        blob, offs, lens = S.trip_batch(n, per_trip)
        assert int(offs[-1] + lens[-1]) < blob.size and lens.size == n
        h, st = B.host_trim_adapter(blob, offs, lens, S.A21, stats=True)
        assert int(st[0]) > 0.95 * n
        for t in range(1, iters):           # another read, and another answer, than one trip earlier
            a, b = h[t * per_trip:(t + 1) * per_trip], h[(t - 1) * per_trip:]
            assert (a != b[:a.size]).all()
        idx, exp = S.trip_reference(n, per_trip, sample=True)
        assert idx.size >= 2000
        for t0 in range(0, n, per_trip):
            t1 = min(n, t0 + per_trip)
            assert set(range(t0, min(t1, t0 + 64))) | set(range(max(t0, t1 - 64), t1)) <= set(idx.tolist())
        assert np.array_equal(h[idx], exp)


def test_budget_cases_sit_at_the_budget():
    assert len(S.BUDGET_ERR_DIVS) == 70
    worst = (2.0, -1)
    for ed in S.BUDGET_ERR_DIVS:
        reads, at_budget, _blob, _offs, lens, exp, _st = S.budget_case(ed)
        assert len(reads) == 128
        hit = (exp[at_budget] == 11).mean()
        worst = min(worst, (hit, ed))
        assert hit >= 0.75, (ed, hit)
        assert (exp[~at_budget] != 11).all(), ed
    print(f"at-budget reads answered at the planted position: worst {worst[0]:.3f} at err_div {worst[1]}")
    # past 64 the budget is 0 at every overlap: the at-budget reads are exact occurrences
    for ed in (65, 66, 100, 1 << 16, (1 << 24) + 1, 0xFFFFFFFF):
        reads, _at, _blob, _offs, _lens, exp, _st = S.budget_case(ed)
        assert np.array_equal(S.np_expected(reads, S.budget_adapter(), 1, 0)[0], exp)


def test_engine_reads_trim_past_the_first_window():
    reads, is_long = S.engine_reads()
    exp, _ = S.np_expected(reads, S.A21, 3, 10)
    full = np.array([len(r) for r in reads])
    assert len(reads) == 2000 and is_long.sum() == 1000
    cut = exp[is_long]
    assert (cut < full[is_long]).sum() >= 500
    assert ((cut >= S.KWIN) & (cut < 3 * S.KWIN)).sum() >= 500
    assert (full[~is_long] <= 60).all()


# ---- on the device -------------------------------------------------------------------------------------------

def _dev(gpu, blob, offs, lens, shift=0):
    """The batch on the device; shift > 0: the blob as a view `shift` bytes into a larger allocation."""
    import torch
    if shift:
        buf = torch.full((blob.size + shift + 16,), ord("#"), dtype=torch.uint8, device=gpu)
        buf[shift:shift + blob.size] = torch.from_numpy(blob).to(gpu)
        b = buf[shift:shift + blob.size]
        assert b.data_ptr() % 16 == shift % 16 and shift % 16
    else:
        b = torch.from_numpy(blob if blob.size else np.zeros(16, np.uint8)).to(gpu)
    return b, torch.from_numpy(offs.view(np.int64)).to(gpu), torch.from_numpy(lens.view(np.int32)).to(gpu)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(out, st, exp, stats, lens, what):
    g = _u32(out)
    bad = np.flatnonzero(g != exp)
    assert bad.size == 0, (what, f"{bad.size} of {g.size} lengths differ; read {int(bad[0])} of length "
                                 f"{int(lens[bad[0]])}: {int(g[bad[0]])}, expected {int(exp[bad[0]])}")
    if st is not None:
        assert [int(x) for x in st.cpu()] == [int(x) for x in stats], what


def _shape_call(gpu, b, o, ln, adapter, mo, ed, out, st, group, staged, n=None):
    import torch
    from shortseq_amd._native import lib
    ad = (C.c_uint8 * 64)(*adapter)
    return lib().ss_trim_adapter3_shape(b.data_ptr(), b.numel(), o.data_ptr(), ln.data_ptr(), ln.numel() if n is None else n,
                                        ad, len(adapter), mo, ed, out.data_ptr(), None if st is None else st.data_ptr(),
                                        0, group, staged, torch.cuda.current_stream(gpu).cuda_stream)


@pytest.mark.gpu
@pytest.mark.parametrize("A,which", S.SEAM_BATCHES)
def test_seams_library_shape(gpu, A, which):
    import torch
    import shortseq_amd.batch as B
    s = S.seam_batch(A, which)
    b, o, ln = _dev(gpu, s.blob, s.offs, s.lens)
    out = torch.full_like(ln, S.PREFILL)
    got, st = B.trim_adapter(b, o, ln, s.adapter, min_overlap=s.min_overlap, err_div=s.err_div, out=out, stats=True)
    _same(got, st, s.exp, s.stats, s.lens, s.name)
    assert np.array_equal(_u32(ln), s.lens)


@pytest.mark.gpu
def test_seams_blob_base_not_aligned(gpu):
    """The same offsets over a blob whose base pointer is 5 past a 16-byte boundary: the chunk residue comes
    from the address."""
    import torch
    import shortseq_amd.batch as B
    s = S.seam_batch(64, 0)
    b, o, ln = _dev(gpu, s.blob, s.offs, s.lens, shift=5)
    out = torch.full_like(ln, S.PREFILL)
    got, st = B.trim_adapter(b, o, ln, s.adapter, min_overlap=s.min_overlap, err_div=s.err_div, out=out, stats=True)
    _same(got, st, s.exp, s.stats, s.lens, s.name + " base + 5")


@pytest.fixture(scope="module")
def shape_dev(gpu):
    return [(name, adapter, mo, ed, _dev(gpu, blob, offs, lens), lens, exp, st)
            for name, adapter, mo, ed, blob, offs, lens, exp, st in S.shape_inputs()]


@pytest.mark.gpu
@pytest.mark.parametrize("group,staged", S.SHAPES)
def test_every_compiled_shape(gpu, shape_dev, group, staged):
    import torch
    from shortseq_amd._native import SS_OK
    for name, adapter, mo, ed, (b, o, ln), lens, exp, stats in shape_dev:
        out = torch.full_like(ln, S.PREFILL)
        st = torch.full((2,), 7, dtype=torch.int64, device=gpu)
        assert _shape_call(gpu, b, o, ln, adapter, mo, ed, out, st, group, staged) == SS_OK
        _same(out, st, exp, stats, lens, (name, group, staged))


@pytest.mark.gpu
def test_shape_entry_refuses_other_groups_and_defaults_to_the_library(gpu, shape_dev):
    import torch
    import shortseq_amd.batch as B
    from shortseq_amd._native import SS_EARG, SS_OK
    name, adapter, mo, ed, (b, o, ln), lens, exp, stats = shape_dev[0]
    out = torch.full_like(ln, S.PREFILL)
    st = torch.full((2,), 7, dtype=torch.int64, device=gpu)
    for group in (1, 3, 64):
        for staged in (1, 0, -1):
            assert _shape_call(gpu, b, o, ln, adapter, mo, ed, out, st, group, staged) == SS_EARG
    torch.cuda.synchronize(gpu)
    assert (_u32(out) == S.PREFILL).all() and [int(x) for x in st.cpu()] == [7, 7]
    assert _shape_call(gpu, b, o, ln, adapter, mo, ed, out, st, 0, -1) == SS_OK
    lib_out, lib_st = B.trim_adapter(b, o, ln, adapter, min_overlap=mo, err_div=ed, stats=True)
    assert torch.equal(out, lib_out) and torch.equal(st, lib_st)
    _same(out, st, exp, stats, lens, name)


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", (False, True))
def test_trips_library_shape(gpu, inplace):
    import torch
    import shortseq_amd.batch as B
    n = S.LIB_TRIP_N
    per_trip, iters = S.trips(n, S.LIB_GROUP)
    assert iters == 2
    blob, offs, lens = S.trip_batch(n, per_trip)
    h, hst = B.host_trim_adapter(blob, offs, lens, S.A21, stats=True)
    b, o, ln = _dev(gpu, blob, offs, lens)
    out = ln if inplace else torch.full_like(ln, S.PREFILL)
    got, st = B.trim_adapter(b, o, ln, S.A21, out=out, stats=True)
    assert got is out
    _same(got, st, h, hst, lens, ("library shape", n, inplace))
    idx, exp = S.trip_reference(n, per_trip, sample=True)
    assert np.array_equal(_u32(got)[idx], exp)
    if not inplace:
        assert np.array_equal(_u32(ln), lens)


@pytest.mark.gpu
@pytest.mark.parametrize("staged", (1, 0))
@pytest.mark.parametrize("n", S.G32_TRIP_NS)
def test_trips_group_32(gpu, n, staged):
    import torch
    from shortseq_amd._native import SS_OK
    per_trip, iters = S.trips(n, 32)
    assert iters == {16384: 1, 16385: 2, 49153: 4}[n]
    blob, offs, lens = S.trip_batch(n, per_trip)
    _idx, exp = S.trip_reference(n, per_trip, sample=False)
    full = lens.astype(np.int64)
    stats = [int((exp < full).sum()), int((full - exp).sum())]
    b, o, ln = _dev(gpu, blob, offs, lens)
    out = torch.full_like(ln, S.PREFILL)
    st = torch.full((2,), 7, dtype=torch.int64, device=gpu)
    assert _shape_call(gpu, b, o, ln, S.A21, 3, 10, out, st, 32, staged) == SS_OK
    _same(out, st, exp, stats, lens, ("group 32", n, staged))


@pytest.mark.gpu
@pytest.mark.parametrize("err_div", S.BUDGET_ERR_DIVS)
def test_budget_multiply(gpu, err_div):
    import torch
    import shortseq_amd.batch as B
    _reads, _at, blob, offs, lens, exp, stats = S.budget_case(err_div)
    b, o, ln = _dev(gpu, blob, offs, lens)
    out = torch.full_like(ln, S.PREFILL)
    got, st = B.trim_adapter(b, o, ln, S.budget_adapter(), min_overlap=1, err_div=err_div, out=out, stats=True)
    _same(got, st, exp, stats, lens, ("err_div", err_div))


def _rows_of(counter):
    """A ShortSeqCounter's dict as the ss_ingest_results layout (lens, counts, words)."""
    lens, cnts, words = [], [], []
    for k, v in counter.items():
        lens.append(len(k))
        cnts.append(v)
        words.extend(int(w) for w in k.packed[:max(0, (len(k) + 31) // 32)])
    return np.array(lens, np.uint32), np.array(cnts, np.uint64), np.array(words, np.uint64)


@pytest.mark.gpu
def test_device_ingest_reads_past_one_window(gpu):
    import shortseq_amd as sq
    import shortseq_amd.batch as B
    reads, is_long = S.engine_reads()
    exp, _ = S.np_expected(reads, S.A21, 3, 10)
    full = np.array([len(r) for r in reads])
    assert (exp[is_long] < full[is_long]).sum() >= is_long.sum() // 2
    trimmed = [r[:k] for r, k in zip(reads, exp)]
    blob, offs, lens = T.layout(np.random.default_rng(3), reads, "junk")
    eng = B.DeviceIngest(gpu, adapter=S.A21)
    try:
        b, o, ln = _dev(gpu, blob, offs, lens)
        eng.count(b, o, ln)
        assert np.array_equal(_u32(ln), lens)
        gl, gc, gw = eng.results()
    finally:
        eng.close()
    el, ec, ew = _rows_of(sq.ShortSeqCounter(trimmed, device="host"))
    assert gl.tolist() == el.tolist()
    assert gc.tolist() == ec.tolist()
    assert np.array_equal(gw, ew)
    assert int(ec.sum()) == len(reads) and (el > 256).sum() >= 50
