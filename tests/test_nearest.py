"""Nearest-reference hamming match (ss_hamming_nearest / _ex, ss_host_hamming_nearest,
batch.hamming_nearest, barcode.correct): every query against a second set of rows.

Expected values come from a brute force written here on the ASCII strings (sum(a != b) per position,
then min, lowest argmin and tie count in numpy); the cases that set the alias bit at position L take
their distances from oracle.hamming_pair_batch.  Every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

SS_EARG = -1
NONE = 0xFFFFFFFF
FILL = 0xDEADBEEF
GUARD = 8
U32_MAX = (1 << 32) - 1


def _W(L):
    return 1 if L <= 32 else (L + 31) // 32


def _P(L):
    """Compared positions: min(L + 1, 32 W)."""
    return min(L + 1, 32 * _W(L))


def _row_tile(L):
    """Query rows per block, as include/shortseq_amd.h documents it."""
    if L > 128:
        return 256
    p = _P(L)
    return 1024 if p <= 16 else (512 if p <= 24 else (256 if p <= 32 else 128))


ACGT = np.frombuffer(b"ACGT", np.uint8)


def _ascii(rng, n, L):
    return ACGT[rng.integers(0, 4, size=(n, L))]


def _mutate(rng, rows, nsub):
    """rows with nsub[i] positions of row i replaced by another base."""
    out = rows.copy()
    L = rows.shape[1]
    for i, k in enumerate(nsub):
        for p in rng.choice(L, size=min(int(k), L), replace=False):
            out[i, p] = ACGT[(int(np.flatnonzero(ACGT == out[i, p])[0]) + int(rng.integers(1, 4))) % 4]
    return out


def _queries_near(rng, refs, nq, L):
    """nq queries: a random reference with 0, 1, 2 substitutions in turn (random rows when there is none)."""
    if refs.shape[0] == 0:
        return _ascii(rng, nq, L)
    return _mutate(rng, refs[rng.integers(0, refs.shape[0], size=nq)], np.arange(nq) % 3)


def _dmatrix(qa, ra):
    """[nq, nr] distances from the ASCII rows, position by position."""
    D = np.zeros((qa.shape[0], ra.shape[0]), dtype=np.int32)
    step = max(1, (1 << 24) // max(1, ra.shape[0] * max(1, ra.shape[1])))
    for i in range(0, qa.shape[0], step):
        D[i:i + step] = (qa[i:i + step, None, :] != ra[None, :, :]).sum(axis=2)
    return D


def _from_dmatrix(D, max_dist):
    """-> (idx, dist, nbest) int64: min, lowest argmin, tie count; -1 / -1 / 0 where the min > max_dist."""
    nq, nr = D.shape
    if nr == 0:
        return np.full(nq, -1, np.int64), np.full(nq, -1, np.int64), np.zeros(nq, np.int64)
    dmin = D.min(axis=1).astype(np.int64)
    idx = D.argmin(axis=1).astype(np.int64)                 # numpy's argmin is the first (lowest) index
    nbest = (D == dmin[:, None]).sum(axis=1).astype(np.int64)
    ok = dmin <= max_dist
    return np.where(ok, idx, -1), np.where(ok, dmin, -1), np.where(ok, nbest, 0)


def _brute(qa, ra, max_dist):
    return _from_dmatrix(_dmatrix(qa, ra), max_dist)


def _encode(oracle, a, L):
    n = a.shape[0]
    if n == 0:
        return np.zeros((0, _W(L)), dtype=np.uint64)
    words, rc, _ = oracle.encode_batch(np.ascontiguousarray(a).reshape(-1), n, L)
    assert rc == 0
    return words.reshape(n, _W(L))


def _pad(rng, words, wpr):
    """The rows at stride wpr, the padding words random bits."""
    n, W = words.shape
    out = rng.integers(0, 1 << 63, size=(n, wpr), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, wpr), dtype=np.uint64)
    out[:, :W] = words
    return np.ascontiguousarray(out)


def _signed(u):
    """u32 outputs -> int64 with SS_NEAREST_NONE as -1."""
    v = u.astype(np.int64)
    return np.where(v == NONE, -1, v)


def _host(q, r, L, max_dist, *, nbest=True, nq=None, nr=None, q_wpr=None, r_wpr=None, null=()):
    """ss_host_hamming_nearest -> (rc, idx, dist, nbest) with raw u32 outputs pre-filled with FILL."""
    from shortseq_amd._native import lib
    nq = q.shape[0] if nq is None else nq
    nr = r.shape[0] if nr is None else nr
    idx = np.full(max(1, q.shape[0]), FILL, dtype=np.uint32)
    dist = np.full(max(1, q.shape[0]), FILL, dtype=np.uint32)
    nb = np.full(max(1, q.shape[0]), FILL, dtype=np.uint32)
    p = lambda name, a: None if name in null else a.ctypes.data      # noqa: E731
    rc = lib().ss_host_hamming_nearest(p("q", q), nq, q.shape[1] if q_wpr is None else q_wpr, p("r", r), nr,
                                       r.shape[1] if r_wpr is None else r_wpr, L, max_dist, p("idx", idx),
                                       p("dist", dist), nb.ctypes.data if nbest else None)
    return rc, idx[:q.shape[0]], dist[:q.shape[0]], nb[:q.shape[0]]


def _host_ok(q, r, L, max_dist):
    rc, idx, dist, nb = _host(q, r, L, max_dist)
    assert rc == 0
    return _signed(idx), _signed(dist), nb.astype(np.int64)


def _same(got, exp, what):
    for g, e, name in zip(got, exp, ("idx", "dist", "nbest")):
        assert np.array_equal(g, e), (what, name, np.flatnonzero(g != e)[:8], g[g != e][:8], e[g != e][:8])


# --------------------------------------------------------------------------------------------------
# CPU: ss_host_hamming_nearest
HOST_L = (1, 7, 8, 12, 16, 31, 32, 33, 64, 96, 128, 129, 200, 1024)


@pytest.mark.parametrize("L", HOST_L)
def test_host_matches_brute_force(oracle, L):
    rng = np.random.default_rng(100 + L)
    for nr in (0, 1, 33):
        ra = _ascii(rng, nr, L)
        r = _encode(oracle, ra, L)
        for nq in (0, 1, 33):
            qa = _queries_near(rng, ra, nq, L)
            q = _encode(oracle, qa, L)
            D = _dmatrix(qa, ra)
            for max_dist in (0, 1, 3, _P(L), U32_MAX):
                _same(_host_ok(q, r, L, max_dist), _from_dmatrix(D, max_dist), (L, nq, nr, max_dist))


def test_host_duplicates_ties_and_substitutions(oracle):
    rng = np.random.default_rng(7)
    L, nr = 16, 33
    ra = _ascii(rng, nr, L)
    ra[nr - 1] = ra[0]                                       # the whitelist names one barcode twice
    r = _encode(oracle, ra, L)
    qa = _mutate(rng, np.repeat(ra[:1], 3, axis=0), [0, 1, 2])
    q = _encode(oracle, qa, L)
    idx, dist, nb = _host_ok(q, r, L, 2)
    assert idx.tolist() == [0, 0, 0] and dist.tolist() == [0, 1, 2] and nb.tolist() == [2, 2, 2]
    _same((idx, dist, nb), _brute(qa, ra, 2), "duplicate")
    idx, dist, nb = _host_ok(q, r, L, 1)
    assert idx.tolist() == [0, 0, -1] and dist.tolist() == [0, 1, -1] and nb.tolist() == [2, 2, 0]
    # a query equidistant from two entries: s with position 3 changed lies 1 from s and 1 from s'
    # (s with positions 3 and 9 changed, position 3 to the query's base)
    s = _ascii(rng, 1, L)
    query = _mutate(rng, s, [0])
    query[0, 3] = ACGT[(int(np.flatnonzero(ACGT == s[0, 3])[0]) + 1) % 4]
    other = query.copy()
    other[0, 9] = ACGT[(int(np.flatnonzero(ACGT == s[0, 9])[0]) + 2) % 4]
    far = _mutate(rng, s, [8])
    ra2 = np.concatenate([far, s, other])
    exp = _brute(query, ra2, 1)
    assert (exp[0].tolist(), exp[1].tolist(), exp[2].tolist()) == ([1], [1], [2])
    _same(_host_ok(_encode(oracle, query, L), _encode(oracle, ra2, L), L, 1), exp, "equidistant")
    _same(_host_ok(_encode(oracle, query, L), _encode(oracle, ra2, L), L, 0), _brute(query, ra2, 0), "equidistant k=0")


@pytest.mark.parametrize("L", [12, 40, 200])
def test_host_strides_and_padding_garbage(oracle, L):
    rng = np.random.default_rng(300 + L)
    ra = _ascii(rng, 33, L)
    qa = _queries_near(rng, ra, 20, L)
    exp = _brute(qa, ra, 2)
    q, r = _encode(oracle, qa, L), _encode(oracle, ra, L)
    W = _W(L)
    _same(_host_ok(_pad(rng, q, W + 1), _pad(rng, r, W + 3), L, 2), exp, "q W+1, r W+3")
    _same(_host_ok(_pad(rng, q, W + 2), _pad(rng, r, W + 1), L, 2), exp, "q W+2, r W+1")
    rc, _i, _d, nb = _host(q, r, L, 2, nbest=False)           # h_nbest = NULL
    assert rc == 0 and (nb == FILL).all()


def test_host_alias_bit(oracle):
    """Position L of a one-word row (the table-path alias bit) counts: distances from the oracle."""
    rng = np.random.default_rng(11)
    for L in (7, 12, 31):
        q, r, D = _alias_case(oracle, rng, L, 20, 33)
        for k in (0, 1, 2):
            _same(_host_ok(q, r, L, k), _from_dmatrix(D, k), ("alias", L, k))


def _alias_case(oracle, rng, L, nq, nr):
    """Queries near the references, the alias bit (bit 2 L) set on a third of the queries and on another
    third of the references -> (q words, r words, the oracle's [nq, nr] distances)."""
    ra = _ascii(rng, nr, L)
    qa = _queries_near(rng, ra, nq, L)
    q, r = _encode(oracle, qa, L), _encode(oracle, ra, L)
    q[0::3, 0] |= np.uint64(1 << (2 * L))
    r[1::3, 0] |= np.uint64(1 << (2 * L))
    a = np.repeat(q, nr, axis=0)
    b = np.tile(r, (nq, 1))
    D = oracle.hamming_pair_batch(a, b, nq * nr, L).astype(np.int32).reshape(nq, nr)
    plain = _dmatrix(qa, ra)
    assert (D != plain).any() and (D >= plain).all() and (D - plain).max() == 1     # the bit is seen, once
    return q, r, D


def test_host_argument_errors(oracle):
    rng = np.random.default_rng(5)
    L = 40
    qa, ra = _ascii(rng, 5, L), _ascii(rng, 9, L)
    q, r = _encode(oracle, qa, L), _encode(oracle, ra, L)
    cases = {
        "null q": dict(null=("q",)), "null ref": dict(null=("r",)), "null idx": dict(null=("idx",)),
        "null dist": dict(null=("dist",)), "L = 0": dict(L=0), "L = 1025": dict(L=1025),
        "q_wpr < W": dict(q_wpr=1), "r_wpr < W": dict(r_wpr=1), "nq = 2^32": dict(nq=1 << 32), "nr = 2^32": dict(nr=1 << 32),
    }
    for name, kw in cases.items():
        rc, idx, dist, nb = _host(q, r, kw.pop("L", L), 1, **kw)
        assert rc == SS_EARG, name
        assert (idx == FILL).all() and (dist == FILL).all() and (nb == FILL).all(), name
    rc, idx, dist, nb = _host(q, r, L, 1)
    assert rc == 0 and not (idx == FILL).any()
    from shortseq_amd._native import lib
    assert lib().ss_host_hamming_nearest(None, 0, 2, None, 0, 2, L, 1, None, None, None) == 0     # nq = 0: a no-op
    assert lib().ss_hamming_nearest_ws_bytes(40, 4099, 16, 1) == 0
    assert lib().ss_hamming_nearest_ws_bytes(40, 4099, 16, 3) == 3 * 40 * 12


# --------------------------------------------------------------------------------------------------
# CPU: barcode.correct
def _barcode_case(seed, nkeys, L=16, nwl=24):
    """-> (counter dict ShortSeq -> count, whitelist strings, key strings): keys are whitelist entries
    with 0 .. 2 substitutions, keys of two other lengths mixed in; entries 0 and 1 differ in two
    positions, so the key between them is ambiguous."""
    import shortseq_amd as ssa
    rng = np.random.default_rng(seed)
    wl = _ascii(rng, nwl, L)
    wl[1] = wl[0]
    wl[1, 2] = ACGT[(int(np.flatnonzero(ACGT == wl[0, 2])[0]) + 1) % 4]
    wl[1, 11] = ACGT[(int(np.flatnonzero(ACGT == wl[0, 11])[0]) + 1) % 4]
    between = wl[0].copy()
    between[2] = wl[1, 2]
    keys = {between.tobytes().decode(): 5}
    while len(keys) < nkeys:
        u = rng.random()
        if u < 0.1:
            s = _ascii(rng, 1, L - 3 if u < 0.05 else L + 20)[0]
        else:
            s = _mutate(rng, wl[rng.integers(0, nwl, size=1)], [int(rng.integers(0, 3))])[0]
        keys.setdefault(s.tobytes().decode(), int(rng.integers(1, 50)))
    wl_s = [w.tobytes().decode() for w in wl]
    assert len(set(wl_s)) == nwl
    return {ssa.from_str(s): c for s, c in keys.items()}, wl_s, list(keys)


def _correct_reference(key_strs, counts, wl, max_dist, ambiguous):
    assign, totals = [], [0] * len(wl)
    for s, c in zip(key_strs, counts):
        j = None
        if len(s) == len(wl[0]):
            d = [sum(x != y for x, y in zip(s, w)) for w in wl]
            m = min(d)
            if m <= max_dist and (d.count(m) == 1 or ambiguous == "first"):
                j = d.index(m)
        assign.append(None if j is None else wl[j])
        if j is not None:
            totals[j] += c
    return assign, [(w, t) for w, t in zip(wl, totals) if t]


def _check_correct(counter, wl, key_strs, max_dist, ambiguous, device, wl_arg=None):
    import shortseq_amd.barcode as BC
    corrected, assign = BC.correct(counter, wl if wl_arg is None else wl_arg, max_dist, ambiguous=ambiguous, device=device)
    exp_assign, exp_corr = _correct_reference(key_strs, list(counter.values()), wl, max_dist, ambiguous)
    assert [str(k) for k in assign] == key_strs                                      # counter's order
    assert [None if v is None else str(v) for v in assign.values()] == exp_assign
    assert [(str(k), v) for k, v in corrected.items()] == exp_corr                   # whitelist order
    return corrected, assign


def test_correct_host():
    import shortseq_amd as ssa
    import shortseq_amd.barcode as BC
    counter, wl, key_strs = _barcode_case(1, 400)
    for max_dist in (0, 1, 2):
        for amb in ("drop", "first"):
            _check_correct(counter, wl, key_strs, max_dist, amb, "host")
    drop = BC.correct(counter, wl, 1, ambiguous="drop", device="host")[1]
    first = BC.correct(counter, wl, 1, ambiguous="first", device="host")[1]
    between = ssa.from_str(key_strs[0])
    assert drop[between] is None and str(first[between]) == wl[0]
    assert any(v is None for k, v in drop.items() if len(k) != 16) and all(drop[k] is None for k in drop if len(k) != 16)
    # whitelist given as bytes / ShortSeq objects: the same
    _check_correct(counter, wl, key_strs, 1, "drop", "host", wl_arg=[w.encode() for w in wl])
    _check_correct(counter, wl, key_strs, 1, "drop", "host", wl_arg=[ssa.from_str(w) for w in wl])
    with pytest.raises(ValueError):
        BC.correct(counter, wl + [wl[3]], device="host")                   # a duplicated entry
    with pytest.raises(ValueError):
        BC.correct(counter, wl + ["ACGT"], device="host")                  # mixed lengths
    assert BC.correct({}, wl, device="host") == ({}, {})
    corrected, assign = BC.correct(counter, [], device="host")
    assert corrected == {} and list(assign.values()) == [None] * len(counter)


# --------------------------------------------------------------------------------------------------
# GPU
def _dev_rows(gpu, rows):
    """rows [n, wpr] on the device at a base that is 8-byte but not 16-byte aligned."""
    import torch
    n, wpr = rows.shape
    buf = torch.zeros(n * wpr + 3, dtype=torch.int64, device=gpu)
    lead = 1 if buf.data_ptr() % 16 == 0 else 2
    t = buf[lead:lead + n * wpr]
    assert n == 0 or t.data_ptr() % 16 == 8
    if n:
        t.copy_(torch.from_numpy(rows.view(np.int64).reshape(-1)).to(gpu))
    return t                                               # (keeps buf alive)


def _gpu_call(gpu, q, r, L, max_dist, *, splits=None, nbest=True, short_ws=0):
    """ss_hamming_nearest (splits None) or _ex through ctypes, the outputs inside larger tensors whose
    guard elements must stay unchanged -> the status when nonzero, else (idx, dist, nbest | None)."""
    import torch
    from shortseq_amd._native import lib
    nq, nr = q.shape[0], r.shape[0]
    dq, dr = _dev_rows(gpu, q), _dev_rows(gpu, r)
    ws_bytes = int(lib().ss_hamming_nearest_ws_bytes(nq, nr, L, 0 if splits is None else splits))
    ws = torch.empty(ws_bytes // 4 + 2, dtype=torch.int32, device=gpu)
    outs = [torch.full((nq + 2 * GUARD,), -7, dtype=torch.int32, device=gpu) for _ in range(3)]
    ptr = [t[GUARD:].data_ptr() for t in outs]
    s = torch.cuda.current_stream(gpu).cuda_stream
    args = (dq.data_ptr(), nq, q.shape[1], dr.data_ptr(), nr, r.shape[1], L, max_dist, ptr[0], ptr[1],
            ptr[2] if nbest else None, ws.data_ptr(), ws_bytes - short_ws)
    rc = lib().ss_hamming_nearest(*args, s) if splits is None else lib().ss_hamming_nearest_ex(*args, splits, s)
    torch.cuda.synchronize(gpu)
    for t in outs:
        assert bool((t[:GUARD] == -7).all()) and bool((t[GUARD + nq:] == -7).all()), "a guard element was written"
    if rc:
        assert all(bool((t == -7).all()) for t in outs), "outputs written by a refused call"
        return rc
    if not nbest:
        assert bool((outs[2] == -7).all())
    got = [t[GUARD:GUARD + nq].cpu().numpy().view(np.uint32) for t in outs]
    return _signed(got[0]), _signed(got[1]), got[2].astype(np.int64) if nbest else None


GEOM_NR = (1, 31, 33, 1023, 1025, 4099)


@pytest.fixture(scope="module")
def geometry(oracle):
    """L -> (q words, r words, distance matrix) for 2 S + 5 queries and 4099 references, computed once."""
    cache = {}

    def get(L):
        if L not in cache:
            rng = np.random.default_rng(900 + L)
            S = _row_tile(L)
            ra = _ascii(rng, GEOM_NR[-1], L)
            # queries near references of every prefix of the set (so small nr see hits too), 0 - 2 errors
            nq = 2 * S + 5
            src = ra[rng.integers(0, np.asarray(GEOM_NR)[rng.integers(0, len(GEOM_NR), size=nq)])]
            qa = _mutate(rng, src, np.arange(nq) % 3)
            cache[L] = (_encode(oracle, qa, L), _encode(oracle, ra, L), _dmatrix(qa, ra))
        return cache[L]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("L", [12, 20, 32, 64, 200])
def test_gpu_geometry(gpu, geometry, L):
    """nq around the row tile S (1024, 512, 256, 128; 256 for the VALU form), nr across the 32-column
    block, one LDS stage and several; q_wpr / r_wpr W or W + 1 in turn, bases 8-B but not 16-B aligned,
    random padding words."""
    q, r, D = geometry(L)
    S, W = _row_tile(L), _W(L)
    rng = np.random.default_rng(L)
    case = 0
    for nq in (1, 31, 33, S - 1, S + 1, 2 * S + 5):
        for nr in GEOM_NR:
            qp = _pad(rng, q[:nq], W + (case & 1))
            rp = _pad(rng, r[:nr], W + ((case >> 1) & 1))
            case += 1
            _same(_gpu_call(gpu, qp, rp, L, 1), _from_dmatrix(D[:nq, :nr], 1), (L, nq, nr))
    assert case == 36


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 7, 8, 9, 12, 16, 31, 32, 33, 64, 96, 128, 129, 200])
def test_gpu_lengths_and_layouts(gpu, oracle, L):
    """Every KS boundary of one word, W = 2 .. 4, the VALU form; all four stride combinations."""
    rng = np.random.default_rng(500 + L)
    W = _W(L)
    ra = _ascii(rng, 100, L)
    qa = _queries_near(rng, ra, 70, L)
    q, r, D = _encode(oracle, qa, L), _encode(oracle, ra, L), _dmatrix(qa, ra)
    for dq in (0, 1):
        for dr in (0, 1):
            qp, rp = _pad(rng, q, W + dq), _pad(rng, r, W + dr)
            for max_dist in (0, 1, 2, _P(L), U32_MAX):
                exp = _from_dmatrix(D, max_dist)
                _same(_gpu_call(gpu, qp, rp, L, max_dist), exp, (L, dq, dr, max_dist))
                _same(_host_ok(qp, rp, L, max_dist), exp, (L, dq, dr, max_dist, "host"))


@pytest.mark.gpu
def test_gpu_hit_regimes(gpu, oracle):
    rng = np.random.default_rng(42)
    L = 16
    # every query an exact match at nr = 96: hits in every tile
    ra = _ascii(rng, 96, L)
    qa = ra[rng.integers(0, 96, size=2100)]
    exp = _brute(qa, ra, 1)
    assert (exp[1] == 0).all()
    _same(_gpu_call(gpu, _encode(oracle, qa, L), _encode(oracle, ra, L), L, 1), exp, "all exact")
    # mixed 0, 1, 2 errors at max_dist 1
    qa = _queries_near(rng, ra, 2100, L)
    exp = _brute(qa, ra, 1)
    assert (exp[1] == -1).any() and (exp[1] == 0).any() and (exp[1] == 1).any()
    q, r = _encode(oracle, qa, L), _encode(oracle, ra, L)
    _same(_gpu_call(gpu, q, r, L, 1), exp, "mixed")
    # max_dist >= P: every reference qualifies, the outputs are the true nearest
    for k in (_P(L), _P(L) + 1, U32_MAX):
        exp = _brute(qa, ra, k)
        assert (exp[1] >= 0).all()
        _same(_gpu_call(gpu, q, r, L, k), exp, ("every reference hits", k))
    # ... and at L = 1 (P = 2) the ties run into the hundreds: nbest up to nr
    qa1, ra1 = _ascii(rng, 50, 1), _ascii(rng, 1500, 1)
    exp = _brute(qa1, ra1, 2)
    assert exp[2].max() > 300
    _same(_gpu_call(gpu, _encode(oracle, qa1, 1), _encode(oracle, ra1, 1), 1, 2), exp, "L = 1")
    # nothing within max_dist: all "none"
    qa32, ra32 = _ascii(rng, 1100, 32), _ascii(rng, 1500, 32)
    exp = _brute(qa32, ra32, 3)
    assert (exp[0] == -1).all() and (exp[1] == -1).all() and (exp[2] == 0).all()
    _same(_gpu_call(gpu, _encode(oracle, qa32, 32), _encode(oracle, ra32, 32), 32, 3), exp, "none")
    # a whitelist of 64 identical rows
    ra = np.repeat(_ascii(rng, 1, L), 64, axis=0)
    qa = _mutate(rng, ra[:40], np.arange(40) % 3)
    got = _gpu_call(gpu, _encode(oracle, qa, L), _encode(oracle, ra, L), L, 1)
    _same(got, _brute(qa, ra, 1), "identical rows")
    assert got[2][0] == 64 and got[0][0] == 0 and got[2][1] == 64 and got[2][2] == 0


SPLITS = (1, 2, 3, 7)


@pytest.mark.gpu
def test_gpu_ties_across_boundaries_and_splits(gpu, oracle):
    """One reference repeated in another 32-column block, another LDS stage and (from 2 ranges on)
    another range; ref_splits 1, 2, 3, 7, auto and far above nr (clamped) give the same outputs."""
    rng = np.random.default_rng(43)
    L, nq, nr = 16, 40, 4099
    ra = _ascii(rng, nr, L)
    for dup in (40, 1500, 3000, 4098):
        ra[dup] = ra[5]
    qa = _queries_near(rng, ra, nq, L)
    qa[0] = ra[5]
    qa[1] = _mutate(rng, ra[5:6], [1])[0]
    q, r = _encode(oracle, qa, L), _encode(oracle, ra, L)
    for k in (0, 1, 2, _P(L)):
        exp = _brute(qa, ra, k)
        assert exp[0][0] == 5 and exp[2][0] == 5
        base = _gpu_call(gpu, q, r, L, k, splits=1)
        _same(base, exp, ("splits 1", k))
        for splits in SPLITS[1:] + (0, 129, 10 ** 6):
            _same(_gpu_call(gpu, q, r, L, k, splits=splits), base, ("splits", splits, k))
        _same(_gpu_call(gpu, q, r, L, k), base, ("plain entry", k))
    # multi-word and VALU forms through the split path
    for L2 in (64, 200):
        ra2 = _ascii(rng, 300, L2)
        ra2[290] = ra2[3]
        qa2 = _queries_near(rng, ra2, 40, L2)
        qa2[0] = ra2[3]
        exp = _brute(qa2, ra2, 2)
        assert exp[2][0] == 2
        for splits in SPLITS:
            _same(_gpu_call(gpu, _encode(oracle, qa2, L2), _encode(oracle, ra2, L2), L2, 2, splits=splits), exp, (L2, splits))


@pytest.mark.gpu
def test_gpu_alias_bit(gpu, oracle):
    rng = np.random.default_rng(12)
    for L in (7, 12, 31):
        q, r, D = _alias_case(oracle, rng, L, 40, 70)
        for k in (0, 1, 2):
            _same(_gpu_call(gpu, q, r, L, k), _from_dmatrix(D, k), ("alias", L, k))


@pytest.mark.gpu
def test_gpu_outputs_workspace_and_arguments(gpu, oracle):
    rng = np.random.default_rng(13)
    L = 16
    ra = _ascii(rng, 300, L)
    qa = _queries_near(rng, ra, 50, L)
    q, r = _encode(oracle, qa, L), _encode(oracle, ra, L)
    exp = _brute(qa, ra, 1)
    idx, dist, nb = _gpu_call(gpu, q, r, L, 1, nbest=False)                       # d_nbest = NULL
    assert nb is None
    _same((idx, dist), exp[:2], "no nbest")
    idx, dist, nb = _gpu_call(gpu, q, r, L, 1, nbest=False, splits=3)
    _same((idx, dist), exp[:2], "no nbest, splits")
    assert _gpu_call(gpu, q, r, L, 1, splits=2, short_ws=1) == SS_EARG            # one byte short
    _same(_gpu_call(gpu, q, r, L, 1, splits=2), exp, "after the refused call")
    assert _gpu_call(gpu, q, r, 0, 1) == SS_EARG
    assert _gpu_call(gpu, q, r, 1025, 1) == SS_EARG
    assert _gpu_call(gpu, q, r, 33, 1) == SS_EARG                                 # wpr 1 < W = 2
    # nr = 0: all "none"; nq = 0: a no-op
    none = _gpu_call(gpu, q, r[:0], L, 1)
    assert (none[0] == -1).all() and (none[1] == -1).all() and (none[2] == 0).all()
    empty = _gpu_call(gpu, q[:0], r, L, 1)
    assert all(len(x) == 0 for x in empty)


@pytest.mark.gpu
def test_gpu_graph_capture(gpu, oracle):
    """One call captured on a single stream and replayed equals the eager call (plain and split forms)."""
    import torch
    from shortseq_amd._native import check, lib
    rng = np.random.default_rng(14)
    L, nq, nr = 16, 1500, 4099
    ra = _ascii(rng, nr, L)
    qa = _queries_near(rng, ra, nq, L)
    q, r = _encode(oracle, qa, L), _encode(oracle, ra, L)
    exp = _brute(qa, ra, 1)
    dq, dr = _dev_rows(gpu, q), _dev_rows(gpu, r)
    for splits in (1, 3):
        ws_bytes = int(lib().ss_hamming_nearest_ws_bytes(nq, nr, L, splits))
        ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.int32, device=gpu)
        outs = [torch.full((nq,), -7, dtype=torch.int32, device=gpu) for _ in range(3)]
        torch.cuda.synchronize(gpu)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream(gpu).cuda_stream
            check(lib().ss_hamming_nearest_ex(dq.data_ptr(), nq, 1, dr.data_ptr(), nr, 1, L, 1, outs[0].data_ptr(),
                                              outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), ws_bytes, splits, s),
                  "captured nearest")
        for t in outs:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize(gpu)
        got = [t.cpu().numpy().view(np.uint32) for t in outs]
        _same((_signed(got[0]), _signed(got[1]), got[2].astype(np.int64)), exp, ("replay", splits))
        _same(_gpu_call(gpu, q, r, L, 1, splits=splits), exp, ("eager", splits))


@pytest.mark.gpu
def test_gpu_more_row_tiles_than_one_launch(gpu, oracle):
    """2^16 row tiles go into one launch; 65536 * 128 + 133 rows of 64 nt (S = 128) need a second one,
    whose blocks start at tile 65536.  The queries repeat a pool of 64 rows, so the expectation is the
    pool's brute force gathered on the device."""
    import torch
    from shortseq_amd._native import check, lib
    rng = np.random.default_rng(16)
    L, npool, nr = 64, 64, 33
    assert _row_tile(L) == 128
    nq = 65536 * 128 + 133
    ra = _ascii(rng, nr, L)
    pa = _queries_near(rng, ra, npool, L)
    exp = _brute(pa, ra, 1)
    assert (exp[1] == -1).any() and (exp[1] == 0).any() and (exp[1] == 1).any()
    pick = torch.arange(nq, device=gpu) % npool
    dq = torch.from_numpy(_encode(oracle, pa, L).view(np.int64)).to(gpu)[pick].contiguous()
    dr = torch.from_numpy(_encode(oracle, ra, L).view(np.int64)).to(gpu)
    want = [torch.from_numpy(e.astype(np.int32)).to(gpu)[pick] for e in exp]       # -1 = SS_NEAREST_NONE as int32
    for splits in (1, 2):
        ws_bytes = int(lib().ss_hamming_nearest_ws_bytes(nq, nr, L, splits))
        assert ws_bytes == (0 if splits == 1 else 2 * 12 * nq)
        ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.int32, device=gpu)
        outs = [torch.full((nq,), -7, dtype=torch.int32, device=gpu) for _ in range(3)]
        check(lib().ss_hamming_nearest_ex(dq.data_ptr(), nq, 2, dr.data_ptr(), nr, 2, L, 1, outs[0].data_ptr(),
                                          outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), ws_bytes, splits,
                                          torch.cuda.current_stream(gpu).cuda_stream), "ss_hamming_nearest_ex")
        torch.cuda.synchronize(gpu)
        for got, e, name in zip(outs, want, ("idx", "dist", "nbest")):
            assert torch.equal(got, e), (splits, name, torch.nonzero(got != e)[:4].tolist())


@pytest.mark.gpu
def test_batch_hamming_nearest_equals_host(gpu, oracle):
    import torch
    import shortseq_amd.batch as B
    rng = np.random.default_rng(15)
    L = 16
    ra = _ascii(rng, 700, L)
    qa = _queries_near(rng, ra, 5000, L)
    q, r = _encode(oracle, qa, L), _encode(oracle, ra, L)
    dq = torch.from_numpy(q.view(np.int64)).to(gpu)
    dr = torch.from_numpy(r.view(np.int64)).to(gpu)
    for k in (0, 1, 2):
        host = _host_ok(q, r, L, k)
        idx, dist, nb = B.hamming_nearest(dq, dr, L, k)
        assert idx.dtype == torch.int64 and dist.dtype == torch.int64 and nb.dtype == torch.int64
        _same((idx.cpu().numpy(), dist.cpu().numpy(), nb.cpu().numpy()), host, ("batch", k))
        idx, dist, nb = B.hamming_nearest(dq, dr, L, k, want_nbest=False, ref_splits=5)
        assert nb is None
        _same((idx.cpu().numpy(), dist.cpu().numpy()), host[:2], ("batch, splits", k))
    _same(host, _brute(qa, ra, 2), "host")


@pytest.mark.gpu
def test_correct_gpu_equals_host(gpu):
    import shortseq_amd.barcode as BC
    counter, wl, key_strs = _barcode_case(2, 3000, nwl=96)
    for amb in ("drop", "first"):
        host = BC.correct(counter, wl, 1, ambiguous=amb, device="host")
        dev = _check_correct(counter, wl, key_strs, 1, amb, "gpu")
        assert list(dev[0].items()) == list(host[0].items())
        assert list(dev[1].items()) == list(host[1].items())
