"""words_fp (csrc/ss_device.h) restated on Python ints, and distinct rows built to share a fingerprint.

fp_step(h, x) = f(h ^ x) with f(t) = (t ^ (t >> 29)) * M1 mod 2^64: an xorshift and an odd multiplier,
both invertible, so f is a bijection and a row's state can be steered through any word that may hold
all 64 bits (a full 32-nt word).  fp_final is a bijection too, up to its clamp of ~0 (the tables'
free-slot value) onto ~1.

A "row" here is the sequence of words the device hashes: the W packed words of a GpuCounter key, or a
length-class row of the drop-in engine -- the W packed words, then the length (W1 = W + 1 words).
The seed depends on the row's width, so a family collides at the width it was built for.
"""
MASK = (1 << 64) - 1
M1 = 0xBF58476D1CE4E5B9
M2 = 0x94D049BB133111EB
M1_INV = pow(M1, -1, 1 << 64)
M2_INV = pow(M2, -1, 1 << 64)
SEED = 0x243F6A8885A308D3
EMPTY = MASK                 # ~0: a free slot
CLAMPED = MASK - 1           # ~1


def seed(W):
    return SEED ^ W


def f(t):
    t ^= t >> 29
    return (t * M1) & MASK


def f_inv(y):
    t = (y * M1_INV) & MASK
    return t ^ (t >> 29) ^ (t >> 58)


def fp_step(h, x):
    return f(h ^ x)


def final_raw(h):
    """fp_final before its clamp."""
    h ^= h >> 32
    h = (h * M2) & MASK
    return h ^ (h >> 29)


def fp_final(h):
    r = final_raw(h)
    return CLAMPED if r == EMPTY else r


def final_inv(y):
    h = y ^ (y >> 29) ^ (y >> 58)
    h = (h * M2_INV) & MASK
    return h ^ (h >> 32)


def state(row, upto=None):
    """The state before word `upto` of `row` (default: after every word)."""
    h = seed(len(row))
    for x in row[:len(row) if upto is None else upto]:
        h = fp_step(h, x)
    return h


def fp(row):
    return fp_final(state(row))


def rand_word(rng):
    """Any 64-bit value (rng: random.Random)."""
    return rng.getrandbits(64)


def family(row, j, K, rng, keep_zero=0, max_draws=100_000):
    """K distinct rows with one fingerprint: `row` and K - 1 rows differing from it in words j and
    j + 1 only.  x_j' is drawn, x_{j+1}' = x_{j+1} ^ fp_step(h_j, x_j) ^ fp_step(h_j, x_j'): the states
    after word j + 1 agree.  Word j must be a full word; the bits of `keep_zero` (those word j + 1
    does not use) must be clear in the difference, so x_j' is drawn again until they are.
    -> (rows as tuples, draws)."""
    row = tuple(row)
    assert 0 <= j and j + 1 < len(row)
    hj = state(row, j)
    s = fp_step(hj, row[j])
    rows, draws = [row], 0
    while len(rows) < K:
        draws += 1
        if draws > max_draws:
            raise AssertionError(f"no collider within {max_draws} draws")
        x = rand_word(rng)
        d = s ^ fp_step(hj, x)
        if d & keep_zero:
            continue
        r = row[:j] + (x, row[j + 1] ^ d) + row[j + 2:]
        if r not in rows:
            rows.append(r)
    return rows, draws


def row_with_state(T, head, tail):
    """The row head + (x,) + tail whose state before fp_final is T (x: a full word)."""
    head, tail = tuple(head), tuple(tail)
    h = seed(len(head) + 1 + len(tail))
    for w in head:
        h = fp_step(h, w)
    for w in reversed(tail):           # state before w = f_inv(state after w) ^ w
        T = f_inv(T) ^ w
    return head + (f_inv(T) ^ h,) + tail


def class_row(words, L):
    """The drop-in engine's row of a read of L nt: its packed words, then its length."""
    return tuple(words) + (L,)


def cross_class_pair(rng):
    """A 96-nt and a 64-nt class row (W1 = 4 and 3: other widths, other seeds) with one fingerprint."""
    b = class_row([rand_word(rng) for _ in range(3)], 96)
    a = row_with_state(state(b), [rand_word(rng)], [64])
    return a, b


def clamp_pair(rng, tail=()):
    """Two rows of two full words (then `tail`: () for a 64-nt GpuCounter key, (64,) for the class row)
    whose fingerprints before the clamp are ~0 and ~1: both are ~1 after it."""
    return tuple(row_with_state(final_inv(y), [rand_word(rng)], tail) for y in (EMPTY, CLAMPED))


# ---- the host codec: which bits a word uses, rows as reads ---------------------------------------

def unused_bits(L):
    """The bits of the last packed word that a read of L nt leaves unused, asked of the host codec:
    a read of G (code 3) sets every bit it uses, a read of A none."""
    import shortseq_amd as sq
    g, a = sq.pack(b"G" * L).packed, sq.pack(b"A" * L).packed
    assert len(g) == (L + 31) // 32 and not any(a)
    assert all(w == MASK for w in g[:-1])
    return ~g[-1] & MASK


def to_read(words, L):
    """Packed words of a read of L nt -> its ASCII bytes, through the host codec."""
    import shortseq_amd as sq
    s = str(sq.from_words(list(words), L)).encode("ascii")
    assert len(s) == L
    return s


def rand_words(rng, L):
    """Packed words of a random read of L nt (the last word's unused bits clear)."""
    W = (L + 31) // 32
    w = [rand_word(rng) for _ in range(W)]
    w[-1] &= ~unused_bits(L) & MASK
    return tuple(w)
