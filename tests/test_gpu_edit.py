"""k-difference pattern search on the GPU (sa_edit / sa_edit_device,
hpc_suffix_array_amd/csrc/sa_edit.h) against the definition written here in
numpy, which uses nothing of the library's search code:

    D(e) = min over s of ed(P, T[s, e)) by the row-wise Sellers DP over the
    whole text (per pattern row: tmp[0] = i, tmp[1:] = minimum(row[:-1] + (t !=
    p[i - 1]), row[1:] + 1), row = minimum.accumulate(tmp - idx) + idx); the
    occurrences are the ends e with D(e) <= k.  A pattern with m <= k is not
    searched: its list is empty.

Distances and starts come from the anchored DP of P reversed against
T[max(0, e - m - k), e) reversed, all ends of a pattern at once: the distance
is the least value of the last row (it must equal D(e)) and the start e - (the
first column that has it).  The candidates of the info words are the exact
occurrences of the k + 1 pieces of the patterns with m > k, counted with
bytes.find.  Offsets, ends, starts, distances and info words are compared
exactly.  The device cases go through DeviceBuilder.edit with 0xA5 guards
around the outputs, the two-call pattern and outputs at a chosen dword offset of
their allocation.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD8 = np.uint8(0xA5)
GUARD32 = np.uint32(0xA5A5A5A5)
GUARD64 = np.uint64(0xA5A5A5A5A5A5A5A5)
PAD = 8
DNA = np.frombuffer(b"ACGT", np.uint8)


def as_u8(x):
    return np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8)


def bounds(m, k):
    return [j * m // (k + 1) for j in range(k + 2)]


def sellers(t, p):
    """D(e) for e = 0 .. n."""
    n = t.size
    idx = np.arange(n + 1, dtype=np.int32)
    row = np.zeros(n + 1, np.int32)
    tmp = np.empty(n + 1, np.int32)
    for i in range(1, p.size + 1):
        tmp[0] = i
        np.minimum(row[:-1] + (t != p[i - 1]), row[1:] + 1, out=tmp[1:])
        row = np.minimum.accumulate(tmp - idx) + idx
    return row


def finish_all(t, p, ends, k):
    """(distance, start) of every end: the anchored DP of p reversed against
    t[max(0, e - m - k), e) reversed, a row of the batch per end; the columns
    past the front of the text cost `wall`.  16-bit cells where they hold."""
    m, w = p.size, p.size + k
    dt, big = (np.int16, 1 << 14) if w < (1 << 13) + 64 else (np.int64, 1 << 20)
    ends = np.asarray(ends, np.int64)
    x = np.arange(1, w + 1, dtype=np.int64)
    at = ends[:, None] - x[None, :]                      # column x compares t[e - x]
    ok = at >= 0
    seg = np.where(ok, t[np.maximum(at, 0)].astype(np.int16), -1)
    idx = np.arange(w + 1, dtype=dt)
    wall = np.concatenate([np.zeros((ends.size, 1), dt), np.where(ok, 0, big).astype(dt)], axis=1)
    row = idx[None, :] + wall
    tmp = np.empty_like(row)
    for i in range(1, m + 1):
        tmp[:, 0] = i
        np.minimum(row[:, :-1] + (seg != p[m - i]), row[:, 1:] + 1, out=tmp[:, 1:])
        row = np.minimum.accumulate(tmp - idx, axis=1) + idx + wall
    d = row.min(axis=1).astype(np.int64)
    return d, ends - row.argmin(axis=1)                  # the first least column: the largest start


def brute_one(t, p, k):
    """(ends, starts, distances) of pattern p in t, by the definition."""
    if p.size <= k:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8)
    D = sellers(t, p)
    ends = np.nonzero(D <= k)[0].astype(np.int64)
    if ends.size == 0:
        return ends, ends.copy(), np.zeros(0, np.uint8)
    d, s = finish_all(t, p, ends, k)
    assert np.array_equal(d, D[ends])                    # the two DPs of the oracle agree
    return ends, s, d.astype(np.uint8)


def count_exact(tb, piece):
    c, at = 0, tb.find(piece)
    while at >= 0:
        c += 1
        at = tb.find(piece, at + 1)
    return c


def brute(text, patterns, k, candidates=True):
    """(offsets, ends, starts, distances) and the info words [total,
    candidates, pieces]; candidates None when they are not counted."""
    t = as_u8(text)
    tb = t.tobytes()
    ends, starts, dist, off, cands = [], [], [], [0], 0
    for p in patterns:
        p = as_u8(p)
        e, s, d = brute_one(t, p, k)
        ends.append(e)
        starts.append(s)
        dist.append(d)
        off.append(off[-1] + e.size)
        if candidates and p.size > k:
            b = bounds(p.size, k)
            pb = p.tobytes()
            cands += sum(count_exact(tb, pb[b[j]:b[j + 1]]) for j in range(k + 1))
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)   # noqa: E731
    return ((np.array(off, np.int64), cat(ends, np.int64), cat(starts, np.int64), cat(dist, np.uint8)),
            [int(off[-1]), cands if candidates else None, len(patterns) * (k + 1)])


_SA = {}


def sa_of(text):
    """The text's suffix array by the library's builder (checked against the
    oracle by the parity tests): built once per text, never changed.  A text
    of one symbol has the suffix array n - 1 .. 0."""
    from hpc_suffix_array_amd import build_suffix_array
    t = as_u8(text)
    key = t.tobytes()
    if key not in _SA:
        if t.size and (t == t[0]).all():
            a = np.arange(t.size - 1, -1, -1, dtype=np.uint32)
        else:
            a = np.ascontiguousarray(build_suffix_array(t), np.uint32)
        a.setflags(write=False)
        _SA[key] = a
    return _SA[key]


def host_check(text, patterns, k, want=None, sa=None):
    from hpc_suffix_array_amd import edit_search
    t = as_u8(text)
    sa = sa_of(t) if sa is None else sa
    want = brute(t, patterns, k) if want is None else want
    (woff, wend, wstart, wdist), winfo = want
    off, end, start, dist, info = edit_search(t, sa, patterns, k, return_info=True)
    assert off.dtype == end.dtype == start.dtype == np.int64 and dist.dtype == np.uint8
    assert np.array_equal(off, woff)
    assert np.array_equal(end, wend)
    assert np.array_equal(dist, wdist)
    assert np.array_equal(start, wstart)
    assert info["total"] == winfo[0] and info["pieces"] == winfo[2]
    if winfo[1] is not None:
        assert info["candidates"] == winfo[1]
    return want


def other(c, rng, sym=None):
    if sym is None:
        return np.uint8(c ^ np.uint8(1 + rng.integers(0, 255)))
    return sym[(int(np.nonzero(sym == c)[0][0]) + 1 + rng.integers(0, sym.size - 1)) % sym.size]


def plant(t, at, m, edits, rng, sym=None):
    """A pattern of m bytes read from t[at ..) with the edits {pattern position:
    "sub" | "ins" | "del"}: a substituted byte, a byte the text does not have,
    a text byte the pattern skips in front of the position.  Returns the
    pattern and the end of the text it was read from: ed <= len(edits) there."""
    p = np.empty(m, np.uint8)
    cur = at
    for x in range(m):
        kind = edits.get(x)
        if kind == "ins":
            p[x] = other(t[min(cur, t.size - 1)], rng, sym)
            continue
        if kind == "del":
            cur += 1
        p[x] = other(t[cur], rng, sym) if kind == "sub" else t[cur]
        cur += 1
    return p, cur


def dna_text(n, seed):
    return DNA[np.random.default_rng(seed).integers(0, 4, n)]


KINDS = ("sub", "ins", "del")


# ---- the base case -----------------------------------------------------------

def random_dna_case(k):
    rng = np.random.default_rng(200 + k)
    t = dna_text(1 << 14, 7)
    pats, planted = [], []
    for i in range(256):
        m = (12, 24, 33, 70)[i % 4]
        at = int(rng.integers(0, t.size - m - k - 2))
        b = bounds(m, k)
        edges = sorted({x for j in range(k + 1) for x in (b[j], b[j + 1] - 1)})
        s = min(i % (k + 2), len(edges))
        where = sorted(rng.choice(edges, size=s, replace=False).tolist()) if s else []
        p, end = plant(t, at, m, {x: KINDS[(i + j) % 3] for j, x in enumerate(where)}, rng, DNA)
        pats.append(p)
        planted.append((end, s))
    return t, pats, planted


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_random_dna(gpu, k):
    """256 patterns of 12, 24, 33 and 70 bytes read from 2^14 bytes of DNA with
    0 .. k + 1 substitutions, insertions and deletions at the first and last
    bytes of the pieces.  The planted end is listed whenever the edits are
    within the budget; with k + 1 of them it is listed exactly when the edits
    happen to have a cheaper script (a deletion at byte 0 only moves the
    start, an insertion next to a deletion is one substitution): the oracle's
    D says which, and some are not."""
    from hpc_suffix_array_amd import find_patterns, locate_intervals
    t, pats, planted = random_dna_case(k)
    want = host_check(t, pats, k)
    (woff, wend, wstart, wdist), winfo = want
    over = listed_over = 0
    for q, (end, s) in enumerate(planted):
        mine = wend[woff[q]:woff[q + 1]]
        if s <= k:
            assert end in mine
        else:
            over += 1
            listed_over += end in mine
    assert 0 < winfo[0] and winfo[0] <= winfo[1] * (2 * k + 1) and listed_over < over
    if k == 0:
        sa = sa_of(t)
        lo, hi = find_patterns(t, sa, pats)
        off, pos = locate_intervals(sa, lo, hi)
        m = np.repeat([p.size for p in pats], np.diff(off))
        assert np.array_equal(off, woff) and np.array_equal(pos + m, wend) and (wdist == 0).all()
        assert np.array_equal(pos, wstart)


# ---- the ends of the text -----------------------------------------------------------

def text_ends_case():
    rng = np.random.default_rng(5)
    n = 331
    t = rng.integers(0, 256, n).astype(np.uint8)
    pats, front = [], {}
    for m in range(1, 41):
        for r in range(8):                                   # starts of every residue mod 8
            p = 8 * int(rng.integers(0, (n - m - 10) // 8)) + r
            kind = KINDS[(m + r) % 3]
            pats.append(plant(t, p, m, {(m * r) // 8: kind} if (m + r) % 4 else {}, rng)[0])
        pats.append(t[1:m + 1].copy())                       # cut at 0, the first byte deleted
        front[m] = len(pats)
        pats.append(np.concatenate([[other(t[0], rng)], t[:m - 1]]).astype(np.uint8))   # a byte in front: diagonal -1
        pats.append(np.concatenate([[other(t[0], rng), other(t[1], rng)], t[:m]]).astype(np.uint8))   # diagonal -2
        pats.append(t[n - m - 1:n - 1].copy())               # cut at the end, the last byte deleted
        pats.append(np.concatenate([t[n - m:], [other(t[n - 1], rng)]]).astype(np.uint8))   # a byte behind the end
        pats.append(np.concatenate([t[n - m:n - 1], [other(t[n - 1], rng)]]).astype(np.uint8))
    return t, pats, front


def test_ends_of_the_text(gpu):
    """m = 1 .. 40 at starts of every residue mod 8 with one edit that walks
    through the pattern, and patterns cut at both ends of the text with a byte
    missing or a byte too many: diagonals below 0 and beyond n - m."""
    t, pats, front = text_ends_case()
    n = t.size
    for k in (1, 2):
        (woff, wend, wstart, wdist), winfo = host_check(t, pats, k)
        assert winfo[0] >= 40 * 8 and (wstart == 0).any() and (wend == n).any() and (wdist > 0).any()
        for m in range(k + 2, 41):                           # P = x T[0, m - 1): e = m - 1, d = 1, start 0
            q = front[m]
            mine = list(zip(wend[woff[q]:woff[q + 1]].tolist(), wdist[woff[q]:woff[q + 1]].tolist(),
                            wstart[woff[q]:woff[q + 1]].tolist()))
            assert (m - 1, 1, 0) in mine


def test_pattern_longer_than_the_text(gpu):
    rng = np.random.default_rng(8)
    for n in (3, 8, 40):
        t = DNA[rng.integers(0, 4, n)]
        for k in (1, 2, 3):
            pats = [np.concatenate([t, DNA[rng.integers(0, 4, extra)]]) for extra in range(1, k + 2)]
            (woff, wend, wstart, wdist), winfo = host_check(t, pats, k)
            assert np.diff(woff)[-1] == 0                     # n + k + 1 bytes: no occurrence
            for q in range(k):                                # n + 1 .. n + k bytes end at n
                assert n in wend[woff[q]:woff[q + 1]]
    (woff, wend, wstart, wdist), winfo = host_check(b"abc", [b"abcd"], 1)
    assert wend.tolist() == [3] and wdist.tolist() == [1] and wstart.tolist() == [0]


def test_pinned_answers(gpu):
    (woff, wend, wstart, wdist), winfo = host_check(b"banana", [b"anan", b"bnana"], 1)
    assert woff.tolist() == [0, 3, 5] and wend.tolist() == [4, 5, 6, 4, 6]
    assert wdist.tolist() == [1, 0, 1, 1, 1] and wstart.tolist() == [1, 1, 3, 0, 2]
    (woff, wend, wstart, wdist), winfo = host_check(b"a" * 64, [b"a" * 6], 2)
    assert winfo == [61, 189, 3] and wend.tolist() == list(range(4, 65))


# ---- many diagonals reach one end -------------------------------------------------------

def test_periodic_texts(gpu):
    """Many diagonals and pieces reach one end, and a query lists more than
    SA_LOCATE_TILE ends; every end appears once."""
    t2 = as_u8(b"ab" * 4000)
    pats2 = [b"ab" * 6, b"ba" * 6, b"ab" * 3 + b"ba" * 3, b"ababaXababab", b"abababababaX", b"bbabababab", b"ab" * 20,
             b"a" + b"ab" * 16]
    (woff, wend, wstart, wdist), winfo = host_check(t2, pats2, 2)
    assert np.diff(woff)[0] > gpu.LOCATE_TILE and winfo[1] > winfo[0]
    t3 = as_u8(b"abc" * 3000)
    pats3 = [b"abc" * 4, b"bca" * 4, b"cab" * 4 + b"c", b"abcabXabcabc", b"abcXbcabcabX", b"acbacbacbacb", b"abc" * 11]
    (woff, wend, wstart, wdist), winfo = host_check(t3, pats3, 3)
    assert np.diff(woff)[0] > gpu.LOCATE_TILE and (wdist == 2).any()
    for q in range(len(pats3)):
        mine = wend[woff[q]:woff[q + 1]]
        assert np.unique(mine).size == mine.size


def one_symbol_want(n, m, k):
    """a^n against a^m: the ends m - k .. n, max(0, m - e), max(0, e - m)."""
    e = np.arange(m - k, n + 1, dtype=np.int64)
    return ((np.array([0, e.size], np.int64), e, np.maximum(0, e - m), np.maximum(0, m - e).astype(np.uint8)),
            [int(e.size), (k + 1) * (n - m // (k + 1) + 1), k + 1])


def test_one_symbol(gpu):
    import ctypes
    from hpc_suffix_array_amd import SAError, edit_search
    t = as_u8(b"a" * 5000)
    want = one_symbol_want(5000, 8, 1)
    assert want[1] == [4994, 9994, 2] and 4994 > gpu.LOCATE_TILE
    got = brute(t, [b"a" * 8], 1)
    assert got[1] == want[1] and all(np.array_equal(x, y) for x, y in zip(got[0], want[0]))
    (woff, wend, wstart, wdist), winfo = host_check(t, [b"a" * 8], 1, want=want)
    assert wend[0] == 7 and wend[-1] == 5000 and wdist[:3].tolist() == [1, 0, 0] and wstart[:4].tolist() == [0, 0, 1, 2]
    sa = sa_of(t)
    with pytest.raises(SAError, match="9994"):
        edit_search(t, sa, [b"a" * 8], 1, max_candidates=9993)
    out = edit_search(t, sa, [b"a" * 8], 1, max_candidates=9994)
    assert all(np.array_equal(x, y) for x, y in zip(out, want[0]))
    # ends alone: the backward pass is skipped
    off, end, start, dist = edit_search(t, sa, [b"a" * 8], 1, return_starts=False)
    assert np.array_equal(off, woff) and np.array_equal(end, wend) and start is None and dist is None
    # the raw call stopped by max_candidates fills the info words and zeroes off
    L = gpu.lib()
    p = as_u8(b"a" * 8)
    po = np.array([0, 8], np.uint64)
    off = np.full(2, 99, np.uint64)
    info = (ctypes.c_uint64 * 3)(7, 7, 7)
    rc = L.sa_edit(t.ctypes.data, 5000, sa.ctypes.data, 4, p.ctypes.data, po.ctypes.data, 1, 1, 9993, 0,
                   off.ctypes.data, None, None, None, 0, info)
    assert rc == gpu.EDIT_TOO_MANY == 1
    assert list(info) == [0, 9994, 2] and (off == 0).all()


def test_more_than_one_sweep_of_the_grid(gpu):
    """About 3.1 M candidates are more tiles of 2048 than the persistent
    grid's 4 x 256 workgroups; the answer is the closed form of one symbol,
    which the oracle confirms at a small size."""
    small = one_symbol_want(300, 6, 2)
    got = brute(np.full(300, ord("a"), np.uint8), [b"a" * 6], 2)
    assert got[1] == small[1] and all(np.array_equal(x, y) for x, y in zip(got[0], small[0]))
    n = 1 << 20
    want = one_symbol_want(n, 6, 2)
    assert want[1][1] == 3 * (n - 1) > 4 * 256 * 2048 and want[1][0] == n - 3
    host_check(np.full(n, ord("a"), np.uint8), [b"a" * 6], 2, want=want)


# ---- degenerate shapes ----------------------------------------------------------------

def test_degenerate_shapes(gpu):
    from hpc_suffix_array_amd import edit_search
    rng = np.random.default_rng(3)
    t = DNA[rng.integers(0, 4, 300)]
    # m <= k: an empty list among normal patterns, the pieces still counted
    (woff, wend, wstart, wdist), winfo = host_check(t, [b"A", t[20:40], b"ACG", b"", t[100:104], b"TTT"], 3)
    assert np.diff(woff)[[0, 2, 3, 5]].tolist() == [0, 0, 0, 0] and (np.diff(woff)[[1, 4]] > 0).all() and winfo[2] == 24
    # m = k + 1: one-byte pieces
    for k in (0, 1, 2, 5):
        host_check(t, [t[50:50 + k + 1], plant(t, 70, k + 1, {0: "sub"}, rng, DNA)[0], t[299 - k:]], k)
    # k = 31: the band's bits 0 and 62
    pats = [t[30:62], plant(t, 100, 64, {3: "ins", 20: "del", 40: "sub", 63: "sub"}, rng, DNA)[0],
            plant(t, 60, 200, {x: KINDS[x % 3] for x in range(0, 200, 9)}, rng, DNA)[0], t[:32], t[268:]]
    (woff, wend, wstart, wdist), winfo = host_check(t, pats, 31)
    assert (np.diff(woff) > 0).all() and wdist.max() == 31
    host_check(t, pats[1:3], 16)
    # n = 1
    for k in (0, 1, 2):
        (woff, wend, wstart, wdist), winfo = host_check(b"a", [b"a", b"b", b"", b"ab", b"ba", b"abc"], k)
        assert np.diff(woff).tolist() == [[1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 0], [0, 0, 0, 0, 0, 1]][k]
    # nq = 1, 3, 4, 5
    pats = [t[10:30], plant(t, 40, 21, {0: "del", 20: "sub"}, rng, DNA)[0], t[100:108],
            plant(t, 200, 33, {16: "ins"}, rng, DNA)[0], t[290:]]
    for nq in (1, 3, 4, 5):
        host_check(t, pats[:nq], 2)
    host_check(t, pats, 7)
    # an empty batch
    off, end, start, dist, info = edit_search(t, sa_of(t), [], 2, return_info=True)
    assert off.tolist() == [0] and end.size == 0 and start.size == 0 and dist.size == 0
    assert info == {"total": 0, "candidates": 0, "pieces": 0}
    # an empty text
    off, end, start, dist = edit_search(b"", np.zeros(0, np.uint32), [b"a", b""], 1)
    assert off.tolist() == [0, 0, 0] and end.size == 0


def test_bytes_00_and_ff(gpu):
    t = as_u8(b"\x00\xff\x00\x00\xff\xff\x00" * 40 + b"\xff")
    pats = [b"\x00\xff\x00\x00", b"\xff\xff\xff\xff\xff", b"\x00" * 9, b"\xff\x00\x00\xff\xff\x00\x00\xff\x00",
            b"\x00\x00\xff\xff\x00\x01\xff\x00\x00\xff\xfe\x00", b"\x00", b"\xff"]
    for k in (0, 1, 2):
        (woff, wend, wstart, wdist), winfo = host_check(t, pats, k)
        assert winfo[0] > 0 and (np.diff(woff)[-2:] > 0).all() == (k == 0)


# ---- long patterns ---------------------------------------------------------------------

LONG = (511, 512, 513, 1031, 4099, 8193)


def long_case(m):
    """Patterns of m bytes read from 9000 bytes of DNA, k = 3: an exact copy,
    one with a substitution and an insertion on the two sides of a piece
    boundary and a deletion at the next (kept), one with four edits far apart
    (rejected)."""
    rng = np.random.default_rng(18 + m)
    t = dna_text(9000, 18)
    k = 3
    at = 100 * LONG.index(m) + LONG.index(m)              # starts at different offsets (mod 8)
    b = bounds(m, k)
    p3, end3 = plant(t, at, m, {b[1] - 1: "sub", b[1] + 1: "ins", b[2]: "del"}, rng, DNA)
    p4, end4 = plant(t, at, m, {0: "sub", b[1] + 5: "del", b[2] - 1: "ins", m - 1: "sub"}, rng, DNA)
    return t, k, [t[at:at + m].copy(), p3, p4], [(at + m, 0), (end3, 3), (end4, None)]


@pytest.mark.parametrize("m", LONG)
def test_long_patterns(gpu, m):
    t, k, pats, planted = long_case(m)
    (woff, wend, wstart, wdist), winfo = host_check(t, pats, k)
    for q, (end, d) in enumerate(planted):
        mine = wend[woff[q]:woff[q + 1]].tolist()
        if d is None:
            assert mine == []
        else:
            at = mine.index(end)
            assert wdist[woff[q] + at] <= d and (wdist[woff[q] + at] > 0) == (d > 0)   # at most what was planted


# ---- the device form -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def builder(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder(1 << 16)
    yield b
    b.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def dev_edit(b, t, sa, pats, k, shift=0, stream=None, with_start=True, with_dist=True):
    """The two-call device pattern with guards: the sizing call, a call with
    out_cap one below the total (nothing written, off and info filled), the
    exact call.  Returns (off, end, start, dist) and the info triple."""
    import torch
    buf = np.concatenate([as_u8(p) for p in pats]) if pats else np.zeros(0, np.uint8)
    poff = np.zeros(len(pats) + 1, np.uint64)
    poff[1:] = np.cumsum([as_u8(p).size for p in pats])
    n, nq = t.size, len(pats)
    d_t, d_sa, d_poff = to_dev(t), to_dev(sa), to_dev(poff)
    d_p = to_dev(buf) if buf.size else None
    offbuf = torch.from_numpy(np.full(nq + 1 + 2 * PAD, GUARD64, np.uint64).view(np.int64)).cuda()
    d_off = offbuf[PAD:PAD + nq + 1]
    torch.cuda.synchronize()
    s = None if stream is None else stream.cuda_stream
    a = (d_t, n, d_sa, d_p, int(buf.size), d_poff, nq, k, d_off)
    info = b.edit(*a, None, None, None, 0, stream=s)
    total = info[0]
    sized = offbuf.cpu().numpy().view(np.uint64)[PAD:PAD + nq + 1].astype(np.int64)
    endbuf = torch.from_numpy(np.full(total + 2 * PAD + 4, GUARD32, np.uint32).view(np.int32)).cuda()
    startbuf = torch.from_numpy(np.full(total + 2 * PAD + 4, GUARD32, np.uint32).view(np.int32)).cuda()
    distbuf = torch.from_numpy(np.full(total + 2 * PAD + 4, GUARD8, np.uint8)).cuda()
    cut = slice(PAD + shift, PAD + shift + max(total, 1))
    d_end = endbuf[cut]
    d_start = startbuf[cut] if with_start else None
    d_dist = distbuf[cut] if with_dist else None
    assert (d_end.data_ptr() // 4) % 4 == (PAD + shift) % 4
    torch.cuda.synchronize()
    if total:
        offbuf[PAD:PAD + nq + 1] = 77
        assert b.edit(*a, d_end, d_start, d_dist, total - 1, stream=s) == info
        torch.cuda.synchronize()
        for bufx, g in ((endbuf, GUARD32), (startbuf, GUARD32)):
            assert (bufx.cpu().numpy().view(np.uint32) == g).all(), "out_cap below the total wrote ends or starts"
        assert (distbuf.cpu().numpy() == GUARD8).all(), "out_cap below the total wrote distances"
        assert np.array_equal(offbuf.cpu().numpy()[PAD:PAD + nq + 1], sized), "out_cap below the total fills d_off"
    assert b.edit(*a, d_end, d_start, d_dist, total, stream=s) == info
    torch.cuda.synchronize()
    ob = offbuf.cpu().numpy().view(np.uint64)
    assert (ob[:PAD] == GUARD64).all() and (ob[PAD + nq + 1:] == GUARD64).all(), "guard around d_off"
    eb = endbuf.cpu().numpy().view(np.uint32)
    sb = startbuf.cpu().numpy().view(np.uint32)
    db = distbuf.cpu().numpy()
    lo, hi = PAD + shift, PAD + shift + total
    assert (eb[:lo] == GUARD32).all() and (eb[hi:] == GUARD32).all(), "guard around d_end"
    assert (sb[:lo] == GUARD32).all() and (sb[hi:] == GUARD32).all(), "guard around d_start"
    assert (db[:lo] == GUARD8).all() and (db[hi:] == GUARD8).all(), "guard around d_dist"
    if not with_start:
        assert (sb == GUARD32).all()
    if not with_dist:
        assert (db == GUARD8).all()
    off = ob[PAD:PAD + nq + 1].astype(np.int64)
    assert np.array_equal(off, sized)              # the sizing call fills d_off
    return off, eb[lo:hi].astype(np.int64), sb[lo:hi].astype(np.int64), db[lo:hi].copy(), list(info)


def device_case():
    rng = np.random.default_rng(44)
    t = dna_text(6000, 44)
    pats = []
    for i in range(60):
        m = (9, 16, 40, 0, 3)[i % 5]
        a = int(rng.integers(0, t.size - 50))
        where = sorted(rng.choice(max(m, 1), size=min(i % 4, m), replace=False).tolist()) if m else []
        pats.append(plant(t, a, m, {x: KINDS[(i + j) % 3] for j, x in enumerate(where)}, rng, DNA)[0])
    pats.append(plant(t, 100, 600, {0: "sub", 299: "ins", 599: "del"}, rng, DNA)[0])
    return t, pats


_WANT = {}


def device_want(k=2):
    if k not in _WANT:
        t, pats = device_case()
        _WANT[k] = (t, pats, brute(t, pats, k))
    return _WANT[k]


def same(got, want):
    return all(np.array_equal(x, y) for x, y in zip(got, want))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_form(builder, shift):
    import torch
    t, pats, (want, winfo) = device_want()
    st = torch.cuda.Stream()
    *got, info = dev_edit(builder, t, sa_of(t), pats, 2, shift=shift, stream=st)
    assert info == winfo and same(got, want)
    # a periodic text on the same stream: a query above the locate tile
    t2 = as_u8(b"ab" * 4000)
    pats2 = [b"ab" * 6, b"ababaXababab", b"ba" * 7]
    if 2 not in _WANT.get("periodic", {}):
        _WANT["periodic"] = {2: brute(t2, pats2, 2)}
    want, winfo = _WANT["periodic"][2]
    *got, info = dev_edit(builder, t2, sa_of(t2), pats2, 2, shift=shift, stream=st)
    assert info == winfo and same(got, want)


def test_device_form_repeats_and_edges(builder):
    import torch
    from hpc_suffix_array_amd import SAError
    t, pats, (want, winfo) = device_want()
    sa = sa_of(t)
    a = dev_edit(builder, t, sa, pats, 2)
    b = dev_edit(builder, t, sa, pats, 2)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                # two equal calls, byte for byte
    # without starts, without distances, ends alone
    for ws, wd in ((False, True), (True, False), (False, False)):
        off, end, start, dist, info = dev_edit(builder, t, sa, pats, 2, with_start=ws, with_dist=wd)
        assert info == winfo and np.array_equal(off, want[0]) and np.array_equal(end, want[1])
        assert not ws or np.array_equal(start, want[2])
        assert not wd or np.array_equal(dist, want[3])
    # an empty batch: off[0] = 0 without a launch
    d_t, d_sa = to_dev(t), to_dev(sa)
    d_off = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_poff = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert builder.edit(d_t, t.size, d_sa, None, 0, d_poff, 0, 2, d_off, None, None, None, 0) == (0, 0, 0)
    assert d_off.cpu().numpy().tolist() == [0, 7, 7]
    # every pattern empty: no pattern buffer at all, nothing searched
    d_poff = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert builder.edit(d_t, t.size, d_sa, None, 0, d_poff, 2, 1, d_off, None, None, None, 0) == (0, 0, 4)
    assert d_off.cpu().numpy().tolist() == [0, 0, 0]
    # max_candidates through the device form
    buf = np.concatenate([as_u8(p) for p in pats])
    poff = np.zeros(len(pats) + 1, np.uint64)
    poff[1:] = np.cumsum([as_u8(p).size for p in pats])
    d_off = torch.zeros(len(pats) + 1, dtype=torch.int64, device="cuda")
    args = (d_t, t.size, d_sa, to_dev(buf), int(buf.size), to_dev(poff), len(pats), 2, d_off, None, None, None, 0)
    cands = winfo[1]
    with pytest.raises(SAError, match=str(cands)):
        builder.edit(*args, max_candidates=cands - 1)
    assert builder.edit(*args, max_candidates=cands) == tuple(winfo)


def test_width_8_host_form(gpu):
    from hpc_suffix_array_amd import edit_search
    t, pats, (want, winfo) = device_want()
    got = edit_search(t, sa_of(t).astype(np.int64), pats, 2)
    assert same(got, want)


def test_suffix_array_object(gpu, golden):
    from hpc_suffix_array_amd import SuffixArray
    names = sorted(golden["cases"], key=lambda c: golden["cases"][c]["n"])
    names = [c for c in names if 40 <= golden["cases"][c]["n"] <= 5000][:2]
    assert len(names) == 2
    rng = np.random.default_rng(9)
    for name in names:
        t = as_u8(golden["cases"][name]["text"])
        n = t.size
        pats = [plant(t, n // 3, 20, {0: "sub", 10: "del"}, rng)[0], t[:11].copy(), plant(t, n - 18, 16, {7: "ins"}, rng)[0],
                t[5:5].copy()]
        want, winfo = brute(t, pats, 2)
        with SuffixArray(t.tobytes()) as s:
            s.build()
            got = s.edit(pats, 2)
            one = s.edit(pats[0].tobytes(), 2)
        assert winfo[0] >= 3, name
        assert same(got, want), name
        hi = want[0][1]
        assert same(one, (want[1][:hi], want[2][:hi], want[3][:hi])), name
