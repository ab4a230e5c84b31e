"""Batched locate on the GPU (sa_locate / sa_locate_device,
hpc_suffix_array_amd/csrc/sa_locate.h) against numpy alone.

The kernels read no text, so most cases take a seeded random permutation of
[0, n) as the suffix array and build the intervals to the exact counts wanted.
Expected values: np.repeat of the query ids, a gather of the SA, and
np.lexsort((position, query id)) for the text order.  The end-to-end cases
compare locate_batch on the oracle's SA with overlapping bytes.find.

The device cases go through DeviceBuilder.locate with 0xA5 guard words on
both sides of d_off and d_pos, the two-call pattern (a sizing call first), and
d_pos at a chosen dword offset of its allocation.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = ["text", "sa"]
GUARD32 = np.uint32(0xA5A5A5A5)
GUARD64 = np.uint64(0xA5A5A5A5A5A5A5A5)
PAD = 8          # guard words on each side


def tile():
    from hpc_suffix_array_amd import _native as N
    return N.LOCATE_TILE


def counts_list():
    T = tile()
    return [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5]


_SA = {}


def perm_sa(n):
    """A seeded random permutation of [0, n): computed once, never changed."""
    if n not in _SA:
        a = np.random.default_rng(1000 + n).permutation(n).astype(np.uint32)
        a.setflags(write=False)
        _SA[n] = a
    return _SA[n]


def intervals(counts, n, seed):
    """lo, hi (uint32) with hi - lo = counts, placed at random."""
    rng = np.random.default_rng(seed)
    c = np.asarray(counts, np.int64)
    lo = (rng.random(c.size) * (n - c + 1)).astype(np.int64)
    return lo.astype(np.uint32), (lo + c).astype(np.uint32)


def expected(sa, lo, hi, max_hits=0, order="text"):
    """(offsets, positions) by numpy; an interval that breaks lo <= hi <= n is empty."""
    n = sa.size
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    c = np.where((lo <= hi) & (hi <= n), hi - lo, 0)
    if max_hits:
        c = np.minimum(c, max_hits)
    off = np.zeros(c.size + 1, np.int64)
    np.cumsum(c, out=off[1:])
    total = int(off[-1])
    qid = np.repeat(np.arange(c.size), c)
    idx = np.repeat(lo, c) + (np.arange(total) - np.repeat(off[:-1], c))
    pos = sa[idx].astype(np.int64)
    if order == "text":
        pos = pos[np.lexsort((pos, qid))]
    return off, pos


@pytest.fixture(scope="module")
def builder(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder((1 << 20) + 3)
    yield b
    b.close()


_DSA = {}


def device_sa(n):
    import torch
    if n not in _DSA:
        _DSA[n] = torch.from_numpy(perm_sa(n).view(np.int32).copy()).cuda()
    return _DSA[n]


def dev_locate(b, d_sa, n, lo, hi, max_hits=0, order="text", shift=0, stream=None, chunks=False, want_total=None):
    """The two-call device pattern with guard words; returns (off, pos) as
    int64 numpy arrays.  Checks on the way: the sizing call and a call with
    pos_cap one below the total return the total and leave d_pos untouched,
    and the guards on both sides of d_off and d_pos stay intact."""
    import torch
    nq = len(lo)
    d_lo = torch.from_numpy(np.asarray(lo, np.uint32).view(np.int32).copy()).cuda()
    d_hi = torch.from_numpy(np.asarray(hi, np.uint32).view(np.int32).copy()).cuda()
    offbuf = torch.from_numpy(np.full(nq + 1 + 2 * PAD, GUARD64, np.uint64).view(np.int64)).cuda()
    d_off = offbuf[PAD:PAD + nq + 1]
    torch.cuda.synchronize()
    s = None if stream is None else stream.cuda_stream
    kw = dict(max_hits=max_hits, order=order, stream=s, _chunks=chunks)
    total = b.locate(n, d_sa, d_lo, d_hi, nq, d_off, None, 0, **kw)          # the sizing call
    if want_total is not None:
        assert total == want_total
    posbuf = torch.from_numpy(np.full(total + 2 * PAD + 4, GUARD32, np.uint32).view(np.int32)).cuda()
    d_pos = posbuf[PAD + shift:PAD + shift + max(total, 1)]
    assert (d_pos.data_ptr() // 4) % 4 == (PAD + shift) % 4
    torch.cuda.synchronize()
    if total:
        assert b.locate(n, d_sa, d_lo, d_hi, nq, d_off, d_pos, total - 1, **kw) == total
        torch.cuda.synchronize()
        assert (posbuf.cpu().numpy().view(np.uint32) == GUARD32).all(), "pos_cap below the total wrote positions"
    assert b.locate(n, d_sa, d_lo, d_hi, nq, d_off, d_pos, total, **kw) == total
    torch.cuda.synchronize()
    ob = offbuf.cpu().numpy().view(np.uint64)
    pb = posbuf.cpu().numpy().view(np.uint32)
    assert (ob[:PAD] == GUARD64).all() and (ob[PAD + nq + 1:] == GUARD64).all(), "guard around d_off"
    assert (pb[:PAD + shift] == GUARD32).all() and (pb[PAD + shift + total:] == GUARD32).all(), "guard around d_pos"
    return ob[PAD:PAD + nq + 1].astype(np.int64), pb[PAD + shift:PAD + shift + total].astype(np.int64)


def check(b, n, lo, hi, max_hits=0, order="text", **kw):
    sa = perm_sa(n)
    woff, wpos = expected(sa, lo, hi, max_hits, order)
    off, pos = dev_locate(b, device_sa(n), n, lo, hi, max_hits, order, want_total=int(woff[-1]), **kw)
    assert np.array_equal(off, woff)
    assert np.array_equal(pos, wpos)
    return off, pos


def spread(counts, seed, empties=True):
    """The counts shuffled, with runs of empty queries in between."""
    rng = np.random.default_rng(seed)
    out = []
    for c in rng.permutation(counts):
        out.append(int(c))
        if empties and rng.random() < 0.4:
            out += [0] * int(rng.integers(1, 6))
    return out


# ---- counts ----------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
def test_each_count_alone(builder, order):
    n = 1 << 16
    for k, c in enumerate(counts_list()):
        lo, hi = intervals([c], n, seed=k)
        check(builder, n, lo, hi, order=order)


@pytest.mark.parametrize("order", ORDERS)
def test_all_counts_in_one_batch(builder, order):
    n = (1 << 17) + 1
    cs = spread(counts_list() * 3, seed=3)
    lo, hi = intervals(cs, n, seed=4)
    check(builder, n, lo, hi, order=order)


# ---- tile packing ----------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
def test_tile_packing(builder, order):
    T, n = tile(), 1 << 16
    shapes = {
        "2T - 1 in one tile": [1] * (T - 1) + [T],
        "2T - 1 after an offset": [T - 1, T, 5],
        "exact tiles": [T] * 5 + [T // 2] * 8 + [T // 64] * 128,
        "one-hit queries": [1] * (3 * T + 1),
        "all empty": [0] * 77,
        "one query": [17],
        "empties around": [0] * 300 + [3] + [0] * 3000 + [T] + [0] * 10,
        "large on a tile's last slot": [1] * (T - 1) + [T + 1, 1, 1],
    }
    for k, (name, cs) in enumerate(shapes.items()):
        lo, hi = intervals(cs, n, seed=10 + k)
        check(builder, n, lo, hi, order=order)


def test_more_tiles_than_workgroups(builder):
    """The small kernel's grid is capped at 4 workgroups per CU and strides
    over the tiles: 2.3 M hits are more tiles than 4 x 256."""
    T, n = tile(), 1 << 20
    rng = np.random.default_rng(21)
    cs = rng.integers(1, 33, size=140_000)
    assert cs.sum() > 4 * 256 * T + T
    lo, hi = intervals(cs, n, seed=22)
    check(builder, n, lo, hi)


# ---- the cap ---------------------------------------------------------------

def test_max_hits(builder):
    T, n = tile(), (1 << 16) + 3
    cs = spread(counts_list() + [3 * T], seed=30)
    lo, hi = intervals(cs, n, seed=31)
    sa = perm_sa(n)
    for cap in (1, 2, 64, T, T + 1):
        check(builder, n, lo, hi, max_hits=cap, order="sa")
        off, pos = check(builder, n, lo, hi, max_hits=cap, order="text")
        # the sorted first max_hits SA entries, stated once more without the helper
        for q in (0, len(cs) // 2, int(np.argmax(cs))):
            want = np.sort(sa[lo[q]:lo[q] + min(cs[q], cap)].astype(np.int64))
            assert np.array_equal(pos[off[q]:off[q + 1]], want)
    # a 3T query made small by the cap, alone and on a tile's last slot
    lo, hi = intervals([1] * (T - 1) + [3 * T], n, seed=32)
    check(builder, n, lo, hi, max_hits=T)
    check(builder, n, lo[-1:], hi[-1:], max_hits=T)


# ---- the large class -------------------------------------------------------

@pytest.mark.parametrize("chunks", [False, True])
def test_large_queries(builder, chunks):
    T, n = tile(), (1 << 18) + 7
    cs = [5, T + 1, 0, 17, 9 * T + 3, T, 2 * T, 1, 40 * T + 1, 0, 0, T + 2, 3]
    lo, hi = intervals(cs, n, seed=40)
    for order in ORDERS:
        check(builder, n, lo, hi, order=order, chunks=chunks)
    # the same large interval twice, between small ones
    lo2 = np.array([lo[0], lo[4], lo[3], lo[4], lo[4]], np.uint32)
    hi2 = np.array([hi[0], hi[4], hi[3], hi[4], hi[4]], np.uint32)
    check(builder, n, lo2, hi2, chunks=chunks)
    # n_large = 1 and n_large = 300
    check(builder, n, lo[4:5], hi[4:5], chunks=chunks)
    rng = np.random.default_rng(41)
    cs = spread(list(T + 1 + rng.integers(0, 50, size=300)) + [7] * 50, seed=42)
    lo, hi = intervals(cs, n, seed=43)
    assert (np.asarray(cs) > T).sum() == 300
    check(builder, n, lo, hi, chunks=chunks)


@pytest.mark.parametrize("chunks", [False, True])
def test_whole_sa(builder, chunks):
    n = (1 << 20) + 3
    lo, hi = np.array([0, 5], np.uint32), np.array([n, 9], np.uint32)
    off, pos = check(builder, n, lo, hi, chunks=chunks)
    assert np.array_equal(pos[:n], np.arange(n))


def test_one_interval_a_thousand_times(builder):
    n = 1 << 16
    lo, hi = intervals([70], n, seed=50)
    lo, hi = np.repeat(lo, 1000), np.repeat(hi, 1000)
    off, pos = check(builder, n, lo, hi)
    assert off[-1] == 70_000 > n


# ---- the device form -------------------------------------------------------

@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_form(builder, shift):
    """A non-default stream, d_pos at every dword offset of a 16-byte line
    (small and large queries: the large class stores 16 bytes at a time),
    guard words, intervals that break lo <= hi <= n."""
    import torch
    T, n = tile(), (1 << 16) + 1
    cs = spread([1, 2, 3, 5, 64, 300, T, T + 1, 2 * T + 3, 5 * T + 2, T + 7], seed=60 + shift)
    lo, hi = intervals(cs, n, seed=61)
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    bad_lo = np.array([9, 0, n + 1, n + 5, 0xFFFFFFFF], np.int64)     # lo > hi, hi > n, lo > n, both, the largest
    bad_hi = np.array([8, n + 1, n + 2, n + 4, 0xFFFFFFFF], np.int64)
    at = len(cs) // 2
    lo = np.concatenate([lo[:at], bad_lo, lo[at:]]).astype(np.uint32)
    hi = np.concatenate([hi[:at], bad_hi, hi[at:]]).astype(np.uint32)
    st = torch.cuda.Stream()
    for order in ORDERS:
        check(builder, n, lo, hi, order=order, shift=shift, stream=st)


def test_host_waits_and_repeatability(builder):
    import torch
    L = builder.L
    T, n = tile(), 1 << 16
    cs = spread([1, 2, 3, 31, 64, 257, T - 1, T] * 4, seed=70)
    lo, hi = intervals(cs, n, seed=71)
    d_sa = device_sa(n)
    d_lo = torch.from_numpy(lo.view(np.int32).copy()).cuda()
    d_hi = torch.from_numpy(hi.view(np.int32).copy()).cuda()
    total = int(np.sum(cs))
    d_off = torch.zeros(len(cs) + 1, dtype=torch.int64, device="cuda")
    outs = []
    for _ in range(2):
        d_pos = torch.zeros(total, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        before = L.sa_host_syncs()
        assert builder.locate(n, d_sa, d_lo, d_hi, len(cs), d_off, d_pos, total) == total
        assert L.sa_host_syncs() - before == 1          # one host wait when no query is large
        outs.append((d_off.cpu().numpy().copy(), d_pos.cpu().numpy().copy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    woff, wpos = expected(perm_sa(n), lo, hi)
    assert np.array_equal(outs[0][0], woff) and np.array_equal(outs[0][1].view(np.uint32), wpos)
    # the sizing call waits once too, with large queries or without
    lo2, hi2 = intervals([T + 1, 3, 4 * T], n, seed=72)
    d_lo2 = torch.from_numpy(lo2.view(np.int32).copy()).cuda()
    d_hi2 = torch.from_numpy(hi2.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    before = L.sa_host_syncs()
    assert builder.locate(n, d_sa, d_lo2, d_hi2, 3, d_off, None, 0) == 5 * T + 4
    assert L.sa_host_syncs() - before == 1
    # nq == 0: off[0] = 0 and a total of 0
    d_off.fill_(7)
    assert builder.locate(n, d_sa, d_lo, d_hi, 0, d_off, None, 0) == 0
    assert d_off.cpu().numpy().tolist()[:2] == [0, 7]


# ---- host forms and end to end ---------------------------------------------

def test_locate_intervals_host_form(gpu):
    from hpc_suffix_array_amd import locate_intervals
    T, n = tile(), (1 << 16) + 5
    sa = perm_sa(n)
    cs = spread(counts_list(), seed=80)
    lo, hi = intervals(cs, n, seed=81)
    for order in ORDERS:
        for cap in (0, 64):
            off, pos = locate_intervals(sa, lo, hi, max_hits=cap, order=order)
            woff, wpos = expected(sa, lo, hi, cap, order)
            assert off.dtype == np.int64 and pos.dtype == np.int64
            assert np.array_equal(off, woff) and np.array_equal(pos, wpos)
    # width-8 SA in, width-8 positions out
    off, pos = locate_intervals(sa.astype(np.int64), lo, hi)
    woff, wpos = expected(sa, lo, hi)
    assert np.array_equal(off, woff) and np.array_equal(pos, wpos)
    # the chunked radix sort through the host form
    off, pos = locate_intervals(sa, lo, hi, _chunks=True)
    assert np.array_equal(off, woff) and np.array_equal(pos, wpos)
    # empty batches
    off, pos = locate_intervals(sa, [], [])
    assert off.tolist() == [0] and pos.size == 0
    off, pos = locate_intervals(sa, [4, 9], [4, 9])
    assert off.tolist() == [0, 0, 0] and pos.size == 0


def occurrences(tb, p):
    """Overlapping occurrences of p in tb, ascending (bytes.find; a sliding
    numpy compare where a short pattern occurs very often)."""
    n, m = len(tb), len(p)
    if m == 0:
        return np.arange(n, dtype=np.int64)
    if m > n:
        return np.zeros(0, np.int64)
    if tb.count(p[:8]) > 2000:
        a = np.frombuffer(tb, np.uint8)
        hit = np.ones(n - m + 1, bool)
        for j in range(m):
            hit &= a[j:n - m + 1 + j] == p[j]
        return np.flatnonzero(hit).astype(np.int64)
    out, i = [], tb.find(p)
    while i >= 0:
        out.append(i)
        i = tb.find(p, i + 1)
    return np.array(out, np.int64)


def text_cases(oracle):
    per = np.frombuffer((b"abracadabra" * 500)[:5000], np.uint8)
    one = np.full(5000, ord("a"), np.uint8)
    return {
        "dna": (oracle.gen_text("dna", 65537, seed=3), [1, 2, 3, 4, 6, 8, 12, 16]),
        "byte256": (oracle.gen_text("byte256", 40_001, seed=4), [1, 2, 3, 8]),
        "periodic": (per, [1, 2, 4, 11, 23, 2000, 4000]),
        "one symbol": (one, [1, 3, 2000, 2952, 2953, 3500, 4990, 5000]),
    }


@pytest.mark.parametrize("name", ["dna", "byte256", "periodic", "one symbol"])
def test_locate_batch_vs_bytes_find(gpu, oracle, name):
    from hpc_suffix_array_amd import locate_batch, locate_patterns
    t, lens = text_cases(oracle)[name]
    tb, n = bytes(t), len(t)
    sa = oracle.sa_c(t)
    if name == "one symbol":
        assert np.array_equal(sa, np.arange(n - 1, -1, -1))      # exactly descending: the sort's worst case
    rng = np.random.default_rng(len(name))
    pats = []
    for m in lens:
        for _ in range(6):
            a = int(rng.integers(n - m + 1))
            pats.append(tb[a:a + m])
    pats += [b"", tb[-3:], b"\x00\x01zz", tb[:7] + b"\xff", tb + b"a"]        # the last three do not occur
    occ = [occurrences(tb, p) for p in pats]
    assert any(o.size == 0 for o in occ) and any(o.size > tile() for o in occ)
    off, pos = locate_batch(t, sa, pats)
    woff = np.concatenate([[0], np.cumsum([o.size for o in occ])])
    assert np.array_equal(off, woff)
    assert np.array_equal(pos, np.concatenate(occ))
    assert np.array_equal(pos, np.concatenate(locate_patterns(t, sa, pats)))
    # SA order: the same sets, as the SA lists them; capped: the first hits in SA order
    off2, pos2 = locate_batch(t, sa, pats, order="sa")
    assert np.array_equal(off2, woff)
    for q in range(len(pats)):
        assert np.array_equal(np.sort(pos2[off2[q]:off2[q + 1]]), occ[q])
    off3, pos3 = locate_batch(t, sa, pats, max_hits=5)
    for q in range(len(pats)):
        k = min(5, occ[q].size)
        assert off3[q + 1] - off3[q] == k
        assert np.array_equal(pos3[off3[q]:off3[q + 1]], np.sort(pos2[off2[q]:off2[q] + k]))
    # width-8 SA
    off4, pos4 = locate_batch(t, sa.astype(np.int64), pats[:10])
    assert np.array_equal(pos4, np.concatenate(occ[:10])) and pos4.dtype == np.int64


def test_golden_locate_batch(gpu, golden):
    from hpc_suffix_array_amd import locate_batch
    for name, c in golden["cases"].items():
        t = c["text"]
        tb, n = bytes(t), len(t)
        rng = np.random.default_rng(c["n"])
        pats = [b"zq\x00\x01"]
        for m in (1, 2, 3, 5, 9):
            for _ in range(8):
                a = int(rng.integers(max(n - m, 0) + 1))
                pats.append(tb[a:a + m])
        occ = [occurrences(tb, p) for p in pats]
        off, pos = locate_batch(t, c["sa"], pats)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([o.size for o in occ])])), name
        assert np.array_equal(pos, np.concatenate(occ)), name
