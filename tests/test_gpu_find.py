"""GPU pattern search over a built suffix array (sa_find / sa_find_device,
hpc_suffix_array_amd/csrc/sa_find.h) against Python alone.

Expected intervals: with tb = bytes(text), sa the oracle's suffix array and
key(r) = tb[sa[r]:sa[r] + m], lo = bisect_left and hi = bisect_right of the
pattern over range(n) by that key -- Python orders bytes as unsigned, the
shorter prefix first, which is the builder's order.  Expected occurrences:
overlapping bytes.find.  Every case runs in the three modes: auto (patterns of
up to FIND_LANE_MAX bytes one per lane, longer ones one per wavefront), lane
and wave (one kernel for every pattern).
"""
import bisect

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ["auto", "lane", "wave"]
KINDS = ["dna", "alnum", "ascii127", "byte256", "binary"]


def ref_interval(tb, sal, p):
    n, m = len(tb), len(p)
    key = lambda r: tb[sal[r]:sal[r] + m]   # noqa: E731
    return bisect.bisect_left(range(n), p, key=key), bisect.bisect_right(range(n), p, key=key)


def ref_intervals(tb, sa, pats):
    sal = np.asarray(sa).tolist()
    got = [ref_interval(tb, sal, bytes(p)) for p in pats]
    return np.array([g[0] for g in got], np.int64), np.array([g[1] for g in got], np.int64)


def occurrences(tb, p):
    """Overlapping occurrences of p in tb, ascending (bytes.find; a sliding
    numpy compare of the same bytes where a short pattern occurs very often)."""
    n, m = len(tb), len(p)
    if m == 0:
        return np.arange(n, dtype=np.int64)
    if m > n:
        return np.zeros(0, np.int64)
    if m <= 8 and tb.count(p) > 2000:
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


def lengths():
    from hpc_suffix_array_amd import _native as N
    T = N.FIND_LANE_MAX
    return [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, T - 1, T, T + 1]


def draw_patterns(t, nq, seed, lens=None):
    """Thirds: cut from the text, cut with the last byte changed, random
    (bytes drawn from the text)."""
    rng = np.random.default_rng(seed)
    tb, n = bytes(t), len(t)
    lens = lens or lengths()
    out = []
    for i in range(nq):
        m = int(lens[rng.integers(len(lens))])
        a = int(rng.integers(n))
        p = bytearray(tb[a:a + m])
        if i % 3 == 1 and p:
            p[-1] = (p[-1] + 1 + int(rng.integers(255))) & 0xFF
        elif i % 3 == 2:
            p = bytearray(t[rng.integers(n, size=m)].tobytes())
        out.append(bytes(p))
    return out


_CASES = {}


def case(oracle, kind, n):
    """Text, oracle SA, 321 drawn + 7 fixed patterns and their expected
    intervals and occurrence lists: computed once, shared by the modes."""
    if (kind, n) not in _CASES:
        t = oracle.gen_text(kind, n, seed=5 * n + len(kind))
        tb = bytes(t)
        sa = oracle.sa_c(t)
        pats = draw_patterns(t, 321, seed=n + len(kind))
        pats += [b"", tb[-5:], tb[-5:] + b"\x00", tb, tb + b"a", b"\x00", b"\xff" * 9]
        lo, hi = ref_intervals(tb, sa, pats)
        occ = [occurrences(tb, p) for p in pats]
        for a, b, o in zip(lo, hi, occ):
            assert b - a == len(o)          # the two references agree
        _CASES[(kind, n)] = dict(text=t, sa=sa, pats=pats, lo=lo, hi=hi, occ=occ)
    return _CASES[(kind, n)]


def test_golden_find_patterns(gpu, golden):
    from hpc_suffix_array_amd import find_patterns
    for name, c in golden["cases"].items():
        tb = bytes(c["text"])
        pats = draw_patterns(c["text"], 50, seed=len(name) + c["n"])
        lo, hi = ref_intervals(tb, c["sa"], pats)
        for mode in MODES:
            glo, ghi = find_patterns(c["text"], c["sa"], pats, mode=mode)
            assert glo.dtype == np.int64 and ghi.dtype == np.int64
            assert (glo == lo).all() and (ghi == hi).all(), (name, mode)


def test_golden_suffix_array_object(gpu, golden):
    """SuffixArray.find / count / locate over the object's own str and sa
    (the drop-in copy ends at the first NUL: those texts are left to
    find_patterns)."""
    from hpc_suffix_array_amd import SuffixArray
    for name, c in golden["cases"].items():
        tb = bytes(c["text"])
        if 0 in tb:
            continue
        pats = draw_patterns(c["text"], 50, seed=len(name) + c["n"])
        lo, hi = ref_intervals(tb, c["sa"], pats)
        with SuffixArray(tb) as s:
            s.build()
            for i, p in enumerate(pats):
                assert s.find(p) == (lo[i], hi[i]), (name, p)
            for mode in ("lane", "wave"):
                for i in range(0, 50, 10):
                    assert s.find(pats[i], mode=mode) == (lo[i], hi[i]), (name, mode, pats[i])
            for i in range(0, 50, 7):
                assert s.count(pats[i]) == hi[i] - lo[i]
                assert np.array_equal(s.locate(pats[i]), occurrences(tb, pats[i])), (name, pats[i])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 9, 4095, 65537, 1_000_003])
@pytest.mark.parametrize("kind", KINDS)
def test_find_vs_python(gpu, oracle, kind, n, mode):
    from hpc_suffix_array_amd import count_patterns, find_patterns, locate_patterns
    c = case(oracle, kind, n)
    lo, hi = find_patterns(c["text"], c["sa"], c["pats"], mode=mode)
    bad = np.flatnonzero((lo != c["lo"]) | (hi != c["hi"]))
    assert bad.size == 0, [(c["pats"][i][:40], len(c["pats"][i]), lo[i], hi[i], c["lo"][i], c["hi"][i]) for i in bad[:5]]
    assert (count_patterns(c["text"], c["sa"], c["pats"], mode=mode) == c["hi"] - c["lo"]).all()
    loc = locate_patterns(c["text"], c["sa"], c["pats"], mode=mode)
    assert len(loc) == len(c["pats"])
    for got, want, p in zip(loc, c["occ"], c["pats"]):
        assert np.array_equal(got, want), p[:40]


def test_find_width8_and_offsets_pair(gpu, oracle):
    from hpc_suffix_array_amd import find_patterns
    from hpc_suffix_array_amd.builder import _pack_patterns
    c = case(oracle, "dna", 4095)
    lo, hi = find_patterns(c["text"], c["sa"].astype(np.int64), c["pats"])
    assert (lo == c["lo"]).all() and (hi == c["hi"]).all()
    buf, off = _pack_patterns(c["pats"])
    lo, hi = find_patterns(c["text"], c["sa"], (np.concatenate([np.zeros(3, np.uint8), buf]), off.astype(np.int64) + 3))
    assert (lo == c["lo"]).all() and (hi == c["hi"]).all()


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257, 5000])
def test_find_batch_shapes(gpu, oracle, nq):
    """Ragged waves and workgroups."""
    from hpc_suffix_array_amd import find_patterns
    t = oracle.gen_text("dna", 65537, seed=11)
    sa = oracle.sa_c(t)
    pats = draw_patterns(t, nq, seed=nq)
    lo, hi = ref_intervals(bytes(t), sa, pats)
    for mode in MODES:
        glo, ghi = find_patterns(t, sa, pats, mode=mode)
        assert (glo == lo).all() and (ghi == hi).all(), mode


def test_find_grid_stride(gpu, oracle):
    """More queries than one launch has lanes (2048 x 256) or wavefront
    slots (2048 x 4 x 8): 5000 checked patterns, repeated."""
    from hpc_suffix_array_amd import find_patterns
    from hpc_suffix_array_amd.builder import _pack_patterns
    t = oracle.gen_text("dna", 65537, seed=11)
    sa = oracle.sa_c(t)
    pats = draw_patterns(t, 5000, seed=5000)
    lo, hi = ref_intervals(bytes(t), sa, pats)
    reps = 107                                    # 535,000 queries
    buf, off = _pack_patterns(pats)
    big_off = np.concatenate([off[:-1].astype(np.int64) + k * buf.size for k in range(reps)] + [[reps * buf.size]])
    for mode in MODES:
        glo, ghi = find_patterns(t, sa, (np.tile(buf, reps), big_off), mode=mode)
        assert (glo == np.tile(lo, reps)).all() and (ghi == np.tile(hi, reps)).all(), mode


@pytest.mark.parametrize("L", [511, 512, 513, 1023, 1025, 70_000])
def test_find_long_patterns(gpu, oracle, L):
    """A random block planted three times in a filler (the construction of
    test_lcp_long_repeats): the 512-byte steps of the wave kernel on both
    sides of their boundaries."""
    from hpc_suffix_array_amd import find_patterns
    rng = np.random.default_rng(7 + L)
    blk = rng.integers(97, 101, size=L, dtype=np.uint8)
    filler = rng.integers(97, 101, size=3 * L + 11, dtype=np.uint8)
    t = np.ascontiguousarray(np.concatenate([filler[:L // 2 + 3], blk, filler[L // 2 + 3:], blk, filler[:5], blk]))
    sa = oracle.sa_c(t)
    b = bytes(blk)
    pats = [b, b[:-1], b[:-1] + bytes([b[-1] ^ 1]), bytes([b[0] ^ 1]) + b[1:], b[1:], b + b"a", b + b"z"]
    lo, hi = ref_intervals(bytes(t), sa, pats)
    assert hi[0] - lo[0] == 3
    for mode in ("wave", "auto", "lane"):
        glo, ghi = find_patterns(t, sa, pats, mode=mode)
        assert (glo == lo).all() and (ghi == hi).all(), mode


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [9, 4097, 1 << 20])
def test_find_one_symbol(gpu, n, mode):
    """SA = n-1 .. 0; a^k occupies [k - 1, n), and [n, n) when k > n: every
    probe shares its whole length with the pattern, the case the l / r
    skipping and the wave kernel exist for."""
    from hpc_suffix_array_amd import find_patterns
    t = np.full(n, ord("a"), np.uint8)
    sa = np.arange(n - 1, -1, -1, dtype=np.uint32)
    ks = [1, 2, 8, 9, 511, 513, n - 1, n, n + 1]
    lo, hi = find_patterns(t, sa, [b"a" * k for k in ks], mode=mode)
    assert lo.tolist() == [k - 1 if k <= n else n for k in ks]
    assert hi.tolist() == [n] * len(ks)
    lo, hi = find_patterns(t, sa, [b"b", b"a" * 20 + b"b", b"A", b"a" * 20 + b"A"], mode=mode)
    assert lo.tolist() == hi.tolist() == [n, n, 0, min(20, n)]


@pytest.mark.parametrize("mode", MODES)
def test_find_periodic(gpu, oracle, mode):
    from hpc_suffix_array_amd import find_patterns
    unit = b"abaababa"
    t = np.tile(np.frombuffer(unit, np.uint8), 40_000)
    sa = oracle.sa_c(t)
    pats = []
    for k in (1, 3, 100, 10_000):
        p = unit * k
        pats += [p, p[:len(p) // 2] + b"c" + p[len(p) // 2 + 1:], p[:len(p) // 2] + b"A" + p[len(p) // 2 + 1:], p[3:]]
    lo, hi = ref_intervals(bytes(t), sa, pats)
    assert hi[12] - lo[12] == len(occurrences(bytes(t), pats[12])) >= 30_001
    glo, ghi = find_patterns(t, sa, pats, mode=mode)
    assert (glo == lo).all() and (ghi == hi).all()


def test_find_device_path(gpu, oracle):
    """DeviceBuilder.find on torch tensors: text and pattern buffer at odd
    addresses, a non-default stream, no host wait inside the call."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder
    from hpc_suffix_array_amd.builder import _pack_patterns
    c = case(oracle, "alnum", 65537)
    n = 65537
    buf, off = _pack_patterns(c["pats"])
    nq = len(c["pats"])
    d_tbuf = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    d_tbuf[1:] = torch.from_numpy(c["text"]).cuda()
    d_text = d_tbuf[1:]
    d_pbuf = torch.zeros(buf.size + 1, dtype=torch.uint8, device="cuda")
    d_pbuf[1:] = torch.from_numpy(buf).cuda()
    d_pat = d_pbuf[1:]
    assert d_text.data_ptr() % 2 == 1 and d_pat.data_ptr() % 2 == 1
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    b = DeviceBuilder(n)
    b.build(d_text, n, d_sa)
    torch.cuda.synchronize()
    assert (d_sa.cpu().numpy().view(np.uint32) == c["sa"]).all()
    stream = torch.cuda.Stream()
    for mode in MODES:
        d_lo = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
        d_hi = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        before = gpu.lib().sa_host_syncs()
        with torch.cuda.stream(stream):
            b.find(d_text, n, d_sa, d_pat, int(buf.size), d_off, nq, d_lo, d_hi, stream=stream.cuda_stream, mode=mode)
        assert gpu.lib().sa_host_syncs() == before
        stream.synchronize()
        assert (d_lo.cpu().numpy().view(np.uint32) == c["lo"]).all(), mode
        assert (d_hi.cpu().numpy().view(np.uint32) == c["hi"]).all(), mode
    b.close()


def test_find_argument_errors(gpu):
    from hpc_suffix_array_amd import SAError, find_patterns
    L = gpu.lib()
    t = np.frombuffer(b"banana", np.uint8)
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    lo, hi = find_patterns(t, sa, [b"ana", b"nab", b""])
    assert lo.tolist() == [1, 5, 0] and hi.tolist() == [3, 5, 6]
    with pytest.raises(SAError):
        find_patterns(t, sa, (b"anana", np.array([0, 4, 3], np.int64)))     # decreasing offsets
    wide = sa.astype(np.int64)
    wide[2] = 6
    with pytest.raises(SAError):
        find_patterns(t, wide, [b"ana"])                                     # width-8 entry >= n
    out = np.zeros(2, np.uint64)
    rc = L.sa_find(t.ctypes.data, 6, sa.ctypes.data, 3, t.ctypes.data, np.array([0, 3], np.uint64).ctypes.data, 1,
                   out.ctypes.data, out.ctypes.data + 8)
    assert rc == -1 and b"sa_width" in L.sa_last_error()
    with pytest.raises(SAError):
        gpu.check(rc, "sa_find")
    lo, hi = find_patterns(t, sa, [])                                        # nq = 0
    assert lo.size == 0 and hi.size == 0 and lo.dtype == np.int64
    lo, hi = find_patterns(np.zeros(0, np.uint8), np.zeros(0, np.uint32), [b"", b"a"])   # n = 0
    assert lo.tolist() == [0, 0] and hi.tolist() == [0, 0]
