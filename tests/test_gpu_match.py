"""GPU longest-match queries and matching statistics over a built suffix
array (sa_match / sa_matching_stats and their _device forms,
hpc_suffix_array_amd/csrc/sa_match.h) against Python alone.

Expected values, independent of the SA: with tb = bytes(text), the length is
the largest l with tb.find(p[:l]) >= 0 -- presence of a prefix is monotone in
l, so a binary search over l finds it.  Expected interval: bisect_left /
bisect_right of p[:length] over the oracle's SA by the key
tb[sa[r]:sa[r] + length], as in test_gpu_find.py.  hi - lo must equal the
overlapping occurrence count of p[:length]: the two references check each
other.  Every case runs in the three modes (auto, lane, wave).
"""
import bisect

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ["auto", "lane", "wave"]
KINDS = ["dna", "alnum", "byte256", "binary"]


def ref_len(tb, p):
    lo, hi = 0, len(p)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if tb.find(p[:mid]) >= 0:
            lo = mid
        else:
            hi = mid - 1
    return lo


def ref_interval(tb, sal, p):
    n, m = len(tb), len(p)
    key = lambda r: tb[sal[r]:sal[r] + m]   # noqa: E731
    return bisect.bisect_left(range(n), p, key=key), bisect.bisect_right(range(n), p, key=key)


def occurrence_count(tb, p):
    """Overlapping occurrences of p in tb (bytes.find; a sliding numpy compare
    of the same bytes where a short pattern occurs very often)."""
    n, m = len(tb), len(p)
    if m == 0:
        return n
    if m > n:
        return 0
    if m <= 8 and tb.count(p) > 2000:
        a = np.frombuffer(tb, np.uint8)
        hit = np.ones(n - m + 1, bool)
        for j in range(m):
            hit &= a[j:n - m + 1 + j] == p[j]
        return int(hit.sum())
    c, i = 0, tb.find(p)
    while i >= 0:
        c += 1
        i = tb.find(p, i + 1)
    return c


def ref_matches(tb, sa, pats):
    """(length, lo, hi) int64 arrays of the patterns; the occurrence count of
    every distinct matched prefix is checked against hi - lo."""
    sal = np.asarray(sa).tolist()
    seen = {}
    out = []
    for p in pats:
        p = bytes(p)
        q = p[:ref_len(tb, p)]
        if q not in seen:
            lo, hi = ref_interval(tb, sal, q)
            assert hi - lo == occurrence_count(tb, q), q[:40]      # the two references agree
            assert len(q) == 0 or hi > lo
            seen[q] = (lo, hi)
        out.append((len(q),) + seen[q])
    return tuple(np.array([o[k] for o in out], np.int64) for k in range(3))


def lengths():
    from hpc_suffix_array_amd import _native as N
    T = N.FIND_LANE_MAX
    return [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, T - 1, T, T + 1]


SHORT = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33]


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


def assert_same(got, want, pats, what):
    for g, w, name in zip(got, want, ("length", "lo", "hi")):
        assert g.dtype == np.int64, (what, name)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, [(pats[i][:40], len(pats[i]), int(g[i]), int(w[i])) for i in bad[:5]])


_CASES = {}


def case(oracle, kind, n):
    """Text, oracle SA, 300 drawn + 7 fixed patterns and their expected
    (length, lo, hi): computed once, shared by the modes."""
    if (kind, n) not in _CASES:
        t = oracle.gen_text(kind, n, seed=7 * n + len(kind))
        tb = bytes(t)
        sa = oracle.sa_c(t)
        pats = draw_patterns(t, 300, seed=3 * n + len(kind))
        pats += [b"", tb[-5:], tb[-5:] + b"\x00", tb, tb + b"a", b"\x00", b"\xff" * 9]
        _CASES[(kind, n)] = dict(text=t, sa=sa, pats=pats, want=ref_matches(tb, sa, pats))
    return _CASES[(kind, n)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 9, 4095, 65537])
@pytest.mark.parametrize("kind", KINDS)
def test_match_vs_python(gpu, oracle, kind, n, mode):
    from hpc_suffix_array_amd import find_patterns, match_patterns
    c = case(oracle, kind, n)
    got = match_patterns(c["text"], c["sa"], c["pats"], mode=mode)
    assert_same(got, c["want"], c["pats"], (kind, n, mode))
    only = match_patterns(c["text"], c["sa"], c["pats"], mode=mode, bounds=False)
    assert isinstance(only, np.ndarray) and only.dtype == np.int64 and (only == c["want"][0]).all()
    # a pattern that occurs whole: exactly what find_patterns returns
    whole = np.flatnonzero(got[0] == np.array([len(p) for p in c["pats"]]))
    assert whole.size >= 3
    flo, fhi = find_patterns(c["text"], c["sa"], c["pats"], mode=mode)
    assert (got[1][whole] == flo[whole]).all() and (got[2][whole] == fhi[whole]).all()


def test_match_width8_and_offsets_pair(gpu, oracle):
    from hpc_suffix_array_amd import match_patterns
    from hpc_suffix_array_amd.builder import _pack_patterns
    c = case(oracle, "dna", 4095)
    assert_same(match_patterns(c["text"], c["sa"].astype(np.int64), c["pats"]), c["want"], c["pats"], "width 8")
    buf, off = _pack_patterns(c["pats"])
    shifted = (np.concatenate([np.zeros(3, np.uint8), buf]), off.astype(np.int64) + 3)
    assert_same(match_patterns(c["text"], c["sa"], shifted), c["want"], c["pats"], "offsets pair")


@pytest.mark.parametrize("B", [511, 512, 513, 1025])
def test_match_wave_steps(gpu, oracle, B):
    """A random block planted three times in a filler (the construction of
    test_find_long_patterns); the block with one byte changed on both sides of
    the wave kernel's 512-byte steps matches up to that byte, or further if
    the reference says so."""
    from hpc_suffix_array_amd import match_patterns
    rng = np.random.default_rng(7 + B)
    blk = rng.integers(97, 101, size=B, dtype=np.uint8)
    filler = rng.integers(97, 101, size=3 * B + 11, dtype=np.uint8)
    t = np.ascontiguousarray(np.concatenate([filler[:B // 2 + 3], blk, filler[B // 2 + 3:], blk, filler[:5], blk]))
    sa = oracle.sa_c(t)
    b = bytes(blk)
    js = [j for j in (0, 511, 512, 513, B - 1) if j < B]
    pats = [b[:j] + bytes([b[j] ^ 1]) + b[j + 1:] for j in js] + [b + b"z"]
    want = ref_matches(bytes(t), sa, pats)
    assert (want[0][:-1] >= np.array(js)).all() and want[0][-1] == B
    assert want[2][-1] - want[1][-1] == 3
    for mode in ("wave", "auto", "lane"):
        assert_same(match_patterns(t, sa, pats, mode=mode), want, pats, mode)
        assert (match_patterns(t, sa, pats, mode=mode, bounds=False) == want[0]).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [9, 4097])
def test_match_one_symbol(gpu, n, mode):
    """SA = n-1 .. 0; a^k matches min(k, n) bytes, at [min(k, n) - 1, n)."""
    from hpc_suffix_array_amd import match_patterns
    t = np.full(n, ord("a"), np.uint8)
    sa = np.arange(n - 1, -1, -1, dtype=np.uint32)
    ks = [1, 8, 9, 513, n, n + 1]
    ln, lo, hi = match_patterns(t, sa, [b"a" * k for k in ks], mode=mode)
    assert ln.tolist() == [min(k, n) for k in ks]
    assert lo.tolist() == [min(k, n) - 1 for k in ks]
    assert hi.tolist() == [n] * len(ks)
    ln, lo, hi = match_patterns(t, sa, [b"a" * 20 + b"b", b"b", b"a" * 20 + b"A"], mode=mode)
    w = min(20, n)
    assert ln.tolist() == [w, 0, w] and lo.tolist() == [w - 1, 0, w - 1] and hi.tolist() == [n, n, n]
    assert match_patterns(t, sa, [b"a" * k for k in ks], mode=mode, bounds=False).tolist() == [min(k, n) for k in ks]


@pytest.mark.parametrize("mode", MODES)
def test_match_periodic(gpu, oracle, mode):
    from hpc_suffix_array_amd import match_patterns
    unit = b"abaababa"
    t = np.tile(np.frombuffer(unit, np.uint8), 5000)
    c = _CASES.get("periodic")
    if c is None:
        sa = oracle.sa_c(t)
        pats = []
        for k in (1, 3, 100):
            p = unit * k
            pats += [p, p[:len(p) // 2] + b"c" + p[len(p) // 2 + 1:], p[:len(p) // 2] + b"A" + p[len(p) // 2 + 1:],
                     p[3:]]
        c = _CASES["periodic"] = dict(sa=sa, pats=pats, want=ref_matches(bytes(t), sa, pats))
    assert c["want"][0][9] == 400 and c["want"][0][8] == 800
    assert_same(match_patterns(t, c["sa"], c["pats"], mode=mode), c["want"], c["pats"], mode)
    assert (match_patterns(t, c["sa"], c["pats"], mode=mode, bounds=False) == c["want"][0]).all()


def shapes_case(oracle):
    """dna text of 65537 bytes, 5000 short patterns and their expected results."""
    if "shapes" not in _CASES:
        t = oracle.gen_text("dna", 65537, seed=11)
        sa = oracle.sa_c(t)
        pats = draw_patterns(t, 5000, seed=5000, lens=SHORT)
        _CASES["shapes"] = dict(text=t, sa=sa, pats=pats, want=ref_matches(bytes(t), sa, pats))
    return _CASES["shapes"]


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257])
def test_match_batch_shapes(gpu, oracle, nq):
    """Ragged waves and workgroups."""
    from hpc_suffix_array_amd import match_patterns
    c = shapes_case(oracle)
    pats = c["pats"][100:100 + nq]
    want = tuple(w[100:100 + nq] for w in c["want"])
    for mode in MODES:
        assert_same(match_patterns(c["text"], c["sa"], pats, mode=mode), want, pats, mode)
        assert (match_patterns(c["text"], c["sa"], pats, mode=mode, bounds=False) == want[0]).all()


def test_match_grid_stride(gpu, oracle):
    """More queries than one launch has lanes (2048 x 256) or wavefront
    slots (2048 x 4 x 8): 5000 checked patterns, repeated."""
    from hpc_suffix_array_amd import match_patterns
    from hpc_suffix_array_amd.builder import _pack_patterns
    c = shapes_case(oracle)
    reps = 107                                    # 535,000 queries
    buf, off = _pack_patterns(c["pats"])
    big_off = np.concatenate([off[:-1].astype(np.int64) + k * buf.size for k in range(reps)] + [[reps * buf.size]])
    big = (np.tile(buf, reps), big_off)
    for mode in MODES:
        got = match_patterns(c["text"], c["sa"], big, mode=mode)
        for g, w in zip(got, c["want"]):
            assert (g == np.tile(w, reps)).all(), mode
    assert (match_patterns(c["text"], c["sa"], big, bounds=False) == np.tile(c["want"][0], reps)).all()


def sliding_case(oracle, kind):
    """Text of 65537 bytes, a query of 2200 bytes (a 2000-byte slice of the
    text with a substitution about every 50 bytes, then 200 random bytes) and
    its matching statistics from Python."""
    key = ("sliding", kind)
    if key not in _CASES:
        n = 65537
        t = oracle.gen_text(kind, n, seed=3 * n + len(kind))
        tb = bytes(t)
        sa = oracle.sa_c(t)
        rng = np.random.default_rng(len(kind))
        q = bytearray(tb[30_000:32_000])
        i = int(rng.integers(50))
        while i < len(q):
            q[i] = int(t[rng.integers(n)]) ^ 1 if kind == "dna" else int(rng.integers(256))
            i += 40 + int(rng.integers(21))
        q = bytes(q) + rng.integers(0, 256, size=200, dtype=np.uint8).tobytes()
        ms = [ref_len(tb, q[i:]) for i in range(len(q))]
        assert all(ms[i + 1] >= ms[i] - 1 for i in range(len(q) - 1))     # the reference's own consistency
        assert max(ms) >= 40
        _CASES[key] = dict(text=t, tb=tb, sa=sa, sal=sa.tolist(), query=q, ms=ms, iv={})
    return _CASES[key]


def sliding_want(c, max_len):
    """Expected (length, lo, hi) per position: the uncapped length cut at the
    cap (presence of a prefix is monotone), the interval by bisect."""
    q, m = c["query"], len(c["query"])
    out = []
    for i in range(m):
        ln = min(c["ms"][i], max_len) if max_len else c["ms"][i]
        p = q[i:i + ln]
        if p not in c["iv"]:
            lo, hi = ref_interval(c["tb"], c["sal"], p)
            assert hi - lo == occurrence_count(c["tb"], p)
            c["iv"][p] = (lo, hi)
        out.append((ln,) + c["iv"][p])
    return tuple(np.array([o[k] for o in out], np.int64) for k in range(3))


@pytest.mark.parametrize("max_len", [0, 1, 8, 9, 64, 600])
@pytest.mark.parametrize("kind", ["dna", "byte256"])
def test_matching_statistics(gpu, oracle, kind, max_len):
    from hpc_suffix_array_amd import match_patterns, matching_statistics
    c = sliding_case(oracle, kind)
    q, m = c["query"], len(c["query"])
    want = sliding_want(c, max_len)
    slices = [q[i:i + max_len] if max_len else q[i:] for i in range(m)]
    for mode in MODES:
        got = matching_statistics(c["text"], c["sa"], q, max_len=max_len, mode=mode)
        assert_same(got, want, slices, (kind, max_len, mode))
        only = matching_statistics(c["text"], c["sa"], q, max_len=max_len, mode=mode, bounds=False)
        assert isinstance(only, np.ndarray) and only.dtype == np.int64 and (only == want[0]).all()
    # each position equals the batch form on the explicit slice
    assert_same(match_patterns(c["text"], c["sa"], slices), want, slices, "batch form on the slices")


@pytest.mark.parametrize("m", [1, 63, 65])
def test_matching_statistics_short_queries(gpu, oracle, m):
    from hpc_suffix_array_amd import matching_statistics
    c = sliding_case(oracle, "dna")
    q = c["query"][40:40 + m]
    sub = dict(c, query=q, ms=[ref_len(c["tb"], q[i:]) for i in range(m)])
    for max_len in (0, 5):
        want = sliding_want(sub, max_len)
        for mode in MODES:
            got = matching_statistics(c["text"], c["sa"].astype(np.int64), np.frombuffer(q, np.uint8), max_len=max_len,
                                      mode=mode)
            assert_same(got, want, [q[i:] for i in range(m)], (m, max_len, mode))
    ln, lo, hi = matching_statistics(c["text"], c["sa"], b"")
    assert ln.size == lo.size == hi.size == 0 and ln.dtype == np.int64
    assert matching_statistics(c["text"], c["sa"], b"", bounds=False).size == 0


def test_golden_longest_match(gpu, golden):
    """SuffixArray.longest_match over the object's own str and sa (the drop-in
    copy ends at the first NUL: those texts are left to match_patterns)."""
    from hpc_suffix_array_amd import SuffixArray
    ran = 0
    for name, c in golden["cases"].items():
        tb = bytes(c["text"])
        if 0 in tb or not tb:
            continue
        pats = draw_patterns(c["text"], 30, seed=len(name) + c["n"], lens=SHORT + [40, 100])
        pats += [tb[-3:] + b"\x01", tb + b"a"]
        want = ref_matches(tb, c["sa"], pats)
        with SuffixArray(tb) as s:
            s.build()
            for i, p in enumerate(pats):
                assert s.longest_match(p) == (want[0][i], want[1][i], want[2][i]), (name, p[:40])
            for mode in ("lane", "wave"):
                for i in range(0, len(pats), 8):
                    assert s.longest_match(pats[i], mode=mode) == (want[0][i], want[1][i], want[2][i]), (name, mode)
        ran += 1
    assert ran >= 1


def test_match_device_path(gpu, oracle):
    """DeviceBuilder.match / matching_statistics on torch tensors: text,
    pattern buffer and query at odd addresses, a non-default stream, no host
    wait inside the calls; lengths only with the two bounds left out."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder
    from hpc_suffix_array_amd.builder import _pack_patterns
    c = case(oracle, "alnum", 65537)
    n = 65537
    buf, off = _pack_patterns(c["pats"])
    nq = len(c["pats"])

    def odd(a):
        d = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
        d[1:] = torch.from_numpy(np.array(a)).cuda()
        assert d[1:].data_ptr() % 2 == 1
        return d[1:]

    d_text, d_pat = odd(c["text"]), odd(buf)
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_sa = torch.from_numpy(c["sa"].view(np.int32)).cuda()
    u32 = lambda d: d.cpu().numpy().view(np.uint32)   # noqa: E731
    b = DeviceBuilder(n)
    stream = torch.cuda.Stream()
    new = lambda k: torch.full((k,), -1, dtype=torch.int32, device="cuda")   # noqa: E731
    for mode in MODES:
        d_len, d_lo, d_hi, d_len2 = new(nq), new(nq), new(nq), new(nq)
        torch.cuda.synchronize()
        before = gpu.lib().sa_host_syncs()
        with torch.cuda.stream(stream):
            b.match(d_text, n, d_sa, d_pat, int(buf.size), d_off, nq, d_len, d_lo, d_hi, stream=stream.cuda_stream,
                    mode=mode)
        assert gpu.lib().sa_host_syncs() == before
        stream.synchronize()
        for d, w in zip((d_len, d_lo, d_hi), c["want"]):
            assert (u32(d) == w).all(), mode
        keep_lo, keep_hi = d_lo.clone(), d_hi.clone()
        with torch.cuda.stream(stream):
            b.match(d_text, n, d_sa, d_pat, int(buf.size), d_off, nq, d_len2, None, None, stream=stream.cuda_stream,
                    mode=mode)
        assert gpu.lib().sa_host_syncs() == before
        stream.synchronize()
        assert (u32(d_len2) == c["want"][0]).all(), mode
        assert torch.equal(d_lo, keep_lo) and torch.equal(d_hi, keep_hi)
    # the sliding form over the same text: its SA is the oracle's
    s = sliding_case(oracle, "dna")
    q = np.frombuffer(s["query"], np.uint8)
    m = q.size
    d_text2, d_q = odd(s["text"]), odd(q)
    d_sa2 = torch.from_numpy(s["sa"].view(np.int32)).cuda()
    for max_len in (0, 9):
        want = sliding_want(s, max_len)
        for mode in MODES:
            d_len, d_lo, d_hi, d_len2 = new(m), new(m), new(m), new(m)
            torch.cuda.synchronize()
            before = gpu.lib().sa_host_syncs()
            with torch.cuda.stream(stream):
                b.matching_statistics(d_text2, n, d_sa2, d_q, m, d_len, d_lo, d_hi, max_len=max_len,
                                      stream=stream.cuda_stream, mode=mode)
                b.matching_statistics(d_text2, n, d_sa2, d_q, m, d_len2, max_len=max_len, stream=stream.cuda_stream,
                                      mode=mode)
            assert gpu.lib().sa_host_syncs() == before
            stream.synchronize()
            for d, w in zip((d_len, d_lo, d_hi), want):
                assert (u32(d) == w).all(), (max_len, mode)
            assert (u32(d_len2) == want[0]).all(), (max_len, mode)
    b.close()


def test_match_argument_errors(gpu):
    from hpc_suffix_array_amd import SAError, match_patterns, matching_statistics
    t = np.frombuffer(b"banana", np.uint8)
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    ln, lo, hi = match_patterns(t, sa, [b"anab", b"nab", b"", b"x", b"banana!"])
    assert ln.tolist() == [3, 2, 0, 0, 6] and lo.tolist() == [1, 4, 0, 0, 3] and hi.tolist() == [3, 6, 6, 6, 4]
    ln, lo, hi = matching_statistics(t, sa, b"bandana")
    assert ln.tolist() == [3, 2, 1, 0, 3, 2, 1]
    assert lo.tolist() == [3, 1, 4, 0, 1, 4, 0] and hi.tolist() == [4, 3, 6, 6, 3, 6, 3]
    assert matching_statistics(t, sa, b"bandana", max_len=2, bounds=False).tolist() == [2, 2, 1, 0, 2, 2, 1]
    with pytest.raises(SAError):
        match_patterns(t, sa, (b"anana", np.array([0, 4, 3], np.int64)))     # decreasing offsets
    wide = sa.astype(np.int64)
    wide[2] = 6
    with pytest.raises(SAError):
        match_patterns(t, wide, [b"ana"])                                     # width-8 entry >= n
    with pytest.raises(SAError):
        matching_statistics(t, wide, b"ana")
    ln, lo, hi = match_patterns(t, sa, [])                                    # nq = 0
    assert ln.size == 0 and lo.size == 0 and hi.size == 0 and ln.dtype == np.int64
    ln, lo, hi = match_patterns(np.zeros(0, np.uint8), np.zeros(0, np.uint32), [b"", b"a"])   # n = 0
    assert ln.tolist() == [0, 0] and lo.tolist() == [0, 0] and hi.tolist() == [0, 0]
    ln, lo, hi = matching_statistics(np.zeros(0, np.uint8), np.zeros(0, np.uint32), b"ab")
    assert ln.tolist() == [0, 0] and lo.tolist() == [0, 0] and hi.tolist() == [0, 0]
