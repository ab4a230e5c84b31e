"""The repeats of a text as SA intervals on the GPU (sa_repeats /
sa_repeats_device, hpc_suffix_array_amd/csrc/sa_repeats.h) against oracles
written here, which use nothing of the library's repeat code:

    (A) the substring dictionary for n <= 200 (and the two sup texts): every
        substring with its occurrences, its followers (the end of the text is
        one) and its preceders (the start of the text is one).  Right-maximal:
        two occurrences and two followers; maximal: two preceders as well;
        supermaximal: maximal and no proper substring of another maximal
        repeat.
    (B) one bottom-up stack pass over the SA and the LCP array in pure Python:
        the LCP intervals with their heads, left-maximal by a count of symbol
        changes, supermaximal by "no child interval and pairwise distinct
        preceding symbols"; sorted by head, asserted equal to (A) wherever (A)
        runs.
    (C) (len, lo, hi) of each kind is compared exactly.

Sizes: the smallest at which a tile edge or a level of the hierarchy changes
(a tile is 4096 ranks, a level is 64 times the one below).  Every kernel of
sa_repeats.h runs one workgroup per tile, none a capped grid; 2^20 + 3 has
more tiles (257) than the device has compute units, so a second wave of
workgroups reads what the first wrote.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD32 = np.uint32(0xA5A5A5A5)
PAD = 8
TILE = 4096
START, END = 256, 256                           # no byte: in front of the text, behind it
REP_KINDS = ("right", "maximal", "supermaximal")
SMALL = [0, 1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1]
LEVEL2 = [64 * 4096 - 1, 64 * 4096 + 1, 64 * 4096 + 5]
LEVEL2_KINDS = ["dna", "one", "a_b", "sawtooth", "rr", "fibonacci"]


def as_u8(x):
    return np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8)


# ---- texts: the thirteen kinds of test_gpu_lz.py, and four of this file's ----

def fibonacci(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def make_text(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "dna":
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
    if kind == "two":
        return np.frombuffer(b"\x00\xff", np.uint8)[rng.integers(0, 2, n)]      # 0x00 and 0xFF present
    if kind == "byte256":
        return rng.integers(0, 256, n).astype(np.uint8)
    if kind == "one":
        return np.full(n, ord("a"), np.uint8)
    if kind in ("a_b", "b_a"):                  # a^(n-1) b: an ascending LCP array; b a^(n-1)
        t = np.full(n, ord("a"), np.uint8)
        if n:
            t[-1 if kind == "a_b" else 0] = ord("b")
        return t
    if kind == "sawtooth":                      # (a^9 b)^j
        t = np.full(n, ord("a"), np.uint8)
        t[9::10] = ord("b")
        return t
    if kind == "period3":
        return as_u8((b"abc" * (n // 3 + 1))[:n])
    if kind == "period7":
        return as_u8((b"abacabd" * (n // 7 + 1))[:n])
    if kind == "fibonacci":
        return as_u8(fibonacci(n))
    if kind == "ascending":
        return (np.arange(n) % 256).astype(np.uint8)
    if kind == "descending":
        return (255 - np.arange(n) % 256).astype(np.uint8)
    if kind == "rr":                            # R + R: one copy of n / 2
        r = rng.integers(0, 256, (n + 1) // 2).astype(np.uint8)
        return np.concatenate([r, r])[:n]
    raise ValueError(kind)


LZ_KINDS = ["dna", "two", "byte256", "one", "a_b", "b_a", "sawtooth", "period3", "period7", "fibonacci", "ascending",
            "descending", "rr"]
SUP257 = b"ab" + b"".join(bytes([c]) + b"ab" for c in range(256))
SUP258 = SUP257 + b"\x07ab"
# in front of them, filler over two bytes that sort below "ab" (its last byte sorts above): the interval
# of "ab" moves up by the filler's length and straddles rank 4096
FILLER = np.random.default_rng(77).integers(1, 3, 3899).astype(np.uint8).tobytes() + b"\xfe"
SPECIAL = {"sup257": SUP257, "sup258": SUP258, "sup257_edge": FILLER + SUP257, "sup258_edge": FILLER + SUP258}
KINDS = LZ_KINDS + ["sup257", "sup258"]


# ---- oracles ---------------------------------------------------------------

def by_dictionary(t, sa, lcp):
    """(A): {kind: [(len, lo, hi)] sorted by head} and {(len, lo, hi): the
    sorted occurrences}."""
    n = len(t)
    raw = bytes(t)
    rank = {int(p): r for r, p in enumerate(sa)}
    longest = int(max(lcp)) if n else 0             # a longer substring occurs once
    d = {}
    for i in range(n):
        for k in range(1, min(longest, n - i) + 1):
            e = d.setdefault(raw[i:i + k], ([], set(), set()))
            e[0].append(i)
            e[1].add(raw[i + k] if i + k < n else END)
            e[2].add(raw[i - 1] if i else START)
    maximal = [w for w, e in d.items() if len(e[0]) >= 2 and len(e[1]) >= 2 and len(e[2]) >= 2]
    inside, todo = set(), list(maximal)
    while todo:                                     # every proper substring of a maximal repeat
        w = todo.pop()
        for s in (w[1:], w[:-1]):
            if s and s not in inside:
                inside.add(s)
                todo.append(s)
    rows = {k: [] for k in REP_KINDS}
    occ = {}
    for w, e in d.items():
        if len(e[0]) < 2 or len(e[1]) < 2:
            continue
        lo = min(rank[i] for i in e[0])
        hi = lo + len(e[0])
        assert sorted(rank[i] for i in e[0]) == list(range(lo, hi))
        head = min(k for k in range(lo + 1, hi) if lcp[k] == len(w))
        row = (head, len(w), lo, hi)
        occ[row[1:]] = sorted(e[0])
        rows["right"].append(row)
        if len(e[2]) >= 2:
            rows["maximal"].append(row)
            if w not in inside:
                rows["supermaximal"].append(row)
    return {k: [r[1:] for r in sorted(v)] for k, v in rows.items()}, occ


def by_stack(t, sa, lcp):
    """(B): {kind: (len, lo, hi) int64 arrays, sorted by head}."""
    n = len(t)
    empty = {k: tuple(np.zeros(0, np.int64) for _ in range(3)) for k in REP_KINDS}
    if n < 2:
        return empty
    s = np.asarray(sa, np.int64)
    prev = np.where(s > 0, np.asarray(t, np.int64)[np.maximum(s, 1) - 1], START)
    changes = np.concatenate([[0], np.cumsum(prev[1:] != prev[:-1])])   # changes[k]: symbol changes at ranks <= k
    l = [int(x) for x in lcp] + [0]
    l[0] = 0
    out = []                                        # (head, len, lo, hi, has a child interval)
    st = [[0, 0, 0, False]]                         # lcp, lb, head, child
    for k in range(1, n + 1):
        v, lb = l[k], k - 1
        child = False
        while st[-1][0] > v:
            x = st.pop()
            out.append((x[2], x[0], x[1], k, x[3]))
            lb = x[1]
            if st[-1][0] >= v:
                st[-1][3] = True
            else:
                child = True
        if st[-1][0] < v:
            st.append([v, lb, k, child])
    out.sort()
    rows = {k: [] for k in REP_KINDS}
    pl = prev.tolist()
    for head, ln, lo, hi, child in out:
        row = (ln, lo, hi)
        rows["right"].append(row)
        if changes[hi - 1] != changes[lo]:
            rows["maximal"].append(row)
            if not child and hi - lo <= 257 and len(set(pl[lo:hi])) == hi - lo:
                rows["supermaximal"].append(row)
    return {k: tuple(np.array([r[j] for r in v], np.int64) for j in range(3)) for k, v in rows.items()}


def filtered(want, min_len, min_occ):
    ln, lo, hi = want
    keep = (ln >= max(min_len, 1)) & (hi - lo >= max(min_occ, 2))
    return ln[keep], lo[keep], hi[keep]


_CASE = {}


def case(kind, n=None):
    """Text, SA and LCP (the library's builder and LCP, checked against the
    oracle by the parity tests) and the oracles' answers: made once, never
    changed."""
    from hpc_suffix_array_amd import build_suffix_array, lcp_array
    key = (kind, n)
    if key not in _CASE:
        t = np.ascontiguousarray(as_u8(SPECIAL[kind]) if kind in SPECIAL else make_text(kind, n))
        m = t.size
        sa = np.ascontiguousarray(build_suffix_array(t), np.uint32) if m else np.zeros(0, np.uint32)
        lcp = np.ascontiguousarray(lcp_array(t, sa)[0], np.uint32) if m else np.zeros(0, np.uint32)
        want = by_stack(t, sa, lcp)
        c = dict(t=t, sa=sa, lcp=lcp, want=want, occ=None)
        if 2 <= m <= 200 or kind in ("sup257", "sup258"):
            a, c["occ"] = by_dictionary(t, sa, lcp)
            for k in REP_KINDS:
                assert a[k] == list(zip(*(x.tolist() for x in want[k]))), (key, k)
        for a in (t, sa, lcp) + tuple(x for v in want.values() for x in v):
            a.setflags(write=False)
        _CASE[key] = c
    return _CASE[key]


def same(got, want, what=None):
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), what


def host_check(c, what=None):
    from hpc_suffix_array_amd import maximal_repeats
    for k in REP_KINDS:
        same(maximal_repeats(c["t"], c["sa"], kind=k), c["want"][k], (what, k))


# ---- the host form over the texts and the sizes ----------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_texts_small_sizes(gpu, kind):
    if kind in SPECIAL:
        host_check(case(kind), kind)
        return
    for n in SMALL:
        host_check(case(kind, n), (kind, n))


def test_definition_at_200(gpu):
    for kind in ("dna", "two", "period7", "rr", "fibonacci", "sawtooth"):
        c = case(kind, 200)
        assert c["occ"] is not None
        host_check(c, kind)


@pytest.mark.parametrize("n", LEVEL2)
@pytest.mark.parametrize("kind", LEVEL2_KINDS)
def test_second_global_level(gpu, kind, n):
    host_check(case(kind, n), (kind, n))


def test_known_answers(gpu):
    from hpc_suffix_array_amd import maximal_repeats
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)                    # a, ana, anana, banana, na, nana
    ln, lo, hi = maximal_repeats(b"banana", sa, kind="right")
    assert list(zip(ln.tolist(), lo.tolist(), hi.tolist())) == [(1, 0, 3), (3, 1, 3), (2, 4, 6)]   # a, ana, na
    ln, lo, hi = maximal_repeats(b"banana", sa)
    assert list(zip(ln.tolist(), lo.tolist(), hi.tolist())) == [(1, 0, 3), (3, 1, 3)]              # na: always after a
    ln, lo, hi = maximal_repeats(b"banana", sa, kind="supermaximal")
    assert list(zip(ln.tolist(), lo.tolist(), hi.tolist())) == [(3, 1, 3)]
    # the largest supermaximal repeat there can be, and one occurrence more
    c = case("sup257")
    w = c["want"]["supermaximal"]
    assert (2, 98, 355) in list(zip(*(x.tolist() for x in w)))
    c8 = case("sup258")                                             # "\x07ab" sorts in front: one rank up
    assert (2, 99, 357) in list(zip(*(x.tolist() for x in c8["want"]["maximal"])))
    assert (2, 99, 357) not in list(zip(*(x.tolist() for x in c8["want"]["supermaximal"])))
    # a^n: a^1 .. a^(n - 1), nested; left-maximal by the start of the text alone; a^(n - 1) is supermaximal
    c = case("one", 4097)
    for k in ("right", "maximal"):
        ln, lo, hi = c["want"][k]
        assert ln.tolist() == list(range(1, 4097)) and lo.tolist() == list(range(4096)) and (hi == 4097).all()
    assert [x.tolist() for x in c["want"]["supermaximal"]] == [[4096], [4095], [4097]]


@pytest.mark.parametrize("kind", ["sup257_edge", "sup258_edge"])
def test_largest_interval_across_a_tile_edge(gpu, kind):
    c = case(kind)
    ln, lo, hi = c["want"]["maximal"]
    first = c["sa"][lo].astype(np.int64)
    ab = (ln == 2) & (c["t"][first] == ord("a")) & (c["t"][np.minimum(first + 1, c["t"].size - 1)] == ord("b"))
    assert ab.sum() == 1 and hi[ab][0] - lo[ab][0] == (257 if kind == "sup257_edge" else 258)
    assert lo[ab][0] < TILE < hi[ab][0]                             # over the edge
    assert not ((c["want"]["supermaximal"][2] - c["want"]["supermaximal"][1]) >= 257).any()   # the filler precedes one
    host_check(c, kind)


@pytest.mark.parametrize("kind", ["dna", "two"])
def test_more_tiles_than_compute_units(gpu, kind):
    c = case(kind, (1 << 20) + 3)
    host_check(c, kind)
    assert len(c["want"]["right"][0]) > (1 << 19)


@pytest.mark.parametrize("min_len", [1, 2, 8])
@pytest.mark.parametrize("min_occ", [2, 3, 300])
def test_filters(gpu, min_len, min_occ):
    from hpc_suffix_array_amd import maximal_repeats
    listed = 0
    for key in (("dna", 4097), ("one", 4097), ("sup258", None), ("two", 2 * 4096 + 1), ("sawtooth", 4096)):
        c = case(*key)
        for k in REP_KINDS:
            want = filtered(c["want"][k], min_len, min_occ)
            same(maximal_repeats(c["t"], c["sa"], min_len=min_len, min_occ=min_occ, kind=k), want, (key, k))
            listed += len(want[0])
    assert listed > 0
    # 0 reads as 1, and 0 and 1 as 2
    c = case("dna", 4097)
    for ml, mo in ((0, 0), (1, 1), (0, 2)):
        same(maximal_repeats(c["t"], c["sa"], min_len=ml, min_occ=mo), c["want"]["maximal"])


def test_lcp_given_and_computed_agree(gpu):
    from hpc_suffix_array_amd import maximal_repeats
    for kind, n in (("dna", 4097), ("sawtooth", 2 * 4096 + 1), ("one", 4096), ("fibonacci", 65), ("dna", 1)):
        c = case(kind, n)
        for k in REP_KINDS:
            same(maximal_repeats(c["t"], c["sa"], kind=k, lcp=c["lcp"]), c["want"][k], (kind, n, k))
    c = case("dna", 4097)
    same(maximal_repeats(c["t"], c["sa"], min_len=8, min_occ=3, lcp=c["lcp"]), filtered(c["want"]["maximal"], 8, 3))


def test_width_8(gpu):
    from hpc_suffix_array_amd import maximal_repeats
    c = case("dna", 4097)
    sa8 = c["sa"].astype(np.int64)
    for k in REP_KINDS:
        same(maximal_repeats(c["t"], sa8, kind=k), c["want"][k], k)
    L = gpu.lib()
    n = 4097
    want = c["want"]["maximal"]
    count, occ = len(want[0]), int((want[2] - want[1]).sum())
    # the C arrays themselves at width 8
    a, b, d = (np.zeros(n, np.int64) for _ in range(3))
    info = (ctypes.c_uint64 * 2)()
    assert L.sa_repeats(c["t"].ctypes.data, n, sa8.ctypes.data, 8, 1, 2, 1, a.ctypes.data, b.ctypes.data, d.ctypes.data,
                        n, info) == 0
    assert list(info) == [count, occ]
    same((a[:count], b[:count], d[:count]), want)
    # the sizing call of the host form: out_cap = 0 and NULL outputs
    info = (ctypes.c_uint64 * 2)()
    assert L.sa_repeats(c["t"].ctypes.data, n, sa8.ctypes.data, 8, 1, 2, 1, None, None, None, 0, info) == 0
    assert list(info) == [count, occ]
    # outputs too short: info is filled, nothing is written
    p, q, r = (np.full(4, 99, np.int64) for _ in range(3))
    info = (ctypes.c_uint64 * 2)()
    assert L.sa_repeats(c["t"].ctypes.data, n, sa8.ctypes.data, 8, 1, 2, 1, p.ctypes.data, q.ctypes.data, r.ctypes.data,
                        3, info) == 0
    assert list(info) == [count, occ] and (p == 99).all() and (q == 99).all() and (r == 99).all()
    # an SA that is not the text's is rejected by the host form
    bad = c["sa"].copy()
    bad[[10, 11]] = bad[[11, 10]]
    assert L.sa_repeats(c["t"].ctypes.data, n, bad.ctypes.data, 4, 1, 2, 1, None, None, None, 0, info) == -1
    assert b"not a valid suffix array" in L.sa_last_error()


# ---- the device form -------------------------------------------------------

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
    return torch.from_numpy(a.copy()).cuda()


def guarded(count, shift):
    """A device buffer of guard words and the `count` words at dword offset
    PAD + shift of it."""
    import torch
    buf = torch.from_numpy(np.full(count + 2 * PAD + 4, GUARD32, np.uint32).view(np.int32)).cuda()
    view = buf[PAD + shift:PAD + shift + max(count, 1)]
    assert (view.data_ptr() // 4) % 4 == (PAD + shift) % 4
    return buf, view


def unguard(buf, count, shift):
    pb = buf.cpu().numpy().view(np.uint32)
    assert (pb[:PAD + shift] == GUARD32).all() and (pb[PAD + shift + count:] == GUARD32).all(), "guard around outputs"
    return pb[PAD + shift:PAD + shift + count].astype(np.int64)


def dev_repeats(b, c, kind, shift=0, stream=None, with_lcp=True, min_len=1, min_occ=2, bare=False):
    """The sizing call, a call with a short out_cap and the writing call
    through the device form, with guard words around every output; the host
    waits are counted.  bare: SA_REP_RIGHT with neither the text nor the SA.
    Returns (len, lo, hi) as int64 and total_occ."""
    import torch
    L = b.L
    n = c["t"].size
    d_t, d_sa, d_lcp = to_dev(c["t"]), to_dev(c["sa"]), to_dev(c["lcp"])
    if bare:
        assert kind == "right" and with_lcp
        d_t = d_sa = None
    lcp_arg = d_lcp if with_lcp else None
    torch.cuda.synchronize()
    s = None if stream is None else stream.cuda_stream
    w0 = L.sa_host_syncs()
    count, occ = b.repeats(d_t, n, d_sa, lcp_arg, min_len, min_occ, kind, None, None, None, 0, stream=s)   # sizing
    if with_lcp:
        assert L.sa_host_syncs() - w0 == 1                          # the header: one
    else:
        assert L.sa_host_syncs() - w0 >= 2                          # sa_lcp_device's own, and that one
    bufs, views = zip(*(guarded(count, (shift + k) % 4) for k in range(3)))
    torch.cuda.synchronize()
    if count > 1:
        assert b.repeats(d_t, n, d_sa, lcp_arg, min_len, min_occ, kind, *views, count - 1, stream=s) == (count, occ)
        torch.cuda.synchronize()
        for x in bufs:
            assert (x.cpu().numpy().view(np.uint32) == GUARD32).all(), "out_cap below the count wrote output"
    w0 = L.sa_host_syncs()
    assert b.repeats(d_t, n, d_sa, lcp_arg, min_len, min_occ, kind, *views, count, stream=s) == (count, occ)
    if with_lcp:
        assert L.sa_host_syncs() - w0 == 1
    torch.cuda.synchronize()
    return tuple(unguard(x, count, (shift + k) % 4) for k, x in enumerate(bufs)), occ


def dev_check(got, want):
    same(got[0], want)
    assert got[1] == int((want[2] - want[1]).sum())                 # info[1]: locate's pos_cap


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_form(builder, shift):
    import torch
    st = torch.cuda.Stream()
    keys = [("dna", 4097), ("sawtooth", 2 * 4096 + 1), ("a_b", 4097), ("two", 4095)]
    c = case(*keys[shift])
    for k in REP_KINDS:
        dev_check(dev_repeats(builder, c, k, shift=shift, stream=st), c["want"][k])
    dev_check(dev_repeats(builder, c, "right", shift=shift, stream=st, bare=True), c["want"]["right"])
    c = case("rr", 2 * 4096 + 1)                                    # on the same stream
    for k in REP_KINDS:
        dev_check(dev_repeats(builder, c, k, shift=shift, stream=st, with_lcp=False), c["want"][k])
    dev_check(dev_repeats(builder, c, "maximal", shift=shift, stream=st, min_len=2, min_occ=3),
              filtered(c["want"]["maximal"], 2, 3))


def test_device_form_second_level_and_equal_calls(builder):
    c = case("dna", LEVEL2[2])
    for k in REP_KINDS:
        a = dev_repeats(builder, c, k)
        dev_check(a, c["want"][k])
        b = dev_repeats(builder, c, k, with_lcp=False)              # d_lcp given and d_lcp = NULL agree
        same(a[0], b[0])
        assert a[1] == b[1]
    c = case("a_b", LEVEL2[1])                                      # every right walk runs to the last rank
    a, b = dev_repeats(builder, c, "right", bare=True), dev_repeats(builder, c, "right", bare=True)   # two equal calls
    dev_check(a, c["want"]["right"])
    same(a[0], b[0])
    c = case("sup258_edge")
    for k in REP_KINDS:
        dev_check(dev_repeats(builder, c, k), c["want"][k])


def test_device_form_edges(builder):
    import torch
    from hpc_suffix_array_amd import SAError
    # n <= 1: a count of 0, no kernel, no wait, nothing written
    out = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    w0 = builder.L.sa_host_syncs()
    for n in (0, 1):
        for k in REP_KINDS:
            assert builder.repeats(None, n, None, None, 1, 2, k, out[0:1], out[1:2], out[2:3], 1) == (0, 0)
            assert builder.repeats(None, n, None, None, 1, 2, k, None, None, None, 0) == (0, 0)
    assert builder.L.sa_host_syncs() == w0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()
    # an output that is not 4-byte aligned is rejected; the dword offsets 0 .. 3 are test_device_form's
    c = case("dna", 65)
    d_t, d_sa, d_lcp = to_dev(c["t"]), to_dev(c["sa"]), to_dev(c["lcp"])
    buf = torch.zeros(4 * 70, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(65, dtype=torch.int32, device="cuda")
    with pytest.raises(SAError, match="4-byte aligned"):
        builder.repeats(d_t, 65, d_sa, d_lcp, 1, 2, "maximal", ok, buf.data_ptr() + 2, buf.data_ptr() + 140, 65)
    with pytest.raises(ValueError, match="unknown kind"):
        builder.repeats(d_t, 65, d_sa, d_lcp, 1, 2, "tandem", None, None, None, 0)
    # n == 2: one level above the entries
    for t2, want in ((b"aa", [(1, 0, 2)]), (b"ab", [])):
        sa2 = np.array([1, 0] if t2 == b"aa" else [0, 1], np.uint32)
        lcp2 = np.array([0, 1] if t2 == b"aa" else [0, 0], np.uint32)
        c2 = dict(t=as_u8(t2), sa=sa2, lcp=lcp2)
        for k in REP_KINDS:
            got, occ = dev_repeats(builder, c2, k)
            assert list(zip(*(x.tolist() for x in got))) == want and occ == 2 * len(want)


def test_arbitrary_lcp_and_sa_stay_inside_the_buffers(builder):
    """An LCP array that is no text's and an SA with entries >= n: the results
    are unspecified, but every walk ends, nothing is read or written outside
    the buffers (the guards around the outputs) and the count written fits."""
    import torch
    rng = np.random.default_rng(5)
    n = 3 * TILE + 17
    for round_ in range(2):
        lcp = rng.integers(0, 40, n).astype(np.uint32)
        lcp[rng.integers(0, n, 50)] = 0xFFFFFFFF
        if round_:
            lcp[0] = 0xFFFFFFFF                                     # entry 0 reads as 0 whatever it holds
        sa = rng.integers(0, n, n).astype(np.uint32)
        sa[rng.integers(0, n, 50)] = 0xFFFFFFFF
        sa[rng.integers(0, n, 50)] = n
        sa[rng.integers(0, n, 50)] = 0
        d_t, d_sa, d_lcp = to_dev(rng.integers(0, 256, n).astype(np.uint8)), to_dev(sa), to_dev(lcp)
        for k in REP_KINDS:
            count, occ = builder.repeats(d_t, n, d_sa, d_lcp, 1, 2, k, None, None, None, 0)
            assert 0 <= count < n
            bufs, views = zip(*(guarded(count, j) for j in range(3)))
            got = builder.repeats(d_t, n, d_sa, d_lcp, 1, 2, k, *views, count)
            torch.cuda.synchronize()
            assert got[0] <= count
            for j, x in enumerate(bufs):
                unguard(x, count, j)


# ---- composition -----------------------------------------------------------

def test_repeats_then_locate(gpu):
    """locate_intervals over (lo, hi) gives every occurrence of every repeat:
    the dictionary's occurrence lists."""
    from hpc_suffix_array_amd import locate_intervals, maximal_repeats
    for key in (("dna", 200), ("period7", 200), ("rr", 200), ("sup258", None)):
        c = case(*key)
        for k in REP_KINDS:
            ln, lo, hi = maximal_repeats(c["t"], c["sa"], kind=k)
            off, pos = locate_intervals(c["sa"], lo, hi)
            assert off[-1] == int((hi - lo).sum()) and len(ln) == len(c["want"][k][0])
            for q in range(len(ln)):
                assert pos[off[q]:off[q + 1]].tolist() == c["occ"][(int(ln[q]), int(lo[q]), int(hi[q]))], (key, k, q)


def test_device_repeats_then_device_locate(builder):
    """The two-call pattern in HBM: the repeats' d_lo and d_hi go to
    DeviceBuilder.locate as they are, with total_occ as its pos_cap."""
    import torch
    c = case("dna", 4097)
    n = 4097
    d_t, d_sa, d_lcp = to_dev(c["t"]), to_dev(c["sa"]), to_dev(c["lcp"])
    count, occ = builder.repeats(d_t, n, d_sa, d_lcp, 8, 2, "maximal", None, None, None, 0)
    d_len, d_lo, d_hi = (torch.empty(count, dtype=torch.int32, device="cuda") for _ in range(3))
    assert builder.repeats(d_t, n, d_sa, d_lcp, 8, 2, "maximal", d_len, d_lo, d_hi, count) == (count, occ)
    d_off = torch.empty(count + 1, dtype=torch.int64, device="cuda")
    d_pos = torch.empty(occ, dtype=torch.int32, device="cuda")
    assert builder.locate(n, d_sa, d_lo, d_hi, count, d_off, d_pos, occ) == occ
    torch.cuda.synchronize()
    ln, lo, hi = filtered(c["want"]["maximal"], 8, 2)
    off, pos = d_off.cpu().numpy(), d_pos.cpu().numpy().view(np.uint32).astype(np.int64)
    assert off[-1] == occ and count == len(ln)
    t = c["t"].tobytes()
    for q in range(count):
        p = pos[off[q]:off[q + 1]]
        assert p.tolist() == sorted(c["sa"][lo[q]:hi[q]].tolist())
        assert len({t[i:i + int(ln[q])] for i in p.tolist()}) == 1  # one string at all of them


def test_suffix_array_object(gpu, golden):
    from hpc_suffix_array_amd import SuffixArray
    names = sorted(golden["cases"], key=lambda k: golden["cases"][k]["n"])
    names = [k for k in names if 8 <= golden["cases"][k]["n"] <= 5000][:2]
    assert len(names) == 2
    for name in names:
        g = golden["cases"][name]
        t = as_u8(g["text"])
        want = by_stack(t, g["sa"], g["lcp"])                       # the fixture's own SA and LCP
        if t.size <= 200:
            a, _ = by_dictionary(t, g["sa"], g["lcp"])
            for k in REP_KINDS:
                assert a[k] == list(zip(*(x.tolist() for x in want[k]))), (name, k)
        with SuffixArray(t.tobytes()) as s:
            s.build()
            for k in REP_KINDS:
                same(s.repeats(kind=k), want[k], (name, k))
            same(s.repeats(), want["maximal"], name)
            same(s.repeats(min_len=3, min_occ=3, kind="right"), filtered(want["right"], 3, 3), name)
            # the longest right-maximal repeat is the longest repeated substring
            s.build_lcp()
            lrs = s.longest_repeated_substring()
            ln, lo, hi = s.repeats(kind="right")
            sa = s.sa
        if len(ln):
            top = np.flatnonzero(ln == ln.max())
            raw = t.tobytes()
            strings = {raw[int(sa[lo[q]]):int(sa[lo[q]]) + int(ln[q])] for q in top}
            if b"\x00" not in raw:
                assert lrs is not None and len(lrs) == int(ln.max()) and lrs in strings, name
        else:
            assert not lrs
