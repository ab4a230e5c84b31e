"""The longest previous factor array and the LZ77 factorisation on the GPU
(sa_lpf / sa_lpf_device / sa_lz77 / sa_lz77_device, hpc_suffix_array_amd/csrc/
sa_lz.h) against oracles written here, which use nothing of the library's LPF
or parse code:

    (A) the definition in O(n^2) numpy for n <= 1,500: run[i, j] = the bytes
        text[i:] and text[j:] share, built row by row from the bottom;
        LPF[i] = max over j < i of run[i, j].
    (B) a sequential two-stack pass over the SA and the LCP array in pure
        Python: the canonical (LPF, SRC) of include/sa_hip.h, asserted equal
        to (A) wherever (A) runs; the phrases by the serial walk over it.
    (C) properties for the large n: src < i, the match holds and is maximal at
        src, LPF[i + 1] >= LPF[i] - 1, and decoding the phrases gives the text.

LPF, SRC and the phrase triples are compared exactly.  No kernel of sa_lz.h
runs a persistent grid over the tiles (one workgroup per tile of 4096), so the
size "just above one sweep" is one with more tiles than the device has compute
units: 2^20 + 3, checked with (C) only.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD32 = np.uint32(0xA5A5A5A5)
PAD = 8
NONE = 0xFFFFFFFF
TILE = 4096
SMALL = [1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1]
LEVEL2 = [64 * 4096 - 1, 64 * 4096 + 1, 64 * 4096 + 5]


def as_u8(x):
    return np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8)


# ---- texts -----------------------------------------------------------------

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
    if kind == "a_b":                       # a^(n-1) b: an ascending SA
        t = np.full(n, ord("a"), np.uint8)
        t[-1] = ord("b")
        return t
    if kind == "b_a":                       # b a^(n-1)
        t = np.full(n, ord("a"), np.uint8)
        t[0] = ord("b")
        return t
    if kind == "sawtooth":                  # (a^k b)^j
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
    if kind == "rr":                        # R + R: one copy of n / 2
        r = rng.integers(0, 256, (n + 1) // 2).astype(np.uint8)
        return np.concatenate([r, r])[:n]
    raise ValueError(kind)


KINDS = ["dna", "two", "byte256", "one", "a_b", "b_a", "sawtooth", "period3", "period7", "fibonacci", "ascending",
         "descending", "rr"]


# ---- oracles ---------------------------------------------------------------

def lpf_by_definition(t):
    """(A): LPF by the run matrix."""
    n = t.size
    lpf = np.zeros(n, np.int64)
    below = np.zeros(n + 1, np.int32)           # run[i + 1, :], with a zero column at n
    for i in range(n - 1, -1, -1):
        row = np.zeros(n + 1, np.int32)
        row[:n] = np.where(t == t[i], below[1:] + 1, 0)
        if i:
            lpf[i] = row[:i].max()
        below = row
    return lpf


def lpf_two_stacks(sa, lcp):
    """(B): the canonical (LPF, SRC), -1 for none, in text order."""
    s, l = [int(x) for x in sa], [int(x) for x in lcp]
    n = len(s)
    la, va, lb, vb = [0] * n, [-1] * n, [0] * n, [-1] * n
    st = []
    for r in range(n):                          # a: the nearest rank below r with a smaller entry
        v, m = s[r], l[r]
        while st and st[-1][0] > v:
            m = min(m, st.pop()[1])
        if st:
            la[r], va[r] = m, st[-1][0]
        st.append((v, m))
    st = []
    for r in range(n - 1, -1, -1):              # b: the nearest rank above r with a smaller entry
        v = s[r]
        m = l[r + 1] if r + 1 < n else 0
        while st and st[-1][0] > v:
            m = min(m, st.pop()[1])
        if st:
            lb[r], vb[r] = m, st[-1][0]
        st.append((v, m))
    lpf, src = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for r in range(n):
        i = s[r]
        lpf[i] = max(la[r], lb[r])
        src[i] = va[r] if la[r] >= lb[r] and la[r] > 0 else (vb[r] if lb[r] > 0 else -1)
    return lpf, src


def serial_parse(lpf, src):
    n = len(lpf)
    pos, ln, sr = [], [], []
    i = 0
    lp, sc = lpf.tolist(), src.tolist()
    while i < n:
        k = max(1, lp[i])
        pos.append(i)
        ln.append(k)
        sr.append(sc[i] if lp[i] else -1)
        i += k
    return np.array(pos, np.int64), np.array(ln, np.int64), np.array(sr, np.int64)


def decode(t, pos, ln, src):
    """The text from its phrases; a literal's byte is the text's own."""
    out = np.zeros(t.size, np.uint8)
    for p, k, s in zip(pos.tolist(), ln.tolist(), src.tolist()):
        if s < 0:
            out[p] = t[p]
        elif s + k <= p:
            out[p:p + k] = out[s:s + k]
        else:                                   # the copy runs into the phrase itself: period p - s
            d = p - s
            reps = -(-k // d)
            out[p:p + k] = np.tile(out[s:p], reps)[:k]
    return out


def check_properties(t, lpf, src, phrases):
    """(C)."""
    n = t.size
    i = np.arange(n)
    has = lpf > 0
    assert ((src == -1) == ~has).all() and lpf[0] == 0
    assert (src[has] < i[has]).all() and (src[has] >= 0).all() and (i + lpf <= n).all()
    assert (lpf[1:] >= lpf[:-1] - 1).all()
    # the match holds (checked at up to 64 offsets spread over each match, its first and last byte
    # among them) and is maximal at src
    for f in np.linspace(0.0, 1.0, 64):
        k = np.floor(f * (lpf[has] - 1)).astype(np.int64)
        assert (t[src[has] + k] == t[i[has] + k]).all()
    end = has & (i + lpf < n)
    assert (t[src[end] + lpf[end]] != t[i[end] + lpf[end]]).all()
    pos, ln, sr = phrases
    assert pos[0] == 0 and (pos[1:] == pos[:-1] + ln[:-1]).all() and pos[-1] + ln[-1] == n
    assert (ln == np.maximum(1, lpf[pos])).all() and (sr == src[pos]).all()
    assert np.array_equal(decode(t, pos, ln, sr), t)


_CASE = {}


def case(kind, n):
    """Text, SA and LCP (the library's builder and LCP, checked against the
    oracle by the parity tests) and the oracle's answers: made once, never
    changed."""
    from hpc_suffix_array_amd import build_suffix_array, lcp_array
    key = (kind, n)
    if key not in _CASE:
        t = np.ascontiguousarray(make_text(kind, n))
        sa = np.ascontiguousarray(build_suffix_array(t), np.uint32)
        lcp = np.ascontiguousarray(lcp_array(t, sa)[0], np.uint32)
        lpf, src = lpf_two_stacks(sa, lcp)
        if n <= 1500:
            assert np.array_equal(lpf, lpf_by_definition(t)), key
            has = lpf > 0
            assert (src[has] < np.arange(n)[has]).all(), key
        c = dict(t=t, sa=sa, lcp=lcp, lpf=lpf, src=src, phrases=serial_parse(lpf, src))
        for v in c.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
        _CASE[key] = c
    return _CASE[key]


def host_check(c):
    from hpc_suffix_array_amd import longest_previous_factor, lz77_factorize
    lpf, src = longest_previous_factor(c["t"], c["sa"])
    assert lpf.dtype == src.dtype == np.int64
    assert np.array_equal(lpf, c["lpf"]) and np.array_equal(src, c["src"])
    got = lz77_factorize(c["t"], c["sa"])
    assert len(got[0]) == len(c["phrases"][0])                      # z against the serial walk
    for g, w in zip(got, c["phrases"]):
        assert g.dtype == np.int64 and np.array_equal(g, w)


# ---- the host forms over the texts and the sizes ---------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_texts_small_sizes(gpu, kind):
    for n in SMALL:
        host_check(case(kind, n))


def test_definition_at_1500(gpu):
    for kind in ("dna", "two", "period7", "rr"):
        host_check(case(kind, 1500))


@pytest.mark.parametrize("kind,n", [("dna", LEVEL2[0]), ("dna", LEVEL2[1]), ("dna", LEVEL2[2]), ("one", LEVEL2[0]),
                                    ("a_b", LEVEL2[1]), ("sawtooth", LEVEL2[2]), ("rr", LEVEL2[1]),
                                    ("fibonacci", LEVEL2[2]), ("b_a", LEVEL2[0])])
def test_second_global_level(gpu, kind, n):
    c = case(kind, n)
    host_check(c)
    check_properties(c["t"], c["lpf"], c["src"], c["phrases"])      # the oracle itself passes (C)


def test_known_answers(gpu):
    from hpc_suffix_array_amd import longest_previous_factor, lz77_factorize
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    lpf, src = longest_previous_factor(b"banana", sa)
    assert lpf.tolist() == [0, 0, 0, 3, 2, 1] and src.tolist() == [-1, -1, -1, 1, 2, 3]
    pos, ln, sr = lz77_factorize(b"banana", sa)
    assert pos.tolist() == [0, 1, 2, 3] and ln.tolist() == [1, 1, 1, 3] and sr.tolist() == [-1, -1, -1, 1]
    c = case("one", 4097)
    assert c["lpf"].tolist() == [0] + list(range(4096, 0, -1)) and len(c["phrases"][0]) == 2
    c = case("a_b", 4097)
    assert len(c["phrases"][0]) == 3 and c["phrases"][1].tolist() == [1, 4095, 1]
    assert len(case("ascending", 4097)["phrases"][0]) == 256 + 1


def test_more_tiles_than_compute_units(gpu):
    from hpc_suffix_array_amd import build_suffix_array, longest_previous_factor, lz77_factorize
    n = (1 << 20) + 3
    t = make_text("dna", n)
    sa = build_suffix_array(t)
    lpf, src = longest_previous_factor(t, sa)
    phrases = lz77_factorize(t, sa)
    check_properties(t, lpf, src, phrases)
    assert n // 12 < len(phrases[0]) < n // 6                       # phrases of about log4(n) bytes


def test_lcp_given_and_computed_agree(gpu):
    from hpc_suffix_array_amd import longest_previous_factor, lz77_factorize
    for kind, n in (("dna", 4097), ("sawtooth", 2 * 4096 + 1), ("one", 4096), ("fibonacci", 65)):
        c = case(kind, n)
        lpf, src = longest_previous_factor(c["t"], c["sa"], lcp=c["lcp"])
        assert np.array_equal(lpf, c["lpf"]) and np.array_equal(src, c["src"])
        for g, w in zip(lz77_factorize(c["t"], c["sa"], lcp=c["lcp"]), c["phrases"]):
            assert np.array_equal(g, w)


def test_width_8(gpu):
    from hpc_suffix_array_amd import longest_previous_factor, lz77_factorize
    import ctypes
    c = case("dna", 4097)
    sa8 = c["sa"].astype(np.int64)
    lpf, src = longest_previous_factor(c["t"], sa8)
    assert np.array_equal(lpf, c["lpf"]) and np.array_equal(src, c["src"])
    for g, w in zip(lz77_factorize(c["t"], sa8), c["phrases"]):
        assert np.array_equal(g, w)
    # "none" is all ones in the C arrays themselves
    L = gpu.lib()
    n = 4097
    a, b = np.zeros(n, np.int64), np.zeros(n, np.int64)
    assert L.sa_lpf(c["t"].ctypes.data, n, sa8.ctypes.data, 8, a.ctypes.data, b.ctypes.data) == 0
    assert np.array_equal(a, c["lpf"]) and np.array_equal(b, c["src"]) and (b == -1).any()
    # the sizing call of the host form: out_cap = 0 and NULL outputs
    z = ctypes.c_uint64(0)
    assert L.sa_lz77(c["t"].ctypes.data, n, sa8.ctypes.data, 8, None, None, None, 0, ctypes.byref(z)) == 0
    assert z.value == len(c["phrases"][0])
    # outputs too short: z is reported, nothing is written
    p, q, r = (np.full(4, 99, np.int64) for _ in range(3))
    z.value = 0
    assert L.sa_lz77(c["t"].ctypes.data, n, sa8.ctypes.data, 8, p.ctypes.data, q.ctypes.data, r.ctypes.data, 3,
                     ctypes.byref(z)) == 0
    assert z.value == len(c["phrases"][0]) and (p == 99).all() and (q == 99).all() and (r == 99).all()
    # an SA that is not the text's is rejected by the host forms
    bad = c["sa"].copy()
    bad[[10, 11]] = bad[[11, 10]]
    assert L.sa_lpf(c["t"].ctypes.data, n, bad.ctypes.data, 4, a.ctypes.data, b.ctypes.data) == -1
    assert b"not a valid suffix array" in L.sa_last_error()


# ---- the device forms ------------------------------------------------------

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


def none_as_minus_one(a):
    a = a.copy()
    a[a == NONE] = -1
    return a


def dev_lz(b, c, shift=0, stream=None, with_lcp=True):
    """LPF and the two-call parse through the device forms with guard words
    around every output; the host waits are counted.  Returns (lpf, src,
    pos, len, fsrc) as int64 with -1 for none."""
    import torch
    L = b.L
    n = c["t"].size
    d_t, d_sa, d_lcp = to_dev(c["t"]), to_dev(c["sa"]), to_dev(c["lcp"])
    lpf_buf, d_lpf = guarded(n, shift)
    src_buf, d_src = guarded(n, (shift + 1) % 4)
    torch.cuda.synchronize()
    s = None if stream is None else stream.cuda_stream
    w0 = L.sa_host_syncs()
    if with_lcp:
        b.lpf(None, n, d_sa, d_lcp, d_lpf, d_src, stream=s)         # the text is not needed
        assert L.sa_host_syncs() - w0 == 0                          # the header: none with d_lcp given
    else:
        b.lpf(d_t, n, d_sa, None, d_lpf, d_src, stream=s)
        assert L.sa_host_syncs() - w0 >= 1                          # sa_lcp_device's own
    w0 = L.sa_host_syncs()
    z = b.lz77(n, d_lpf, d_src, None, None, None, 0, stream=s)      # the sizing call
    assert L.sa_host_syncs() - w0 == 3                              # the header: three
    bufs, views = zip(*(guarded(z, (shift + k) % 4) for k in range(3)))
    torch.cuda.synchronize()
    if z > 1:
        assert b.lz77(n, d_lpf, d_src, *views, z - 1, stream=s) == z
        torch.cuda.synchronize()
        for x in bufs:
            assert (x.cpu().numpy().view(np.uint32) == GUARD32).all(), "out_cap below z wrote output"
    w0 = L.sa_host_syncs()
    assert b.lz77(n, d_lpf, d_src, *views, z, stream=s) == z
    assert L.sa_host_syncs() - w0 == 3
    torch.cuda.synchronize()
    lpf = unguard(lpf_buf, n, shift)
    src = none_as_minus_one(unguard(src_buf, n, (shift + 1) % 4))
    outs = [unguard(x, z, (shift + k) % 4) for k, x in enumerate(bufs)]
    return lpf, src, outs[0], outs[1], none_as_minus_one(outs[2])


def dev_check(got, c):
    assert np.array_equal(got[0], c["lpf"]) and np.array_equal(got[1], c["src"])
    for g, w in zip(got[2:], c["phrases"]):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_form(builder, shift):
    import torch
    st = torch.cuda.Stream()
    kinds = [("dna", 4097), ("sawtooth", 2 * 4096 + 1), ("a_b", 4097), ("two", 4095)]
    c = case(*kinds[shift])
    dev_check(dev_lz(builder, c, shift=shift, stream=st), c)
    c = case("rr", 2 * 4096 + 1)                                    # on the same stream
    dev_check(dev_lz(builder, c, shift=shift, stream=st, with_lcp=False), c)


def test_device_form_second_level_and_repeats(builder):
    c = case("dna", LEVEL2[2])
    a = dev_lz(builder, c)
    dev_check(a, c)
    b = dev_lz(builder, c, with_lcp=False)                          # d_lcp given and d_lcp = NULL agree
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = case("a_b", LEVEL2[1])                                      # every right walk runs to the last rank
    a, b = dev_lz(builder, c), dev_lz(builder, c)                   # two equal calls
    dev_check(a, c)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_device_form_edges(builder):
    import torch
    from hpc_suffix_array_amd import SAError
    # n == 1: LPF = [0], SRC = [none], one literal
    d_sa = to_dev(np.zeros(1, np.uint32))
    d_lcp = to_dev(np.zeros(1, np.uint32))
    out = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    builder.lpf(None, 1, d_sa, d_lcp, out[0:1], out[1:2])
    assert builder.lz77(1, out[0:1], out[1:2], out[2:3], out[3:4], out[4:5], 1) == 1
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == [0, NONE, 0, 1, NONE, 7, 7, 7]
    # n == 0: no kernel, z = 0
    w0 = builder.L.sa_host_syncs()
    builder.lpf(None, 0, None, None, None, None)
    assert builder.lz77(0, None, None, None, None, None, 0) == 0
    assert builder.L.sa_host_syncs() == w0
    # an output that is not 4-byte aligned is rejected; the dword offsets 0 .. 3 are test_device_form's
    c = case("dna", 65)
    d_sa, d_lcp = to_dev(c["sa"]), to_dev(c["lcp"])
    buf = torch.zeros(4 * 70, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(65, dtype=torch.int32, device="cuda")
    with pytest.raises(SAError, match="4-byte aligned"):
        builder.lpf(None, 65, d_sa, d_lcp, buf.data_ptr() + 2, ok)
    with pytest.raises(SAError, match="4-byte aligned"):
        builder.lz77(65, d_sa, d_lcp, ok, buf.data_ptr() + 1, buf.data_ptr() + 140, 65)
    # an arbitrary d_lpf terminates and stays inside the buffers (guards), whatever it says
    rng = np.random.default_rng(5)
    n = 3 * TILE + 17
    lp = rng.integers(0, 40, n).astype(np.uint32)
    lp[rng.integers(0, n, 50)] = NONE
    d_lp, d_sr = to_dev(lp), to_dev(np.zeros(n, np.uint32))
    z = builder.lz77(n, d_lp, d_sr, None, None, None, 0)
    assert 0 < z <= n
    bufs, views = zip(*(guarded(z, k) for k in range(3)))
    assert builder.lz77(n, d_lp, d_sr, *views, z) == z
    pos, ln = unguard(bufs[0], z, 0), unguard(bufs[1], z, 1)
    unguard(bufs[2], z, 2)
    assert pos[0] == 0 and (pos[1:] == pos[:-1] + ln[:-1]).all() and pos[-1] + ln[-1] == n


def test_more_candidates_than_one_sweep_of_the_grid(builder):
    """The candidate kernels run a capped grid of 8 workgroups per compute
    unit with a stride loop.  LPF = 4096 everywhere makes every position from
    4096 on the exit of the one a tile before it, so nearly every position is
    a candidate: more than 8 * 256 * 256 of them, a second sweep of the loop,
    and 20 reach rounds along a path of 160 tiles."""
    n = 160 * TILE + 5
    cands = n - TILE + 1                                            # position 0 and the exits 4096 .. n - 1
    assert cands > 8 * 256 * 256
    lp = np.full(n, TILE, np.uint32)
    sr = (np.arange(n, dtype=np.int64) * 7 % 1000).astype(np.uint32)
    d_lp, d_sr = to_dev(lp), to_dev(sr)
    z = builder.lz77(n, d_lp, d_sr, None, None, None, 0)
    assert z == 161
    bufs, views = zip(*(guarded(z, k) for k in range(3)))
    assert builder.lz77(n, d_lp, d_sr, *views, z) == z
    pos, ln, fs = (unguard(x, z, k) for k, x in enumerate(bufs))
    want = np.arange(z, dtype=np.int64) * TILE
    assert np.array_equal(pos, want) and np.array_equal(ln, np.minimum(TILE, n - want))
    assert np.array_equal(fs, sr[want].astype(np.int64))


def test_suffix_array_object(gpu, golden):
    from hpc_suffix_array_amd import SuffixArray
    names = sorted(golden["cases"], key=lambda k: golden["cases"][k]["n"])
    names = [k for k in names if 8 <= golden["cases"][k]["n"] <= 5000][:2]
    assert len(names) == 2
    for name in names:
        g = golden["cases"][name]
        t = as_u8(g["text"])
        lpf, src = lpf_two_stacks(g["sa"], g["lcp"])                # the fixture's own SA and LCP
        if t.size <= 1500:
            assert np.array_equal(lpf, lpf_by_definition(t)), name
        with SuffixArray(t.tobytes()) as s:
            s.build()
            got_lpf, got_src = s.lpf()
            got = s.lz77()
        assert np.array_equal(got_lpf, lpf) and np.array_equal(got_src, src), name
        for a, w in zip(got, serial_parse(lpf, src)):
            assert np.array_equal(a, w), name
