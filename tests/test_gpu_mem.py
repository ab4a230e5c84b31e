"""Maximal exact matches on the GPU (sa_mems / sa_mems_device,
hpc_suffix_array_amd/csrc/sa_mem.h) against a brute force written here, which
uses nothing of the library's search code:

    run[i, p] = the bytes query[i:] and text[p:] share, built row by row from
    the bottom with numpy; the MEMs are the (i, p) with run >= L that cannot be
    extended to the left; max_occ through a Counter of the text's L-mers.

The triples, the CSR offsets and the info words are compared exactly, in the
three modes (auto, lane, wave) unless stated.  The device cases go through
DeviceBuilder.mems with 0xA5 guard words around the outputs, the two-call
pattern and outputs at a chosen dword offset of their allocation.
"""
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ["auto", "lane", "wave"]
GUARD32 = np.uint32(0xA5A5A5A5)
GUARD64 = np.uint64(0xA5A5A5A5A5A5A5A5)
PAD = 8


def as_u8(x):
    return np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8)


def brute_mems(text, query, L, max_occ=0):
    """(qpos, tpos, length) sorted by (qpos, tpos), the CSR offsets, and the
    info words [total, candidates, skipped], by the definition."""
    t, q = as_u8(text), as_u8(query)
    n, m = t.size, q.size
    off = np.zeros(m + 1, np.int64)
    empty = np.zeros(0, np.int64)
    if n == 0 or m == 0 or L > min(n, m):
        return (empty, empty, empty), off, [0, 0, 0]
    run = np.zeros((m + 1, n + 1), np.int32)
    for i in range(m - 1, -1, -1):
        run[i, :n] = np.where(t == q[i], run[i + 1, 1:] + 1, 0)
    run = run[:m, :n]
    seed = run >= L                               # (i, p): the seed of i occurs at p
    occ = seed.sum(axis=1)
    tb = t.tobytes()
    lmers = Counter(tb[p:p + L] for p in range(n - L + 1))
    qb = q.tobytes()
    for i in range(0, m - L + 1, max(1, (m - L + 1) // 50)):   # the Counter and the matrix agree
        assert lmers.get(qb[i:i + L], 0) == occ[i]
    drop = np.array([bool(max_occ) and i + L <= m and lmers.get(qb[i:i + L], 0) > max_occ for i in range(m)])
    seed[drop] = False
    left = np.zeros((m, n), bool)                 # extendable to the left
    left[1:, 1:] = q[:-1, None] == t[None, :-1]
    mem = seed & ~left
    qpos, tpos = np.nonzero(mem)                  # row-major: sorted by (i, p)
    length = run[qpos, tpos].astype(np.int64)
    off[1:] = np.cumsum(mem.sum(axis=1))
    return (qpos.astype(np.int64), tpos.astype(np.int64), length), off, [int(qpos.size), int(seed.sum()), int(drop.sum())]


_SA = {}


def sa_of(text):
    """The text's suffix array by the library's builder (checked against the
    oracle by the parity tests): built once per text, never changed."""
    from hpc_suffix_array_amd import build_suffix_array
    t = as_u8(text)
    key = t.tobytes()
    if key not in _SA:
        a = np.ascontiguousarray(build_suffix_array(t), np.uint32)
        a.setflags(write=False)
        _SA[key] = a
    return _SA[key]


def host_check(text, query, L, max_occ=0, modes=MODES, want=None, sa=None):
    from hpc_suffix_array_amd import maximal_exact_matches
    t, q = as_u8(text), as_u8(query)
    sa = sa_of(t) if sa is None else sa
    want = brute_mems(t, q, L, max_occ) if want is None else want
    (wq, wt, wl), woff, winfo = want
    for mode in modes:
        gq, gt, gl, info = maximal_exact_matches(t, sa, q, L, max_occ=max_occ, mode=mode, return_info=True)
        assert gq.dtype == gt.dtype == gl.dtype == np.int64
        assert [info["total"], info["candidates"], info["skipped"]] == winfo, mode
        assert np.array_equal(info["offsets"], woff), mode
        assert np.array_equal(gq, wq) and np.array_equal(gt, wt), mode
        assert np.array_equal(gl, wl), mode
    return want


def dna_case():
    rng = np.random.default_rng(4099)
    t = rng.integers(0, 4, 4099).astype(np.uint8)
    t = np.frombuffer(b"ACGT", np.uint8)[t]
    q = np.concatenate([t[1000:1700], t[3100:3900]]).copy()
    for k in range(17, q.size, 37):
        q[k] = ord("A") if q[k] != ord("A") else ord("C")
    return t, q


# ---- texts -----------------------------------------------------------------

@pytest.mark.parametrize("L", [4, 8, 12])
def test_random_dna(gpu, L):
    t, q = dna_case()
    want = host_check(t, q, L)
    total, cands, _ = want[2]
    assert 0 < total < cands                       # the left check drops some, and something stays
    if L == 4:
        assert cands > 3 * 2048                    # the candidate list crosses tiles
    else:
        assert total * 5 < cands                   # nearly every candidate fails the left check


def test_one_symbol(gpu):
    from hpc_suffix_array_amd import SAError, maximal_exact_matches
    t, q, L = b"a" * 300, b"a" * 200, 3
    (wq, wt, wl), woff, winfo = host_check(t, q, L)
    n, m = 300, 200
    assert winfo == [495, 59_004, 0] and 495 == (m - L + 1) + (n - L + 1) - 1
    assert ((wq + wl == m) | (wt + wl == n)).all()           # every MEM ends at an end of a string
    assert host_check(t, q, L, max_occ=64)[2] == [0, 0, 198]
    assert host_check(t, q, L, max_occ=298)[2] == [495, 59_004, 0]
    sa = sa_of(t)
    for mode in MODES:
        with pytest.raises(SAError, match="59004"):
            maximal_exact_matches(t, sa, q, L, max_candidates=59_003, mode=mode)
        out = maximal_exact_matches(t, sa, q, L, max_candidates=59_004, mode=mode)
        assert np.array_equal(out[0], wq) and np.array_equal(out[1], wt) and np.array_equal(out[2], wl)


def test_too_many_fills_the_info_words(gpu):
    import ctypes
    L = gpu.lib()
    t, q = as_u8(b"a" * 300), as_u8(b"a" * 200)
    sa = sa_of(t)
    off = np.full(201, 99, np.uint64)
    info = (ctypes.c_uint64 * 3)(7, 7, 7)
    rc = L.sa_mems(t.ctypes.data, 300, sa.ctypes.data, 4, q.ctypes.data, 200, 3, 0, 59_003, 0, off.ctypes.data, None,
                   None, 0, info)
    assert rc == gpu.MEM_TOO_MANY == 1
    assert list(info) == [0, 59_004, 0] and (off == 0).all()


def test_position_above_the_locate_tile(gpu):
    t, q = b"a" * 5000, b"a" * 40
    assert 4997 > gpu.LOCATE_TILE
    want = host_check(t, q, 4)
    assert want[2] == [5033, 184_889, 0]


def test_more_than_one_sweep_of_the_grid(gpu):
    """About 3.0 M candidates are more tiles of 2048 than the persistent
    grid's 4 x 256 workgroups."""
    t, q = b"a" * 3000, b"a" * 1000
    want = host_check(t, q, 2, modes=["auto"])
    assert want[2][1] == 999 * 2999 > 4 * 256 * 2048


def test_periodic(gpu):
    t = b"abc" * 700 + b"abd"
    q = b"bcabcabd" + b"abc" * 60
    want = host_check(t, q, 5)
    assert want[2][0] == 1458 and want[0][2].max() == 180 and want[2][1] == 125_182


PLANTED = [7, 8, 9, 15, 16, 17, 24, 63, 64, 65, 511, 512, 513, 519, 520, 521, 1031]


def planted_case():
    """Random bytes with common blocks of the planted lengths, each with
    distinct bytes just before and after on both sides, at varying offsets
    mod 8 in the text and in the query."""
    rng = np.random.default_rng(6000)
    t = rng.integers(0, 256, 6000).astype(np.uint8)
    q = rng.integers(0, 256, 5000).astype(np.uint8)
    tp, qp = 3, 5
    for k, ln in enumerate(PLANTED):
        tp += (k * 3) % 8 + 2
        qp += (k * 5) % 8 + 2
        block = rng.integers(0, 256, ln).astype(np.uint8)
        t[tp:tp + ln] = block
        q[qp:qp + ln] = block
        for a, b in ((tp - 1, qp - 1), (tp + ln, qp + ln)):       # the bytes around differ
            if t[a] == q[b]:
                q[b] ^= 0x55
        tp += ln + 1
        qp += ln + 1
    assert tp < 6000 and qp < 5000
    return t, q


def test_planted_lengths(gpu):
    t, q = planted_case()
    (wq, wt, wl), woff, winfo = host_check(t, q, 8)
    assert winfo[0] > 0
    assert set(PLANTED[1:]) <= set(wl.tolist()) and 7 not in wl.tolist()


def test_ends_and_bytes(gpu):
    rng = np.random.default_rng(77)
    body = rng.integers(0, 256, 400).astype(np.uint8)
    block = rng.integers(0, 256, 40).astype(np.uint8)
    # a block that runs to the last byte of T but not of Q, and the reverse; MEMs at i == 0 and at p == 0
    t = np.concatenate([block[:11], body[:200], block])
    q = np.concatenate([block[:13], body[200:300], block, body[300:310], block[:11]])
    want = host_check(t, q, 6)
    (wq, wt, wl) = want[0]
    assert ((wt + wl == t.size) & (wq + wl < q.size)).any() and ((wq + wl == q.size) & (wt + wl < t.size)).any()
    assert ((wq == 0) & (wt == 0)).any() and (wq == 0).any() and (wt == 0).any()
    host_check(q, t, 6)
    # 0x00 and 0xFF are ordinary bytes
    z = np.frombuffer(b"\x00\xff\x00\x00\xff\xff\x00" * 30 + b"\xff", np.uint8)
    w = np.frombuffer(b"\xff\x00\x00\xff\x00" * 20, np.uint8)
    assert host_check(z, w, 3)[2][0] > 0
    # one byte on either side
    assert host_check(b"a", b"a", 1)[2] == [1, 1, 0]
    assert host_check(b"a", b"b", 1)[2] == [0, 0, 0]
    assert host_check(b"abcab", b"b", 1)[2][0] == 2
    assert host_check(b"b", b"abcab", 1)[2][0] == 2
    # L = 1 on four symbols
    t4 = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 200)]
    q4 = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)]
    assert host_check(t4, q4, 1)[2][0] > 1000
    # L = min(n, m) and one more
    assert host_check(t4, t4[20:50], 30)[2][0] >= 1
    assert host_check(t4, t4[20:50], 31)[2] == [0, 0, 0]
    assert host_check(t4[20:50], t4, 30)[2][0] >= 1
    assert host_check(t4[20:50], t4, 31)[2] == [0, 0, 0]


# ---- the device form -------------------------------------------------------

@pytest.fixture(scope="module")
def builder(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder(1 << 16)
    yield b
    b.close()


def to_dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def dev_mems(b, t, sa, q, L, shift=0, stream=None, mode="auto", max_occ=0):
    """The two-call device pattern with guard words: the sizing call, a call
    with out_cap one below the total (nothing written), the exact call.
    Returns (off, tpos, len) as int64 and the info triple."""
    import torch
    n, m = t.size, q.size
    d_t, d_sa, d_q = to_dev(t), to_dev(sa), to_dev(q)
    offbuf = torch.from_numpy(np.full(m + 1 + 2 * PAD, GUARD64, np.uint64).view(np.int64)).cuda()
    d_off = offbuf[PAD:PAD + m + 1]
    torch.cuda.synchronize()
    s = None if stream is None else stream.cuda_stream
    kw = dict(max_occ=max_occ, mode=mode, stream=s)
    info = b.mems(d_t, n, d_sa, d_q, m, L, d_off, None, None, 0, **kw)
    total = info[0]
    sized = offbuf.cpu().numpy().view(np.uint64)[PAD:PAD + m + 1].astype(np.int64)
    bufs = [torch.from_numpy(np.full(total + 2 * PAD + 4, GUARD32, np.uint32).view(np.int32)).cuda() for _ in range(2)]
    d_tp, d_ln = (x[PAD + shift:PAD + shift + max(total, 1)] for x in bufs)
    assert (d_tp.data_ptr() // 4) % 4 == (PAD + shift) % 4
    torch.cuda.synchronize()
    if total:
        assert b.mems(d_t, n, d_sa, d_q, m, L, d_off, d_tp, d_ln, total - 1, **kw) == info
        torch.cuda.synchronize()
        for x in bufs:
            assert (x.cpu().numpy().view(np.uint32) == GUARD32).all(), "out_cap below the total wrote output"
    assert b.mems(d_t, n, d_sa, d_q, m, L, d_off, d_tp, d_ln, total, **kw) == info
    torch.cuda.synchronize()
    ob = offbuf.cpu().numpy().view(np.uint64)
    assert (ob[:PAD] == GUARD64).all() and (ob[PAD + m + 1:] == GUARD64).all(), "guard around d_off"
    outs = []
    for x in bufs:
        pb = x.cpu().numpy().view(np.uint32)
        assert (pb[:PAD + shift] == GUARD32).all() and (pb[PAD + shift + total:] == GUARD32).all(), "guard around outputs"
        outs.append(pb[PAD + shift:PAD + shift + total].astype(np.int64))
    off = ob[PAD:PAD + m + 1].astype(np.int64)
    assert np.array_equal(off, sized)              # the sizing call fills d_off
    return off, outs[0], outs[1], list(info)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_form(builder, shift):
    import torch
    t, q = planted_case()
    sa = sa_of(t)
    (wq, wt, wl), woff, winfo = brute_mems(t, q, 8)
    st = torch.cuda.Stream()
    mode = MODES[shift % 3]
    off, tp, ln, info = dev_mems(builder, t, sa, q, 8, shift=shift, stream=st, mode=mode)
    assert info == winfo and np.array_equal(off, woff)
    assert np.array_equal(tp, wt) and np.array_equal(ln, wl)
    # a periodic text on the same stream: long extensions, many survivors per tile
    t2 = as_u8(b"abc" * 700 + b"abd")
    q2 = as_u8(b"bcabcabd" + b"abc" * 60)
    (wq, wt, wl), woff, winfo = brute_mems(t2, q2, 5)
    off, tp, ln, info = dev_mems(builder, t2, sa_of(t2), q2, 5, shift=shift, stream=st, mode=mode, max_occ=0)
    assert info == winfo and np.array_equal(off, woff) and np.array_equal(tp, wt) and np.array_equal(ln, wl)


def test_device_form_repeats_and_edges(builder):
    import torch
    t, q = dna_case()
    sa = sa_of(t)
    a = dev_mems(builder, t, sa, q, 8)
    b = dev_mems(builder, t, sa, q, 8)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # no kernel: L > min(n, m); d_off is zeroed, info is zero
    d_t, d_sa, d_q = to_dev(t), to_dev(sa), to_dev(q[:5])
    d_off = torch.full((6,), 7, dtype=torch.int64, device="cuda")
    assert builder.mems(d_t, t.size, d_sa, d_q, 5, 6, d_off, None, None, 0) == (0, 0, 0)
    assert d_off.cpu().numpy().tolist() == [0] * 6
    # max_candidates through the device form
    from hpc_suffix_array_amd import SAError
    d_off = torch.zeros(q.size + 1, dtype=torch.int64, device="cuda")
    cands = a[3][1]
    with pytest.raises(SAError, match=str(cands)):
        builder.mems(d_t, t.size, d_sa, to_dev(q), q.size, 8, d_off, None, None, 0, max_candidates=cands - 1)
    assert builder.mems(d_t, t.size, d_sa, to_dev(q), q.size, 8, d_off, None, None, 0, max_candidates=cands)[1] == cands


def test_width_8_host_form(gpu):
    from hpc_suffix_array_amd import maximal_exact_matches
    t, q = dna_case()
    (wq, wt, wl), woff, winfo = brute_mems(t, q, 12)
    gq, gt, gl = maximal_exact_matches(t, sa_of(t).astype(np.int64), q, 12)
    assert np.array_equal(gq, wq) and np.array_equal(gt, wt) and np.array_equal(gl, wl)


def test_agrees_with_the_parts(gpu):
    """The candidates are the hits that matching_statistics with max_len = L
    and locate_intervals give for the positions whose longest match is L."""
    from hpc_suffix_array_amd import locate_intervals, matching_statistics, maximal_exact_matches
    t, q = dna_case()
    sa = sa_of(t)
    for L, max_occ in ((8, 0), (4, 20)):
        ln, lo, hi = matching_statistics(t, sa, q, max_len=L)
        keep = (ln == L) & ((hi - lo <= max_occ) | (max_occ == 0))
        off, pos = locate_intervals(sa, lo[keep], hi[keep])
        info = maximal_exact_matches(t, sa, q, L, max_occ=max_occ, return_info=True)[3]
        assert info["candidates"] == int(off[-1]) == pos.size
        assert info["skipped"] == int(((ln == L) & ~keep).sum())


def test_suffix_array_object(gpu, golden):
    from hpc_suffix_array_amd import SuffixArray
    names = sorted(golden["cases"], key=lambda k: golden["cases"][k]["n"])
    names = [k for k in names if 8 <= golden["cases"][k]["n"] <= 5000][:2]
    assert len(names) == 2
    for name in names:
        t = as_u8(golden["cases"][name]["text"])
        n = t.size
        q = np.concatenate([t[n // 3:n // 3 + min(300, n // 2)], t[:min(200, n // 2)]]).copy()
        q[q.size // 2] ^= 1
        L = 3
        want = brute_mems(t, q, L)
        with SuffixArray(t.tobytes()) as s:
            s.build()
            gq, gt, gl = s.mems(q, L)
        assert want[2][0] > 0, name
        assert np.array_equal(gq, want[0][0]) and np.array_equal(gt, want[0][1]) and np.array_equal(gl, want[0][2]), name
