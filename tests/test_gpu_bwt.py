"""GPU Burrows-Wheeler transform and inverse suffix array of a built SA
(sa_bwt / sa_bwt_device / sa_inverse / sa_inverse_device,
hpc_suffix_array_amd/csrc/sa_bwt.h) against numpy alone.

Expected values, with t and sa numpy arrays (sa from the oracle up to 2^20
bytes, from the GPU build followed by check_suffix_array above that):
    bwt     = t[(sa - 1) % n]
    primary = flatnonzero(sa == 0)[0]
    runs    = 1 + count_nonzero(bwt[1:] != bwt[:-1])
    counts  = bincount(t, minlength=256)
    isa     = empty(n); isa[sa] = arange(n)
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def expected(t, sa):
    n = int(t.size)
    exp = t[(sa.astype(np.int64) - 1) % n]
    primary = int(np.flatnonzero(sa == 0)[0])
    runs = 1 + int(np.count_nonzero(exp[1:] != exp[:-1]))
    return exp, primary, runs, np.bincount(t, minlength=256).astype(np.int64)


def check_bwt(t, sa, what=""):
    """Both kernel instantiations through the host form, everything exact."""
    from hpc_suffix_array_amd import bwt
    exp, primary, runs, counts = expected(t, sa)
    b, p, r, c = bwt(t, sa, stats=True)
    assert b.dtype == np.uint8 and b.shape == exp.shape, what
    assert (b == exp).all(), what
    assert (p, r) == (primary, runs), what
    assert c.dtype == np.int64 and c.shape == (256,) and (c == counts).all(), what
    b, p = bwt(t, sa)
    assert (b == exp).all() and p == primary, what


@functools.lru_cache(maxsize=None)
def _text_sa(kind, n, seed):
    """(text, SA), computed once per module; read-only."""
    from oracle import oracle as O
    from hpc_suffix_array_amd import build_suffix_array, check_suffix_array
    t = O.gen_text(kind, n, seed=seed)
    if n <= 1 << 20:
        sa = O.sa_c(t).astype(np.uint32)
    else:
        sa = build_suffix_array(t)
        assert check_suffix_array(t, sa)
    t.setflags(write=False)
    sa.setflags(write=False)
    return t, sa


def test_golden(gpu, golden):
    from hpc_suffix_array_amd import SuffixArray
    for name, c in golden["cases"].items():
        t, sa = np.ascontiguousarray(c["text"], np.uint8), np.asarray(c["sa"])
        check_bwt(t, sa, name)
        if 0 not in bytes(t):
            exp, primary, _, _ = expected(t, sa)
            with SuffixArray(bytes(t)) as s:
                s.build()
                assert s.bwt() == (exp.tobytes(), primary), name


def test_convention_is_the_rotation_bwt(gpu, oracle):
    """A text that ends in a unique smallest byte: the bytes and the primary
    index are those of its sorted rotations."""
    from hpc_suffix_array_amd import bwt
    rng = np.random.default_rng(11)
    for n, hi in ((1, 2), (2, 2), (17, 3), (100, 5), (200, 256)):
        t = np.concatenate([rng.integers(1, hi, size=n - 1, dtype=np.uint8), np.zeros(1, np.uint8)])
        tb = bytes(t)
        rot = sorted(range(n), key=lambda i: tb[i:] + tb[:i])
        b, p = bwt(t, oracle.sa_c(t))
        assert bytes(b) == bytes(tb[i - 1] for i in rot)
        assert p == rot.index(0)


@pytest.mark.parametrize("kind", ["dna", "binary", "byte256"])
def test_tile_edges(gpu, oracle, kind):
    from hpc_suffix_array_amd import _native as N
    T = N.BWT_TILE
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3):
        t = oracle.gen_text(kind, n, seed=5 * n + len(kind))
        check_bwt(t, oracle.sa_c(t), f"{kind} n={n}")


def test_sweep_wrap(gpu):
    """The persistent grid is 8 workgroups per CU, each taking BWT_TILE ranks
    per iteration: one sweep of the grid covers 8 * CUs * BWT_TILE ranks
    (2^23 on the 256 CUs of an MI355X).  n lies one tile and a few ranks above
    that, so the first workgroups take a second tile and one of them a partial
    one."""
    import torch
    from hpc_suffix_array_amd import _native as N
    sweep = 8 * torch.cuda.get_device_properties(0).multi_processor_count * N.BWT_TILE
    n = sweep + N.BWT_TILE + 7
    assert n <= (1 << 24) + 5
    t, sa = _text_sa("dna", n, 21)
    check_bwt(t, sa)


def test_structured_texts(gpu, oracle):
    from hpc_suffix_array_amd import _native as N, bwt
    n = N.BWT_TILE + 1
    a, b = np.full(n, ord("a"), np.uint8), np.full(n, ord("b"), np.uint8)
    one = a
    out, p, r, _ = bwt(one, oracle.sa_c(one), stats=True)
    assert (r, p) == (1, n - 1) and (out == ord("a")).all()
    ab = b.copy()
    ab[0] = ord("a")
    assert bwt(ab, oracle.sa_c(ab))[1] == 0
    ba = a.copy()
    ba[0] = ord("b")
    assert bwt(ba, oracle.sa_c(ba))[1] == n - 1
    every = np.concatenate([np.arange(256, dtype=np.uint8), oracle.gen_text("byte256", n - 256, seed=8)])
    for t in (one, ab, ba, np.tile(np.frombuffer(b"ab", np.uint8), n // 2), every):
        check_bwt(t, oracle.sa_c(t))


def test_device_form_alignment_and_guards(gpu, oracle):
    """sa_bwt_device into a buffer of 0xA5 at byte offsets 0..3 from a 16-byte
    boundary: [0, n) exact, 32 bytes on either side untouched; on a stream of
    its own; the statistics of two calls in a row equal; d_stats=None."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    T = N.BWT_TILE
    bld = DeviceBuilder(1 << 16)
    stream = torch.cuda.Stream()
    for n in (1, 5, T + 1, T + 2, T + 3):
        t = oracle.gen_text("dna", n, seed=n)
        sa = oracle.sa_c(t).astype(np.uint32)
        exp, primary, runs, counts = expected(t, sa)
        want = np.concatenate([[primary, runs], counts]).astype(np.int64)
        d_text = torch.from_numpy(t).cuda()
        d_sa = torch.from_numpy(sa.view(np.int32).copy()).cuda()
        for off in range(4):
            buf = torch.full((32 + 3 + n + 32 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            lo = 32 + off
            d_stats = torch.full((N.BWT_STATS,), 123456789, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            bld.bwt(d_text, n, d_sa, buf.data_ptr() + lo, d_stats, stream=stream.cuda_stream)
            stream.synchronize()
            first = d_stats.cpu().numpy().copy()
            got = buf.cpu().numpy()
            assert (got[lo:lo + n] == exp).all(), (n, off)
            assert (got[:lo] == 0xA5).all() and (got[lo + n:] == 0xA5).all(), (n, off)
            assert (first == want).all(), (n, off)
            bld.bwt(d_text, n, d_sa, buf.data_ptr() + lo, d_stats, stream=stream.cuda_stream)
            stream.synchronize()
            assert (d_stats.cpu().numpy() == first).all(), (n, off)          # zeroed by the call, not doubled
            buf.fill_(0xA5)
            torch.cuda.synchronize()
            bld.bwt(d_text, n, d_sa, buf.data_ptr() + lo, None, stream=stream.cuda_stream)
            stream.synchronize()
            got = buf.cpu().numpy()
            assert (got[lo:lo + n] == exp).all(), (n, off)
            assert (got[:lo] == 0xA5).all() and (got[lo + n:] == 0xA5).all(), (n, off)
    bld.close()


def test_width_8(gpu, oracle):
    from hpc_suffix_array_amd import bwt
    t = oracle.gen_text("alnum", 70_001, seed=3)
    sa = oracle.sa_c(t)
    exp, primary, runs, counts = expected(t, sa)
    b, p, r, c = bwt(t, sa.astype(np.int64), stats=True)
    assert (b == exp).all() and (p, r) == (primary, runs) and (c == counts).all()
    b, p = bwt(t, sa.astype(np.int64))
    assert (b == exp).all() and p == primary


def test_invalid_sa_is_contained(gpu, oracle):
    """Entries >= n are clamped, never dereferenced: SA_OK, the primary index
    in [0, n], and every untouched rank has its byte."""
    from hpc_suffix_array_amd import bwt
    n = 1000
    t = oracle.gen_text("dna", n, seed=6)
    sa = oracle.sa_c(t).astype(np.uint32)
    exp = expected(t, sa)[0]
    bad = sa.copy()
    ranks = np.random.default_rng(2).choice(n, size=10, replace=False)
    bad[ranks] = np.array([n, n + 1, 0xFFFFFFFF] * 4, np.uint32)[:10]
    b, p, _, _ = bwt(t, bad, stats=True)
    keep = np.ones(n, bool)
    keep[ranks] = False
    assert (b[keep] == exp[keep]).all()
    assert 0 <= p <= n


INVERSE_SIZES = [1, 2, 3, (1 << 14) - 1, 1 << 14, (1 << 14) + 1, (1 << 20) + 3, (1 << 24) + 5]


@pytest.mark.parametrize("n", INVERSE_SIZES)
def test_inverse(gpu, n):
    """(2^24 + 5 engages the 8 level-1 stripes of the permutation.)"""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder, inverse_suffix_array
    t, sa = _text_sa("dna", n, 31)
    isa = inverse_suffix_array(sa)
    assert isa.dtype == np.uint32 and isa.shape == (n,)
    assert (isa[sa] == np.arange(n, dtype=np.uint32)).all()
    if n == (1 << 14) + 1:
        wide = inverse_suffix_array(sa.astype(np.int64), width=8)
        assert wide.dtype == np.int64 and (wide == isa).all()
    if n in ((1 << 14) + 1, (1 << 20) + 3):
        bld = DeviceBuilder(n)
        d_sa = torch.from_numpy(sa.view(np.int32).copy()).cuda()
        d_isa = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bld.inverse(n, d_sa, d_isa)
        got = d_isa.cpu().numpy()
        assert (got[:n].view(np.uint32) == isa).all()
        assert (got[n:] == -7).all()
        bld.close()


def test_inverse_rejects(gpu, oracle):
    import torch
    from hpc_suffix_array_amd import DeviceBuilder, SAError, inverse_suffix_array
    n = 5000
    t = oracle.gen_text("dna", n, seed=9)
    sa = oracle.sa_c(t).astype(np.uint32)
    dup = sa.copy()
    dup[7] = dup[8]
    with pytest.raises(SAError, match="not a permutation"):
        inverse_suffix_array(dup)
    far = sa.copy()
    far[100] = n
    with pytest.raises(SAError, match="not a permutation"):
        inverse_suffix_array(far)
    bld = DeviceBuilder(n)
    d_sa = torch.from_numpy(sa.view(np.int32)).cuda()
    d_isa = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(SAError, match="aligned"):
        bld.inverse(n, d_sa, d_isa[1:])
    with pytest.raises(SAError, match="alias"):
        bld.inverse(n, d_sa, d_sa)
    bld.inverse(n, d_sa, d_isa)                      # and the context still works
    assert (d_isa.cpu().numpy()[:n].view(np.uint32)[sa] == np.arange(n, dtype=np.uint32)).all()
    bld.close()
