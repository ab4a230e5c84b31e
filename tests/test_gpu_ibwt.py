"""GPU LF-mapping and inverse Burrows-Wheeler transform (sa_lf / sa_lf_device /
sa_ibwt / sa_ibwt_device, hpc_suffix_array_amd/csrc/sa_ibwt.h) against numpy
alone.

Expected values, with t and sa numpy arrays (sa from the oracle up to 2^20
bytes, from the GPU build followed by check_suffix_array above that):
    bwt, primary = t[(sa - 1) % n], flatnonzero(sa == 0)[0]
    rows = [primary, 0, 1, .. without primary]
    lf[rows[argsort(bwt[rows], stable)]] = arange(n)
    inverse_bwt(bwt, primary) = (t, sa)
The bound on the longest sublist is the union bound for a splitter rule that
does not see the data: S (ln(n / S) + 14) at density 1 / S fails with
probability e^-14."""
import ctypes
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bwt_of(t, sa):
    n = int(t.size)
    return t[(sa.astype(np.int64) - 1) % n], int(np.flatnonzero(sa == 0)[0])


def lf_of(b, p):
    """The definition: the rows in the order p, 0, 1, .. sorted stably by byte."""
    n = int(b.size)
    rows = np.concatenate([[p], np.arange(p), np.arange(p + 1, n)]).astype(np.int64)
    lf = np.empty(n, np.int64)
    lf[rows[np.argsort(b[rows], kind="stable")]] = np.arange(n)
    return lf


def check_round_trip(t, sa, what="", widths=(4, 8), lf=True):
    """LF, text and SA through the host forms, everything exact."""
    from hpc_suffix_array_amd import inverse_bwt, lf_mapping
    b, p = bwt_of(t, sa)
    n = int(t.size)
    if lf:
        want = lf_of(b, p)
        for w in widths:
            got = lf_mapping(b, p, width=w)
            assert got.dtype == (np.uint32 if w == 4 else np.int64) and got.shape == (n,), what
            assert (got == want).all(), what
    text = inverse_bwt(b, p)
    assert text.dtype == np.uint8 and text.shape == t.shape and (text == t).all(), what
    for w in widths:
        text, s, info = inverse_bwt(b, p, return_sa=True, width=w, return_info=True)
        assert s.dtype == (np.uint32 if w == 4 else np.int64), what
        assert (text == t).all() and (s == sa).all(), what
        assert info["steps"] == n - 1, (what, info)
    return info


@functools.lru_cache(maxsize=None)
def _text_sa(kind, n, seed):
    """(text, SA), computed once per module; read-only."""
    from oracle import oracle as O
    t = O.gen_text(kind, n, seed=seed)
    return _with_sa(t)


def _with_sa(t):
    from oracle import oracle as O
    from hpc_suffix_array_amd import build_suffix_array, check_suffix_array
    if t.size <= 1 << 20:
        sa = O.sa_c(t).astype(np.uint32)
    else:
        sa = build_suffix_array(t)
        assert check_suffix_array(t, sa)
    t.setflags(write=False)
    sa.setflags(write=False)
    return t, sa


def test_golden(gpu, golden):
    # (width 8 on two cases: every width-8 download allocates its pinned staging ring, which is slow on a busy host)
    for k, (name, c) in enumerate(sorted(golden["cases"].items())):
        t, sa = np.ascontiguousarray(c["text"], np.uint8), np.asarray(c["sa"])
        if t.size:
            check_round_trip(t, sa, name, widths=(4, 8) if k in (0, 30) else (4,))


@pytest.mark.parametrize("kind", ["dna", "binary", "byte256"])
def test_tile_edges(gpu, oracle, kind):
    from hpc_suffix_array_amd import _native as N
    T = N.LF_TILE
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3):
        t = oracle.gen_text(kind, n, seed=7 * n + len(kind))
        check_round_trip(t, oracle.sa_c(t), f"{kind} n={n}", widths=(4, 8) if n in (5, T + 1) else (4,))


def test_around_powers_of_s(gpu, oracle):
    from hpc_suffix_array_amd import _native as N
    S = N.IBWT_S
    for n in (S - 1, S, S + 1, S * S - 1, S * S, S * S + 1, S ** 3 - 1, S ** 3, S ** 3 + 1, N.IBWT_TILE - 1, N.IBWT_TILE + 1):
        t = oracle.gen_text("dna", n, seed=n)
        check_round_trip(t, oracle.sa_c(t), f"n={n}", widths=(4,))


@pytest.mark.parametrize("kind,n", [("dna", (1 << 20) + 3), ("byte256", (1 << 20) + 3), ("dna", (1 << 22) + 1),
                                    ("byte256", (1 << 22) + 1), ("dna", (1 << 24) + 5)])
def test_large(gpu, kind, n):
    from hpc_suffix_array_amd import _native as N
    t, sa = _text_sa(kind, n, 3)
    info = check_round_trip(t, sa, f"{kind} n={n}", widths=(4,) if n > 1 << 22 else (4, 8))
    assert abs(info["splitters"] - (n / N.IBWT_S + 1)) <= 0.02 * (n / N.IBWT_S + 1)


def _structured(n):
    fib = [b"b", b"a"]
    while len(fib[-1]) < n:
        fib.append(fib[-1] + fib[-2])
    i = np.arange(n, dtype=np.uint64)
    pop = np.zeros(n, np.uint8)
    for k in range(32):
        pop ^= ((i >> np.uint64(k)) & np.uint64(1)).astype(np.uint8)
    last_b = np.full(n, ord("a"), np.uint8)
    last_b[-1] = ord("b")
    return {"one symbol": np.full(n, ord("a"), np.uint8),
            "(ab)^k": np.tile(np.frombuffer(b"ab", np.uint8), n // 2),
            "a^(n-1)b": last_b,
            "fibonacci": np.frombuffer(fib[-1][:n], np.uint8).copy(),
            "thue-morse": (pop + ord("a")).astype(np.uint8),
            "(1..64)^k": (1 + np.arange(n) % 64).astype(np.uint8)}


@pytest.mark.parametrize("n", [1 << 18, 1 << 22])
def test_structured_texts(gpu, n):
    """Texts whose chains are as regular as a chain can be: the splitters are
    hashed, so no sublist is long.  The bound is the docstring's."""
    from hpc_suffix_array_amd import _native as N
    S = N.IBWT_S
    bound = S * (math.log(n / S) + 14)
    primaries = set()
    for name, t in _structured(n).items():
        assert t.size == n
        t, sa = _with_sa(t)
        primaries.add(bwt_of(t, sa)[1])
        info = check_round_trip(t, sa, name, widths=(4,), lf=n <= 1 << 18)
        print(f"{name} n={n}: splitters {info['splitters']}, longest sublist {info['longest_sublist']} (bound {bound:.0f})")
        assert info["longest_sublist"] <= bound, (name, info, bound)
        assert abs(info["splitters"] - (n / S + 1)) <= 0.02 * (n / S + 1), (name, info)
    assert 0 in primaries and n - 1 in primaries


def _follow(b, p):
    """Steps of the chain from LF[p] until it meets p, in plain Python."""
    lf = lf_of(b, p).tolist()
    r, steps = lf[p], 0
    while r != p:
        r = lf[r]
        steps += 1
    return steps


def _call_ibwt(sa_lib, b, p, with_sa=True):
    """sa_ibwt_ex on pre-filled outputs: (rc, message, info, text, sa)."""
    n = int(b.size)
    text = np.full(n, 0xA5, np.uint8)
    s = np.full(n, 0xA5A5A5A5, np.uint32)
    info = (ctypes.c_uint64 * 3)(9, 9, 9)
    L = sa_lib.lib()
    rc = L.sa_ibwt_ex(b.ctypes.data, n, p, text.ctypes.data, s.ctypes.data if with_sa else None, 4, info)
    return rc, L.sa_last_error(), list(info), text, s


def test_primary_out_of_range(gpu):
    from hpc_suffix_array_amd import SAError, inverse_bwt, lf_mapping
    for p in (6, 11):
        for f in (inverse_bwt, lf_mapping):
            with pytest.raises(SAError, match="primary index"):
                f(b"nnbaaa", p)


@pytest.mark.parametrize("n", [1000, 4097, 1 << 16])
def test_random_bytes_random_primary(gpu, sa_lib, n):
    """Any bytes and any primary index: LF is still a permutation, the verdict
    and the steps are the chain's, and a rejected call writes nothing."""
    from hpc_suffix_array_amd import lf_mapping
    rng = np.random.default_rng(n)
    rejected = 0
    for sigma in (2, 4, 256):
        b = rng.integers(0, sigma, size=n, dtype=np.uint8)
        p = int(rng.integers(0, n))
        assert (lf_mapping(b, p) == lf_of(b, p)).all()
        steps = _follow(b, p)
        rc, msg, info, text, s = _call_ibwt(sa_lib, b, p)
        assert info[2] == steps, (sigma, info, steps)
        if steps == n - 1:
            assert rc == 0
            continue
        rejected += 1
        assert rc == -1 and b"not a BWT" in msg, (rc, msg)
        assert (text == 0xA5).all() and (s == 0xA5A5A5A5).all()
    assert rejected >= 2   # a random permutation is one cycle with probability 1 / n


def test_swapped_bytes(gpu, sa_lib):
    """A BWT of 2^20 bytes with two unequal bytes swapped: rejected, or the
    BWT of another text, which then is the text that comes back."""
    from hpc_suffix_array_amd import SAError, build_suffix_array, bwt, inverse_bwt
    n = 1 << 20
    t, sa = _text_sa("dna", n, 17)
    good, p = bwt_of(t, sa)
    rejected = 0
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        b = good.copy()
        while True:
            i, j = (int(x) for x in rng.integers(0, n, size=2))
            if b[i] != b[j]:
                break
        b[i], b[j] = b[j], b[i]
        try:
            t2 = inverse_bwt(b, p)
        except SAError as e:
            assert "not a BWT" in str(e)
            rejected += 1
            rc, msg, info, text, s = _call_ibwt(sa_lib, b, p)
            assert rc == -1 and info[2] < n - 1 and (text == 0xA5).all() and (s == 0xA5A5A5A5).all()
            continue
        b2, p2 = bwt(t2, build_suffix_array(t2))
        assert p2 == p and (b2 == b).all(), seed
    assert rejected >= 1


def test_device_path_alignment_and_guards(gpu, oracle):
    """DeviceBuilder.bwt -> DeviceBuilder.ibwt on torch tensors, no host copy
    in between; input and output at byte offsets 0..3, 32 guard bytes on either
    side untouched; on a stream of its own; with and without d_sa."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    bld = DeviceBuilder(1 << 17)
    stream = torch.cuda.Stream()
    for k, n in enumerate((1, 2, 5, 67, 4099, N.LF_TILE + 1, 2 * N.LF_TILE + 2, 70001)):
        t = oracle.gen_text("dna" if k % 2 else "byte256", n, seed=n)
        sa = oracle.sa_c(t).astype(np.uint32)
        b, p = bwt_of(t, sa)
        d_text = torch.from_numpy(t).cuda()
        d_sa = torch.from_numpy(sa.view(np.int32)).cuda()
        for off in range(4):
            ob = (off + k) % 4
            buf_b = torch.full((n + 64 + 3,), 0xA5, dtype=torch.uint8, device="cuda")
            buf_t = torch.full((n + 64 + 3,), 0xA5, dtype=torch.uint8, device="cuda")
            d_bwt, d_out = buf_b[32 + ob:32 + ob + n], buf_t[32 + off:32 + off + n]
            d_sa2 = torch.full((n + 16,), -1, dtype=torch.int32, device="cuda")
            d_lf = torch.full((n + 16,), -1, dtype=torch.int32, device="cuda")
            d_stats = torch.zeros(N.BWT_STATS, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()   # the fills ran on the default stream
            with torch.cuda.stream(stream):
                bld.bwt(d_text, n, d_sa, d_bwt, d_stats, stream=stream.cuda_stream)
                bld.lf(d_bwt, n, p, d_lf[8:], stream=stream.cuda_stream)
                info = bld.ibwt(d_bwt, n, p, d_out, d_sa2[8:] if off != 1 else None, stream=stream.cuda_stream)
            stream.synchronize()
            assert int(d_stats[0]) == p and info["steps"] == n - 1
            got = buf_t.cpu().numpy()
            assert (got[32 + off:32 + off + n] == t).all(), (n, off)
            assert (got[:32 + off] == 0xA5).all() and (got[32 + off + n:] == 0xA5).all(), (n, off)
            s2 = d_sa2.cpu().numpy()
            assert (s2[:8] == -1).all() and (s2[8 + n:] == -1).all()
            assert (s2[8:8 + n].view(np.uint32) == sa).all() if off != 1 else (s2 == -1).all()
            l2 = d_lf.cpu().numpy()
            assert (l2[:8] == -1).all() and (l2[8 + n:] == -1).all() and (l2[8:8 + n] == lf_of(b, p)).all()
    bld.close()


def test_device_rejection_leaves_outputs(gpu):
    import torch
    from hpc_suffix_array_amd import DeviceBuilder, SAError
    n = 5000
    b = np.full(n, ord("a"), np.uint8)   # a^n has primary n - 1 only
    bld = DeviceBuilder(1 << 16)
    d_bwt = torch.from_numpy(b).cuda()
    d_text = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    d_sa = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(SAError, match="not a BWT"):
        bld.ibwt(d_bwt, n, 17, d_text, d_sa)
    assert bool((d_text == 0x5A).all()) and bool((d_sa == -7).all())
    assert bld.ibwt(d_bwt, n, n - 1, d_text, d_sa)["steps"] == n - 1
    assert bool((d_text == ord("a")).all()) and (d_sa.cpu().numpy() == np.arange(n)[::-1]).all()
    bld.close()


def test_host_waits_and_determinism(gpu, sa_lib):
    """sa_host_syncs() rises by exactly 1 per ibwt and by 0 per lf; two calls
    agree bit for bit."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder
    n = (1 << 20) + 3
    t, sa = _text_sa("dna", n, 3)
    b, p = bwt_of(t, sa)
    bld = DeviceBuilder(n)
    d_bwt = torch.from_numpy(b).cuda()
    outs = []
    for _ in range(2):
        d_text = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_sa = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_lf = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        before = sa_lib.lib().sa_host_syncs()
        bld.lf(d_bwt, n, p, d_lf)
        assert sa_lib.lib().sa_host_syncs() == before
        info = bld.ibwt(d_bwt, n, p, d_text, d_sa)
        assert sa_lib.lib().sa_host_syncs() == before + 1
        info2 = bld.ibwt(d_bwt, n, p, d_text, None)
        assert sa_lib.lib().sa_host_syncs() == before + 2 and info2 == info
        torch.cuda.synchronize()
        outs.append((d_text.cpu().numpy(), d_sa.cpu().numpy(), d_lf.cpu().numpy(), info))
    assert (outs[0][0] == t).all() and (outs[0][1].view(np.uint32) == sa).all()
    for x, y in zip(outs[0][:3], outs[1][:3]):
        assert x.tobytes() == y.tobytes()
    assert outs[0][3] == outs[1][3]
    bld.close()
