"""The host-compilable arithmetic of the LCE index (hpc_suffix_array_amd/csrc/
sa_lce.h): g++ builds tests/cpp/lce_check.cpp, which builds the index on the
host by the tables' definitions, answers rank ranges by the query
decomposition (which masked block words and which cells a range reads) and
compares with a brute-force minimum -- every range for every n in 1 .. 200,
structured ranges around 4096, 8192 and 2^18 -- once plainly and once with
-fsanitize=address,undefined as a stand-alone program on exact-size heap
buffers.  Plus the constants' copies, the exported symbols, the Python names,
sa_lce_index_bytes against the formula, and what the sa_lce_* entry points
decide before they touch a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "lce_check.cpp")

DEVICE_SYMBOLS = ("sa_lce_build_device", "sa_lcp_min_device", "sa_lce_device", "sa_substr_compare_device")
HOST_SYMBOLS = ("sa_lcp_min", "sa_lce", "sa_substr_compare")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 1000000, out.stdout


def test_lce_arithmetic_matches_brute_force(tmp_path):
    _build_and_run(tmp_path, "lce_check", ["-O2"], 300)


def test_lce_arithmetic_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: the LCP array and the
    two tables are exact-size heap buffers, so a masked word past n or a cell
    past its section aborts, and a shift by a level that does not exist is
    reported."""
    _build_and_run(tmp_path, "lce_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_lce.h")).read()

    def h(name):
        return int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, hdr).group(1), 0)

    def s(name):
        return int(re.search(r"%s\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?" % name, src).group(1), 0)

    assert h("SA_LCE_NONE") == s("kLceNone") == sa_lib.LCE_NONE == 0xFFFFFFFF
    assert h("SA_LCE_PROBE") == s("kLceProbe") == sa_lib.LCE_PROBE == 16
    assert h("SA_LCE_BLOCK") == s("kLceBlock") == sa_lib.LCE_BLOCK == 64
    assert h("SA_LCE_SUPER") == s("kLceSuper") == sa_lib.LCE_SUPER == 4096
    assert s("kLceHeaderBytes") == sa_lib.LCE_HEADER == 4096
    assert sa_lib.LCE_SUPER == 64 * sa_lib.LCE_BLOCK


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    for name in DEVICE_SYMBOLS + HOST_SYMBOLS:
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\bint %s\(" % name, hdr), name
    assert "sa_lce_index_bytes" in sa_lib.EXT_SYMBOLS and re.search(r"\buint64_t sa_lce_index_bytes\(", hdr)
    for name in ("longest_common_extension", "lcp_range_min", "compare_substrings", "LCEIndex"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("lce_build", "lcp_min", "lce", "substr_compare", "lce_index_bytes"):
        assert callable(getattr(pkg.DeviceBuilder, name))
    for name in ("from_text", "from_sa", "lce", "compare", "interval_depth", "to_bytes", "from_bytes", "close",
                 "__enter__", "__exit__"):
        assert callable(getattr(pkg.LCEIndex, name))
    assert callable(pkg.SuffixArray.lce)


def _formula(n):
    nb = (n + 63) // 64
    ns = (nb + 63) // 64
    levels = ns.bit_length()          # floor(log2 ns) + 1, 0 for no superblock
    return (4096 + 4 * (6 * nb + levels * ns) + 15) // 16 * 16


def test_index_bytes_formula(sa_lib):
    L = sa_lib.lib()
    rng = np.random.default_rng(5)
    sizes = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8192, 8193, 262143, 262144, 262145, 3 * 2**18 + 7, 2**20, 2**24,
             2**28, 2**31, 2**32 - 1] + [int(x) for x in rng.integers(1, 2**32, 200)]
    for n in sizes:
        assert L.sa_lce_index_bytes(n) == _formula(n), n
    assert L.sa_lce_index_bytes(0) == 4096
    assert L.sa_lce_index_bytes(1) == 4096 + 32          # six block levels and one top cell, rounded up to 16
    assert L.sa_lce_index_bytes(2**32) == 0              # n too large
    for n in (2**20, 2**24, 2**28, 2**32 - 1):
        assert L.sa_lce_index_bytes(n) < 0.40 * n + 8192
    assert L.sa_lce_index_bytes(2**32 - 1) < 1.6 * 2**30


def _rejections(L, call, cases):
    """Every case returns SA_E_INVALID with its word in the message; returns the distinct messages."""
    msgs = set()
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = L.sa_last_error()
        assert word in msg, (kw, msg)
        msgs.add(msg.split(b" 0x")[0])
    return msgs


def test_device_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call: the pointers are
    fake addresses that are never dereferenced."""
    L = sa_lib.lib()
    p, p2, p3, p4, p5, p6, p7, p8, p9 = (ctypes.c_void_p(4096 * k) for k in range(1, 10))
    odd4 = ctypes.c_void_p(4100)     # 4-byte aligned, not 16
    odd = ctypes.c_void_p(4098)
    need = L.sa_lce_index_bytes(1000)

    def build(n=1000, lcp=p, index=p2, nbytes=need):
        return L.sa_lce_build_device(n, lcp, index, nbytes, None)

    msgs = _rejections(L, build, (
        ({"n": 1 << 32}, b"n too large"), ({"index": None}, b"d_index is NULL"), ({"lcp": None}, b"d_lcp is NULL"),
        ({"index": odd4}, b"d_index is not 16-byte aligned"), ({"lcp": odd4}, b"d_lcp is not 16-byte aligned"),
        ({"nbytes": need - 1}, b"is below the"), ({"nbytes": 0}, b"is below the"), ({"index": p}, b"alias d_lcp")))
    assert len(msgs) == 8

    def rmin(n=1000, lcp=p, index=p2, nbytes=need, lo=p3, hi=p4, nq=5, out=p5):
        return L.sa_lcp_min_device(n, lcp, index, nbytes, lo, hi, nq, out, None)

    msgs = _rejections(L, rmin, (
        ({"n": 1 << 32}, b"n too large"), ({"nq": 1 << 32}, b"nq too large"), ({"index": None}, b"d_index is NULL"),
        ({"lcp": None}, b"d_lcp is NULL"), ({"lo": None}, b"d_lo is NULL"), ({"hi": None}, b"d_hi is NULL"),
        ({"out": None}, b"d_out is NULL"), ({"index": odd4}, b"d_index is not 16-byte"),
        ({"lcp": odd4}, b"d_lcp is not 16-byte"), ({"out": odd}, b"d_out is not 4-byte aligned"),
        ({"out": p3}, b"d_out may not alias"), ({"out": p4}, b"may not alias"), ({"out": p}, b"may not alias"),
        ({"out": p2}, b"may not alias")))
    assert len(msgs) == 11           # the four aliases share one message
    assert rmin(nq=0, lo=None, hi=None, out=None) == 0      # nothing to do: no launch

    def lce(n=1000, text=p6, isa=p7, lcp=p, index=p2, nbytes=need, i=p3, j=p4, nq=5, out=p5):
        return L.sa_lce_device(n, text, isa, lcp, index, nbytes, i, j, nq, out, None)

    msgs = _rejections(L, lce, (
        ({"n": 1 << 32}, b"n too large"), ({"nq": 1 << 32}, b"nq too large"), ({"index": None}, b"d_index is NULL"),
        ({"lcp": None}, b"d_lcp is NULL"), ({"isa": None}, b"d_isa is NULL"), ({"i": None}, b"d_i is NULL"),
        ({"j": None}, b"d_j is NULL"), ({"out": None}, b"d_lce is NULL"), ({"index": odd4}, b"d_index is not"),
        ({"lcp": odd4}, b"d_lcp is not"), ({"out": odd}, b"d_lce is not 4-byte aligned"),
        ({"out": p3}, b"d_lce may not alias"), ({"out": p7}, b"d_lce may not alias"),
        ({"out": p6}, b"d_lce may not alias")))
    assert len(msgs) == 12
    assert lce(nq=0, i=None, j=None, out=None) == 0

    def cmp_(n=1000, text=None, isa=p7, lcp=p, index=p2, nbytes=need, i=p3, li=p8, j=p4, lj=p9, nq=5, out=p5):
        return L.sa_substr_compare_device(n, text, isa, lcp, index, nbytes, i, li, j, lj, nq, out, None)

    msgs = _rejections(L, cmp_, (
        ({"n": 1 << 32}, b"n too large"), ({"nq": 1 << 32}, b"nq too large"), ({"index": None}, b"d_index is NULL"),
        ({"lcp": None}, b"d_lcp is NULL"), ({"isa": None}, b"d_isa is NULL"), ({"i": None}, b"d_i is NULL"),
        ({"j": None}, b"d_j is NULL"), ({"li": None}, b"d_li is NULL"), ({"lj": None}, b"d_lj is NULL"),
        ({"out": None}, b"d_order is NULL"), ({"index": odd4}, b"d_index is not"),
        ({"out": p8}, b"d_order may not alias"), ({"out": p2}, b"d_order may not alias")))
    assert len(msgs) == 12
    assert cmp_(nq=0, i=None, j=None, li=None, lj=None, out=None) == 0


def test_host_arguments_rejected_before_any_device(sa_lib):
    """The host forms check everything before they ask for a device, so all of
    this runs without one; the arrays are real (the checks read them)."""
    L = sa_lib.lib()
    err = L.sa_last_error
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    lcp = np.array([0, 1, 3, 0, 0, 2], np.uint32)           # banana
    out = np.full(2, 99, np.uint64)

    def rmin(a=lcp, n=6, width=4, lo=(0, 1), hi=(3, 3), nq=2, o=out):
        x, y = np.array(lo, np.uint64), np.array(hi, np.uint64)
        return L.sa_lcp_min(ptr(a), n, width, x.ctypes.data, y.ctypes.data, nq, ptr(o))

    assert rmin(width=3) == -1 and b"sa_width" in err()
    assert rmin(n=1 << 32) == -1 and b"too large" in err()
    assert rmin(nq=1 << 32) == -1 and b"nq too large" in err()
    assert rmin(o=None) == -1 and b"out is NULL" in err()
    assert rmin(a=None) == -1 and b"lcp is NULL" in err()
    assert L.sa_lcp_min(ptr(lcp), 6, 4, None, ptr(out), 2, ptr(out)) == -1 and b"NULL interval array" in err()
    assert L.sa_lcp_min(ptr(lcp), 6, 4, ptr(out), ptr(out), 2, ptr(out)) == -1 and b"alias" in err()
    assert rmin(a=np.array([0, 1, 3, 0, -1, 2], np.int64), width=8) == -1 and b"LCP entry out of range" in err()
    assert rmin(a=np.array([0, 1, 1 << 32, 0, 0, 2], np.int64), width=8) == -1 and b"out of range" in err()
    assert (out == 99).all()
    assert rmin(nq=0) == 0 and (out == 99).all()
    # no interval of two or more ranks: answered without a device
    assert rmin(lo=(2, 5), hi=(3, 2)) == 0 and out.tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    assert rmin(lo=(0, 4), hi=(7, 1 << 40)) == 0 and out.tolist() == [0xFFFFFFFF, 0xFFFFFFFF]

    text = np.frombuffer(b"banana", np.uint8)
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    res = np.full(2, 99, np.uint64)
    qi, qj = np.array([0, 1], np.uint64), np.array([2, 3], np.uint64)

    def lce(t=text, n=6, s=sa, width=4, i=qi, j=qj, nq=2, o=res):
        return L.sa_lce(ptr(t), n, ptr(s), width, ptr(i), ptr(j), nq, ptr(o))

    assert lce(width=5) == -1 and b"sa_width" in err()
    assert lce(n=1 << 32) == -1 and b"too large" in err()
    assert lce(nq=1 << 32) == -1 and b"nq too large" in err()
    assert lce(i=None) == -1 and b"NULL position array" in err()
    assert lce(o=None) == -1 and b"out is NULL" in err()
    assert lce(o=qi) == -1 and b"alias" in err()
    assert lce(t=None) == -1 and b"NULL host pointer" in err()
    assert lce(s=None) == -1 and b"NULL host pointer" in err()
    assert lce(s=np.array([5, 3, 1, 0, 4, 6], np.int64), width=8) == -1 and b"SA entry out of range" in err()
    assert (res == 99).all()
    assert lce(nq=0) == 0 and (res == 99).all()
    assert lce(t=None, s=None, n=0) == 0 and res.tolist() == [0, 0]     # the empty text needs no device

    ql = np.array([3, 2], np.uint64)
    order = np.full(2, 99, np.int8)

    def cmp_(t=text, n=6, s=sa, width=4, i=qi, li=ql, j=qj, lj=ql, nq=2, o=order):
        return L.sa_substr_compare(ptr(t), n, ptr(s), width, ptr(i), ptr(li), ptr(j), ptr(lj), nq, ptr(o))

    assert cmp_(width=2) == -1 and b"sa_width" in err()
    assert cmp_(n=1 << 32) == -1 and b"too large" in err()
    assert cmp_(li=None) == -1 and b"NULL length array" in err()
    assert cmp_(j=None) == -1 and b"NULL position array" in err()
    assert cmp_(o=None) == -1 and b"out is NULL" in err()
    assert cmp_(s=None) == -1 and b"NULL host pointer" in err()
    assert (order == 99).all()
    assert cmp_(nq=0) == 0 and (order == 99).all()
    assert cmp_(t=None, s=None, n=0) == 0 and order.tolist() == [0, 0]


def test_no_lce_without_device(sa_lib):
    if sa_lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    from hpc_suffix_array_amd import (LCEIndex, SAError, SuffixArray, compare_substrings, lcp_range_min,
                                      longest_common_extension)
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    lcp = np.array([0, 1, 3, 0, 0, 2], np.uint32)
    with pytest.raises(SAError):
        lcp_range_min(lcp, [0], [3])
    with pytest.raises(SAError):
        longest_common_extension(b"banana", sa, [1], [3])
    with pytest.raises(SAError):
        compare_substrings(b"banana", sa, [1], [3], [3], [3])
    with pytest.raises(SAError):
        LCEIndex.from_text(b"banana")
    with pytest.raises(SAError):
        LCEIndex.from_sa(b"banana", sa)
    with pytest.raises(SAError):
        LCEIndex.from_bytes(b"SALCEBL1" + bytes(24) + bytes(4096))
    with SuffixArray(b"banana") as s:
        with pytest.raises(SAError):
            s.lce(1, 3)


def test_lce_python_arguments():
    from hpc_suffix_array_amd import LCEIndex, SAError, compare_substrings, lcp_range_min, longest_common_extension
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    lcp = np.array([0, 1, 3, 0, 0, 2], np.uint32)
    with pytest.raises(ValueError):
        lcp_range_min(lcp, [0, 1], [3])
    with pytest.raises(ValueError):
        lcp_range_min(lcp, [-1], [3])
    with pytest.raises(ValueError):
        longest_common_extension(b"banana", sa, [1, 2], [3])
    with pytest.raises(ValueError):
        longest_common_extension(b"banana", sa, [1], [-3])
    with pytest.raises(ValueError):
        longest_common_extension(b"banana", sa[:5], [1], [3])
    with pytest.raises(ValueError):
        compare_substrings(b"banana", sa, [1], [3, 3], [3], [3])
    with pytest.raises(SAError):
        LCEIndex.from_bytes(b"not an index")
    with pytest.raises(SAError):
        LCEIndex.from_bytes(b"SALCEBL1" + bytes(24))         # n = 0 with an index of 0 bytes
    # no query, no interval with a minimum, no text: nothing needs a device
    assert lcp_range_min(lcp, [], []).size == 0
    assert lcp_range_min(lcp, [2, 5, 0], [3, 2, 9]).tolist() == [-1, -1, -1]
    assert longest_common_extension(b"banana", sa, [], []).size == 0
    assert longest_common_extension(b"", np.zeros(0, np.uint32), [0, 3], [0, 1]).tolist() == [0, 0]
    assert compare_substrings(b"", np.zeros(0, np.uint32), [0], [2], [1], [5]).tolist() == [0]
