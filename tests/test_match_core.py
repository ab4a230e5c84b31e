"""The scalar core of the longest-match search (sa::match_scalar,
hpc_suffix_array_amd/csrc/sa_match.h) on the host: g++ builds
tests/cpp/match_check.cpp, which checks it against a brute-force scan of the
sorted suffixes (random, periodic and memory-less synthetic inputs up to
n = 2^32 - 1, with and without the bounds), once plainly and once with
-fsanitize=address,undefined as a stand-alone program.  Plus what sa_match,
sa_matching_stats and their _device forms decide before they touch a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "match_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 8000, out.stdout


def test_match_scalar_matches_brute_force(tmp_path):
    _build_and_run(tmp_path, "match_check", ["-O2"], 300)


def test_match_scalar_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: text, SA and pattern
    are exact-size heap buffers read bytewise, so a probe that reads past an
    end aborts."""
    _build_and_run(tmp_path, "match_check_san",
                   ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 900)


def test_match_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call."""
    L = sa_lib.lib()
    t = np.frombuffer(b"banana", np.uint8)
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    pat = np.frombuffer(b"anana", np.uint8)
    ln, lo, hi = np.zeros(8, np.uint64), np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    outs = (ln.ctypes.data, lo.ctypes.data, hi.ctypes.data)

    def match(n=6, sa_arr=sa, width=4, off=(0, 3, 5), nq=2, pat_arr=pat, out=outs, flags=0, text=t):
        o = np.array(off, np.uint64)
        return L.sa_match(text.ctypes.data if text is not None else None, n,
                          sa_arr.ctypes.data if sa_arr is not None else None, width,
                          pat_arr.ctypes.data if pat_arr is not None else None, o.ctypes.data, nq, *out, flags)

    def stats(n=6, sa_arr=sa, width=4, m=5, max_len=0, query=pat, out=outs, flags=0, text=t):
        return L.sa_matching_stats(text.ctypes.data if text is not None else None, n,
                                   sa_arr.ctypes.data if sa_arr is not None else None, width,
                                   query.ctypes.data if query is not None else None, m, max_len, *out, flags)

    wide_hi = np.array([5, 3, 1, 0, 4, 6], np.int64)
    wide_neg = np.array([5, 3, 1, 0, 4, -1], np.int64)
    for f in (match, stats):
        assert f(width=3) == -1 and b"sa_width" in L.sa_last_error()
        assert f(n=1 << 32) == -1 and b"too large" in L.sa_last_error()
        assert f(flags=3) == -1 and b"flags" in L.sa_last_error()
        assert f(text=None) == -1 and b"NULL" in L.sa_last_error()
        assert f(sa_arr=None) == -1 and b"NULL" in L.sa_last_error()
        assert f(out=(None, outs[1], outs[2])) == -1 and b"NULL" in L.sa_last_error()
        assert f(out=(outs[0], outs[1], None)) == -1 and b"both or neither" in L.sa_last_error()
        assert f(out=(outs[0], None, outs[2])) == -1 and b"both or neither" in L.sa_last_error()
        assert f(sa_arr=wide_hi, width=8) == -1 and b"out of range" in L.sa_last_error()
        assert f(sa_arr=wide_neg, width=8) == -1 and b"out of range" in L.sa_last_error()
    assert match(pat_arr=None) == -1 and b"NULL" in L.sa_last_error()
    assert stats(query=None) == -1 and b"NULL" in L.sa_last_error()
    assert match(off=(0, 4, 3)) == -1 and b"offsets" in L.sa_last_error()
    assert match(off=(5, 4, 4)) == -1 and b"offsets" in L.sa_last_error()
    assert L.sa_match(t.ctypes.data, 6, sa.ctypes.data, 4, pat.ctypes.data, None, 2, *outs, 0) == -1
    assert match(nq=0) == 0                      # nothing to search: no device needed
    assert stats(m=0) == 0
    assert match(nq=0, out=(None, None, None)) == 0 and stats(m=0, out=(None, None, None)) == 0

    # device forms: a fake non-NULL address is never dereferenced on these paths
    p = ctypes.c_void_p(4096)

    def dmatch(text=p, n=6, sa_=p, pat_=p, off=p, nq=2, ln_=p, lo_=p, hi_=p, flags=0):
        return L.sa_match_device(text, n, sa_, pat_, 5, off, nq, ln_, lo_, hi_, flags, None)

    def dstats(text=p, n=6, sa_=p, pat_=p, nq=5, ln_=p, lo_=p, hi_=p, flags=0):
        return L.sa_matching_stats_device(text, n, sa_, pat_, nq, 0, ln_, lo_, hi_, flags, None)

    for f in (dmatch, dstats):
        assert f(nq=0) == 0                                                  # no queries: no launch
        assert f(nq=0, lo_=None, hi_=None) == 0
        assert f(text=None) == -1 and b"NULL" in L.sa_last_error()
        assert f(sa_=None) == -1 and b"NULL" in L.sa_last_error()
        assert f(pat_=None) == -1 and b"NULL" in L.sa_last_error()
        assert f(ln_=None) == -1 and b"NULL" in L.sa_last_error()
        assert f(hi_=None) == -1 and b"both or neither" in L.sa_last_error()
        assert f(lo_=None) == -1 and b"both or neither" in L.sa_last_error()
        assert f(n=1 << 32) == -1 and b"too large" in L.sa_last_error()
        assert f(n=1 << 32, lo_=None, hi_=None) == -1 and b"too large" in L.sa_last_error()
        assert f(flags=3) == -1 and b"flags" in L.sa_last_error()
        assert f(flags=7, nq=0) == -1 and b"flags" in L.sa_last_error()
    assert dmatch(off=None) == -1 and b"NULL" in L.sa_last_error()


def test_no_match_without_device(sa_lib):
    if sa_lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    from hpc_suffix_array_amd import SAError, match_patterns, matching_statistics
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(SAError):
        match_patterns(b"banana", sa, [b"anab"])
    with pytest.raises(SAError):
        match_patterns(b"banana", sa, [b"anab"], bounds=False)
    with pytest.raises(SAError):
        matching_statistics(b"banana", sa, b"bandana")
    with pytest.raises(SAError):
        matching_statistics(b"banana", sa, b"bandana", max_len=3, mode="lane", bounds=False)
    L = sa_lib.lib()
    t = np.frombuffer(b"banana", np.uint8)
    out = np.zeros(3, np.uint64)
    rc = L.sa_match(t.ctypes.data, 6, sa.ctypes.data, 4, t.ctypes.data, np.array([0, 3], np.uint64).ctypes.data, 1,
                    out.ctypes.data, out.ctypes.data + 8, out.ctypes.data + 16, 0)
    assert rc < 0 and b"device" in L.sa_last_error()
    rc = L.sa_matching_stats(t.ctypes.data, 6, sa.ctypes.data, 4, t.ctypes.data, 1, 0,
                             out.ctypes.data, out.ctypes.data + 8, out.ctypes.data + 16, 0)
    assert rc < 0 and b"device" in L.sa_last_error()


def test_match_python_argument_errors():
    from hpc_suffix_array_amd import match_patterns, matching_statistics
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(ValueError):
        matching_statistics(b"banana", sa, b"ban", mode="both")
    with pytest.raises(ValueError):
        matching_statistics(b"banana", sa, b"ban", max_len=-1)
    with pytest.raises(ValueError):
        match_patterns(b"banana", sa[:5], [b"ban"])            # SA and text differ in length
