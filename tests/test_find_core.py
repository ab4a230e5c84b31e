"""The scalar core of the pattern search (sa::find_scalar,
hpc_suffix_array_amd/csrc/sa_find.h) on the host: g++ builds
tests/cpp/find_check.cpp, which checks it against a brute-force scan of the
sorted suffixes (random, periodic and memory-less synthetic inputs up to
n = 2^32 - 1), once plainly and once with -fsanitize=address,undefined as a
stand-alone program.  Plus what sa_find / sa_find_device decide before they
touch a device, and the Python side's pattern packing."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "find_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 8000, out.stdout


def test_find_scalar_matches_brute_force(tmp_path):
    _build_and_run(tmp_path, "find_check", ["-O2"], 300)


def test_find_scalar_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: text, SA and pattern
    are exact-size heap buffers read bytewise, so a probe that reads past an
    end aborts.  (About ten times the plain run: the synthetic cases at
    n = 2^32 - 1 step through 4 GiB of pattern by words.)"""
    _build_and_run(tmp_path, "find_check_san",
                   ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 900)


def test_threshold_constant_agrees(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_find.h")).read()
    in_hdr = int(re.search(r"#define\s+SA_FIND_LANE_MAX\s+(\d+)", hdr).group(1))
    in_src = int(re.search(r"kFindLaneMax\s*=\s*(\d+)", src).group(1))
    assert in_hdr == in_src == sa_lib.FIND_LANE_MAX
    assert sa_lib.FIND_LANE_MAX > 17            # above the lengths at which the scalar probe changes path
    assert (sa_lib.FIND_LANE, sa_lib.FIND_WAVE) == (1, 2)
    assert int(re.search(r"#define\s+SA_FIND_LANE\s+(\d+)", hdr).group(1)) == 1
    assert int(re.search(r"#define\s+SA_FIND_WAVE\s+(\d+)", hdr).group(1)) == 2


def test_find_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call."""
    L = sa_lib.lib()
    t = np.frombuffer(b"banana", np.uint8)
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    pat = np.frombuffer(b"anana", np.uint8)
    lo, hi = np.zeros(2, np.uint64), np.zeros(2, np.uint64)

    def find(n=6, sa_arr=sa, width=4, off=(0, 3, 5), nq=2, pat_arr=pat):
        o = np.array(off, np.uint64)
        return L.sa_find(t.ctypes.data, n, sa_arr.ctypes.data, width, pat_arr.ctypes.data if pat_arr is not None else None,
                         o.ctypes.data, nq, lo.ctypes.data, hi.ctypes.data)

    assert find(width=3) == -1 and b"sa_width" in L.sa_last_error()
    assert find(off=(0, 4, 3)) == -1 and b"offsets" in L.sa_last_error()
    assert find(off=(5, 4, 4)) == -1
    assert find(n=1 << 32) == -1 and b"too large" in L.sa_last_error()
    assert find(pat_arr=None) == -1
    wide = np.array([5, 3, 1, 0, 4, 6], np.int64)
    assert find(sa_arr=wide, width=8) == -1 and b"out of range" in L.sa_last_error()
    wide[5] = -1
    assert find(sa_arr=wide, width=8) == -1
    assert find(nq=0) == 0                       # nothing to search: no device needed
    assert L.sa_find_ex(t.ctypes.data, 6, sa.ctypes.data, 4, pat.ctypes.data, np.array([0, 5], np.uint64).ctypes.data,
                        1, lo.ctypes.data, hi.ctypes.data, 3) == -1
    # device variant: a fake non-NULL address is never dereferenced on these paths
    p = ctypes.c_void_p(4096)
    assert L.sa_find_device(p, 6, p, p, 5, p, 0, p, p, 0, None) == 0          # nq == 0: no launch
    assert L.sa_find_device(None, 6, p, p, 5, p, 2, p, p, 0, None) == -1
    assert L.sa_find_device(p, 6, p, p, 5, p, 2, p, None, 0, None) == -1
    assert L.sa_find_device(p, 1 << 32, p, p, 5, p, 2, p, p, 0, None) == -1
    assert L.sa_find_device(p, 6, p, p, 5, p, 2, p, p, 7, None) == -1 and b"flags" in L.sa_last_error()


def test_no_search_without_device(sa_lib):
    if sa_lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    from hpc_suffix_array_amd import SAError, find_patterns
    with pytest.raises(SAError):
        find_patterns(b"banana", np.array([5, 3, 1, 0, 4, 2], np.uint32), [b"ana"])
    L = sa_lib.lib()
    t, sa = np.frombuffer(b"banana", np.uint8), np.array([5, 3, 1, 0, 4, 2], np.uint32)
    lo, hi = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    rc = L.sa_find(t.ctypes.data, 6, sa.ctypes.data, 4, t.ctypes.data, np.array([0, 3], np.uint64).ctypes.data, 1,
                   lo.ctypes.data, hi.ctypes.data)
    assert rc < 0 and b"device" in L.sa_last_error()


def test_pattern_packing():
    from hpc_suffix_array_amd.builder import _pack_patterns
    buf, off = _pack_patterns([b"ab", "c\xff", np.array([0, 1, 2], np.uint8), b"", bytearray(b"z")])
    assert bytes(buf) == b"abc\xff\x00\x01\x02z" and off.tolist() == [0, 2, 4, 7, 7, 8]
    assert off.dtype == np.uint64 and buf.dtype == np.uint8
    buf, off = _pack_patterns([])
    assert buf.size == 0 and off.tolist() == [0]
    buf, off = _pack_patterns([b"", b""])
    assert buf.size == 0 and off.tolist() == [0, 0, 0]
    buf, off = _pack_patterns((b"abcdef", np.array([1, 3, 3, 6], np.int64)))
    assert bytes(buf) == b"abcdef" and off.tolist() == [1, 3, 3, 6]
    buf, off = _pack_patterns((b"ab", b"cd"))                      # two patterns, not a pair
    assert bytes(buf) == b"abcd" and off.tolist() == [0, 2, 4]
    with pytest.raises(ValueError):
        _pack_patterns((b"abc", np.array([0, 4], np.int64)))       # ends past the buffer
    with pytest.raises(ValueError):
        _pack_patterns((b"abc", np.array([-1, 2], np.int64)))
    with pytest.raises(TypeError):
        _pack_patterns(b"abc")
