"""The host-compilable core of the repeat enumeration (hpc_suffix_array_amd/
csrc/sa_repeats.h): g++ builds tests/cpp/repeats_check.cpp, which checks the
nearest-smaller walks over LCP minima (fan-out 64 and 4, whole and
window-then-whole as the kernel composes them), the break-rank query and the
supermaximal scan against the substring dictionary for all three kinds, and
the arithmetic at n = 2^32 - 1, once plainly and once with
-fsanitize=address,undefined as a stand-alone program.  Plus the constants'
copies, the exported symbols, and what the two entry points decide before they
touch a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "repeats_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    # 310 texts of 0 .. 300 bytes and the four around sup257, two fan-outs, six checks per head
    assert int(out.stdout.split()[1]) > 200_000, out.stdout
    assert int(out.stdout.split()[4]) >= 300, out.stdout


def test_repeats_core_matches_dictionary(tmp_path):
    _build_and_run(tmp_path, "repeats_check", ["-O2"], 300)


def test_repeats_core_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: every level of the
    hierarchy and every break array is an exact-size heap array, so a walk or
    a rank query that leaves one aborts."""
    _build_and_run(tmp_path, "repeats_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_repeats.h")).read()
    for name, const, value in (("SA_REP_RIGHT", "kRepRight", 0), ("SA_REP_MAXIMAL", "kRepMaximal", 1),
                               ("SA_REP_SUPERMAXIMAL", "kRepSupermaximal", 2), ("SA_REP_INFO", "kRepInfo", 2)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == value
        assert int(re.search(r"%s\s*=\s*(\d+)" % const, src).group(1)) == value
    assert re.search(r"static_assert\(SA_REP_RIGHT == kRepRight", src)
    assert sa_lib.REP_KINDS == {"right": 0, "maximal": 1, "supermaximal": 2}
    assert (sa_lib.REP_RIGHT, sa_lib.REP_MAXIMAL, sa_lib.REP_SUPERMAXIMAL, sa_lib.REP_INFO) == (0, 1, 2, 2)
    assert int(re.search(r"kRepSuperMax\s*=\s*(\d+)", src).group(1)) == 257 and "hi - lo <=\n *                        257" in hdr
    # the tile and the fan-out are sa_lz.h's
    assert "kLzTile" in src and sa_lib.LZ_TILE == 4096
    # the host wait the header states is the source's
    assert "Host waits per call: one with d_lcp given" in hdr
    assert "sa_repeats_device with d_lcp: one" in src
    # the header comes after sa_lz.h and is a dependency of the library
    build = open(os.path.join(CSRC, "sa_build.hip")).read()
    assert build.index('#include "sa_lz.h"') < build.index('#include "sa_repeats.h"')
    assert "sa_repeats.h" in open(os.path.join(CSRC, "Makefile")).read()


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    for name in ("sa_repeats_device", "sa_repeats"):
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\bint %s\(" % name, hdr)
    assert "maximal_repeats" in pkg.__all__ and callable(pkg.maximal_repeats)
    assert callable(pkg.DeviceBuilder.repeats) and callable(pkg.SuffixArray.repeats)


P = [ctypes.c_void_p(4096 * k) for k in range(1, 9)]


def _info(a=7, b=7):
    return (ctypes.c_uint64 * 2)(a, b)


def test_device_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call: the pointers are
    fake addresses that are never dereferenced."""
    L = sa_lib.lib()
    info = _info()

    def dev(ctx=P[0], text=P[1], n=6, sa=P[2], lcp=P[3], kind=1, ln=P[4], lo=P[5], hi=P[6], inf=info):
        return L.sa_repeats_device(ctx, text, n, sa, lcp, 1, 2, kind, ln, lo, hi, 10, inf, None)

    cases = (({"ctx": None}, b"context"), ({"inf": None}, b"info is NULL"), ({"n": 1 << 32}, b"n too large"),
             ({"kind": 3}, b"unknown kind"), ({"kind": 0xFFFFFFFF}, b"unknown kind"),
             ({"ln": None}, b"all or none"), ({"lo": None}, b"all or none"), ({"hi": None}, b"all or none"),
             ({"ln": None, "hi": None}, b"all or none"),
             ({"text": None}, b"d_text is NULL"), ({"sa": None}, b"d_sa is NULL"),                 # maximal reads both
             ({"text": None, "kind": 2}, b"d_text is NULL"), ({"sa": None, "kind": 2}, b"d_sa is NULL"),
             ({"text": None, "kind": 0, "lcp": None}, b"d_text is NULL"),                          # the LCP is computed
             ({"sa": None, "kind": 0, "lcp": None}, b"d_sa is NULL"),
             ({"lo": ctypes.c_void_p(4096 * 6 + 2)}, b"not 4-byte aligned"),
             ({"hi": ctypes.c_void_p(4096 * 7 + 1)}, b"not 4-byte aligned"),
             ({"ln": P[1]}, b"aliases"), ({"lo": P[2]}, b"aliases"), ({"hi": P[3]}, b"aliases"),
             ({"ln": P[5]}, b"one buffer"), ({"hi": P[4]}, b"one buffer"), ({"lo": P[6]}, b"one buffer"))
    msgs = set()
    for kw, word in cases:
        assert dev(**kw) == -1, kw
        msg = L.sa_last_error()
        assert word in msg, (kw, msg)
        msgs.add(re.sub(rb"\d+", b"#", msg))
    assert len(msgs) == 10                                          # each rejection has its own message
    assert list(info) == [7, 7]                                     # a rejected call writes nothing
    # n <= 1: SA_OK and a count of 0 without a kernel, whatever the pointers
    for n in (0, 1):
        info = _info()
        assert L.sa_repeats_device(P[0], None, n, None, None, 1, 2, 1, None, None, None, 0, info, None) == 0
        assert list(info) == [0, 0]
        info = _info()
        assert dev(n=n, inf=info) == 0 and list(info) == [0, 0]
        assert dev(n=n, lo=None) == -1 and b"all or none" in L.sa_last_error()
        assert dev(n=n, ctx=None) == -1
    # SA_REP_RIGHT with d_lcp needs neither the text nor the SA: these arguments pass the checks, which is
    # all that can be seen without a device (with one, tests/test_gpu_repeats.py runs exactly this call)


def _host_arrays(width):
    t = np.frombuffer(b"banana", np.uint8)
    s = np.array([5, 3, 1, 0, 4, 2], np.int64 if width == 8 else np.uint32)
    return t, s, np.dtype(np.int64 if width == 8 else np.uint32)


def test_host_form_arguments_rejected_before_any_device(sa_lib):
    L = sa_lib.lib()
    t, s, dt = _host_arrays(4)
    a, b, c = (np.full(7, 99, dt) for _ in range(3))
    info = _info()
    T, S, A, B, C = t.ctypes.data, s.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data
    for args, word in (((T, 6, S, 3, 1, 2, 1, A, B, C, 7, info), b"sa_width"),
                       ((T, 1 << 32, S, 4, 1, 2, 1, A, B, C, 7, info), b"too large"),
                       ((T, 6, S, 4, 1, 2, 1, A, B, C, 7, None), b"info is NULL"),
                       ((T, 6, S, 4, 1, 2, 3, A, B, C, 7, info), b"unknown kind"),
                       ((None, 6, S, 4, 1, 2, 1, A, B, C, 7, info), b"text is NULL"),
                       ((T, 6, None, 4, 1, 2, 1, A, B, C, 7, info), b"sa is NULL"),
                       ((T, 6, S, 4, 1, 2, 1, None, B, C, 7, info), b"all or none"),
                       ((T, 6, S, 4, 1, 2, 1, A, B, None, 7, info), b"all or none"),
                       ((T, 6, S, 4, 1, 2, 1, A, A, C, 7, info), b"one buffer"),
                       ((T, 6, S, 4, 1, 2, 1, A, B, T, 7, info), b"aliases"),
                       ((T, 6, S, 4, 1, 2, 1, S, B, C, 7, info), b"aliases")):
        assert L.sa_repeats(*args) == -1, args
        assert word in L.sa_last_error(), (args, L.sa_last_error())
    assert list(info) == [7, 7] and (a == 99).all() and (b == 99).all() and (c == 99).all()
    # a width-8 SA entry outside [0, n) is rejected before any device work
    t, s, dt = _host_arrays(8)
    a, b, c = (np.full(7, 99, dt) for _ in range(3))
    for bad in (6, -1):
        s2 = s.copy()
        s2[5] = bad
        assert L.sa_repeats(t.ctypes.data, 6, s2.ctypes.data, 8, 1, 2, 1, a.ctypes.data, b.ctypes.data, c.ctypes.data,
                            7, info) == -1
        assert b"out of range" in L.sa_last_error()
    assert list(info) == [7, 7]


def test_host_form_returns_without_a_device(sa_lib):
    """n <= 1: SA_OK, a count of 0, nothing written, with or without a GPU."""
    L = sa_lib.lib()
    a, b, c = (np.full(4, 99, np.uint32) for _ in range(3))
    one = np.frombuffer(b"x", np.uint8)
    sa1 = np.zeros(1, np.uint32)
    for kind in (0, 1, 2):
        info = _info()
        assert L.sa_repeats(None, 0, None, 4, 1, 2, kind, a.ctypes.data, b.ctypes.data, c.ctypes.data, 4, info) == 0
        assert list(info) == [0, 0]
        info = _info()
        assert L.sa_repeats(None, 0, None, 8, 0, 0, kind, None, None, None, 0, info) == 0 and list(info) == [0, 0]
        info = _info()
        assert L.sa_repeats(one.ctypes.data, 1, sa1.ctypes.data, 4, 1, 2, kind, a.ctypes.data, b.ctypes.data,
                            c.ctypes.data, 4, info) == 0
        assert list(info) == [0, 0]
    assert (a == 99).all() and (b == 99).all() and (c == 99).all()
    if sa_lib.device_count() <= 0:
        # anything longer needs the device, and without one the call says so
        from hpc_suffix_array_amd import SAError, maximal_repeats
        t, s, _ = _host_arrays(4)
        info = _info()
        assert L.sa_repeats(t.ctypes.data, 6, s.ctypes.data, 4, 1, 2, 1, a.ctypes.data, b.ctypes.data, c.ctypes.data,
                            4, info) < 0
        assert b"device" in L.sa_last_error()
        with pytest.raises(SAError):
            maximal_repeats(b"banana", s)


def test_python_arguments():
    from hpc_suffix_array_amd import maximal_repeats
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(ValueError):
        maximal_repeats(b"banana", sa[:5])
    with pytest.raises(ValueError, match="unknown kind"):
        maximal_repeats(b"banana", sa, kind="tandem")
    with pytest.raises(ValueError, match="negative"):
        maximal_repeats(b"banana", sa, min_len=-1)
