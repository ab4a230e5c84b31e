"""The host-compilable core of the longest previous factor array and the LZ77
parse (hpc_suffix_array_amd/csrc/sa_lz.h): g++ builds tests/cpp/lz_check.cpp,
which checks the nearest-smaller walks with LCP minima (fan-out 64 and 4, whole
and window-then-whole as the kernel composes them) against the O(n^2)
definition, the tiled parse (B = 4, 8, 16) against the serial walk, and the
64-bit arithmetic at n = 2^32 - 1, once plainly and once with
-fsanitize=address,undefined as a stand-alone program.  Plus the constants'
copies, the exported symbols, and what the four entry points decide before
they touch a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "lz_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    # 310 texts of 0 .. 300 bytes, two fan-outs, two walks per rank, three tile sizes
    assert int(out.stdout.split()[1]) > 200_000, out.stdout
    assert int(out.stdout.split()[4]) >= 300, out.stdout


def test_lz_core_matches_definition(tmp_path):
    _build_and_run(tmp_path, "lz_check", ["-O2"], 300)


def test_lz_core_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: every level of the
    hierarchy, every tile and every candidate list is an exact-size heap
    array, so a walk or a jump that leaves one aborts."""
    _build_and_run(tmp_path, "lz_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_lz.h")).read()
    assert int(re.search(r"#define\s+SA_LPF_NONE\s+(0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == sa_lib.LPF_NONE == 0xFFFFFFFF
    assert int(re.search(r"kLpfNone\s*=\s*(0x[0-9A-Fa-f]+)u", src).group(1), 16) == sa_lib.LPF_NONE
    assert re.search(r"static_assert\(SA_LPF_NONE == kLpfNone", src)
    assert int(re.search(r"kLzTile\s*=\s*(\d+)", src).group(1)) == sa_lib.LZ_TILE == 4096
    assert int(re.search(r"kLzFan\s*=\s*(\d+)", src).group(1)) ** 2 == sa_lib.LZ_TILE
    # the host waits the header states are the source's
    assert "Host waits per call: three" in hdr and "Host waits per call: none with d_lcp given" in hdr
    assert "sa_lz77_device: three" in src and "sa_lpf_device with d_lcp: none" in src


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    for name in ("sa_lpf_device", "sa_lpf", "sa_lz77_device", "sa_lz77"):
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\bint %s\(" % name, hdr)
    for name in ("longest_previous_factor", "lz77_factorize"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert callable(pkg.DeviceBuilder.lpf) and callable(pkg.DeviceBuilder.lz77)
    assert callable(pkg.SuffixArray.lpf) and callable(pkg.SuffixArray.lz77)


P = [ctypes.c_void_p(4096 * k) for k in range(1, 9)]


def _reject(L, call, cases, n_messages):
    msgs = set()
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = L.sa_last_error()
        assert word in msg, (kw, msg)
        msgs.add(msg)
    assert len(msgs) == n_messages   # each rejection has its own message


def test_lpf_device_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call: the pointers are
    fake addresses that are never dereferenced."""
    L = sa_lib.lib()

    def dev(ctx=P[0], text=P[1], n=6, sa=P[2], lcp=P[3], lpf=P[4], src=P[5]):
        return L.sa_lpf_device(ctx, text, n, sa, lcp, lpf, src, None)

    _reject(L, dev, (({"ctx": None}, b"context"), ({"n": 1 << 32}, b"n too large"), ({"sa": None}, b"d_sa is NULL"),
                     ({"lpf": None}, b"d_lpf is NULL"), ({"src": None}, b"d_src is NULL"),
                     ({"text": None, "lcp": None}, b"both NULL"),
                     ({"lpf": ctypes.c_void_p(4096 * 5 + 2)}, b"d_lpf is not 4-byte aligned"),
                     ({"src": ctypes.c_void_p(4096 * 6 + 1)}, b"d_src is not 4-byte aligned"),
                     ({"lpf": P[1]}, b"aliases"), ({"lpf": P[2]}, b"aliases"), ({"src": P[3]}, b"aliases"),
                     ({"src": P[4]}, b"one buffer")), 10)
    # n == 0: nothing to do, whatever the pointers; a NULL context is still an error
    assert L.sa_lpf_device(P[0], None, 0, None, None, None, None, None) == 0
    assert L.sa_lpf_device(None, None, 0, None, None, None, None, None) == -1


def test_lz77_device_arguments_rejected_before_any_device(sa_lib):
    L = sa_lib.lib()
    z = ctypes.c_uint64(7)

    def dev(ctx=P[0], n=6, lpf=P[1], src=P[2], pos=P[3], ln=P[4], fsrc=P[5], zz=ctypes.byref(z)):
        return L.sa_lz77_device(ctx, n, lpf, src, pos, ln, fsrc, 10, zz, None)

    _reject(L, dev, (({"ctx": None}, b"context"), ({"zz": None}, b"z is NULL"), ({"n": 1 << 32}, b"n too large"),
                     ({"lpf": None}, b"d_lpf is NULL"), ({"src": None}, b"d_src is NULL"),
                     ({"pos": None}, b"all or none"), ({"ln": None}, b"all or none"), ({"fsrc": None}, b"all or none"),
                     ({"pos": None, "ln": None}, b"all or none"),
                     ({"ln": ctypes.c_void_p(4096 * 5 + 2)}, b"not 4-byte aligned"),
                     ({"pos": P[1]}, b"aliases"), ({"fsrc": P[2]}, b"aliases"),
                     ({"pos": P[4]}, b"one buffer"), ({"fsrc": P[3]}, b"one buffer"), ({"ln": P[5]}, b"one buffer")), 9)
    assert z.value == 7   # a rejected call writes nothing
    # n == 0: SA_OK and z = 0 without a kernel, with or without outputs
    assert L.sa_lz77_device(P[0], 0, None, None, None, None, None, 0, ctypes.byref(z), None) == 0 and z.value == 0
    z.value = 7
    assert dev(n=0) == 0 and z.value == 0
    assert dev(n=0, pos=None) == -1 and b"all or none" in L.sa_last_error()


def _host_arrays(width):
    t = np.frombuffer(b"banana", np.uint8)
    s = np.array([5, 3, 1, 0, 4, 2], np.int64 if width == 8 else np.uint32)
    return t, s, np.dtype(np.int64 if width == 8 else np.uint32)


def test_host_forms_arguments_rejected_before_any_device(sa_lib):
    L = sa_lib.lib()
    t, s, dt = _host_arrays(4)
    a, b, c = (np.full(7, 99, dt) for _ in range(3))
    z = ctypes.c_uint64(7)
    zp = ctypes.byref(z)
    T, S, A, B, C = t.ctypes.data, s.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data
    for args, word in (((T, 6, S, 3, A, B), b"sa_width"), ((T, 1 << 32, S, 4, A, B), b"too large"),
                       ((None, 6, S, 4, A, B), b"text is NULL"), ((T, 6, None, 4, A, B), b"sa is NULL"),
                       ((T, 6, S, 4, None, B), b"lpf_out is NULL"), ((T, 6, S, 4, A, None), b"src_out is NULL"),
                       ((T, 6, S, 4, A, A), b"aliases"), ((T, 6, S, 4, T, B), b"aliases"), ((T, 6, S, 4, A, S), b"aliases")):
        assert L.sa_lpf(*args) == -1, args
        assert word in L.sa_last_error(), (args, L.sa_last_error())
    for args, word in (((T, 6, S, 5, A, B, C, 7, zp), b"sa_width"), ((T, 1 << 32, S, 4, A, B, C, 7, zp), b"too large"),
                       ((None, 6, S, 4, A, B, C, 7, zp), b"text is NULL"), ((T, 6, None, 4, A, B, C, 7, zp), b"sa is NULL"),
                       ((T, 6, S, 4, A, B, C, 7, None), b"z is NULL"), ((T, 6, S, 4, None, B, C, 7, zp), b"all or none"),
                       ((T, 6, S, 4, A, B, None, 7, zp), b"all or none"), ((T, 6, S, 4, A, A, C, 7, zp), b"one buffer"),
                       ((T, 6, S, 4, A, B, T, 7, zp), b"aliases"), ((T, 6, S, 4, S, B, C, 7, zp), b"aliases")):
        assert L.sa_lz77(*args) == -1, args
        assert word in L.sa_last_error(), (args, L.sa_last_error())
    assert z.value == 7 and (a == 99).all() and (b == 99).all() and (c == 99).all()
    # a width-8 SA entry outside [0, n) is rejected before any device work
    t, s, dt = _host_arrays(8)
    a, b, c = (np.full(7, 99, dt) for _ in range(3))
    for bad in (6, -1):
        s2 = s.copy()
        s2[5] = bad
        assert L.sa_lpf(t.ctypes.data, 6, s2.ctypes.data, 8, a.ctypes.data, b.ctypes.data) == -1
        assert b"out of range" in L.sa_last_error()
        assert L.sa_lz77(t.ctypes.data, 6, s2.ctypes.data, 8, a.ctypes.data, b.ctypes.data, c.ctypes.data, 7, zp) == -1
        assert b"out of range" in L.sa_last_error()


def test_host_forms_return_without_a_device(sa_lib):
    """n == 0: SA_OK, z = 0, nothing written, with or without a GPU."""
    L = sa_lib.lib()
    a, b, c = (np.full(4, 99, np.uint32) for _ in range(3))
    z = ctypes.c_uint64(7)
    assert L.sa_lpf(None, 0, None, 4, a.ctypes.data, b.ctypes.data) == 0
    assert L.sa_lpf(None, 0, None, 8, None, None) == 0
    assert L.sa_lz77(None, 0, None, 4, a.ctypes.data, b.ctypes.data, c.ctypes.data, 4, ctypes.byref(z)) == 0
    assert z.value == 0
    z.value = 7
    assert L.sa_lz77(None, 0, None, 8, None, None, None, 0, ctypes.byref(z)) == 0 and z.value == 0
    assert (a == 99).all() and (b == 99).all() and (c == 99).all()
    if sa_lib.device_count() <= 0:
        # anything longer needs the device, and without one the call says so
        from hpc_suffix_array_amd import SAError, longest_previous_factor, lz77_factorize
        t, s, _ = _host_arrays(4)
        assert L.sa_lpf(t.ctypes.data, 6, s.ctypes.data, 4, a.ctypes.data, b.ctypes.data) < 0
        assert b"device" in L.sa_last_error()
        with pytest.raises(SAError):
            longest_previous_factor(b"banana", s)
        with pytest.raises(SAError):
            lz77_factorize(b"banana", s)


def test_python_arguments():
    from hpc_suffix_array_amd import longest_previous_factor, lz77_factorize
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(ValueError):
        longest_previous_factor(b"banana", sa[:5])
    with pytest.raises(ValueError):
        lz77_factorize(b"banana", sa[:5])
