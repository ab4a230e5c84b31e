"""The host-compilable core of the k-difference search (hpc_suffix_array_amd/
csrc/sa_edit.h): g++ builds tests/cpp/edit_check.cpp, which checks the band
step, a candidate's mask, the backward finish and the clipping at 0 and n
against the plain full DP, once plainly and once with
-fsanitize=address,undefined as a stand-alone program.  Plus the constants'
copies, the exported symbols, what sa_edit / sa_edit_device decide before they
touch a device, and the Python errors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "edit_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 1_000_000, out.stdout


def test_edit_core_matches_the_full_dp(tmp_path):
    _build_and_run(tmp_path, "edit_check", ["-O2"], 300)


def test_edit_core_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: texts and patterns
    are exact-size heap buffers, so a window that reads past either end of
    either aborts."""
    _build_and_run(tmp_path, "edit_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_edit.h")).read()
    assert int(re.search(r"#define\s+SA_EDIT_MAX_K\s+(\d+)", hdr).group(1)) == sa_lib.EDIT_MAX_K == 31
    assert int(re.search(r"#define\s+SA_EDIT_INFO\s+(\d+)", hdr).group(1)) == sa_lib.EDIT_INFO == 3
    assert int(re.search(r"#define\s+SA_EDIT_TOO_MANY\s+(\d+)", hdr).group(1)) == sa_lib.EDIT_TOO_MANY == 1
    # the source asserts each of the header's values at compile time; the band of the largest budget fits a word
    assert re.search(r"static_assert\(SA_EDIT_MAX_K == 31 && SA_EDIT_INFO == 3 && SA_EDIT_TOO_MANY == 1", src)
    assert int(re.search(r"kEditMaxK\s*=\s*(\d+)", src).group(1)) == sa_lib.EDIT_MAX_K
    assert 2 * sa_lib.EDIT_MAX_K + 1 <= 63
    assert "sa_edit.h" in open(os.path.join(CSRC, "Makefile")).read()
    build = open(os.path.join(CSRC, "sa_build.hip")).read()
    assert build.index('#include "sa_hamming.h"') < build.index('#include "sa_edit.h"')


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    for name in ("sa_edit_device", "sa_edit"):
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    assert re.search(r"\bint sa_edit_device\(", hdr) and re.search(r"\bint sa_edit\(", hdr)
    assert "edit_search" in pkg.__all__ and callable(pkg.edit_search)
    assert callable(pkg.DeviceBuilder.edit) and callable(pkg.SuffixArray.edit)


def test_device_form_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call: the pointers are
    fake addresses that are never dereferenced."""
    L = sa_lib.lib()
    P = [ctypes.c_void_p(4096 * k) for k in range(1, 10)]
    info = (ctypes.c_uint64 * 3)(7, 7, 7)

    def dev(ctx=P[0], text=P[1], n=6, sa=P[2], pat=P[3], pat_bytes=4, poff=P[4], nq=1, k=1, flags=0, off=P[5],
            end=P[6], start=P[7], dist=P[8], inf=info):
        return L.sa_edit_device(ctx, text, n, sa, pat, pat_bytes, poff, nq, k, 0, flags, off, end, start, dist, 10,
                                inf, None)

    msgs = set()
    cases = (({"ctx": None}, b"context"), ({"text": None}, b"d_text"), ({"sa": None}, b"d_sa"),
             ({"pat": None}, b"d_pat is NULL"), ({"poff": None}, b"d_pat_off"), ({"off": None}, b"d_off"),
             ({"inf": None}, b"info"), ({"n": 1 << 32}, b"n too large"), ({"nq": 1 << 32}, b"nq too large"),
             ({"k": 32}, b"SA_EDIT_MAX_K"), ({"k": 256}, b"SA_EDIT_MAX_K"), ({"k": 1 << 40}, b"SA_EDIT_MAX_K"),
             ({"nq": 1 << 27, "k": 31}, b"pieces"), ({"nq": (1 << 32) - 1, "k": 1}, b"pieces"),
             ({"flags": 1}, b"unknown flags"), ({"flags": 2}, b"unknown flags"), ({"flags": 0x80000000}, b"unknown flags"),
             ({"end": None, "dist": None}, b"d_start without d_end"), ({"end": None, "start": None}, b"d_dist without d_end"),
             ({"end": None}, b"without d_end"),
             ({"off": P[1]}, b"aliases"), ({"end": P[2]}, b"aliases"), ({"start": P[3]}, b"aliases"),
             ({"dist": P[4]}, b"aliases"), ({"start": P[1]}, b"aliases"),
             ({"end": P[5]}, b"one buffer"), ({"start": P[5]}, b"one buffer"), ({"dist": P[5]}, b"one buffer"),
             ({"start": P[6]}, b"one buffer"), ({"dist": P[6]}, b"one buffer"), ({"dist": P[7]}, b"one buffer"))
    for kw, word in cases:
        assert dev(**kw) == -1, kw
        msg = L.sa_last_error()
        assert word in msg, (kw, msg)
        msgs.add(re.sub(rb"[0-9]+|0x[0-9a-f]+", b"#", msg))
    assert len(msgs) == 16          # each rejection has its own message
    assert list(info) == [7, 7, 7]  # a rejected call writes nothing


def _host(L, text=b"banana", sa=(5, 3, 1, 0, 4, 2), width=4, pat=b"anan", poff=(0, 4), n=None, nq=None, k=1, flags=0,
          outs=True, cap=16, info=None, same=None, only=None):
    t = np.frombuffer(text, np.uint8)
    s = np.array(sa, np.int64 if width == 8 else np.uint32)
    p = np.frombuffer(pat, np.uint8)
    po = np.array(poff, np.uint64)
    n = len(text) if n is None else n
    nq = len(poff) - 1 if nq is None else nq
    wide = np.int64 if width == 8 else np.uint32
    off = np.full(len(poff) + 2, 99, np.uint64)
    end = np.full(cap + 1, 99, wide)
    start = np.full(cap + 1, 99, wide)
    ds = np.full(cap + 1, 99, np.uint8)
    info = (ctypes.c_uint64 * 3)(7, 7, 7) if info is None else info
    ep = end.ctypes.data if outs else None
    sp = start.ctypes.data if outs or only == "start" else None
    dp = ds.ctypes.data if outs or only == "dist" else None
    op = off.ctypes.data
    if same == "end":
        ep = t.ctypes.data
    if same == "start":
        sp = s.ctypes.data
    if same == "off":
        op = po.ctypes.data
    if same == "dist":
        dp = ep
    if same == "start_end":
        sp = ep
    rc = L.sa_edit(t.ctypes.data if n else None, n, s.ctypes.data if n else None, width,
                   p.ctypes.data if len(pat) else None, po.ctypes.data, nq, k, 0, flags, op, ep, sp, dp, cap, info)
    return rc, off, end, start, ds, list(info)


def test_host_form_arguments_rejected_before_any_device(sa_lib):
    L = sa_lib.lib()
    for kw, word in (({"width": 3}, b"sa_width"), ({"n": 1 << 32}, b"too large"), ({"nq": 1 << 32}, b"nq too large"),
                     ({"k": 32}, b"SA_EDIT_MAX_K"), ({"nq": 1 << 27, "k": 31}, b"pieces"),
                     ({"flags": 1}, b"unknown flags"), ({"flags": 4}, b"unknown flags"),
                     ({"outs": False, "only": "start"}, b"start_out without end_out"),
                     ({"outs": False, "only": "dist"}, b"dist_out without end_out"),
                     ({"poff": (0, 4, 2)}, b"offsets decrease"),
                     ({"same": "end"}, b"aliases"), ({"same": "start"}, b"aliases"), ({"same": "off"}, b"aliases"),
                     ({"same": "dist"}, b"one buffer"), ({"same": "start_end"}, b"one buffer"),
                     ({"sa": (5, 3, 1, 0, 4, 6), "width": 8}, b"out of range"),
                     ({"sa": (5, 3, 1, 0, 4, -1), "width": 8}, b"out of range")):
        rc, off, end, start, ds, info = _host(L, **kw)
        assert rc == -1, kw
        assert word in L.sa_last_error(), (kw, L.sa_last_error())
        assert info == [7, 7, 7] and (end == 99).all() and (start == 99).all() and (ds == 99).all(), kw
        if kw.get("same") != "off":
            assert (off == 99).all(), kw
    t = np.frombuffer(b"banana", np.uint8)
    s = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    po = np.array([0, 4], np.uint64)
    off = np.zeros(2, np.uint64)
    out = np.zeros(4, np.uint32)
    info = (ctypes.c_uint64 * 3)()
    a = (t.ctypes.data, 6, s.ctypes.data, 4, t.ctypes.data, po.ctypes.data, 1, 1, 0, 0)
    assert L.sa_edit(*a, None, out.ctypes.data, None, None, 4, info) == -1 and b"off_out" in L.sa_last_error()
    assert L.sa_edit(*a, off.ctypes.data, None, None, None, 0, None) == -1 and b"info" in L.sa_last_error()
    b = (po.ctypes.data, 1, 1, 0, 0, off.ctypes.data, None, None, None, 0, info)
    assert L.sa_edit(None, 6, s.ctypes.data, 4, t.ctypes.data, *b) == -1 and b"text is NULL" in L.sa_last_error()
    assert L.sa_edit(t.ctypes.data, 6, None, 4, t.ctypes.data, *b) == -1 and b"sa is NULL" in L.sa_last_error()
    assert L.sa_edit(t.ctypes.data, 6, s.ctypes.data, 4, None, *b) == -1 and b"pat is NULL" in L.sa_last_error()
    assert L.sa_edit(t.ctypes.data, 6, s.ctypes.data, 4, t.ctypes.data, None, *b[1:]) == -1 \
        and b"pat_off is NULL" in L.sa_last_error()


def test_host_form_returns_without_a_device(sa_lib):
    """nq == 0 and n == 0: SA_OK, off all zero, the pieces counted, nothing
    else written, with or without a GPU."""
    L = sa_lib.lib()
    for kw, nq, k in (({"n": 0}, 1, 1), ({"n": 0, "poff": (0, 2, 4), "k": 3}, 2, 3), ({"nq": 0, "poff": (0,)}, 0, 1),
                      ({"n": 0, "nq": 0, "poff": (0,)}, 0, 1), ({"n": 0, "outs": False}, 1, 1),
                      ({"n": 0, "k": 31}, 1, 31)):
        rc, off, end, start, ds, info = _host(L, **kw)
        assert rc == 0, kw
        assert (off[:nq + 1] == 0).all() and (off[nq + 1:] == 99).all(), kw
        assert (end == 99).all() and (start == 99).all() and (ds == 99).all() and info == [0, 0, nq * (k + 1)], kw
    # anything else needs the device, and without one the call says so
    if sa_lib.device_count() <= 0:
        from hpc_suffix_array_amd import SAError, edit_search
        rc = _host(L)[0]
        assert rc < 0 and b"device" in L.sa_last_error()
        with pytest.raises(SAError):
            edit_search(b"banana", np.array([5, 3, 1, 0, 4, 2], np.uint32), [b"anan"], 1)


def test_edit_python_arguments():
    from hpc_suffix_array_amd import edit_search
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(ValueError):
        edit_search(b"banana", sa[:5], [b"anan"], 1)
    with pytest.raises(ValueError):
        edit_search(b"banana", sa, [b"anan"], 32)
    with pytest.raises(ValueError):
        edit_search(b"banana", sa, [b"anan"], -1)
    with pytest.raises(ValueError):
        edit_search(b"banana", sa, [b"anan"], 1, max_candidates=-1)
    with pytest.raises(TypeError):
        edit_search(b"banana", sa, b"anan", 1)
