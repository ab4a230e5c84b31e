"""The host-compilable core of the LF-mapping and the inverse BWT
(hpc_suffix_array_amd/csrc/sa_ibwt.h): g++ builds tests/cpp/ibwt_check.cpp,
which runs the LF rule with the primary row apart, the splitter predicate and
directory, walk 1, the pointer jumping, the verdict and walk 2 with its byte
packing against brute force: every (bwt, primary) over {a,b}^n for n <= 10,
texts of 0 .. 300 bytes over 1, 2, 4 and 256 symbols, one rank in 64 and one
in 4 a splitter, and the arithmetic at n = 2^32 - 1; once plainly and once with
-fsanitize=address,undefined as a stand-alone program.  Plus the constants'
copies, the exported symbols, the host waits the header states, and what the
entry points decide before they touch a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "ibwt_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    w = out.stdout.split()
    assert int(w[1]) > 1_000_000, out.stdout                        # checks
    assert int(w[4]) >= 300, out.stdout                             # texts
    # {a,b}^n, n <= 10, every primary: 18,434 pairs, 2,046 of them the image of a text (and random pairs on top)
    assert int(w[9]) >= 18_434 and int(w[6]) >= 2_046, out.stdout


def test_ibwt_core_matches_brute_force(tmp_path):
    _build_and_run(tmp_path, "ibwt_check", ["-O2"], 300)


def test_ibwt_core_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: LF, first[], the
    splitter words and counts, both node buffers, the text and the SA are
    exact-size heap arrays, so a walk or a store that leaves one aborts."""
    _build_and_run(tmp_path, "ibwt_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_ibwt.h")).read()
    assert int(re.search(r"#define\s+SA_IBWT_INFO\s+(\d+)", hdr).group(1)) == 3
    assert int(re.search(r"kIbwtInfo\s*=\s*(\d+)", src).group(1)) == 3 == sa_lib.IBWT_INFO
    assert re.search(r"static_assert\(SA_IBWT_INFO == kIbwtInfo", src)
    assert int(re.search(r"kLfTile\s*=\s*(\d+)", src).group(1)) == sa_lib.LF_TILE
    assert 1 << int(re.search(r"kIbwtSplitBits\s*=\s*(\d+)", src).group(1)) == sa_lib.IBWT_S == 64
    words, ranks = (int(re.search(r"%s\s*=\s*(\d+)" % k, src).group(1)) for k in ("kIbwtTileWords", "kIbwtWordRanks"))
    assert words * ranks == sa_lib.IBWT_TILE
    assert "0x9E3779B1u" in src
    # the header comes after sa_bwt.h and what it needs, and is a dependency of the library
    build = open(os.path.join(CSRC, "sa_build.hip")).read()
    for dep in ("sa_bwt.h", "sa_host.h", "sa_locate.h", "sa_mem.h"):
        assert build.index('#include "%s"' % dep) < build.index('#include "sa_ibwt.h"')
    assert build.index("static int scan_i64(") < build.index('#include "sa_ibwt.h"')
    assert "sa_ibwt.h" in open(os.path.join(CSRC, "Makefile")).read()


def test_host_waits_stated_and_counted():
    """The statements about host waits in sa_hip.h and sa_ibwt.h agree with
    each other and with the source: the only host_sync of the device forms is
    ibwt_device's one, and lf_device / lf_launch have none."""
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_ibwt.h")).read()
    assert "sa_lf_device: none.  sa_ibwt_device: one" in src
    assert "Asynchronous on `stream`: no host wait" in hdr and "Host waits\n * per call: one" in hdr

    def body(name):
        at = src.index("static int %s(" % name)
        return src[at:src.index("\n}\n", at)]

    assert body("ibwt_device").count("host_sync(") == 1
    for name in ("lf_device", "lf_launch", "lf_check_args", "ibwt_check_args"):
        assert "host_sync" not in body(name) and "hipMemcpy(" not in body(name)
    # walk 2 is enqueued before that wait and reads the verdict on the device
    b = body("ibwt_device")
    assert b.index("k_ibwt_walk2") < b.index("host_sync(")
    assert "if (dinfo[2] != n) return;" in src


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    for name in ("sa_lf_device", "sa_ibwt_device", "sa_lf", "sa_ibwt", "sa_ibwt_ex"):
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\bint %s\(" % name, hdr)
    for name in ("lf_mapping", "inverse_bwt"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert callable(pkg.DeviceBuilder.lf) and callable(pkg.DeviceBuilder.ibwt)


P = [ctypes.c_void_p(4096 * k) for k in range(1, 9)]


def _info(v=7):
    return (ctypes.c_uint64 * 3)(v, v, v)


def test_device_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call: the pointers are
    fake addresses that are never dereferenced."""
    L = sa_lib.lib()
    info = _info()

    def ibwt(ctx=P[0], bwt=P[1], n=6, p=3, text=P[2], sa=P[3], inf=info):
        return L.sa_ibwt_device(ctx, bwt, n, p, text, sa, inf, None)

    def lf(ctx=P[0], bwt=P[1], n=6, p=3, out=P[2]):
        return L.sa_lf_device(ctx, bwt, n, p, out, None)

    msgs = set()
    for call, cases in ((ibwt, (({"ctx": None}, b"context"), ({"n": 1 << 32}, b"n too large"), ({"bwt": None}, b"d_bwt is NULL"),
                                ({"text": None}, b"d_text is NULL"), ({"p": 6}, b"primary index 6"), ({"p": 11}, b"primary index 11"),
                                ({"p": (1 << 64) - 1}, b"primary index"), ({"text": P[1]}, b"d_text may not alias"),
                                ({"sa": P[1]}, b"d_sa may not alias"), ({"sa": P[2]}, b"d_sa may not alias"),
                                ({"sa": ctypes.c_void_p(4096 * 4 + 2)}, b"d_sa is not 4-byte aligned"))),
                        (lf, (({"ctx": None}, b"context"), ({"n": 1 << 32}, b"n too large"), ({"bwt": None}, b"d_bwt is NULL"),
                              ({"out": None}, b"d_lf is NULL"), ({"p": 6}, b"primary index 6"), ({"p": 1 << 40}, b"primary index"),
                              ({"out": P[1]}, b"d_lf may not alias"),
                              ({"out": ctypes.c_void_p(4096 * 3 + 1)}, b"d_lf is not 4-byte aligned")))):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            msg = L.sa_last_error()
            assert word in msg, (kw, msg)
            msgs.add(re.sub(rb"\d+", b"#", msg))
    assert len(msgs) == 11                                          # each rejection has its own message
    assert list(info) == [7, 7, 7]                                  # a rejected call writes nothing
    # n == 0: SA_OK without a device, the info words zeroed, whatever the pointers and the primary index
    info = _info()
    assert L.sa_ibwt_device(P[0], None, 0, 0, None, None, info, None) == 0 and list(info) == [0, 0, 0]
    info = _info()
    assert ibwt(n=0, p=9, inf=info) == 0 and list(info) == [0, 0, 0]
    assert ibwt(n=0, inf=None) == 0 and ibwt(n=0, ctx=None) == -1
    assert lf(n=0) == 0 and L.sa_lf_device(P[0], None, 0, 5, None, None) == 0 and lf(n=0, ctx=None) == -1
    # a d_sa of NULL and an info of NULL are what the text-only call passes: they get past every check,
    # which is all that can be seen without a device (tests/test_gpu_ibwt.py runs that call)


def test_host_form_arguments_rejected_before_any_device(sa_lib):
    L = sa_lib.lib()
    b = np.frombuffer(b"annb$aa".replace(b"$", b"a"), np.uint8).copy()
    n = int(b.size)
    text = np.full(n, 99, np.uint8)
    out = np.full(n, 99, np.uint32)
    info = _info()
    B, T, O = b.ctypes.data, text.ctypes.data, out.ctypes.data
    for args, word in (((B, n, 3, T, O, 3, info), b"sa_width"), ((B, n, 3, T, O, 0, info), b"sa_width"),
                       ((B, 1 << 32, 3, T, O, 4, info), b"too large"),
                       ((None, n, 3, T, O, 4, info), b"NULL host pointer"), ((B, n, 3, None, O, 4, info), b"NULL host pointer"),
                       ((B, n, n, T, O, 4, info), b"primary index 7"), ((B, n, n + 5, T, O, 8, info), b"primary index 12"),
                       ((B, n, 3, B, O, 4, info), b"text_out may not alias"),
                       ((B, n, 3, T, B, 4, info), b"sa_out may not alias"), ((B, n, 3, T, T, 4, info), b"sa_out may not alias")):
        assert L.sa_ibwt_ex(*args) == -1, args
        assert word in L.sa_last_error(), (args, L.sa_last_error())
        assert L.sa_ibwt(*args[:6]) == -1 and word in L.sa_last_error()
        assert list(info) == [0, 0, 0]                              # zeroed first, as the header says
        info[0] = info[1] = info[2] = 7
    for args, word in (((B, n, 3, O, 2), b"sa_width"), ((B, 1 << 32, 3, O, 4), b"too large"), ((None, n, 3, O, 4), b"NULL host pointer"),
                       ((B, n, 3, None, 8), b"NULL host pointer"), ((B, n, n, O, 4), b"primary index 7"),
                       ((B, n, n + 5, O, 4), b"primary index 12"), ((B, n, 3, B, 4), b"lf_out may not alias")):
        assert L.sa_lf(*args) == -1, args
        assert word in L.sa_last_error(), (args, L.sa_last_error())
    assert (text == 99).all() and (out == 99).all()


def test_host_forms_return_without_a_device(sa_lib):
    """n == 0: SA_OK, nothing written, with or without a GPU."""
    L = sa_lib.lib()
    text = np.full(4, 99, np.uint8)
    out = np.full(4, 99, np.uint32)
    info = _info()
    assert L.sa_ibwt_ex(None, 0, 0, text.ctypes.data, out.ctypes.data, 4, info) == 0 and list(info) == [0, 0, 0]
    assert L.sa_ibwt(None, 0, 7, None, None, 8) == 0
    assert L.sa_lf(None, 0, 0, out.ctypes.data, 4) == 0 and L.sa_lf(None, 0, 3, None, 8) == 0
    assert (text == 99).all() and (out == 99).all()
    from hpc_suffix_array_amd import SAError, inverse_bwt, lf_mapping
    assert inverse_bwt(b"", 0).size == 0 and lf_mapping(b"", 0).size == 0
    t, s, i = inverse_bwt(b"", 0, return_sa=True, width=8, return_info=True)
    assert t.dtype == np.uint8 and s.dtype == np.int64 and s.size == 0 and i == {"splitters": 0, "longest_sublist": 0, "steps": 0}
    if sa_lib.device_count() <= 0:
        # anything longer needs the device, and without one the call says so
        assert L.sa_ibwt(b"nnbaaa", 6, 3, text.ctypes.data, None, 4) < 0 and b"device" in L.sa_last_error()
        with pytest.raises(SAError, match="device"):
            inverse_bwt(b"nnbaaa", 3)
        with pytest.raises(SAError, match="device"):
            lf_mapping(b"nnbaaa", 3)


def test_python_arguments():
    from hpc_suffix_array_amd import SAError, inverse_bwt, lf_mapping
    for f in (lf_mapping, inverse_bwt):
        with pytest.raises(ValueError, match="width"):
            f(b"nnbaaa", 3, width=2)
        with pytest.raises(ValueError, match="negative"):
            f(b"nnbaaa", -1)
        # primary = n and n + 5: the library's rejection, before any device work
        for p in (6, 11):
            with pytest.raises(SAError, match="primary index %d" % p):
                f(b"nnbaaa", p)
