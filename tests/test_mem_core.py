"""The host-compilable core of the maximal exact matches (hpc_suffix_array_amd/
csrc/sa_mem.h): g++ builds tests/cpp/mem_check.cpp, which checks the right
extension, the left check, the seed rule, the clamp and the compaction
argument against brute force, once plainly and once with
-fsanitize=address,undefined as a stand-alone program.  Plus the constants'
copies, the exported symbols, and what sa_mems / sa_mems_device decide before
they touch a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "mem_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 1_000_000, out.stdout


def test_mem_core_matches_brute_force(tmp_path):
    _build_and_run(tmp_path, "mem_check", ["-O2"], 300)


def test_mem_core_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: texts and queries are
    exact-size heap buffers, so an extension or a left check that reads past
    either end of either string aborts."""
    _build_and_run(tmp_path, "mem_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_mem.h")).read()
    assert int(re.search(r"#define\s+SA_MEM_INFO\s+(\d+)", hdr).group(1)) == sa_lib.MEM_INFO == 3
    assert int(re.search(r"#define\s+SA_MEM_TOO_MANY\s+(\d+)", hdr).group(1)) == sa_lib.MEM_TOO_MANY == 1
    assert int(re.search(r"#define\s+SA_MEM_LANE\s+(\d+)u", hdr).group(1)) == sa_lib.MEM_LANE == 1
    assert int(re.search(r"#define\s+SA_MEM_WAVE\s+(\d+)u", hdr).group(1)) == sa_lib.MEM_WAVE == 2
    assert sa_lib.MEM_MODES == {"auto": 0, "lane": sa_lib.MEM_LANE, "wave": sa_lib.MEM_WAVE}
    # the source asserts the header's values at compile time, and the hand-over the header states is the source's
    assert re.search(r"static_assert\(SA_MEM_INFO == 3 && SA_MEM_TOO_MANY == 1 && SA_MEM_LANE == 1u && "
                     r"SA_MEM_WAVE == 2u", src)
    lane_bytes = int(re.search(r"kMemLaneBytes\s*=\s*(\d+)", src).group(1))
    assert lane_bytes % 8 == 0 and f"passes {lane_bytes} bytes" in hdr


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    for name in ("sa_mems_device", "sa_mems"):
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    assert re.search(r"\bint sa_mems_device\(", hdr) and re.search(r"\bint sa_mems\(", hdr)
    assert "maximal_exact_matches" in pkg.__all__ and callable(pkg.maximal_exact_matches)
    assert callable(pkg.DeviceBuilder.mems) and callable(pkg.SuffixArray.mems)


def test_device_form_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call: the pointers are
    fake addresses that are never dereferenced."""
    L = sa_lib.lib()
    P = [ctypes.c_void_p(4096 * k) for k in range(1, 8)]
    info = (ctypes.c_uint64 * 3)(7, 7, 7)

    def dev(ctx=P[0], text=P[1], n=6, sa=P[2], query=P[3], m=4, min_len=2, flags=0, off=P[4], tpos=P[5], ln=P[6],
            inf=info):
        return L.sa_mems_device(ctx, text, n, sa, query, m, min_len, 0, 0, flags, off, tpos, ln, 10, inf, None)

    msgs = set()
    cases = (({"ctx": None}, b"context"), ({"text": None}, b"d_text"), ({"sa": None}, b"d_sa"),
             ({"query": None}, b"d_query"), ({"off": None}, b"d_off"), ({"inf": None}, b"info"),
             ({"n": 1 << 32}, b"n too large"), ({"m": 1 << 32}, b"m too large"), ({"min_len": 0}, b"min_len"),
             ({"flags": 4}, b"unknown flags"), ({"flags": 0x80000000}, b"unknown flags"), ({"flags": 3}, b"exclude"),
             ({"tpos": None}, b"both or neither"), ({"ln": None}, b"both or neither"),
             ({"off": P[1]}, b"aliases"), ({"tpos": P[2]}, b"aliases"), ({"ln": P[3]}, b"aliases"),
             ({"tpos": P[6]}, b"one buffer"), ({"tpos": P[4]}, b"one buffer"))
    for kw, word in cases:
        assert dev(**kw) == -1, kw
        msg = L.sa_last_error()
        assert word in msg, (kw, msg)
        msgs.add(msg.split(b" 0x")[0])
    assert len(msgs) == 14          # each rejection has its own message
    assert list(info) == [7, 7, 7]  # a rejected call writes nothing


def _host(L, text=b"banana", sa=(5, 3, 1, 0, 4, 2), width=4, query=b"anan", n=None, m=None, min_len=2, flags=0,
          outs=True, cap=16, off=None, info=None, same=None):
    t = np.frombuffer(text, np.uint8)
    s = np.array(sa, np.int64 if width == 8 else np.uint32)
    q = np.frombuffer(query, np.uint8)
    n = len(text) if n is None else n
    m = len(query) if m is None else m
    off = np.full(max(m, len(query)) + 1 if m < (1 << 20) else 1, 99, np.uint64) if off is None else off
    tpos = np.full(cap + 1, 99, np.uint32)
    ln = np.full(cap + 1, 99, np.uint32)
    info = (ctypes.c_uint64 * 3)(7, 7, 7) if info is None else info
    tp = tpos.ctypes.data if outs else None
    lp = ln.ctypes.data if outs else None
    if same == "tpos":
        tp = t.ctypes.data
    if same == "off":
        rc = L.sa_mems(t.ctypes.data, n, s.ctypes.data, width, q.ctypes.data, m, min_len, 0, 0, flags,
                       q.ctypes.data, tp, lp, cap, info)
    else:
        rc = L.sa_mems(t.ctypes.data if n else None, n, s.ctypes.data if n else None, width,
                       q.ctypes.data if m else None, m, min_len, 0, 0, flags, off.ctypes.data, tp, lp, cap, info)
    return rc, off, tpos, ln, list(info)


def test_host_form_arguments_rejected_before_any_device(sa_lib):
    L = sa_lib.lib()
    for kw, word in (({"width": 3}, b"sa_width"), ({"n": 1 << 32}, b"too large"), ({"m": 1 << 32}, b"m too large"),
                     ({"min_len": 0}, b"min_len"), ({"flags": 4}, b"unknown flags"), ({"flags": 3}, b"exclude"),
                     ({"same": "tpos"}, b"aliases"), ({"same": "off"}, b"aliases"),
                     ({"sa": (5, 3, 1, 0, 4, 6), "width": 8}, b"out of range"),
                     ({"sa": (5, 3, 1, 0, 4, -1), "width": 8}, b"out of range")):
        rc = _host(L, **kw)[0]
        assert rc == -1, kw
        assert word in L.sa_last_error(), (kw, L.sa_last_error())
    t = np.frombuffer(b"banana", np.uint8)
    s = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    off = np.zeros(5, np.uint64)
    out = np.zeros(4, np.uint32)
    info = (ctypes.c_uint64 * 3)()
    a = (t.ctypes.data, 6, s.ctypes.data, 4, t.ctypes.data, 4, 2, 0, 0, 0)
    assert L.sa_mems(*a, None, out.ctypes.data, out.ctypes.data, 4, info) == -1 and b"off_out" in L.sa_last_error()
    assert L.sa_mems(*a, off.ctypes.data, out.ctypes.data, None, 4, info) == -1 and b"both or neither" in L.sa_last_error()
    assert L.sa_mems(*a, off.ctypes.data, None, None, 0, None) == -1 and b"info" in L.sa_last_error()
    assert L.sa_mems(None, 6, s.ctypes.data, 4, t.ctypes.data, 4, 2, 0, 0, 0, off.ctypes.data, None, None, 0,
                     info) == -1 and b"text is NULL" in L.sa_last_error()
    assert L.sa_mems(t.ctypes.data, 6, None, 4, t.ctypes.data, 4, 2, 0, 0, 0, off.ctypes.data, None, None, 0,
                     info) == -1 and b"sa is NULL" in L.sa_last_error()
    assert L.sa_mems(t.ctypes.data, 6, s.ctypes.data, 4, None, 4, 2, 0, 0, 0, off.ctypes.data, None, None, 0,
                     info) == -1 and b"query is NULL" in L.sa_last_error()


def test_host_form_returns_without_a_device(sa_lib):
    """n == 0, m == 0 and min_len > min(n, m): SA_OK, off all zero, info zero,
    nothing else written, with or without a GPU."""
    L = sa_lib.lib()
    for kw in ({"n": 0}, {"m": 0}, {"min_len": 5}, {"min_len": 7}, {"min_len": 1 << 40},
               {"text": b"ab", "sa": (0, 1), "min_len": 3}, {"n": 0, "m": 0}, {"min_len": 5, "outs": False}):
        rc, off, tpos, ln, info = _host(L, **kw)
        m = kw.get("m", 4)
        assert rc == 0, kw
        assert (off[:m + 1] == 0).all() and (off[m + 1:] == 99).all(), kw
        assert (tpos == 99).all() and (ln == 99).all() and info == [0, 0, 0], kw
    # L == min(n, m) is not one of them: it needs the device, and without one the call says so
    if sa_lib.device_count() <= 0:
        from hpc_suffix_array_amd import SAError, maximal_exact_matches
        rc = _host(L, min_len=4)[0]
        assert rc < 0 and b"device" in L.sa_last_error()
        with pytest.raises(SAError):
            maximal_exact_matches(b"banana", np.array([5, 3, 1, 0, 4, 2], np.uint32), b"anan", 2)


def test_mems_python_arguments():
    from hpc_suffix_array_amd import maximal_exact_matches
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(ValueError):
        maximal_exact_matches(b"banana", sa, b"anan", 2, mode="warp")
    with pytest.raises(ValueError):
        maximal_exact_matches(b"banana", sa[:5], b"anan", 2)
