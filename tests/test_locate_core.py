"""The host-compilable arithmetic of the batched locate (hpc_suffix_array_amd/
csrc/sa_locate.h): g++ builds tests/cpp/locate_check.cpp, which checks the
capped count and class, the queries of an output tile, the composite key and
the output split against brute force, once plainly and once with
-fsanitize=address,undefined as a stand-alone program.  Plus the constants'
copies, the exported symbols, and what sa_locate / sa_locate_device decide
before they touch a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "locate_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 10000, out.stdout


def test_locate_arithmetic_matches_brute_force(tmp_path):
    _build_and_run(tmp_path, "locate_check", ["-O2"], 300)


def test_locate_arithmetic_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: the offset arrays are
    exact-size heap buffers, so a search that reads past off[nq] aborts, and a
    shift by the key's full width or an overflowing product is reported."""
    _build_and_run(tmp_path, "locate_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_locate.h")).read()
    in_hdr = int(re.search(r"#define\s+SA_LOCATE_TILE\s+(\d+)", hdr).group(1))
    in_src = int(re.search(r"kLocateTile\s*=\s*(\d+)", src).group(1))
    assert in_hdr == in_src == sa_lib.LOCATE_TILE
    assert int(re.search(r"#define\s+SA_LOCATE_SA_ORDER\s+(\d+)u", hdr).group(1)) == sa_lib.LOCATE_SA_ORDER == 1
    assert int(re.search(r"#define\s+SA_LOCATE_SMALL_CHUNKS\s+(\d+)u", hdr).group(1)) == sa_lib.LOCATE_SMALL_CHUNKS
    assert sa_lib.LOCATE_ORDERS == {"text": 0, "sa": sa_lib.LOCATE_SA_ORDER}


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    for name in ("sa_locate_device", "sa_locate"):
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    assert re.search(r"\bint sa_locate_device\(", hdr) and re.search(r"\bint sa_locate\(", hdr)
    for name in ("locate_intervals", "locate_batch"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert callable(pkg.DeviceBuilder.locate)


def test_locate_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call: the pointers are
    fake addresses that are never dereferenced."""
    L = sa_lib.lib()
    p = ctypes.c_void_p(4096)
    p2 = ctypes.c_void_p(8192)
    tot = ctypes.c_uint64(77)
    T = ctypes.byref(tot)

    def dev(ctx=p, n=6, sa=p, lo=p, hi=p, nq=2, flags=0, off=p, pos=p2, total=T):
        return L.sa_locate_device(ctx, n, sa, lo, hi, nq, 0, flags, off, pos, 10, total, None)

    msgs = set()
    for kw, word in (({"ctx": None}, b"context"), ({"sa": None}, b"d_sa"), ({"lo": None}, b"d_lo"),
                     ({"hi": None}, b"d_hi"), ({"off": None}, b"d_off"), ({"total": None}, b"total"),
                     ({"n": 1 << 32}, b"n too large"), ({"pos": p}, b"alias"), ({"flags": 4}, b"flags"),
                     ({"flags": 0x80000000}, b"flags"), ({"nq": 1 << 32}, b"nq too large")):
        assert dev(**kw) == -1, kw
        msg = L.sa_last_error()
        assert word in msg, (kw, msg)
        msgs.add(msg.split(b" 0x")[0])
    assert len(msgs) == 10          # each rejection has its own message (the two flag cases share one)

    # host form
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    off = np.full(3, 99, np.uint64)
    pos = np.full(8, 99, np.uint32)

    def host(sa_arr=sa, n=6, width=4, lo=(1, 0), hi=(4, 2), nq=2, max_hits=0, flags=0, cap=8):
        a, b = np.array(lo, np.uint64), np.array(hi, np.uint64)
        return L.sa_locate(sa_arr.ctypes.data, n, width, a.ctypes.data, b.ctypes.data, nq, max_hits, flags,
                           off.ctypes.data, pos.ctypes.data, cap)

    assert host(width=3) == -1 and b"sa_width" in L.sa_last_error()
    assert host(lo=(3, 0), hi=(2, 2)) == -1 and b"interval 0" in L.sa_last_error()
    assert host(hi=(4, 7)) == -1 and b"interval 1" in L.sa_last_error()
    assert host(cap=4) == -1 and b"pos_cap" in L.sa_last_error()         # total 5
    assert host(cap=3, max_hits=2) == -1                                 # total 4 under the cap
    assert host(n=1 << 32) == -1 and b"too large" in L.sa_last_error()
    assert host(flags=8) == -1 and b"flags" in L.sa_last_error()
    wide = np.array([5, 3, 1, 0, 4, 6], np.int64)
    assert host(sa_arr=wide, width=8) == -1 and b"out of range" in L.sa_last_error()
    wide[5] = -1
    assert host(sa_arr=wide, width=8) == -1
    # nothing to locate: no device needed, the offsets are filled
    assert host(nq=0) == 0 and off[0] == 0
    off[:] = 99
    assert host(lo=(2, 5), hi=(2, 5)) == 0 and off.tolist() == [0, 0, 0]
    assert (pos == 99).all()


def test_no_locate_without_device(sa_lib):
    if sa_lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    from hpc_suffix_array_amd import SAError, locate_batch, locate_intervals
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(SAError):
        locate_intervals(sa, [1], [4])
    with pytest.raises(SAError):
        locate_batch(b"banana", sa, [b"ana"])
    L = sa_lib.lib()
    lo, hi = np.array([1], np.uint64), np.array([4], np.uint64)
    off, pos = np.zeros(2, np.uint64), np.zeros(3, np.uint32)
    rc = L.sa_locate(sa.ctypes.data, 6, 4, lo.ctypes.data, hi.ctypes.data, 1, 0, 0, off.ctypes.data, pos.ctypes.data, 3)
    assert rc < 0 and b"device" in L.sa_last_error()
    assert off.tolist() == [0, 3]


def test_locate_python_arguments():
    from hpc_suffix_array_amd import locate_intervals
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(ValueError):
        locate_intervals(sa, [1], [4], order="rank")
    with pytest.raises(ValueError):
        locate_intervals(sa, [1], [4], max_hits=-1)
    with pytest.raises(ValueError):
        locate_intervals(sa, [1, 2], [4])
