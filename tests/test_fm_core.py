"""The host-compilable core of the FM-index
(hpc_suffix_array_amd/csrc/sa_fm.h): g++ builds tests/cpp/fm_check.cpp, which
builds the index on the host the way the kernels do and runs the class rule,
the size arithmetic, the header check, occ with its SWAR count and partial-word
mask, the backward search, the LF step and the locate walk against brute force:
every text over {a,b} up to 10 bytes, texts of 0 .. 300 bytes over 1, 2, 4, 5,
16, 17 and 256 symbols, s in {0, 1, 2, 3, 32}, an index overwritten with random
bytes, and the arithmetic at n = 2^32 - 1; once plainly and once with
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
SRC = os.path.join(ROOT, "tests", "cpp", "fm_check.cpp")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    w = out.stdout.split()
    assert int(w[1]) > 1_000_000, out.stdout                        # checks
    # {a,b}^n, n <= 10: 2,047 texts; 7 alphabets x 81 lengths on top
    assert int(w[4]) >= 2_047 + 7 * 81, out.stdout
    assert int(w[6]) > 154_200, out.stdout                          # patterns


def test_fm_core_matches_brute_force(tmp_path):
    _build_and_run(tmp_path, "fm_check", ["-O2"], 300)


def test_fm_core_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: every index is an
    exact-size heap buffer, so an occ, a walk or a search that leaves it, on a
    good index or on one overwritten with random bytes, aborts."""
    _build_and_run(tmp_path, "fm_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_fm.h")).read()
    assert int(re.search(r"#define\s+SA_FM_INFO\s+(\d+)", hdr).group(1)) == 4 == sa_lib.FM_INFO
    assert int(re.search(r"kFmInfo\s*=\s*(\d+)", src).group(1)) == 4
    assert int(re.search(r"#define\s+SA_FM_MAX_SAMPLE\s+(\d+)", hdr).group(1)) == sa_lib.FM_MAX_SAMPLE == 4096
    assert int(re.search(r"kFmMaxSample\s*=\s*(\d+)", src).group(1)) == sa_lib.FM_MAX_SAMPLE
    assert int(re.search(r"kFmHeaderBytes\s*=\s*(\d+)", src).group(1)) == sa_lib.FM_HEADER
    assert re.search(r"static_assert\(SA_FM_INFO == kFmInfo && SA_FM_MAX_SAMPLE == kFmMaxSample", src)
    rows = re.search(r"fm_rows\(uint32_t cls\) \{ return cls == 0 \? (\d+)u : cls == 1 \? (\d+)u : (\d+)u; \}", src)
    assert tuple(int(x) for x in rows.groups()) == sa_lib.FM_ROWS == (64, 256, 4096)
    assert bytes.fromhex("%016x" % int(re.search(r"kFmMagic = (0x[0-9A-F]+)ull", src).group(1), 16))[::-1] == b"SAMFIDX1"
    # the header comes after what it needs, and is a dependency of the library
    build = open(os.path.join(CSRC, "sa_build.hip")).read()
    for dep in ("sa_host.h", "sa_find.h", "sa_locate.h", "sa_mem.h", "sa_ibwt.h"):
        assert build.index('#include "%s"' % dep) < build.index('#include "sa_fm.h"')
    assert "sa_fm.h" in open(os.path.join(CSRC, "Makefile")).read()


def test_size_arithmetic(sa_lib):
    """sa_fm_index_bytes is pure host arithmetic: the bound of the issue at
    s = 32, and the sections it is made of."""
    L = sa_lib.lib()
    for n in (1 << 20, (1 << 20) + 1, (1 << 24) + 5, 1 << 28, (1 << 31) + 7, (1 << 32) - 1):
        assert L.sa_fm_index_bytes(n, 32) <= 1.6 * n + 65536, n
        assert L.sa_fm_index_bytes(n, 32) >= 1.5625 * n
        assert L.sa_fm_index_bytes(n, 0) <= 1.25 * n + 4096 + 5120
    assert L.sa_fm_index_bytes(0, 0) == 4096 + 5120 and L.sa_fm_index_bytes(0, 32) == 4096 + 5120 + 16
    for n, s in ((1000, 1), (1000, 7), (70001, 64), (5, 4096)):
        tiles = -(-n // 16384)
        marks = tiles * 256 * 12 + -(-(tiles + 1) * 8 // 16) * 16 + -(-(-(-n // s)) * 4 // 16) * 16
        assert L.sa_fm_index_bytes(n, s) == 4096 + max((n // r + 1) * (r + r // 4) for r in sa_lib.FM_ROWS) + marks


def test_host_waits_stated_and_counted():
    """The statements about host waits in sa_hip.h and sa_fm.h agree with each
    other and with the source: one host_sync in the build, none in the count,
    and locate's before sa_locate_device's own."""
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_fm.h")).read()
    assert "sa_fm_build_device: one" in src and "sa_fm_count_device: none" in src
    assert "Host waits\n * per call: one (the byte counts" in hdr and "no host wait, no context, no workspace" in hdr

    def body(name):
        at = src.index("static int %s(" % name)
        return src[at:src.index("\n}\n", at)]

    assert body("fm_build_device").count("host_sync(") == 1
    for name in ("fm_count_device", "fm_build_check", "fm_locate_check"):
        assert "host_sync" not in body(name) and "hipMemcpy" not in body(name) and "hipMalloc" not in body(name)
    b = body("fm_build_device")
    assert b.index("host_sync(") < b.index("k_fm_records") < b.index("k_fm_samples")
    b = body("fm_locate_device")
    assert b.count("host_sync(") == 2 and b.index("host_sync(") < b.index("k_fm_resolve") < b.index("tmp.sort(")
    # the sort is sa_query.h's step: it adds no wait of its own in front of sa_locate_device's
    q = open(os.path.join(CSRC, "sa_query.h")).read()
    for start, end in (("static int sort_lists(", "\n}\n"), ("struct ListSort {", "\n};\n")):
        step = q[q.index(start):q.index(end, q.index(start))]
        assert "host_sync(" not in step and "hipMemcpy" not in step
    assert step.index("k_list_ranges") < step.index("sort_lists(") and "locate_device_n(" in q[q.index("static int sort_lists("):]


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    for name in ("sa_fm_index_bytes", "sa_fm_build_device", "sa_fm_count_device", "sa_fm_locate_device", "sa_fm_build",
                 "sa_fm_count", "sa_fm_locate"):
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\b(int|uint64_t) %s\(" % name, hdr)
    assert "FMIndex" in pkg.__all__
    for name in ("from_text", "from_sa", "from_bwt", "from_bytes", "to_bytes", "count", "find", "locate"):
        assert callable(getattr(pkg.FMIndex, name))
    for name in ("fm_build", "fm_count", "fm_locate", "fm_index_bytes"):
        assert callable(getattr(pkg.DeviceBuilder, name))


P = [ctypes.c_void_p(4096 * k) for k in range(1, 12)]


def test_device_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call: the pointers are
    fake addresses that are never dereferenced."""
    L = sa_lib.lib()
    info = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    need = L.sa_fm_index_bytes(6, 2)

    def build(ctx=P[0], bwt=P[1], n=6, p=3, sa=P[2], s=2, idx=P[3], nbytes=need):
        return L.sa_fm_build_device(ctx, bwt, n, p, sa, s, idx, nbytes, info, None)

    def count(idx=P[3], pat=P[4], off=P[5], nq=3, lo=P[6], hi=P[7]):
        return L.sa_fm_count_device(idx, need, pat, 9, off, nq, lo, hi, None)

    total = ctypes.c_uint64(7)

    def locate(ctx=P[0], idx=P[3], lo=P[6], hi=P[7], nq=3, flags=0, off=P[8], tot=ctypes.byref(total)):
        return L.sa_fm_locate_device(ctx, idx, need, lo, hi, nq, 0, flags, off, P[9], 100, tot, None)

    odd = ctypes.c_void_p(4096 * 4 + 8)
    for distinct, call, cases in ((12, build, (({"ctx": None}, b"context is NULL"), ({"n": 1 << 32, "nbytes": 1 << 40}, b"n too large"),
                                 ({"s": 4097}, b"sa_sample 4097"), ({"idx": None}, b"d_index is NULL"),
                                 ({"idx": odd}, b"d_index is not 16-byte aligned"),
                                 ({"nbytes": need - 1}, b"is below sa_fm_index_bytes"), ({"nbytes": 0}, b"is below sa_fm_index_bytes"),
                                 ({"bwt": None}, b"d_bwt is NULL"), ({"p": 6}, b"primary index 6"), ({"p": 1 << 40}, b"primary index"),
                                 ({"sa": None}, b"d_sa is NULL with sa_sample 2"),
                                 ({"s": 0, "nbytes": need}, b"d_sa is given with sa_sample 0"),
                                 ({"sa": ctypes.c_void_p(4096 * 3 + 2)}, b"d_sa is not 4-byte aligned"),
                                 ({"idx": P[1]}, b"d_index may not alias"), ({"idx": P[2]}, b"d_index may not alias"))),
                        (3, count, (({"idx": None}, b"NULL device pointer"), ({"pat": None}, b"NULL device pointer"),
                                 ({"off": None}, b"NULL device pointer"), ({"lo": None}, b"NULL device pointer"),
                                 ({"hi": None}, b"NULL device pointer"), ({"idx": odd}, b"d_index is not 16-byte aligned"),
                                 ({"nq": 1 << 32}, b"nq too large"))),
                        (9, locate, (({"ctx": None}, b"context is NULL"), ({"tot": None}, b"total is NULL"),
                                  ({"idx": None}, b"d_index is NULL"), ({"idx": odd}, b"d_index is not 16-byte aligned"),
                                  ({"lo": None}, b"d_lo is NULL"), ({"hi": None}, b"d_hi is NULL"), ({"off": None}, b"d_off is NULL"),
                                  ({"nq": 1 << 32}, b"nq too large"), ({"flags": 4}, b"unknown flags")))):
        msgs = set()
        for kw, word in cases:
            assert call(**kw) == -1, kw
            msg = L.sa_last_error()
            assert word in msg, (kw, msg)
            msgs.add(re.sub(rb"\d+", b"#", msg))
        assert len(msgs) == distinct, msgs                          # each rejection has its own message
    assert list(info) == [7, 7, 7, 7] and total.value == 7          # a rejected call writes nothing
    assert count(nq=0) == 0 and count(nq=0, idx=None) == 0          # no queries: SA_OK without a launch


def _empty_index(sa_lib, s=32):
    L = sa_lib.lib()
    cap = L.sa_fm_index_bytes(0, s)
    buf = np.full(cap + 64, 0xA5, np.uint8)
    info = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    assert L.sa_fm_build(None, 0, 0, None, 4, s, buf.ctypes.data, cap, info) == 0
    assert list(info)[:2] == [0, 0] and info[2] <= cap and info[3] == 0
    assert (buf[cap:] == 0xA5).all()
    return buf, int(info[2])


def test_host_forms_rejected_before_any_device(sa_lib):
    L = sa_lib.lib()
    b = np.frombuffer(b"nnbaaa", np.uint8).copy()
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    n = 6
    cap = L.sa_fm_index_bytes(n, 2)
    out = np.full(cap, 0xA5, np.uint8)
    B, S, O = b.ctypes.data, sa.ctypes.data, out.ctypes.data
    for args, word in (((B, n, 3, S, 3, 2, O, cap, None), b"sa_width"), ((B, 1 << 32, 3, S, 4, 2, O, cap, None), b"too large"),
                       ((B, n, 3, S, 4, 4097, O, cap, None), b"sa_sample 4097"), ((B, n, 3, S, 4, 2, None, cap, None), b"index_out is NULL"),
                       ((B, n, 3, S, 4, 2, O, cap - 1, None), b"is below sa_fm_index_bytes"),
                       ((None, n, 3, S, 4, 2, O, cap, None), b"NULL host pointer"), ((B, n, n, S, 4, 2, O, cap, None), b"primary index 6"),
                       ((B, n, 3, None, 4, 2, O, cap, None), b"sa is NULL with sa_sample 2"),
                       ((B, n, 3, S, 4, 0, O, cap, None), b"sa is given with sa_sample 0")):
        assert L.sa_fm_build(*args) == -1, args
        assert word in L.sa_last_error(), (args, L.sa_last_error())
    wide = np.array([5, 3, 1, 0, 4, 6], np.int64)                   # a width-8 entry outside [0, n)
    assert L.sa_fm_build(B, n, 3, wide.ctypes.data, 8, 2, O, cap, None) == -1 and b"out of range" in L.sa_last_error()
    assert (out == 0xA5).all()
    # what is no index: a truncated header, a wrong magic, a wrong version, a section running past the end
    buf, used = _empty_index(sa_lib)
    lo, hi = np.full(2, 9, np.uint64), np.full(2, 9, np.uint64)
    off = np.array([0, 0, 1], np.uint64)
    pat = np.frombuffer(b"a", np.uint8).copy()
    pos = np.full(4, 9, np.uint32)
    ooff = np.full(3, 9, np.uint64)

    def count(data, nbytes):
        return L.sa_fm_count(data.ctypes.data, nbytes, pat.ctypes.data, off.ctypes.data, 2, lo.ctypes.data, hi.ctypes.data)

    def locate(data, nbytes):
        z = np.zeros(2, np.uint64)
        return L.sa_fm_locate(data.ctypes.data, nbytes, z.ctypes.data, z.ctypes.data, 2, 0, 0, ooff.ctypes.data, pos.ctypes.data, 4, 4)

    assert count(buf, used) == 0 and locate(buf, used) == 0
    magic, version, big_n, blocks = buf.copy(), buf.copy(), buf.copy(), buf.copy()
    magic[3] ^= 0x20
    version[8] = 2
    big_n[16:24].view(np.uint64)[0] = 4096                           # n raised: the sections would run past the end
    blocks[72:80].view(np.uint64)[0] += 1                            # one more record than the buffer holds
    for call in (count, locate):
        for data, nbytes in ((buf, sa_lib.FM_HEADER - 1), (buf, used - 1), (buf, 0), (magic, used), (version, used), (big_n, used),
                             (blocks, used)):
            lo[:] = hi[:] = 9
            assert call(data, nbytes) == -1 and b"not an FM-index" in L.sa_last_error(), (call, nbytes)
            assert (lo == 9).all() and (hi == 9).all() and (pos == 9).all()
    assert L.sa_fm_count(None, used, pat.ctypes.data, off.ctypes.data, 2, lo.ctypes.data, hi.ctypes.data) == -1
    nos, used0 = _empty_index(sa_lib, 0)
    assert count(nos, used0) == 0 and locate(nos, used0) == -1 and b"no samples" in L.sa_last_error()
    assert L.sa_fm_locate(buf.ctypes.data, used, None, None, 0, 0, 8, ooff.ctypes.data, None, 4, 0) == -1 and b"unknown flags" in L.sa_last_error()
    assert L.sa_fm_locate(buf.ctypes.data, used, None, None, 0, 0, 0, ooff.ctypes.data, None, 3, 0) == -1 and b"sa_width" in L.sa_last_error()
    one = np.array([1], np.uint64)
    z = np.zeros(1, np.uint64)
    assert L.sa_fm_locate(buf.ctypes.data, used, z.ctypes.data, one.ctypes.data, 1, 0, 0, ooff.ctypes.data, None, 4, 0) == -1
    assert b"interval 0 is [0, 1) of 0" in L.sa_last_error()


def test_empty_index_without_a_device(sa_lib):
    """n == 0: a valid empty index, built, queried and round-tripped with or
    without a GPU."""
    from hpc_suffix_array_amd import FMIndex, SAError
    for s in (0, 1, 32):
        fm = FMIndex.from_text(b"", sa_sample=s)
        assert (fm.n, fm.sigma, fm.sa_sample) == (0, 0, s) and fm.nbytes <= sa_lib.lib().sa_fm_index_bytes(0, s)
        again = FMIndex.from_bytes(fm.to_bytes())
        assert again.to_bytes() == fm.to_bytes() and (again.n, again.sigma, again.sa_sample, again.nbytes) == (0, 0, s, fm.nbytes)
        for f in (fm, again, FMIndex.from_bwt(b"", 0, sa_sample=s), FMIndex.from_sa(b"", np.zeros(0, np.uint32), sa_sample=s)):
            assert f.to_bytes() == fm.to_bytes()
            assert f.count([b"", b"a", b"ab"]).tolist() == [0, 0, 0]
            lo, hi = f.find([b"", b"a"])
            assert lo.tolist() == [0, 0] and hi.tolist() == [0, 0] and lo.dtype == np.int64
            assert f.count([]).size == 0
            if s:
                off, pos = f.locate([b"", b"a"], max_hits=3, order="sa")
                assert off.tolist() == [0, 0, 0] and pos.size == 0
            else:
                with pytest.raises(SAError, match="no samples"):
                    f.locate([b"a"])
    with pytest.raises(SAError, match="not an FM-index"):
        FMIndex.from_bytes(b"")
    with pytest.raises(SAError, match="not an FM-index"):
        FMIndex.from_bytes(b"x" * 5000)
    with pytest.raises(SAError, match="not an FM-index"):
        FMIndex.from_bytes(FMIndex.from_text(b"").to_bytes()[:-16])
    with pytest.raises(ValueError, match="order"):
        FMIndex.from_text(b"").locate([b"a"], order="up")
    with pytest.raises(ValueError, match="negative"):
        FMIndex.from_text(b"", sa_sample=-1)
    if sa_lib.device_count() <= 0:
        # anything longer needs the device, and without one the call says so
        with pytest.raises(SAError, match="device"):
            FMIndex.from_text(b"banana")
        with pytest.raises(SAError, match="device"):
            FMIndex.from_bwt(b"nnbaaa", 3, np.array([5, 3, 1, 0, 4, 2], np.uint32))
