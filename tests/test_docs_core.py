"""The host-compilable arithmetic of the document collections (hpc_suffix_array_amd/
csrc/sa_docs.h): g++ builds tests/cpp/docs_check.cpp, which checks the
boundary search with empty documents at every place, the PRV <= lo predicate,
the capped count, the class of a query and the key width of D against brute
force, once plainly and once with -fsanitize=address,undefined as a
stand-alone program.  Plus the constants' copies, the exported symbols, the
Python names, and what the sa_doc_* entry points decide before they touch a
device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "docs_check.cpp")

DEVICE_SYMBOLS = ("sa_doc_array_device", "sa_doc_of_device", "sa_doc_frequency_device", "sa_doc_list_device")
HOST_SYMBOLS = ("sa_doc_array", "sa_doc_of", "sa_doc_frequency", "sa_doc_list")


def _build_and_run(tmp_path, name, flags, timeout):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 10000, out.stdout


def test_docs_arithmetic_matches_brute_force(tmp_path):
    _build_and_run(tmp_path, "docs_check", ["-O2"], 300)


def test_docs_arithmetic_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan: the offsets are
    exact-size heap buffers of D entries, so a search that reads doc_off[D] or
    beyond aborts, and a shift by a key's full width is reported."""
    _build_and_run(tmp_path, "docs_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 600)


def test_constants_agree(sa_lib):
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = open(os.path.join(CSRC, "sa_docs.h")).read()

    def h(name):
        return int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, hdr).group(1), 0)

    def s(name):
        return int(re.search(r"%s\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?" % name, src).group(1), 0)

    assert h("SA_DOC_TILE") == s("kDocTile") == sa_lib.DOC_TILE
    assert h("SA_DOC_GROUP_MAX") == s("kDocGroupMax") == sa_lib.DOC_GROUP_MAX
    assert h("SA_DOC_LDS_DOCS") == s("kDocLdsDocs") == sa_lib.DOC_LDS_DOCS
    assert h("SA_DOC_NONE") == s("kDocNone") == sa_lib.DOC_NONE == 0xFFFFFFFF
    assert h("SA_DOC_RANK_ORDER") == sa_lib.DOC_RANK_ORDER == 1
    assert sa_lib.DOC_ORDERS == {"doc": 0, "rank": sa_lib.DOC_RANK_ORDER}
    assert sa_lib.DOC_GROUP_MAX < sa_lib.DOC_TILE


def test_symbols_exported_and_listed(sa_lib):
    import hpc_suffix_array_amd as pkg
    L = sa_lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    for name in DEVICE_SYMBOLS + HOST_SYMBOLS:
        assert name in sa_lib.EXT_SYMBOLS
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\bint %s\(" % name, hdr), name
    for name in ("document_array", "doc_of_positions", "document_frequency", "list_documents", "Collection"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("doc_array", "doc_of", "doc_frequency", "doc_list"):
        assert callable(getattr(pkg.DeviceBuilder, name))
    for name in ("count", "document_frequency", "list_documents", "locate", "close", "__enter__", "__exit__"):
        assert callable(getattr(pkg.Collection, name))
    assert isinstance(pkg.Collection.doc_offsets, property)


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
    p, p2, p3, p4, p5, p6 = (ctypes.c_void_p(4096 * k) for k in range(1, 7))
    odd = ctypes.c_void_p(4098)
    tot = ctypes.c_uint64(77)
    T = ctypes.byref(tot)

    def arr(ctx=p, n=6, sa=p2, off=p3, D=2, da=p4, prev=p5):
        return L.sa_doc_array_device(ctx, n, sa, off, D, da, prev, None)

    msgs = _rejections(L, arr, (
        ({"ctx": None}, b"context"), ({"sa": None}, b"d_sa"), ({"off": None}, b"d_doc_off"),
        ({"da": None, "prev": None}, b"both NULL"), ({"n": 1 << 32}, b"n too large"), ({"D": 0}, b"D is 0"),
        ({"D": (1 << 32) - 1}, b"D too large"), ({"da": odd}, b"d_da is not 4-byte aligned"),
        ({"prev": odd}, b"d_prev is not 4-byte aligned"), ({"prev": p4}, b"alias d_prev"),
        ({"da": p2}, b"alias d_sa"), ({"prev": p3}, b"alias d_sa or d_doc_off")))
    assert len(msgs) == 11          # the two input aliases share one message
    assert arr(n=0, sa=None) == 0   # nothing to do: no launch

    def of(off=p3, D=2, n=6, pos=p2, count=3, doc=p4, rel=p5):
        return L.sa_doc_of_device(off, D, n, pos, count, doc, rel, None)

    msgs = _rejections(L, of, (
        ({"off": None}, b"d_doc_off"), ({"pos": None}, b"d_pos"), ({"doc": None, "rel": None}, b"both NULL"),
        ({"n": 1 << 32}, b"n too large"), ({"D": 0}, b"D is 0"), ({"D": 1 << 32}, b"D too large"),
        ({"doc": odd}, b"d_doc is not"), ({"rel": odd}, b"d_rel is not"), ({"rel": p4}, b"alias d_rel"),
        ({"doc": p2}, b"alias d_pos")))
    assert len(msgs) == 10
    assert of(count=0, pos=None) == 0

    def freq(n=6, prev=p, lo=p2, hi=p3, nq=2, df=p4):
        return L.sa_doc_frequency_device(n, prev, lo, hi, nq, df, None)

    msgs = _rejections(L, freq, (
        ({"prev": None}, b"d_prev"), ({"lo": None}, b"d_lo"), ({"hi": None}, b"d_hi"), ({"df": None}, b"d_df is NULL"),
        ({"n": 1 << 32}, b"n too large"), ({"nq": 1 << 32}, b"nq too large"), ({"df": odd}, b"not 4-byte aligned"),
        ({"df": p}, b"alias"), ({"df": p3}, b"alias")))
    assert len(msgs) == 8
    assert freq(nq=0, lo=None, hi=None, df=None) == 0

    def lst(ctx=p, n=6, da=p, prev=p2, lo=p3, hi=p4, nq=2, flags=0, off=p5, docs=p6, total=T):
        return L.sa_doc_list_device(ctx, n, da, prev, lo, hi, nq, 0, flags, off, docs, 10, total, None)

    msgs = _rejections(L, lst, (
        ({"ctx": None}, b"context"), ({"total": None}, b"total"), ({"da": None}, b"d_da"), ({"prev": None}, b"d_prev"),
        ({"lo": None}, b"d_lo"), ({"hi": None}, b"d_hi"), ({"off": None}, b"d_off is NULL"),
        ({"n": 1 << 32}, b"n too large"), ({"nq": 1 << 32}, b"nq too large"), ({"flags": 2}, b"flags"),
        ({"flags": 0x80000000}, b"flags"), ({"off": ctypes.c_void_p(4100)}, b"d_off is not 8-byte aligned"),
        ({"docs": odd}, b"d_docs is not 4-byte aligned"), ({"docs": p}, b"alias an input"),
        ({"off": p2}, b"alias an input"), ({"docs": p5}, b"alias d_off")))
    assert len(msgs) == 14          # the two flag cases and the two input aliases share theirs
    assert tot.value == 77          # nothing was written before the checks


def test_host_arguments_rejected_before_any_device(sa_lib):
    """The host forms check everything before they ask for a device, so all of
    this runs without one; the arrays are real (the checks read them)."""
    L = sa_lib.lib()
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    off = np.array([0, 2, 2, 6], np.uint64)
    da = np.full(6, 99, np.uint32)
    prev = np.full(6, 99, np.uint32)

    def arr(sa_arr=sa, n=6, width=4, o=off, D=3, a=da, b=prev):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return L.sa_doc_array(ptr(sa_arr), n, width, ptr(o), D, ptr(a), ptr(b))

    err = L.sa_last_error
    assert arr(width=3) == -1 and b"sa_width" in err()
    assert arr(n=1 << 32) == -1 and b"too large" in err()
    assert arr(D=0) == -1 and b"D is 0" in err()
    assert arr(D=(1 << 32) - 1) == -1 and b"D too large" in err()
    assert arr(o=None) == -1 and b"doc_off is NULL" in err()
    assert arr(o=np.array([1, 2, 2, 6], np.uint64)) == -1 and b"doc_off[0]" in err()
    assert arr(o=np.array([0, 3, 2, 6], np.uint64)) == -1 and b"decreases at document 1" in err()
    assert arr(o=np.array([0, 2, 2, 5], np.uint64)) == -1 and b"ends at 5" in err()
    assert arr(a=None, b=None) == -1 and b"both NULL" in err()
    assert arr(b=da) == -1 and b"alias prev_out" in err()
    assert arr(sa_arr=None) == -1 and b"sa is NULL" in err()
    assert arr(a=sa) == -1 and b"alias sa" in err()
    wide = np.array([5, 3, 1, 0, 4, 6], np.int64)
    assert arr(sa_arr=wide, width=8) == -1 and b"out of range" in err()
    assert (da == 99).all() and (prev == 99).all()
    # an empty text needs no device
    assert arr(sa_arr=None, n=0, o=np.array([0, 0, 0], np.uint64), D=2) == 0

    pos = np.array([0, 5, 6], np.uint32)
    doc, rel = np.full(3, 99, np.uint32), np.full(3, 99, np.uint32)

    def of(o=off, D=3, n=6, ps=pos, count=3, width=4, a=doc, b=rel):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return L.sa_doc_of(ptr(o), D, n, ptr(ps), count, width, ptr(a), ptr(b))

    assert of(width=5) == -1 and b"sa_width" in err()
    assert of(o=np.array([0, 2, 1, 6], np.uint64)) == -1 and b"decreases" in err()
    assert of(n=7) == -1 and b"ends at 6" in err()
    assert of(a=None, b=None) == -1 and b"both NULL" in err()
    assert of(b=doc) == -1 and b"alias rel_out" in err()
    assert of(ps=None) == -1 and b"pos is NULL" in err()
    assert of(a=pos) == -1 and b"alias pos" in err()
    assert of(ps=np.array([0, -1, 2], np.int64), width=8) == -1 and b"position entry out of range" in err()
    assert of(ps=np.array([0, 1 << 32, 2], np.int64), width=8) == -1 and b"out of range" in err()
    assert of(count=0, ps=None) == 0
    assert (doc == 99).all() and (rel == 99).all()

    pv = np.array([0, 0, 1, 2, 3, 0], np.uint32)      # DA = 0 1 0 1 0 2
    dav = np.array([0, 1, 0, 1, 0, 2], np.uint32)
    df = np.full(2, 99, np.uint64)

    def freq(p=pv, n=6, width=4, lo=(1, 0), hi=(4, 2), nq=2, out=df):
        a, b = np.array(lo, np.uint64), np.array(hi, np.uint64)
        return L.sa_doc_frequency(None if p is None else p.ctypes.data, n, width, a.ctypes.data, b.ctypes.data, nq,
                                  None if out is None else out.ctypes.data)

    assert freq(width=2) == -1 and b"sa_width" in err()
    assert freq(n=1 << 32) == -1 and b"too large" in err()
    assert freq(nq=1 << 32) == -1 and b"nq too large" in err()
    assert freq(out=None) == -1 and b"df_out is NULL" in err()
    assert freq(lo=(3, 0), hi=(2, 2)) == -1 and b"interval 0" in err()
    assert freq(hi=(4, 7)) == -1 and b"interval 1" in err()
    assert freq(p=None) == -1 and b"prev is NULL" in err()
    assert freq(p=np.array([0, 0, 1, 2, 7, 0], np.int64), width=8) == -1 and b"PRV entry out of range" in err()
    assert freq(nq=0) == 0
    assert (df == 99).all()
    assert freq(n=0, lo=(0, 0), hi=(0, 0), p=None) == 0 and df.tolist() == [0, 0]

    offs = np.full(3, 99, np.uint64)
    docs = np.full(8, 99, np.uint32)

    def lst(d=dav, p=pv, n=6, width=4, lo=(1, 0), hi=(4, 2), nq=2, max_docs=0, flags=0, o=offs, out=docs, cap=8):
        a, b = np.array(lo, np.uint64), np.array(hi, np.uint64)
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return L.sa_doc_list(ptr(d), ptr(p), n, width, a.ctypes.data, b.ctypes.data, nq, max_docs, flags, ptr(o),
                             ptr(out), cap)

    assert lst(width=3) == -1 and b"sa_width" in err()
    assert lst(n=1 << 32) == -1 and b"too large" in err()
    assert lst(flags=2) == -1 and b"flags" in err()
    assert lst(o=None) == -1 and b"off_out is NULL" in err()
    assert lst(lo=(3, 0), hi=(2, 2)) == -1 and b"interval 0" in err()
    assert lst(hi=(4, 7)) == -1 and b"interval 1" in err()
    assert lst(d=None) == -1 and b"da or prev is NULL" in err()
    assert lst(out=dav) == -1 and b"docs_out may not alias" in err()
    assert lst(d=np.array([0, 1, 0, 1, 0, -2], np.int64), p=pv.astype(np.int64), width=8) == -1 and b"DA entry" in err()
    assert lst(d=dav.astype(np.int64), p=np.array([0, 0, 1, 2, 3, 9], np.int64), width=8) == -1 and b"PRV entry" in err()
    # df = 2 and 2: the host fills the offsets itself; docs_cap below the total is rejected
    assert lst(cap=3) == -1 and b"docs_cap 3 is below the 4 ids" in err() and offs.tolist() == [0, 2, 4]
    assert lst(cap=1, max_docs=1) == -1 and b"below the 2 ids" in err()
    offs[:] = 99
    assert lst(out=None, cap=0) == 0 and offs.tolist() == [0, 2, 4]        # the sizing call
    assert lst(nq=0) == 0 and offs[0] == 0
    offs[:] = 99
    assert lst(lo=(2, 5), hi=(2, 5)) == 0 and offs.tolist() == [0, 0, 0]  # nothing to list: no device
    assert (docs == 99).all()


def test_no_docs_without_device(sa_lib):
    if sa_lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    from hpc_suffix_array_amd import (Collection, SAError, doc_of_positions, document_array, document_frequency,
                                      list_documents)
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    prev = np.array([0, 0, 1, 2, 3, 0], np.uint32)
    da = np.array([0, 1, 0, 1, 0, 2], np.uint32)
    with pytest.raises(SAError):
        document_array(sa, [0, 2, 2, 6])
    with pytest.raises(SAError):
        doc_of_positions([0, 2, 2, 6], 6, [1])
    with pytest.raises(SAError):
        document_frequency(prev, [1], [4])
    with pytest.raises(SAError):
        list_documents(da, prev, [1], [4])
    with pytest.raises(SAError):
        Collection([b"ab", b"ba"])


def test_docs_python_arguments():
    from hpc_suffix_array_amd import Collection, document_array, document_frequency, list_documents
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    prev = np.array([0, 0, 1, 2, 3, 0], np.uint32)
    da = np.array([0, 1, 0, 1, 0, 2], np.uint32)
    with pytest.raises(ValueError):
        document_array(sa, [6])
    with pytest.raises(ValueError):
        document_array(sa, [0, -1, 6])
    with pytest.raises(ValueError):
        document_frequency(prev, [1, 2], [4])
    with pytest.raises(ValueError):
        list_documents(da, prev, [1], [4], order="text")
    with pytest.raises(ValueError):
        list_documents(da, prev, [1], [4], max_docs=-1)
    with pytest.raises(ValueError):
        list_documents(da[:5], prev, [1], [4])
    with pytest.raises(ValueError):
        Collection([])
    with pytest.raises(ValueError):
        Collection([b"ab"], separator=b"ab")
    # no interval, no text: nothing needs a device
    assert document_frequency(prev, [], []).size == 0
    off, docs = list_documents(da, prev, [2, 5], [2, 5])
    assert off.tolist() == [0, 0, 0] and docs.size == 0
    a, b = document_array(np.zeros(0, np.uint32), [0, 0, 0])
    assert a.size == 0 and b.size == 0
