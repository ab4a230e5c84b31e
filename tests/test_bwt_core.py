"""What the Burrows-Wheeler transform and inverse-suffix-array entry points
(sa_bwt, sa_bwt_device, sa_inverse, sa_inverse_device; include/sa_hip.h,
hpc_suffix_array_amd/csrc/sa_bwt.h) fix without a device: the constants the
header, the kernel and the binding share, the exported symbols, and every
argument check made before the first HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sa_hip.h")
KERNEL = os.path.join(ROOT, "hpc_suffix_array_amd", "csrc", "sa_bwt.h")
SYMBOLS = ["sa_bwt_device", "sa_bwt", "sa_inverse_device", "sa_inverse"]


def _read(path):
    with open(path) as f:
        return f.read()


def test_constants_agree(sa_lib):
    m = re.search(r"^#define\s+SA_BWT_STATS\s+(\d+)", _read(HEADER), re.M)
    assert m and int(m.group(1)) == sa_lib.BWT_STATS == 258
    m = re.search(r"constexpr\s+uint32_t\s+kBwtTile\s*=\s*(\d+)\s*;", _read(KERNEL))
    assert m and int(m.group(1)) == sa_lib.BWT_TILE


def test_symbols_exported_and_listed(sa_lib):
    L = sa_lib.lib()
    h = _read(HEADER)
    for s in SYMBOLS:
        assert s in sa_lib.EXT_SYMBOLS
        assert getattr(L, s) is not None
        assert re.search(r"\bint\s+%s\s*\(" % s, h), s
    import hpc_suffix_array_amd as P
    assert callable(P.bwt) and callable(P.inverse_suffix_array)
    assert "bwt" in P.__all__ and "inverse_suffix_array" in P.__all__
    assert callable(P.SuffixArray.bwt) and callable(P.DeviceBuilder.bwt) and callable(P.DeviceBuilder.inverse)


def test_bwt_arguments_rejected_before_any_device(sa_lib):
    """Everything here returns before the first HIP call."""
    L = sa_lib.lib()
    t = np.frombuffer(b"banana", np.uint8)
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    out = np.zeros(8, np.uint8)
    st = np.full(sa_lib.BWT_STATS, 7, np.uint64)

    def bwt(text=t, n=6, sa_arr=sa, width=4, out_=out, stats=None):
        return L.sa_bwt(text.ctypes.data if text is not None else None, n,
                        sa_arr.ctypes.data if sa_arr is not None else None, width,
                        out_.ctypes.data if out_ is not None else None,
                        stats.ctypes.data if stats is not None else None)

    assert bwt(width=3) == -1 and b"sa_width" in L.sa_last_error()
    assert bwt(n=1 << 32) == -1 and b"too large" in L.sa_last_error()
    assert bwt(text=None) == -1 and b"NULL" in L.sa_last_error()
    assert bwt(out_=None) == -1 and b"NULL" in L.sa_last_error()
    assert bwt(sa_arr=None) == -1 and b"NULL" in L.sa_last_error()
    assert bwt(sa_arr=np.array([5, 3, 1, 0, 4, 6], np.int64), width=8) == -1 and b"out of range" in L.sa_last_error()
    assert bwt(sa_arr=np.array([5, 3, 1, 0, 4, -1], np.int64), width=8) == -1 and b"out of range" in L.sa_last_error()
    # n == 0: no device, the statistics zeroed
    assert bwt(n=0, stats=st) == 0 and not st.any()
    assert bwt(n=0, text=None, sa_arr=None, out_=None) == 0

    # device form: a fake non-NULL address is never dereferenced on these paths
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)

    def dbwt(text=p, n=6, sa_=q, bwt_=r, stats=None):
        return L.sa_bwt_device(text, n, sa_, bwt_, stats, None)

    assert dbwt(text=None) == -1 and b"NULL" in L.sa_last_error()
    assert dbwt(sa_=None) == -1 and b"NULL" in L.sa_last_error()
    assert dbwt(bwt_=None) == -1 and b"NULL" in L.sa_last_error()
    assert dbwt(bwt_=p) == -1 and b"alias" in L.sa_last_error()
    assert dbwt(bwt_=q) == -1 and b"alias" in L.sa_last_error()
    assert dbwt(n=1 << 32) == -1 and b"too large" in L.sa_last_error()
    assert dbwt(n=0) == 0
    assert dbwt(n=0, text=None, sa_=None, bwt_=None) == 0


def test_inverse_arguments_rejected_before_any_device(sa_lib):
    L = sa_lib.lib()
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    out = np.zeros(8, np.int64)

    def inv(sa_arr=sa, n=6, width=4, out_=out):
        return L.sa_inverse(sa_arr.ctypes.data if sa_arr is not None else None, n, width,
                            out_.ctypes.data if out_ is not None else None)

    assert inv(width=3) == -1 and b"sa_width" in L.sa_last_error()
    assert inv(n=1 << 32) == -1 and b"too large" in L.sa_last_error()
    assert inv(sa_arr=None) == -1 and b"NULL" in L.sa_last_error()
    assert inv(out_=None) == -1 and b"NULL" in L.sa_last_error()
    assert inv(sa_arr=np.array([5, 3, 1, 0, 4, 6], np.int64), width=8) == -1 and b"out of range" in L.sa_last_error()
    assert inv(sa_arr=np.array([5, 3, 1, 0, 4, -1], np.int64), width=8) == -1 and b"out of range" in L.sa_last_error()
    assert inv(n=0) == 0
    assert inv(n=0, sa_arr=None, out_=None) == 0
    # the device form needs a context before anything else
    p = ctypes.c_void_p(4096)
    assert L.sa_inverse_device(None, 6, p, p, None) == -1 and b"context" in L.sa_last_error()


def test_no_bwt_without_device(sa_lib):
    if sa_lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    from hpc_suffix_array_amd import SAError, bwt, inverse_suffix_array
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(SAError):
        bwt(b"banana", sa)
    with pytest.raises(SAError):
        bwt(b"banana", sa, stats=True)
    with pytest.raises(SAError):
        inverse_suffix_array(sa)
    with pytest.raises(SAError):
        inverse_suffix_array(sa, width=8)
    L = sa_lib.lib()
    t = np.frombuffer(b"banana", np.uint8)
    out = np.zeros(8, np.uint64)
    rc = L.sa_bwt(t.ctypes.data, 6, sa.ctypes.data, 4, out.ctypes.data, None)
    assert rc < 0 and b"device" in L.sa_last_error()
    rc = L.sa_inverse(sa.ctypes.data, 6, 4, out.ctypes.data)
    assert rc < 0 and b"device" in L.sa_last_error()


def test_python_argument_errors():
    from hpc_suffix_array_amd import SAError, bwt, inverse_suffix_array
    sa = np.array([5, 3, 1, 0, 4, 2], np.uint32)
    with pytest.raises(ValueError):
        bwt(b"banana", sa[:5])                                  # SA and text differ in length
    with pytest.raises(ValueError):
        inverse_suffix_array(sa, width=3)
    with pytest.raises(SAError):
        inverse_suffix_array(np.array([0, 1, 1 << 32], np.int64), width=4)   # would wrap when narrowed
