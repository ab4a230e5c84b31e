"""What the host-pointer entry points answer before their first HIP call
(sa_check, sa_lcp, sa_build_ex here; sa_find, sa_match, sa_bwt, sa_inverse and
sa_locate have their own *_core files): one table of (entry point, what is
wrong, return code, word of sa_last_error()), and for every host form the
order of its checks: a call with two things wrong reports the one the form
looks at first.  None of this needs a device; the rows that expect "no HIP
device" are skipped when one is visible."""
import ctypes

import numpy as np
import pytest

TEXT = np.frombuffer(b"banana", np.uint8)
SA4 = np.array([5, 3, 1, 0, 4, 2], np.uint32)
SA8 = SA4.astype(np.int64)
SA8_HIGH = np.array([5, 3, 1, 0, 4, 6], np.int64)     # an entry >= n
SA8_NEG = np.array([5, 3, 1, 0, 4, -1], np.int64)
OUT = np.zeros(8, np.uint64)                          # room for 6 entries at either width
NEG = "negative"                                      # any error code (the no-device rows)


def _p(a):
    return None if a is None else a.ctypes.data


def check(L, text=TEXT, n=6, sa=SA4, width=4):
    return L.sa_check(_p(text), n, _p(sa), width)


def lcp(L, text=TEXT, n=6, sa=SA4, width=4, out=OUT):
    """sa_lcp with lrs_len / lrs_pos preset to 7: every row also checks that
    the call zeroed them (nothing repeats in a call that fails or has n == 0)."""
    ln, pos = ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = L.sa_lcp(_p(text), n, _p(sa), width, _p(out), ctypes.byref(ln), ctypes.byref(pos))
    assert (ln.value, pos.value) == (0, 0)
    return rc


def build(L, text=TEXT, n=6, out=OUT, width=4, stats=None):
    return L.sa_build_ex(_p(text), n, _p(out), width, None, None if stats is None else ctypes.byref(stats))


# entry point, what is wrong, return code, word of sa_last_error() (None: not looked at)
ROWS = [
    (check, dict(width=3), -1, b"sa_width"),
    (check, dict(n=0), 1, None),
    (check, dict(n=0, text=None, sa=None), 1, None),
    (check, dict(text=None), -1, b"NULL"),
    (check, dict(sa=None), -1, b"NULL"),
    (check, dict(n=1 << 32), -1, b"too large"),
    (check, dict(sa=SA8_HIGH, width=8), 0, None),      # not a suffix array, and not an error
    (check, dict(sa=SA8_NEG, width=8), 0, None),
    (check, dict(), NEG, b"device"),
    (check, dict(sa=SA8, width=8), NEG, b"device"),
    (lcp, dict(width=3), -1, b"sa_width"),
    (lcp, dict(n=0), 0, None),
    (lcp, dict(n=0, text=None, sa=None, out=None), 0, None),
    (lcp, dict(text=None), -1, b"NULL"),
    (lcp, dict(sa=None), -1, b"NULL"),
    (lcp, dict(out=None), -1, b"NULL"),
    (lcp, dict(n=1 << 32), -1, b"too large"),
    (lcp, dict(sa=SA8_HIGH, width=8), -1, b"out of range"),
    (lcp, dict(sa=SA8_NEG, width=8), -1, b"out of range"),
    (lcp, dict(), NEG, b"device"),
    (lcp, dict(sa=SA8, width=8), NEG, b"device"),
    (build, dict(width=3), -1, b"sa_width"),           # test_abi.py's rows, with their messages
    (build, dict(text=None, n=4, out=None), -1, b"NULL"),
    (build, dict(text=None), -1, b"NULL"),
    (build, dict(out=None), -1, b"NULL"),
    (build, dict(n=0, text=None, out=None), 0, None),
    (build, dict(), NEG, b"device"),
]


@pytest.mark.parametrize("row", ROWS, ids=[f"{i:02d}-{r[0].__name__}-{'-'.join(r[1]) or 'valid'}"
                                            for i, r in enumerate(ROWS)])
def test_table(sa_lib, row):
    f, kw, want, word = row
    if word == b"device" and sa_lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = sa_lib.lib()
    rc = f(L, **kw)
    assert rc < 0 if want is NEG else rc == want, rc
    if word is not None:
        assert word in L.sa_last_error(), L.sa_last_error()


def test_build_ex_empty_text_fills_stats(sa_lib):
    L = sa_lib.lib()
    st = sa_lib.SaStats()
    ctypes.memset(ctypes.byref(st), 0xFF, ctypes.sizeof(st))
    assert build(L, n=0, stats=st) == 0
    assert st.n_kinds == sa_lib.SA_K_COUNT
    assert st.rounds == 0 and st.total_ms == 0.0 and st.h2d_ms == 0.0 and st.d2h_ms == 0.0


def test_order_of_checks(sa_lib):
    """Two things wrong: the form reports the one it looks at first.  Every
    argument check comes before the first HIP call, "no HIP device" last."""
    L = sa_lib.lib()
    pat = np.frombuffer(b"anaxy", np.uint8)
    off = np.array([0, 3, 5], np.uint64)
    off_dec = np.array([0, 4, 3], np.uint64)
    lo, hi = np.array([1, 0], np.uint64), np.array([4, 2], np.uint64)
    out = [np.full(8, 99, np.uint64) for _ in range(3)]
    stats = np.full(sa_lib.BWT_STATS, 7, np.uint64)

    def find(text=TEXT, n=6, sa=SA4, width=4, off_=off, nq=2, flags=0):
        return L.sa_find_ex(_p(text), n, _p(sa), width, _p(pat), _p(off_), nq, _p(out[0]), _p(out[1]), flags)

    def match(text=TEXT, n=6, sa=SA4, width=4, off_=off, nq=2, flags=0, lo_=out[1], hi_=out[2]):
        return L.sa_match(_p(text), n, _p(sa), width, _p(pat), _p(off_), nq, _p(out[0]), _p(lo_), _p(hi_), flags)

    def stats_(text=TEXT, n=6, sa=SA4, width=4, m=5, flags=0, lo_=out[1], hi_=out[2]):
        return L.sa_matching_stats(_p(text), n, _p(sa), width, _p(pat), m, 0, _p(out[0]), _p(lo_), _p(hi_), flags)

    def bwt(text=TEXT, n=6, sa=SA4, width=4, st=None):
        return L.sa_bwt(_p(text), n, _p(sa), width, _p(out[0]), _p(st))

    def inverse(sa=SA4, n=6, width=4, out_=out[0]):
        return L.sa_inverse(_p(sa), n, width, _p(out_))

    def locate(sa=SA4, n=6, width=4, lo_=lo, hi_=hi, nq=2, flags=0, off_=out[0], pos=out[1], cap=8):
        return L.sa_locate(_p(sa), n, width, _p(lo_), _p(hi_), nq, 0, flags, _p(off_), _p(pos), cap)

    for f in (find, match):
        assert f(width=3, flags=7) == -1 and b"sa_width" in L.sa_last_error()
        assert f(flags=7, nq=0) == -1 and b"flags" in L.sa_last_error()       # flags before "no queries"
        assert f(nq=0, text=None, sa=None) == 0
        assert f(text=None, n=1 << 32) == -1 and b"NULL" in L.sa_last_error()
        assert f(n=1 << 32, off_=off_dec) == -1 and b"too large" in L.sa_last_error()
        assert f(off_=off_dec, sa=SA8_HIGH, width=8) == -1 and b"offsets" in L.sa_last_error()
        assert f(sa=SA8_HIGH, width=8) == -1 and b"out of range" in L.sa_last_error()   # never "no HIP device"
    for f in (match, stats_):
        assert f(hi_=None, n=1 << 32) == -1 and b"both or neither" in L.sa_last_error()
        assert f(text=None, hi_=None) == -1 and b"NULL" in L.sa_last_error()
    assert stats_(width=3, flags=7) == -1 and b"sa_width" in L.sa_last_error()
    assert stats_(flags=7, m=0) == -1 and b"flags" in L.sa_last_error()
    assert stats_(sa=SA8_NEG, width=8) == -1 and b"out of range" in L.sa_last_error()

    assert bwt(width=3, n=1 << 32, st=stats) == -1 and b"sa_width" in L.sa_last_error()
    assert not stats.any()                                                   # zeroed before anything is checked
    assert bwt(n=1 << 32, text=None) == -1 and b"too large" in L.sa_last_error()
    assert bwt(text=None, sa=SA8_HIGH, width=8) == -1 and b"NULL" in L.sa_last_error()
    assert bwt(width=3, n=0) == -1 and b"sa_width" in L.sa_last_error()

    assert inverse(width=3, n=1 << 32) == -1 and b"sa_width" in L.sa_last_error()
    assert inverse(n=1 << 32, sa=None) == -1 and b"too large" in L.sa_last_error()
    assert inverse(out_=None, sa=SA8_HIGH, width=8) == -1 and b"NULL" in L.sa_last_error()
    assert inverse(width=3, n=0) == -1 and b"sa_width" in L.sa_last_error()

    assert locate(width=3, n=1 << 32) == -1 and b"sa_width" in L.sa_last_error()
    assert locate(n=1 << 32, flags=8) == -1 and b"too large" in L.sa_last_error()
    assert locate(flags=8, off_=None) == -1 and b"flags" in L.sa_last_error()
    assert locate(off_=None, nq=0) == -1 and b"off_out" in L.sa_last_error()
    out[0][:] = 99
    assert locate(cap=4, sa=None) == -1 and b"pos_cap" in L.sa_last_error()   # the cap before the SA is looked at
    assert out[0][:3].tolist() == [0, 3, 5]                                  # and the offsets are the host's own
    assert locate(sa=None) == -1 and b"sa is NULL" in L.sa_last_error()
    assert locate(sa=SA8_HIGH, width=8, pos=None) == -1 and b"out of range" in L.sa_last_error()
    z = np.array([2, 5], np.uint64)
    assert locate(sa=SA8_HIGH, width=8, lo_=z, hi_=z) == -1 and b"out of range" in L.sa_last_error()
    assert locate(lo_=z, hi_=z, pos=None) == 0                               # no hits: no pos_out, no device
    assert locate(lo_=None, cap=0) == -1 and b"interval array" in L.sa_last_error()

    assert check(L, width=3, n=0) == -1 and b"sa_width" in L.sa_last_error()
    assert check(L, text=None, n=1 << 32) == -1 and b"NULL" in L.sa_last_error()
    assert lcp(L, width=3, n=0) == -1 and b"sa_width" in L.sa_last_error()
    assert lcp(L, out=None, n=1 << 32) == -1 and b"NULL" in L.sa_last_error()
    assert lcp(L, n=1 << 32, sa=SA8_HIGH, width=8) == -1 and b"too large" in L.sa_last_error()
    assert build(L, width=3, text=None) == -1 and b"sa_width" in L.sa_last_error()
    assert build(L, width=3, n=0) == -1 and b"sa_width" in L.sa_last_error()
