"""Document collections on the GPU (sa_doc_array / sa_doc_of / sa_doc_frequency /
sa_doc_list and their _device forms, hpc_suffix_array_amd/csrc/sa_docs.h)
against numpy and Python alone.

The kernels read no text, so most cases take a seeded random permutation of
[0, n) as the suffix array.  Expected values: DA by np.searchsorted over the
offsets, PRV by a stable np.argsort of DA, the documents of an interval by
np.unique of its slice of DA.  The frequency and listing cases take DA and
PRV from numpy, so they do not depend on the document-array kernel.  The
end-to-end cases compare Collection with a Python loop over the documents.

Device outputs sit between 0xA5 guard words; every comparison is exact.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD32 = np.uint32(0xA5A5A5A5)
GUARD64 = np.uint64(0xA5A5A5A5A5A5A5A5)
PAD = 8          # guard words on each side
NONE = 0xFFFFFFFF


def consts():
    from hpc_suffix_array_amd import _native as N
    return N.DOC_TILE, N.DOC_GROUP_MAX, N.DOC_LDS_DOCS


_SA = {}


def perm_sa(n):
    """A seeded random permutation of [0, n): computed once, never changed."""
    if n not in _SA:
        a = np.random.default_rng(3000 + n).permutation(n).astype(np.uint32)
        a.setflags(write=False)
        _SA[n] = a
    return _SA[n]


def offsets(n, D, seed, mostly_one=False):
    """D + 1 offsets over [0, n]: random cuts, with empty documents forced at
    the front, at the back and in a run of three in the middle (where D
    allows); mostly_one: one document holds all but two positions."""
    rng = np.random.default_rng(seed)
    off = np.zeros(D + 1, np.uint64)
    off[D] = n
    if D > 1:
        off[1:D] = np.sort(rng.integers(0, n + 1, D - 1))
    if mostly_one:
        assert D >= 5 and n >= 4
        off[1:D] = n - 1
        off[1], off[2] = 1, 1          # document 0 one byte, 1 empty, 2 all but two, the last one byte
        off[D - 1] = n - 1
        off[3:D - 1] = n - 1
    else:
        if D >= 2:
            off[1] = 0
        if D >= 3:
            off[D - 1] = n
        if D >= 8:
            m = D // 2
            off[m + 1:m + 4] = off[m]
    assert (np.diff(off.astype(np.int64)) >= 0).all() and off[0] == 0 and off[D] == n
    return off


def expected_da(sa, off):
    return (np.searchsorted(off, sa.astype(np.uint64), "right") - 1).astype(np.uint32)


def expected_prev(da):
    order = np.argsort(da, kind="stable")
    prev = np.zeros(da.size, np.uint32)
    same = da[order][1:] == da[order][:-1]
    prev[order[1:][same]] = order[:-1][same] + 1
    return prev


@pytest.fixture(scope="module")
def builder(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder((1 << 20) + 3)
    yield b
    b.close()


def up32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


def up64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def guarded32(count, shift=0):
    """(buffer, view of `count` words at PAD + shift) filled with guard words."""
    import torch
    buf = torch.from_numpy(np.full(count + 2 * PAD + 4, GUARD32, np.uint32).view(np.int32)).cuda()
    return buf, buf[PAD + shift:PAD + shift + max(count, 1)]


def read32(buf, count, shift=0, what="output"):
    a = buf.cpu().numpy().view(np.uint32)
    assert (a[:PAD + shift] == GUARD32).all() and (a[PAD + shift + count:] == GUARD32).all(), f"guard around {what}"
    return a[PAD + shift:PAD + shift + count].copy()


# ---- document array and PRV ---------------------------------------------------
NS = [1, 63, 64, 65, 4097, (1 << 16) + 3, (1 << 20) + 3]
DS = [1, 2, 3, 255, 256, 257, 8192, 8193, 65537]     # 8192 / 8193: the last D searched in LDS and the first in global memory


def dev_doc_array(b, d_sa, n, d_off, D, da=True, prev=True, stream=None):
    import torch
    bufa, va = guarded32(n)
    bufp, vp = guarded32(n)
    torch.cuda.synchronize()
    b.doc_array(n, d_sa, d_off, D, va if da else None, vp if prev else None,
                stream=None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    ra, rp = read32(bufa, n if da else 0, what="d_da"), read32(bufp, n if prev else 0, what="d_prev")
    return (ra if da else None), (rp if prev else None)


@pytest.mark.parametrize("n", NS)
def test_document_array(builder, n):
    import torch
    assert consts()[2] == 8192
    sa = perm_sa(n)
    d_sa = up32(sa)
    side = torch.cuda.Stream()
    cases = [(D, False) for D in DS if D <= n + 4]
    if n == 4097:
        cases.append((5, True))
    for D, mostly in cases:
        off = offsets(n, D, 17 * n + D, mostly)
        want_da = expected_da(sa, off)
        want_prev = expected_prev(want_da)
        d_off = up64(off)
        da, prev = dev_doc_array(builder, d_sa, n, d_off, D)
        assert np.array_equal(da, want_da), (n, D)
        assert np.array_equal(prev, want_prev), (n, D)
        # each output alone, a second call, a side stream: the same bytes
        assert np.array_equal(dev_doc_array(builder, d_sa, n, d_off, D, prev=False)[0], want_da)
        assert np.array_equal(dev_doc_array(builder, d_sa, n, d_off, D, da=False)[1], want_prev)
        side.wait_stream(torch.cuda.current_stream())
        da2, prev2 = dev_doc_array(builder, d_sa, n, d_off, D, stream=side)
        assert np.array_equal(da2, want_da) and np.array_equal(prev2, want_prev), (n, D, "side stream")
    if n == 4097:
        # the document that holds all but two positions
        da = expected_da(sa, offsets(n, 5, 0, True))
        assert np.bincount(da, minlength=5).tolist() == [1, 0, n - 2, 0, 1]


def test_doc_of(builder):
    import torch
    for n, D in ((4097, 40), ((1 << 16) + 3, 8193)):
        off = offsets(n, D, 5 * D)
        o = off.astype(np.int64)
        cand = np.concatenate([[0, n - 1, n, n + 5], o, o - 1])
        pos = np.unique(cand[(cand >= 0) & (cand <= n + 5)]).astype(np.uint32)
        rng = np.random.default_rng(D)
        pos = np.concatenate([pos, rng.integers(0, n, 500).astype(np.uint32)])
        want_doc = (np.searchsorted(off, pos.astype(np.uint64), "right") - 1).astype(np.int64)
        want_rel = pos.astype(np.int64) - o[np.minimum(want_doc, D - 1)]
        out = pos >= n
        assert out.sum() >= 2
        want_doc[out] = NONE
        want_rel[out] = NONE
        assert (np.diff(o)[want_doc[~out]] > 0).all()          # never an empty document
        d_off, d_pos = up64(off), up32(pos)
        for doc, rel in ((True, True), (True, False), (False, True)):
            bufd, vd = guarded32(pos.size)
            bufr, vr = guarded32(pos.size)
            torch.cuda.synchronize()
            builder.doc_of(d_off, D, n, d_pos, pos.size, vd if doc else None, vr if rel else None)
            torch.cuda.synchronize()
            gd, gr = read32(bufd, pos.size if doc else 0), read32(bufr, pos.size if rel else 0)
            if doc:
                assert np.array_equal(gd.astype(np.int64), want_doc), (n, D)
            if rel:
                assert np.array_equal(gr.astype(np.int64), want_rel), (n, D)


# ---- frequency and listing ----------------------------------------------------
QN = 20011
_COLL = {}


def collection(D):
    """(DA, PRV, device DA, device PRV) of the permutation of QN cut into D documents, by numpy."""
    if D not in _COLL:
        da = expected_da(perm_sa(QN), offsets(QN, D, 900 + D))
        prev = expected_prev(da)
        _COLL[D] = (da, prev, up32(da), up32(prev))
    return _COLL[D]


def base_queries(n, seed):
    """Every length of the list at a random place, at lo = 0 and at hi = n;
    intervals that break lo <= hi <= n; repeated and overlapping ones."""
    T, G, _ = consts()
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2, 31, 32, 33, 63, 64, 65, G - 1, G, G + 1, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5, n]
    assert G == 256
    lo, hi = [], []
    for c in lens:
        a = int(rng.integers(0, n - c + 1))
        lo += [a, 0, n - c]
        hi += [a + c, c, n]
    lo += [10, n - 5, n + 3, 7, 7, 7, 100, 150]
    hi += [5, n + 1, n + 9, 300, 300, 5000, 4000, 3000]      # lo > hi, hi > n, both; repeats; overlaps
    return np.array(lo, np.int64), np.array(hi, np.int64)


def queries(n, nq, seed):
    lo, hi = base_queries(n, seed)
    if nq <= lo.size:
        pick = np.random.default_rng(seed + 1).permutation(lo.size)[:nq]
        if nq == 1:
            pick = np.array([3 * 16 + 0])                     # 3T + 5 at a random place
        return lo[pick], hi[pick]
    rng = np.random.default_rng(seed + 2)
    c = rng.integers(0, 40, nq - lo.size)
    a = (rng.random(c.size) * (n - c + 1)).astype(np.int64)
    perm = rng.permutation(nq)
    return np.concatenate([lo, a])[perm], np.concatenate([hi, a + c])[perm]


def expected_list(da, lo, hi, max_docs=0, order="doc"):
    n = da.size
    rows = []
    for a, b in zip(lo.tolist(), hi.tolist()):
        if not (a <= b <= n):
            rows.append(np.zeros(0, np.int64))
            continue
        seg = da[a:b]
        _, first = np.unique(seg, return_index=True)
        row = seg[np.sort(first)].astype(np.int64)             # first occurrences in rank order
        if max_docs:
            row = row[:max_docs]
        rows.append(np.sort(row) if order == "doc" else row)
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([r.size for r in rows], out=off[1:])
    return off, (np.concatenate(rows) if rows else np.zeros(0, np.int64))


def dev_frequency(b, n, d_prev, lo, hi, stream=None):
    import torch
    nq = len(lo)
    d_lo, d_hi = up32(lo.astype(np.uint32)), up32(hi.astype(np.uint32))
    buf, v = guarded32(nq)
    torch.cuda.synchronize()
    s = None if stream is None else stream.cuda_stream
    b.doc_frequency(n, d_prev, d_lo, d_hi, nq, v, stream=s)
    b.doc_frequency(n, d_prev, d_lo, d_hi, nq, v, stream=s)    # twice: the call zeroes what it adds into
    torch.cuda.synchronize()
    return read32(buf, nq, what="d_df").astype(np.int64)


def dev_list(b, n, d_da, d_prev, lo, hi, max_docs=0, order="doc", shift=0, want_total=None):
    """The two-call device pattern with guard words: the sizing call and a call
    with docs_cap one below the total return the total and leave d_docs
    untouched; the guards around d_off and d_docs survive."""
    import torch
    nq = len(lo)
    d_lo, d_hi = up32(lo.astype(np.uint32)), up32(hi.astype(np.uint32))
    offbuf = torch.from_numpy(np.full(nq + 1 + 2 * PAD, GUARD64, np.uint64).view(np.int64)).cuda()
    d_off = offbuf[PAD:PAD + nq + 1]
    torch.cuda.synchronize()
    kw = dict(max_docs=max_docs, order=order)
    total = b.doc_list(n, d_da, d_prev, d_lo, d_hi, nq, d_off, None, 0, **kw)
    if want_total is not None:
        assert total == want_total
    buf, d_docs = guarded32(total, shift)
    assert (d_docs.data_ptr() // 4) % 4 == (PAD + shift) % 4
    torch.cuda.synchronize()
    if total:
        assert b.doc_list(n, d_da, d_prev, d_lo, d_hi, nq, d_off, d_docs, total - 1, **kw) == total
        torch.cuda.synchronize()
        assert (buf.cpu().numpy().view(np.uint32) == GUARD32).all(), "docs_cap below the total wrote ids"
    assert b.doc_list(n, d_da, d_prev, d_lo, d_hi, nq, d_off, d_docs, total, **kw) == total
    torch.cuda.synchronize()
    ob = offbuf.cpu().numpy().view(np.uint64)
    assert (ob[:PAD] == GUARD64).all() and (ob[PAD + nq + 1:] == GUARD64).all(), "guard around d_off"
    return ob[PAD:PAD + nq + 1].astype(np.int64), read32(buf, total, shift, "d_docs").astype(np.int64)


@pytest.mark.parametrize("D", [1, 3, 64, 65, 5000])
def test_frequency_and_listing(builder, D):
    T = consts()[0]
    da, prev, d_da, d_prev = collection(D)
    lo, hi = base_queries(QN, 40 + D)
    woff, wdocs = expected_list(da, lo, hi)
    want_df = np.diff(woff)
    assert want_df.max() == min(D, np.unique(da).size) and (D < 5000 or want_df.max() > T)
    df = dev_frequency(builder, QN, d_prev, lo, hi)
    assert np.array_equal(df, want_df)
    k = 0
    for order in ("doc", "rank"):
        for max_docs in (0, 1, 2, T, T + 1):
            eoff, edocs = expected_list(da, lo, hi, max_docs, order)
            off, docs = dev_list(builder, QN, d_da, d_prev, lo, hi, max_docs, order, shift=k % 4,
                                 want_total=int(eoff[-1]))
            k += 1
            assert np.array_equal(off, eoff), (D, order, max_docs)
            assert np.array_equal(docs, edocs), (D, order, max_docs)
            if max_docs == 0:
                assert np.array_equal(np.diff(off), df)        # df = the row lengths of the uncapped listing


@pytest.mark.parametrize("nq", [0, 1, 65, 4099])
def test_query_counts(builder, nq):
    import torch
    D = 65
    da, prev, d_da, d_prev = collection(D)
    lo, hi = queries(QN, nq, 7 * nq + 1)
    assert lo.size == nq
    eoff, edocs = expected_list(da, lo, hi)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert np.array_equal(dev_frequency(builder, QN, d_prev, lo, hi), np.diff(eoff))
    assert np.array_equal(dev_frequency(builder, QN, d_prev, lo, hi, stream=side), np.diff(eoff))
    for order in ("doc", "rank"):
        eoff, edocs = expected_list(da, lo, hi, 0, order)
        off, docs = dev_list(builder, QN, d_da, d_prev, lo, hi, 0, order, shift=1, want_total=int(eoff[-1]))
        assert np.array_equal(off, eoff) and np.array_equal(docs, edocs), (nq, order)


def test_garbage_arrays_stay_in_bounds(builder):
    """PRV and DA of random 32-bit words: the results are unspecified, but the
    calls return, the guards survive, and off is non-decreasing with
    off[nq] == total (the kernels clamp; nothing is read outside the arrays)."""
    rng = np.random.default_rng(99)
    lo, hi = queries(QN, 300, 5)
    valid = (lo <= hi) & (hi <= QN)
    for small in (False, True):
        g_da = rng.integers(0, 1 << 32, QN, dtype=np.uint64).astype(np.uint32)
        g_prev = rng.integers(0, 1 << 32, QN, dtype=np.uint64).astype(np.uint32)
        if small:   # half of PRV below 2n, so that many ranks qualify (some pointing above their own rank)
            g_prev[::2] = rng.integers(0, 2 * QN, g_prev[::2].size)
        d_da, d_prev = up32(g_da), up32(g_prev)
        df = dev_frequency(builder, QN, d_prev, lo, hi)
        assert (df <= np.where(valid, hi - lo, 0)).all()
        assert not small or df.max() > 256
        for order in ("doc", "rank"):
            for max_docs in (0, 3):
                off, docs = dev_list(builder, QN, d_da, d_prev, lo, hi, max_docs, order)
                assert (np.diff(off) >= 0).all() and off[0] == 0 and off[-1] == docs.size
                if max_docs == 0:
                    assert np.array_equal(np.diff(off), df)


# ---- end to end -----------------------------------------------------------------
def documents():
    rng = np.random.default_rng(2025)
    docs = [bytes(rng.choice(list(b"acgt"), int(rng.integers(1, 13))).astype(np.uint8)) for _ in range(40)]
    docs[0] = b""
    docs[7] = docs[3]                    # identical
    docs[12] = docs[3]
    docs[20] = docs[21] = docs[22] = b""
    docs[30] = docs[5][:max(1, len(docs[5]) // 2)]   # a prefix of another
    docs[17] = b"acgtacgg"
    docs[18] = b"ttgaccta"               # "acggttga" occurs only across the boundary 17 | 18
    docs[39] = b""
    return docs


def patterns(docs):
    rng = np.random.default_rng(7)
    pats = [b"acggttga", b"a", b"c", b"gt", b"tt", docs[3], docs[5], docs[30], b"acgtacgg", b"gggggggggg"]
    while len(pats) < 30:
        d = docs[int(rng.integers(0, len(docs)))]
        if len(d) >= 2:
            a = int(rng.integers(0, len(d) - 1))
            pats.append(d[a:a + int(rng.integers(1, 5))])
    return pats


def occurrences(hay, pat):
    out, p = [], hay.find(pat)
    while p >= 0:
        out.append(p)
        p = hay.find(pat, p + 1)
    return out


@pytest.mark.parametrize("separator", [b"\x00", None])
def test_collection_end_to_end(gpu, separator):
    from hpc_suffix_array_amd import Collection
    docs = documents()
    pats = patterns(docs)
    across = pats[0]
    assert all(across not in d for d in docs) and len(occurrences(b"".join(docs), across)) == 1
    if separator is not None:
        want = [[(d, p) for d, doc in enumerate(docs) for p in occurrences(doc, pat)] for pat in pats]
        woff = np.concatenate([[0], np.cumsum([len(d) + 1 for d in docs])])
    else:
        woff = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
        text = b"".join(docs)
        want = []
        for pat in pats:
            ps = np.array(occurrences(text, pat), np.int64)
            ds = np.searchsorted(woff, ps, "right") - 1
            want.append(list(zip(ds.tolist(), (ps - woff[ds]).tolist())))
    with Collection(docs, separator=separator) as c:
        assert np.array_equal(c.doc_offsets, woff)
        count, df = c.count(pats), c.document_frequency(pats)
        off, listed = c.list_documents(pats)
        loc = c.locate(pats)
        off2, listed2 = c.list_documents(pats, max_docs=2)
    for q, pat in enumerate(pats):
        wdocs = sorted({d for d, _ in want[q]})
        assert count[q] == len(want[q]), pat
        assert df[q] == len(wdocs), pat
        assert listed[off[q]:off[q + 1]].tolist() == wdocs, pat
        assert off2[q + 1] - off2[q] == min(2, len(wdocs)) and set(listed2[off2[q]:off2[q + 1]].tolist()) <= set(wdocs)
        assert list(zip(loc[q][0].tolist(), loc[q][1].tolist())) == want[q], pat
    # the pattern that occurs only across a boundary
    assert df[0] == (0 if separator is not None else 1)
    if separator is None:
        assert listed[off[0]:off[1]].tolist() == [17]
    assert df[1] > 20 and df[9] == 0


def test_repeats_compose_with_document_frequency(gpu):
    """maximal_repeats(kind="right") -> document_frequency: for each repeat the
    number of distinct doc(SA[r]) over its interval."""
    from hpc_suffix_array_amd import Collection, document_array, document_frequency, maximal_repeats
    with Collection(documents(), separator=b"\x00") as c:
        text, sa, off = c.text, c.sa, c.doc_offsets
    length, lo, hi = maximal_repeats(text, sa, kind="right")
    assert lo.size > 20
    _, prev = document_array(sa, off)
    df = document_frequency(prev, lo, hi)
    docs = np.searchsorted(off, sa.astype(np.int64), "right") - 1
    want = [np.unique(docs[a:b]).size for a, b in zip(lo.tolist(), hi.tolist())]
    assert df.tolist() == want
    assert max(want) > 1 and min(want) >= 1


# ---- host forms -------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
def test_host_forms(gpu, width):
    L = gpu.lib()
    n, D = QN, 65
    dt = np.uint32 if width == 4 else np.int64
    sa = perm_sa(n).astype(dt)
    off = offsets(n, D, 900 + D)
    want_da = expected_da(perm_sa(n), off)
    want_prev = expected_prev(want_da)
    da, prev = np.zeros(n, dt), np.zeros(n, dt)
    assert L.sa_doc_array(sa.ctypes.data, n, width, off.ctypes.data, D, da.ctypes.data, prev.ctypes.data) == 0
    assert np.array_equal(da, want_da) and np.array_equal(prev, want_prev)
    only = np.zeros(n, dt)
    assert L.sa_doc_array(sa.ctypes.data, n, width, off.ctypes.data, D, None, only.ctypes.data) == 0
    assert np.array_equal(only, want_prev)

    pos = np.array([0, 1, n - 1, n, n + 5, int(off[3]), int(off[D // 2])], dt)
    doc, rel = np.zeros(pos.size, dt), np.zeros(pos.size, dt)
    assert L.sa_doc_of(off.ctypes.data, D, n, pos.ctypes.data, pos.size, width, doc.ctypes.data, rel.ctypes.data) == 0
    wd = np.searchsorted(off, pos.astype(np.uint64), "right") - 1
    wr = pos.astype(np.int64) - off.astype(np.int64)[np.minimum(wd, D - 1)]
    wd[pos.astype(np.int64) >= n] = NONE
    wr[pos.astype(np.int64) >= n] = NONE
    assert doc.astype(np.int64).tolist() == wd.tolist() and rel.astype(np.int64).tolist() == wr.tolist()

    lo, hi = base_queries(n, 11)
    ok = (lo <= hi) & (hi <= n)              # the host forms reject the others
    lo, hi = lo[ok].astype(np.uint64), hi[ok].astype(np.uint64)
    nq = lo.size
    eoff, edocs = expected_list(want_da, lo.astype(np.int64), hi.astype(np.int64))
    df = np.zeros(nq, np.uint64)
    assert L.sa_doc_frequency(prev.ctypes.data, n, width, lo.ctypes.data, hi.ctypes.data, nq, df.ctypes.data) == 0
    assert np.array_equal(df.astype(np.int64), np.diff(eoff))
    for flags, order in ((0, "doc"), (gpu.DOC_RANK_ORDER, "rank")):
        eoff, edocs = expected_list(want_da, lo.astype(np.int64), hi.astype(np.int64), 3, order)
        o = np.zeros(nq + 1, np.uint64)
        out = np.zeros(int(eoff[-1]), dt)
        assert L.sa_doc_list(da.ctypes.data, prev.ctypes.data, n, width, lo.ctypes.data, hi.ctypes.data, nq, 3, flags,
                             o.ctypes.data, out.ctypes.data, out.size) == 0, L.sa_last_error()
        assert np.array_equal(o.astype(np.int64), eoff) and np.array_equal(out.astype(np.int64), edocs)


def test_python_functions(gpu):
    from hpc_suffix_array_amd import doc_of_positions, document_array, document_frequency, list_documents
    n, D = 4097, 257
    sa = perm_sa(n)
    off = offsets(n, D, 3)
    da, prev = document_array(sa, off)
    assert da.dtype == np.uint32 and np.array_equal(da, expected_da(sa, off)) and np.array_equal(prev, expected_prev(da))
    assert np.array_equal(document_array(sa.astype(np.int64), off, prev=False), da.astype(np.int64))
    doc, rel = doc_of_positions(off, n, [0, n - 1, n, n + 5])
    assert doc[2:].tolist() == [-1, -1] and rel[2:].tolist() == [-1, -1]
    assert doc[1] == np.searchsorted(off, n - 1, "right") - 1 and rel[0] == 0
    lo, hi = np.array([0, 5, 100, 9]), np.array([n, 5, 700, 3000])
    eoff, edocs = expected_list(da, lo, hi)
    assert np.array_equal(document_frequency(prev, lo, hi), np.diff(eoff))
    o, d = list_documents(da, prev, lo, hi)
    assert np.array_equal(o, eoff) and np.array_equal(d, edocs)
    eoff, edocs = expected_list(da, lo, hi, 4, "rank")
    o, d = list_documents(da, prev, lo, hi, max_docs=4, order="rank")
    assert np.array_equal(o, eoff) and np.array_equal(d, edocs)
