"""The first bucket pass (sa_split.h k_split_text) at the edges of its tile
staging: the text's end inside the tile, inside the halo, on a 16-byte chunk
edge and on both sides of the whole-tile / interior-tile boundaries; a text
pointer that is not 16-byte aligned; the non-compact key layout over a short
last tile; the unpacked and non-compact layouts at a ragged size.

Every build is forced to the bucketed first round and compared with the
oracle.  T = 6144 positions is the tile of the power-of-two alphabets' kernels
(512 threads x 12 items; the others take 12288), 11 T the smallest multiple
that still takes the bucketed round.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 6144
KINDS = ["dna", "binary", "byte256", "alnum"]   # the DNA, generic POW2, IDENT and NP2 kernels

_wants = {}


def _text(oracle, kind, n):
    t = oracle.gen_text(kind, n, seed=3 * n + len(kind))
    t[-1] = t.max()   # no tail run of the smallest symbol: the compact layout
    return t


def _want(oracle, t):
    """The oracle's SA of t, computed once per text."""
    key = (len(t), t[:64].tobytes(), t[-64:].tobytes())
    if key not in _wants:
        _wants[key] = oracle.sa_c(t)
    return _wants[key]


def _bucketed(t, **kw):
    from hpc_suffix_array_amd import build_suffix_array
    got, st = build_suffix_array(t, return_stats=True, round1="bucketed", **kw)
    assert st["round1"] == "bucketed", st
    return got, st


@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges(gpu, oracle, kind):
    """n = 11 T + d for d in {-1, 0, 1, K - 1, K, 63, 64, 65} and n = 65537."""
    _, st = _bucketed(_text(oracle, kind, 11 * T))
    K = st["init_chars"]
    sizes = sorted({11 * T + d for d in (-1, 0, 1, K - 1, K, 63, 64, 65)} | {65537})
    for n in sizes:
        t = _text(oracle, kind, n)
        got, st = _bucketed(t)
        assert st["init_chars"] == K, (kind, n, st["init_chars"], K)
        assert (got == _want(oracle, t)).all(), (kind, n)


@pytest.mark.parametrize("kind", ["dna", "alnum"])
def test_unaligned_text(gpu, oracle, kind):
    """DeviceBuilder.build on a device view 1, 4, 8 and 15 bytes into an
    allocation: the same SA as from an aligned copy of the same bytes."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder
    n = 11 * T + 5
    t = _text(oracle, kind, n)
    want = _want(oracle, t)
    b = DeviceBuilder(n)
    try:
        d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
        d_al = torch.from_numpy(t).cuda()
        assert d_al.data_ptr() % 16 == 0
        st = b.build(d_al, n, d_sa, round1="bucketed")
        torch.cuda.synchronize()
        assert st["round1"] == "bucketed", st
        aligned = d_sa.cpu().numpy().view(np.uint32).copy()
        assert (aligned == want).all(), kind
        buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        for off in (1, 4, 8, 15):
            view = buf[off:off + n]
            view.copy_(d_al)
            assert view.data_ptr() % 16 == off
            d_sa.fill_(-1)
            st = b.build(view, n, d_sa, round1="bucketed")
            torch.cuda.synchronize()
            assert st["round1"] == "bucketed", st
            assert (d_sa.cpu().numpy().view(np.uint32) == aligned).all(), (kind, off)
    finally:
        b.close()


@pytest.mark.parametrize("tail", [b"GAA", b"A" * 9])
def test_short_last_tile_noncompact(gpu, oracle, tail):
    """Several whole tiles, then a short one ending in a run of the smallest
    symbol: the original (non-compact) key layout (sa_round1.h
    short_suffix_ties), so the per-item key loop and bucket_low run over the
    staged tile."""
    n = 11 * T + 37
    t = np.concatenate([oracle.gen_text("dna", n - len(tail), seed=n + len(tail)), np.frombuffer(tail, np.uint8)])
    got, st = _bucketed(t)
    assert not st["round1_layout"]["compact"], st["round1_layout"]
    assert (got == _want(oracle, t)).all(), tail


@pytest.mark.parametrize("layout", ["no_pk8", "no_cmp"])
@pytest.mark.parametrize("kind", KINDS)
def test_layout_flags_ragged(gpu, oracle, kind, layout):
    """The unpacked (12-byte) items and the original key layout at one ragged
    size per kind."""
    n = 11 * T + 65
    t = _text(oracle, kind, n)
    got, st = _bucketed(t, debug=(layout,))
    lay = st["round1_layout"]
    if layout == "no_pk8":
        assert not lay["pk8"], (kind, lay)
    else:
        assert not lay["compact"], (kind, lay)
    assert (got == _want(oracle, t)).all(), (kind, layout)
