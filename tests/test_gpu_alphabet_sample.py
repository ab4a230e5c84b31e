"""The alphabet from a sample of the text, proven by the first bucket pass
(sa_build.hip build_packed, sa_split.h k_split_text alpha_bad, sa_alpha.h).

alpha_sample_small makes the sample the text's first 4096 bytes at any size,
so both outcomes are reached at sizes the oracle sorts: a text whose symbols
all occur there builds with the sampled alphabet ("sampled"); one foreign byte
further on refutes it in the first pass and the build runs again with the
exact alphabet ("refuted").  Every case asserts stats["alphabet"], so none
passes by silently taking the exact path, and compares the SA with the
oracle's.

T = 6144 positions is the tile of the power-of-two alphabets' first pass
(512 threads x 12 items; the others take 12288).

The host also holds the text's last 64 bytes (the tail copy of the key layout's
check): a byte there that the sample lacks shows before any pass that the
sample is incomplete, and the exact scan runs at once ("exact", one first
pass).  Position 11 T + 5 of the 11 T + 37 byte text lies inside that tail
(32 bytes before the end), so it is such a case; the short last tile outside
the tail copy is reached at n = 11 T + 101 instead, where it refutes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 6144
SMALL = ("alpha_sample_small",)
N_REF = 11 * T + 37
POSITIONS = {"first-outside-sample": 4096, "mid-tile": 3 * T + 1000, "tile-end": 5 * T - 1, "tile-start": 5 * T,
             "before-tail": N_REF - 100}

_wants = {}


def _want(oracle, t):
    """The oracle's SA of t, computed once per text."""
    key = t.tobytes()
    if key not in _wants:
        _wants[key] = oracle.sa_c(t)
    return _wants[key]


def _text(oracle, kind, n):
    t = oracle.gen_text(kind, n, seed=3 * n + len(kind))
    t[-1] = t.max()   # no tail run of the smallest symbol: the compact layout
    return t


def _dna_with(oracle, n, p, b):
    t = _text(oracle, "dna", n)
    t[p] = b
    return t


@pytest.fixture(scope="module")
def builder(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder((1 << 20) + 64)
    yield b
    b.close()


def _build(gpu, builder, d_text, n, round1="bucketed", debug=SMALL, profile=False):
    import torch
    d_sa = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    before = gpu.lib().sa_host_syncs()
    st = builder.build(d_text, n, d_sa, round1=round1, debug=debug, profile=profile)
    syncs = gpu.lib().sa_host_syncs() - before
    torch.cuda.synchronize()
    return d_sa.cpu().numpy().view(np.uint32), st, syncs


def _build_host(gpu, builder, t, **kw):
    import torch
    return _build(gpu, builder, torch.from_numpy(t).cuda(), int(t.size), **kw)


def _sigma(t):
    return int(np.unique(t).size)


@pytest.mark.parametrize("kind", ["dna", "binary", "alnum", "byte256"])
def test_proven(gpu, oracle, builder, kind):
    n = 11 * T + 65
    t = _text(oracle, kind, n)
    assert set(t[:4096].tolist()) == set(t.tolist()), "the sample must hold every symbol"
    got, st, syncs = _build_host(gpu, builder, t)
    print(kind, "alphabet", st["alphabet"], "sigma", st["sigma"], "host waits", syncs)
    assert st["alphabet"] == "sampled" and st["round1"] == "bucketed", st
    assert st["sigma"] == _sigma(t)
    assert (got == _want(oracle, t)).all(), kind
    alt, st_alt, syncs_alt = _build_host(gpu, builder, t, debug=("no_alpha_sample",))
    assert st_alt["alphabet"] == "exact" and (alt == got).all()
    assert syncs == syncs_alt, (syncs, syncs_alt)   # no new host wait


@pytest.mark.parametrize("where", sorted(POSITIONS))
@pytest.mark.parametrize("b", ["N", "B", "a", "U", "E"])   # the last four collide with valid SWAR digits
def test_refuted_dna(gpu, oracle, builder, b, where):
    t = _dna_with(oracle, N_REF, POSITIONS[where], ord(b))
    got, st, _ = _build_host(gpu, builder, t)
    assert st["alphabet"] == "refuted", (b, where, st["alphabet"])
    assert st["sigma"] == 5
    assert (got == _want(oracle, t)).all(), (b, where)


@pytest.mark.parametrize("b", ["N", "B", "a", "U", "E"])
def test_short_last_tile(gpu, oracle, builder, b):
    """Position 11 T + 5: inside the host's tail copy at n = 11 T + 37 (the
    sample is dropped before any pass), outside it at n = 11 T + 101 (the
    byte-wise staging of the short last tile refutes it)."""
    p = 11 * T + 5
    t = _dna_with(oracle, N_REF, p, ord(b))
    got, st, _ = _build_host(gpu, builder, t, profile=True)
    assert st["alphabet"] == "exact" and st["sigma"] == 5, (b, st["alphabet"])
    assert st["kernels"]["scatter_first"]["launches"] == 1
    assert (got == _want(oracle, t)).all(), b
    n = 11 * T + 101
    t = _dna_with(oracle, n, p, ord(b))
    got, st, _ = _build_host(gpu, builder, t)
    assert st["alphabet"] == "refuted" and st["sigma"] == 5, (b, st["alphabet"])
    assert (got == _want(oracle, t)).all(), b


def test_refuted_alnum(gpu, oracle, builder):
    t = _text(oracle, "alnum", N_REF)
    t[3 * T + 7] = ord("!")
    assert ord("!") not in t[:4096] and _sigma(t[:4096]) == 62
    got, st, _ = _build_host(gpu, builder, t)
    assert st["alphabet"] == "refuted" and st["sigma"] == 63, st
    assert (got == _want(oracle, t)).all()


def test_refuted_255_of_256(gpu, oracle, builder):
    """Sampled sigma 255 (the byte map's largest digit, 254, beside the absent
    marker), true sigma 256: the re-run takes the 8-byte-window kernel."""
    t = np.random.RandomState(5).randint(0, 255, size=N_REF).astype(np.uint8)
    t[-1] = 254
    t[3 * T + 7] = 0xFF
    assert set(t[:4096].tolist()) == set(range(255))
    got, st, _ = _build_host(gpu, builder, t)
    assert st["alphabet"] == "refuted" and st["sigma"] == 256 and st["round1"] == "bucketed", st
    assert (got == _want(oracle, t)).all()
    # and proven without the 0xFF: digit 254 is no marker
    t[3 * T + 7] = 7
    got, st, _ = _build_host(gpu, builder, t)
    assert st["alphabet"] == "sampled" and st["sigma"] == 255, st
    assert (got == _want(oracle, t)).all()


@pytest.mark.parametrize("back", [1, 10])
def test_tail(gpu, oracle, builder, back):
    """A foreign byte the host sees in the tail copy: no wasted pass."""
    t = _dna_with(oracle, N_REF, N_REF - back, ord("N"))
    got, st, _ = _build_host(gpu, builder, t, profile=True)
    assert st["alphabet"] == "exact" and st["sigma"] == 5, st["alphabet"]
    assert st["kernels"]["scatter_first"]["launches"] == 1
    assert (got == _want(oracle, t)).all(), back


def test_unaligned_text(gpu, oracle, builder):
    """One proven and one refuted DNA text on device views 1 and 15 bytes into
    an allocation (the 4-byte loads of k_split_text)."""
    import torch
    n = 11 * T + 5
    good = _text(oracle, "dna", n)
    bad = _dna_with(oracle, n, 3 * T + 1000, ord("B"))
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for t, outcome, sigma in ((good, "sampled", 4), (bad, "refuted", 5)):
        want = _want(oracle, t)
        for off in (1, 15):
            view = buf[off:off + n]
            view.copy_(torch.from_numpy(t).cuda())
            assert view.data_ptr() % 16 == off
            got, st, _ = _build(gpu, builder, view, n)
            assert st["alphabet"] == outcome and st["sigma"] == sigma, (outcome, off, st["alphabet"])
            assert (got == want).all(), (outcome, off)


def test_not_bucketed(gpu, oracle, builder):
    """sigma 1 in the sample: the exact scan runs right there."""
    n = (1 << 20) + 3
    t = np.full(n, ord("a"), np.uint8)
    t[n // 2] = ord("b")
    got, st, _ = _build_host(gpu, builder, t, round1="auto")
    assert st["alphabet"] == "exact" and st["sigma"] == 2, st
    assert (got == _want(oracle, t)).all()


def test_defaults(gpu, oracle, builder):
    n = 11 * T + 65
    t = _text(oracle, "dna", n)
    want = _want(oracle, t)
    for debug in ((), ("no_alpha_sample", "alpha_sample_small")):
        got, st, _ = _build_host(gpu, builder, t, debug=debug)
        assert st["alphabet"] == "exact", (debug, st["alphabet"])
        assert (got == want).all(), debug


def test_rerun_leaves_context_clean(gpu, oracle, builder):
    bad = _dna_with(oracle, N_REF, 3 * T + 1000, ord("N"))
    got, st, _ = _build_host(gpu, builder, bad)
    assert st["alphabet"] == "refuted"
    assert (got == _want(oracle, bad)).all()
    good = _text(oracle, "dna", 11 * T + 65)
    got, st, _ = _build_host(gpu, builder, good)
    assert st["alphabet"] == "sampled", st["alphabet"]
    assert (got == _want(oracle, good)).all()
