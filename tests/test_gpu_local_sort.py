"""The fixed-span 32-bit local sort of the bucketed first round (sa_bucket.h
k_bucket_sort) against the oracle, at sizes the oracle sorts in a second.

Production reaches that kernel from 2^28 suffixes (sa_round1.h fast32: an
average bucket of four window strides); debug flag fast32_small drops that
size term, and the texts of tests/local_sort_texts.py hold runs of buckets
large enough to be one-bucket windows, with sub-buckets of every size class,
windows at the kernel's size edges and tie groups.  tests/test_local_sort_texts.py
asserts that coverage on the CPU; here every build must

  * equal the oracle's suffix array,
  * take the bucketed round,
  * send exactly the windows the model predicts to the fixed-span kernel and
    to the measured-span retry (sa_stats.round1_windows), and
  * leave the groups (D_j of every round) the LSD first round leaves at the
    same init_chars.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_sort_texts as L   # noqa: E402

pytestmark = pytest.mark.gpu

_wants = {}
_lsd = {}


def _want(oracle, name):
    """The oracle's SA of a text, computed once."""
    if name not in _wants:
        _wants[name] = oracle.sa_c(L.text(name))
    return _wants[name]


def _lsd_distinct(name, K):
    """D_j of the LSD first round at init_chars K, once per (text, K)."""
    from hpc_suffix_array_amd import build_suffix_array
    if (name, K) not in _lsd:
        _, st = build_suffix_array(L.text(name), return_stats=True, round1="lsd", init_chars=K)
        assert st["round1"] == "lsd" and st["init_chars"] == K, st
        _lsd[name, K] = st["distinct"]
    return _lsd[name, K]


def _leg(oracle, name, debug=(), init_chars=0, tune=0):
    from hpc_suffix_array_amd import build_suffix_array
    m = L.model(name, init_chars, "eonly" in debug)
    got, st = build_suffix_array(L.text(name), return_stats=True, round1="bucketed", init_chars=init_chars,
                                 debug=("fast32_small",) + tuple(debug), tune=tune)
    tag = (name, debug, init_chars, tune)
    w = st["round1_windows"]
    print(tag, "windows", w, "model", (m.listed, m.one_bucket_windows, m.retried), st["round1_layout"], flush=True)
    assert st["round1"] == "bucketed", (tag, st["round1"], st["largest_window"])
    assert st["init_chars"] == m.plan["K"], (tag, st["init_chars"], m.plan["K"])
    lay = st["round1_layout"]
    assert (lay["compact"], lay["eonly"]) == (m.plan["cmp"] != 0, m.plan["cmp"] == 2), (tag, lay)
    assert st["largest_window"] == m.largest_window, (tag, st["largest_window"], m.largest_window)
    assert w[0] == m.listed, (tag, w, m.listed)
    assert w[1] == m.one_bucket_windows, (tag, w, m.one_bucket_windows)
    if m.plan["fast32"]:
        assert w[2] == m.retried, (tag, w, m.retried, m.clustered)
    assert st["sparse_ranks"] == (not m.dense), (tag, st["sparse_ranks"], m.unsorted)
    assert st["distinct"][0] == m.distinct, (tag, st["distinct"][0], m.distinct)
    assert (got == _want(oracle, name)).all(), tag
    assert st["distinct"] == _lsd_distinct(name, st["init_chars"]), (tag, st["distinct"])
    return st


@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_default(gpu, oracle, name):
    """Every window class, size edge and the dense / sparse second launch,
    default variant, packed 8-byte items."""
    st = _leg(oracle, name)
    assert st["round1_layout"]["pk8"] and not st["round1_layout"]["xq"], st["round1_layout"]


@pytest.mark.parametrize("v", [1, 2, 3, 4])
@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_variants(gpu, oracle, name, v):
    """k_bucket_sort's LSV variants (sa_opts.tune bits 16-19): unconditional
    network reads, indices written back by the sorting threads, both."""
    _leg(oracle, name, tune=v << 16)


@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_key1_samples(gpu, oracle, name):
    """no_key1_round: the kernel writes the sorted key1 samples
    (for_each_sample, mn + ...) and round 2 searches them."""
    _leg(oracle, name, debug=("no_key1_round",))
    _leg(oracle, name, debug=("no_key1_round",), tune=3 << 16)   # LSV & 2 keeps the words for the samples


@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_span_edges(gpu, oracle, name):
    """The key span through init_chars: 2, 4 and kLowMax = 18 key bits below
    the sub-bucket (R = 6, 7, 14); one symbol more (R = 15) is too wide for
    the 32-bit words and no window may take the fixed-span kernel."""
    st0 = _leg(oracle, name)
    s = L.model(name).plan["s"]
    R0 = st0["init_chars"] - s
    for R in (6, 7, 14):
        if R == R0:
            continue
        st = _leg(oracle, name, init_chars=s + R)
        assert st["round1_windows"][1] >= 100
    st = _leg(oracle, name, init_chars=s + 15)
    assert st["round1_windows"][1] == 0, st["round1_windows"]


@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_unpacked_items(gpu, oracle, name):
    """no_pk8: 12-byte first-pass items feed the same sort."""
    st = _leg(oracle, name, debug=("no_pk8",))
    assert not st["round1_layout"]["pk8"], st["round1_layout"]


@pytest.mark.parametrize("debug", [(), ("no_key1_round",), ("eonly",), ("eonly", "no_key1_round")])
@pytest.mark.parametrize("name", ["byte256", "alnum"])
def test_other_alphabets(gpu, oracle, name, debug):
    """sigma = 256 (IDENT first pass) and alnum (non-power-of-two buckets of
    ~226 D values: the window header's Dmin is not the bucket id, and the key
    samples add it back), compact and E-only lows."""
    _leg(oracle, name, debug=debug)


def test_xq_loads(gpu, oracle):
    """The per-XCD loads (k_bucket_sort<.., XQ = true>, load_items_cr /
    load_items_xq, k_window_rows, k_window_gather) on the dense DNA recipe at
    2^23 suffixes, the smallest power of two at which the recipe's second
    pass keeps its per-XCD regions (at 2^22 a queue's share of the anchored
    digit outgrows its sub-region and the round re-runs with one region).
    The regions need keys_u's slack, which a context gets with unsorted-set
    buffers for 2^26 suffixes: one build of that size comes first.  Both row
    forms (sa_opts.tune bit 29).  k_window_split also sends one-bucket windows
    whose chunks do not fit the row table to the measured-span kernel, so the
    count is bounded, not modelled.  (The oracle takes ~7 s on this text.)"""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder
    n, n0 = 1 << 23, 1 << 26
    t = L.xq_text(n)
    want = torch.from_numpy(oracle.sa_c(t).view(np.int32)).cuda()
    b = DeviceBuilder(n0)
    try:
        big = torch.empty(n0, dtype=torch.uint8, device="cuda")
        sa = torch.empty(n0, dtype=torch.int32, device="cuda")
        b.generate_text(big, n0, b"ACGT", seed=1)
        b.build(big, n0, sa)
        del big
        d = torch.from_numpy(t).cuda()
        sa = sa[:n]
        ref = b.build(d, n, sa, round1="lsd", init_chars=L.min_chars(4, n))
        assert bool((sa == want).all().item())
        for tune in (0, 1 << 29):
            sa.fill_(-1)
            st = b.build(d, n, sa, round1="bucketed", debug=("fast32_small",), tune=tune)
            print("xq", tune >> 29, st["round1_layout"], st["round1_windows"], flush=True)
            assert st["round1"] == "bucketed" and st["round1_layout"]["xq"], (tune, st["round1"], st["round1_layout"])
            assert st["round1_windows"][1] > 100, st["round1_windows"]
            assert st["init_chars"] == ref["init_chars"] and st["distinct"] == ref["distinct"], (tune, st["distinct"])
            assert bool((sa == want).all().item()), tune
    finally:
        b.close()
