"""The coverage of tests/test_gpu_local_sort.py is a condition, checked here on
the CPU: the window model (tests/local_sort_texts.py) must show, for every
text the GPU tests build, enough one-bucket windows of every kind that the
fixed-span local sort (sa_bucket.h k_bucket_sort) takes each of its paths.
Parameters of the texts are chosen against these assertions, never against
what the GPU returns."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_sort_texts as L   # noqa: E402


def test_model_on_a_small_text():
    """The model's windows against a direct restatement on a text small
    enough to walk: every window's buckets from the sorted bucket ids."""
    rng = np.random.default_rng(1)
    t = rng.integers(0, 4, 40_000, dtype=np.uint8) + 65
    t[-1] = 68
    m = L.WindowModel(t, init_chars=12)
    p = m.plan
    assert (p["s"], p["R"], p["rb"], p["bits1"]) == (8, 4, 9, 9) and not p["fast32"]   # span under kSubBits
    m = L.WindowModel(t, init_chars=15)
    assert m.plan["bits1"] == 15 and m.plan["fast32"]
    dig = (t - 65).astype(np.int64)
    pad = np.concatenate([dig, np.zeros(8, np.int64)])
    D = sum(pad[q:q + len(t)] * 4 ** (7 - q) for q in range(8))   # bucket = D (one value per bucket)
    bs = np.sort(D)
    n, listed, one = len(t), 0, 0

    def start(x):
        """The first bucket start g >= x and the lowest bucket id starting
        there: the empty buckets after item g - 1's bucket start at g too."""
        if x >= n:
            return n, 1 << 16
        if x == 0:
            return 0, 0
        g = x
        while g < n and bs[g] == bs[g - 1]:
            g += 1
        return g, int(bs[g - 1]) + 1

    for j in range((n + 1023) // 1024):
        (a, ba), (b, bb) = start(j * 1024), start((j + 1) * 1024)
        listed += b > a
        one += b > a and bb - ba == 1
    assert (m.listed, m.one_bucket_windows) == (listed, one)
    assert m.distinct + m.unsorted - m.groups == n


@pytest.mark.parametrize("name", L.TEXTS)
def test_text_coverage(name):
    m = L.model(name)
    s = m.summary()
    print(name, s)
    assert m.plan["cmp"] == 1 and m.plan["fast32"], s
    assert m.one_bucket_windows >= 100, s
    assert min(m.class_counts()) >= 5, s
    assert m.largest_window <= L.K_BS_CAP, s                      # no LSD fallback of the whole round
    assert m.retried > m.listed - m.one_bucket_windows, s         # clustered windows join the retry list
    assert m.largest_group > 8, s                                 # the U walk meets groups longer than a pair


@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_size_edges(name):
    sz = L.model(name).one_sizes
    row = L.K_WAVE_ROW
    assert ((sz > L.K_BS_CAP - row) & (sz <= L.K_BS_CAP)).any(), sz.max()   # within one wave-row of kBsCap
    assert (sz < 64).any(), sz.min()                                       # under one wavefront
    big = sz[sz >= row - 8]
    assert ((big % row >= 1) & (big % row <= 8)).any()                     # a few items past a wave's slots
    assert (big % row >= row - 8).any() and (big % row == 0).any()         # a few short of them, and exactly


def test_dense_and_sparse():
    """One DNA text leaves more than n / kSparseDiv suffixes unsorted (the
    local sort runs a second time, SegOut full), the other fewer."""
    assert L.model("dna_dense").dense and not L.model("dna_sparse").dense
    assert not L.model("byte256").dense and not L.model("alnum").dense


def test_anchor_rule():
    """Only anchored block starts begin with the anchor, so the planned bucket
    sizes are exact: the near-kBsCap bucket holds exactly what was asked."""
    for name in L.DNA_TEXTS:
        t = L.text(name)
        assert len(t) == L.DNA_N and t[-1] == ord("T")
        at = np.flatnonzero((t[:-3] == 67) & (t[1:-2] == 67) & (t[2:-1] == 67) & (t[3:] == 67))
        assert (at % 16 == 0).all()
        assert (L.model(name).one_sizes == L.K_BS_CAP - 200).sum() == 1
    for name in ("byte256", "alnum"):
        t = L.text(name)
        a = L.ALPHABETS[name][1]
        assert (np.flatnonzero(t == a) % 8 == 0).all()
        assert len(np.unique(t)) == len(L.ALPHABETS[name])


def test_span_edges_of_the_dna_texts():
    """init_chars steps the span: R = 6 / 7 / 14 give 2 / 4 / 18 = kLowMax key
    bits below the sub-bucket, R = 15 no fixed-span window at all."""
    for name in L.DNA_TEXTS:
        s = L.model(name).plan["s"]
        for R, low in ((6, 2), (7, 4), (14, L.K_LOW_MAX)):
            m = L.model(name, s + R)
            assert m.plan["bits1"] - L.K_SUB_BITS == low and m.one_bucket_windows >= 100, (name, R, m.summary())
        m = L.model(name, s + 15)
        assert not m.plan["fast32"] and m.one_bucket_windows == 0
