"""The coverage of tests/test_gpu_second_pass.py is a condition, checked here
on the CPU: the model of the second bucket pass's work units
(tests/local_sort_texts.py second_pass_units, a restatement of sa_split.h
k_split_seg's unit numbering and k_xq_dh's sub-regions) must show that the
texts the GPU tests build reach the pass's edges at 16, 17 and 18 bucket bits
-- empty segments and digits, segments of two units, last units under one
wavefront, queues that own no unit of a segment -- and that every text run
with per-XCD queues fits the queues' sub-regions.  Sizes and seeds of the
texts are chosen against these assertions, never against what the GPU
returns."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_sort_texts as L   # noqa: E402

BBS = L.SP_BBS


def test_units_on_a_small_example():
    """second_pass_units against a direct walk: units numbered segment by
    segment, dealt to the queues round robin, every item counted once."""
    rng = np.random.default_rng(5)
    bb, unit = 17, 100
    bucket = rng.integers(0, 1 << bb, 30_000)
    bucket = bucket[(bucket & 255) % 7 != 3]                      # empty segments
    bucket = bucket[((bucket >> 8) % 5 != 1) | (bucket & 1 == 0)]
    bucket[(bucket & 255) == 9] |= 0x1FF00                        # segment 9: one digit only
    u = L.SecondPassUnits(bucket, bb, unit)
    seg, size, owns, share = [], [], np.zeros((8, 256), bool), np.zeros((8, 512), np.int64)
    for l in range(256):
        items = np.sort(bucket[(bucket & 255) == l] >> 8)         # any order inside a unit
        for at in range(0, len(items), unit):
            q = len(seg) % 8
            seg.append(l)
            size.append(min(unit, len(items) - at))
            owns[q, l] = True
            share[q] += np.bincount(items[at:at + unit], minlength=512)
    assert (u.unit_seg == seg).all() and (u.unit_size == size).all()
    assert (u.unit_queue == np.arange(len(seg)) % 8).all()
    assert (u.owns == owns).all() and (u.seg_sizes == 0).sum() >= 30
    assert u.count.sum() == len(bucket) == u.unit_size.sum()
    assert (u.digit_tot == np.bincount(bucket >> 8, minlength=512)).all()
    # the bound holds for every split of a segment's items among its units
    assert (share <= u.ub).all() and share.sum() == len(bucket)
    assert (u.cap == u.digit_tot // 8 + u.digit_tot // 128 + 2048).all()
    # ... and is exact where every segment is one unit
    u1 = L.SecondPassUnits(bucket, bb, 1 << 20)
    assert (u1.seg_units <= 1).all() and u1.ub.sum() == len(bucket)


def test_plan_takes_the_forced_width():
    """bb17 / bb18 raise the bucket bits and never lower them; without them
    the size decides (sa_round1.h plan_bucketed)."""
    for n, auto in ((1 << 20, 16), (3 << 20, 16), ((1 << 29) + 1, 17), ((1 << 30) + 1, 18), (1 << 33, 18)):
        K = L.min_chars(4, n)
        assert L.plan_bucketed(4, n, K)["bb"] == auto, n
        for bb in (None, 16, 17, 18):
            assert L.plan_bucketed(4, n, K, 1, bb)["bb"] == max(auto, bb or 0), (n, bb)


@pytest.mark.parametrize("bb", BBS)
@pytest.mark.parametrize("name", L.SP_TEXTS + ("dna_rounds",))
def test_a_plan_exists(name, bb):
    """Every kind at its size: the compact layout (the texts end in their
    largest symbol), the original one under no_cmp, packed items where the
    GPU test asserts them; the E-only layout for the texts that force it."""
    t = L.sp_text(name)
    assert t[-1] == t.max()
    p = L.sp_plan(name, bb)
    print(name, bb, p)
    assert p is not None and p["bb"] == bb and p["cmp"] == 1, p
    assert p["pk8"], p
    p0 = L.sp_plan(name, bb, no_cmp=True)
    assert p0 is not None and p0["bb"] == bb and p0["cmp"] == 0, p0
    if name in ("alnum", "ascii127", "dna_uniform", "dna_no_tt"):
        pe = L.sp_plan(name, bb, eonly=True)
        assert pe is not None and pe["bb"] == bb and pe["cmp"] == 2, pe


@pytest.mark.parametrize("bb", BBS)
def test_dna_uniform_units(bb):
    """Segments of about one unit of packed items: many of two units, many
    whose last unit is under one wavefront; with 12-byte items every segment
    is two units."""
    u = L.sp_units("dna_uniform", bb, L.UNIT_PK)
    print(u.summary())
    assert (u.seg_units == 2).sum() >= 100, u.summary()
    assert ((u.last_unit >= 1) & (u.last_unit <= 63)).sum() >= 20, u.summary()
    assert (u.seg_units == 1).sum() >= 100, u.summary()
    assert (L.sp_units("dna_uniform", bb, L.UNIT_B).seg_units == 2).all()


@pytest.mark.parametrize("bb", BBS)
def test_dna_no_tt_gaps(bb):
    """Empty segments (the published bases hop over them), empty digits, and
    a non-empty segment 0: suffixes shorter than s pad onto it."""
    for name in ("dna_no_tt", "dna_no_tt_small"):
        t = L.sp_text(name)
        assert not ((t[1:] == ord("T")) & (t[:-1] == ord("T"))).any() and t[-1] == ord("T")
        u = L.sp_units(name, bb, L.UNIT_PK)
        print(name, u.summary())
        empty = u.seg_sizes == 0
        assert empty.sum() >= 20 and (u.digit_tot == 0).sum() >= 40, u.summary()
        assert u.seg_sizes[0] > 0
        # runs of empty segments between non-empty ones, and after the last one
        gaps = np.flatnonzero(empty[1:] & ~empty[:-1])
        assert len(gaps) >= 8 and empty[-1], u.summary()          # (8 runs at 17 bits, 15 at 16 and 18)
        assert (empty[1:] & empty[:-1]).any()                     # a hop over more than one
    u = L.sp_units("dna_no_tt", bb, L.UNIT_PK)
    assert (u.seg_units == 1).sum() >= 40 and (u.seg_units == 2).sum() >= 40, u.summary()


@pytest.mark.parametrize("unit", [L.UNIT_PK, L.UNIT_B])
@pytest.mark.parametrize("bb", BBS)
def test_dna_no_tt_small_units(bb, unit):
    """Every segment a fraction of a unit, and every queue skips non-empty
    segments it owns no unit of."""
    u = L.sp_units("dna_no_tt_small", bb, unit)
    assert u.seg_sizes.max() < unit // 8 and (u.seg_units <= 1).all(), u.summary()
    nonempty = u.seg_sizes > 0
    for q in range(L.K_XQ):
        assert (nonempty & ~u.owns[q]).sum() >= 100, q
        # ... also between two segments it owns (its chain hops over them)
        mine = np.flatnonzero(u.owns[q])
        assert any(nonempty[a + 1:b].any() for a, b in zip(mine[:-1], mine[1:])), q


def _xq_cases():
    for name in L.SP_XQ_DNA:
        for bb in BBS:
            yield name, bb
    for name in L.SP_XQ_OTHER:
        for bb in (17, 18):
            yield name, bb


@pytest.mark.parametrize("name,bb", list(_xq_cases()))
def test_queue_shares_fit(name, bb):
    """Every text run with per-XCD queues: each queue's share of each digit,
    bounded by ub(q, h), fits k_xq_dh's sub-region, so the pass must not
    overflow; and the plan allows the fixed-span local sort the queues need."""
    p = L.sp_plan(name, bb, init_chars=L.SP_XQ_CHARS.get(name, 0))
    assert p is not None and p["bb"] == bb and p["fast32"], p
    u = L.sp_units(name, bb, L.UNIT_PK if p["pk8"] else L.UNIT_B)
    print(name, u.summary())
    assert (u.ub <= u.cap).all(), u.summary()
    # sub-regions of exactly tot(h) / 8 (debug xq_overflow) must overflow: the
    # eight queues' items of a digit total tot(h), so one holds tot(h) / 8 or
    # more, and more wherever 8 does not divide the digit or the shares differ
    assert (u.digit_tot % 8 != 0).any()
