"""The numbers tests/test_gpu_perm_stripes.py relies on, asserted on the CPU
(tests/perm_stripes_model.py restates plan_check / plan_stripes / pad_elems
of sa_build.hip and the striped level 1 of sa_check.h's k_chk_bin).

Striping depends on the capacity the context was created for, not only on the
call's n: the regions (8 nb1 scap pairs) must fit the context's keys[0].  A
context below 2^26 symbols has no slack there and never stripes a call of its
own size; n = 2^24 stripes from a capacity of 20,971,520, and the GPU tests run
it on a context of 2^26 (keys[0] of 79,691,776).  The periodic text's suffix array sends
each bin's 65,536 pairs to one stripe region of 10,240 slots (every bin
overflows), and the identity with two runs of k entries exchanged fills two
regions to 8192 + k: k = 2048 is exactly the capacity, 2049 one pair more.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perm_stripes_model as M   # noqa: E402

N24 = 1 << 24
CAP26 = 1 << 26


def test_pad_elems_and_context_capacity():
    assert M.pad_elems(CAP26) == 79_691_776
    assert M.pad_elems(N24) == N24
    assert M.pad_elems((1 << 26) - 1) == 1 << 26
    assert M.pad_elems(25_700_000) == M.align_up(25_700_000, 64)


def test_smallest_striped_plan():
    p = M.plan_check(N24)
    assert p == M.Plan(16, 14, 256, 4)
    bs = M.plan_stripes(CAP26, N24, p)
    assert bs == M.Stripes(8, 10_240)
    assert 8 * 256 * 10_240 == 20_971_520 <= M.pad_elems(CAP26)
    # pass B: the same bins, sub-bins of 2^13
    assert M.plan_check(N24, M.SUB_B) == M.Plan(16, 13, 256, 8)
    assert M.plan_stripes(CAP26, N24, M.plan_check(N24, M.SUB_B)) == bs
    # one symbol fewer: below the threshold
    assert not M.is_striped(CAP26, N24 - 1)


def test_plan_one_past_a_power_of_two():
    n = N24 + 5
    p = M.plan_check(n)
    assert p == M.Plan(17, 14, 129, 8)
    assert M.plan_stripes(CAP26, n, p) == M.Stripes(8, 18_432)
    assert n - (128 << 17) == 5          # the last bin holds 5 entries


@pytest.mark.parametrize("cap", [N24, N24 + 5, 20_971_520, 25_700_000, 1 << 25, (1 << 25) + 1, (1 << 26) - 1])
def test_context_sized_for_its_call_below_2_26_never_stripes(cap):
    """keys[0] of a context below 2^26 has no slack: the regions of a call as
    large as the context (8 scap > 2^s1 per bin) never fit."""
    for s2 in (M.SUB_A, M.SUB_B):
        assert not M.is_striped(cap, cap, s2)
        assert not M.is_striped(cap, cap - 1, s2)


def test_smaller_call_on_a_larger_context_stripes():
    """The plan asks for 8 nb1 scap elements of the context's keys[0], whatever
    the context was sized for: n = 2^24 stripes from a capacity of 20,971,520."""
    need = 8 * 256 * 10_240
    assert need == 20_971_520
    assert not M.is_striped(need - 64, N24) and M.is_striped(need, N24)
    assert M.is_striped(25_700_000, N24) and M.is_striped(25_700_000, N24 + 5)   # 129 x 8 x 18,432 = 19,021,824
    assert not M.is_striped(N24, N24) and not M.is_striped(N24 + 5, N24 + 5)


def test_ab_shapes_stripe_too():
    """tune bits 20-23 = 1 / 2: 10 / 9 level-1 bin bits, tiles of 7168."""
    for b1, nb1 in ((10, 1024), (9, 512)):
        for s2 in (M.SUB_A, M.SUB_B):
            p = M.plan_check(N24, s2, b1)
            assert p.nb1 == nb1 and M.level1_tile(p) == M.TILE_WIDE
            assert M.plan_stripes(CAP26, N24, p).st == 8
            assert not M.is_striped(N24, N24, s2, b1)


def test_periodic_sa_overflows_pass_a_not_pass_b():
    reps = 1 << 16
    sa = M.periodic_sa(reps)
    p = M.plan_check(N24)
    bs = M.plan_stripes(CAP26, N24, p)
    fa = M.region_fill(sa, p)                      # pass A, PHI, ISA + 1, the inverse: dest SA[r]
    assert (fa.max(axis=1) == 1 << 16).all()       # each bin whole in one region
    assert ((fa > bs.scap).sum(axis=1) == 1).all() and fa.sum() == N24
    isa = np.empty(N24, np.int64)
    isa[sa] = np.arange(N24)
    fb = M.region_fill(isa, p)                     # pass B, PLCP: dest ISA[i]
    assert fb.max() == 8192 and fb.min() == 8192


@pytest.mark.parametrize("k, full", [(2048, 10_240), (2049, 10_241)])
def test_swapped_identity_at_the_capacity(k, full):
    p = M.plan_check(N24)
    bs = M.plan_stripes(CAP26, N24, p)
    f = M.region_fill(M.swapped_identity(N24, k), p)
    assert f[0, 0] == full and f[1, 1] == full
    assert f[0, 1] == 8192 - k and f[1, 0] == 8192 - k
    g = f.copy()
    g[0, :2] = g[1, :2] = 8192
    assert (g == 8192).all()
    assert (f > bs.scap).any() == (k > 2048)


def test_random_permutation_stays_under_the_capacity():
    p = M.plan_check(N24)
    bs = M.plan_stripes(CAP26, N24, p)
    f = M.region_fill(np.random.default_rng(24).permutation(N24), p)
    assert 8192 < f.max() < 9000 < bs.scap


def test_periodic_formulas_against_the_oracle(oracle):
    reps = 64
    t = M.periodic_text(reps)
    assert bytes(t) == bytes(range(256)) * reps
    sa = oracle.sa_c(t)
    assert (M.periodic_sa(reps) == sa).all()
    assert (M.periodic_lcp(reps) == oracle.lcp_c(t, sa)).all()
    assert oracle.check_c(t, M.periodic_sa(reps))
