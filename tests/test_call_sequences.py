"""The call-order model of tests/call_sequences.py, on the CPU: the walk
tests/test_gpu_call_sequences.py runs on one context really covers every
ordered pair of operations, and the epoch arithmetic of the wrap legs."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_sequences as S   # noqa: E402


def test_operations_are_distinct_and_complete():
    ops = S.OPERATIONS
    assert len(set(ops)) == len(ops)
    assert set(S.BUILD_VARIANTS) <= set(ops) and len(S.BUILD_VARIANTS) == 9
    for name in ("check_valid", "check_swapped", "lcp_valid", "lcp_duplicate", "inverse_valid", "inverse_duplicate",
                 "locate", "mems", "lpf_lz77", "repeats", "lf_ibwt", "fm_build_locate", "argsort", "pack_keys",
                 "generate_text"):
        assert name in ops


def test_walk_covers_every_ordered_pair_once():
    ops = S.OPERATIONS
    k = len(ops)
    w = S.walk()
    assert len(w) == k * k + 1
    assert w[0] == w[-1]                                   # closed
    p = S.pairs(w)
    assert len(p) == k * k and len(set(p)) == k * k        # each edge once
    assert set(p) == {(a, b) for a in ops for b in ops}    # loops included
    for a in ops:
        assert (a, a) in p


def test_walk_is_deterministic():
    assert S.walk() == S.walk()
    assert S.eulerian_walk(7) == S.eulerian_walk(7)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 24, 31])
def test_eulerian_walk_any_size(k):
    w = S.eulerian_walk(k)
    assert len(w) == k * k + 1 and w[0] == w[-1] == 0
    assert set(S.pairs(w)) == {(a, b) for a in range(k) for b in range(k)}


def test_eulerian_walk_rejects_empty():
    with pytest.raises(ValueError):
        S.eulerian_walk(0)


def test_epoch_constants_match_the_library_source():
    """kEpochBits of csrc/sa_onesweep.h, read from the source."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "hpc_suffix_array_amd", "csrc", "sa_onesweep.h")) as f:
        m = re.search(r"constexpr uint32_t kEpochBits = (\d+);", f.read())
    assert m and int(m.group(1)) == S.EPOCH_BITS
    assert S.EPOCH_LAST == 16383


def test_epoch_arithmetic():
    assert S.argsort_passes(64) == 8 and S.argsort_passes(8) == 1 and S.argsort_passes(9) == 2
    assert S.argsort_passes(1) == 1 and S.argsort_passes(63) == 8
    # a fresh context (tag 0): the 16384th pass wraps
    assert S.epoch_after(0, 16383) == 16383 and S.epoch_after(0, 16384) == 1
    for j in (0, 3, 7):            # the wrap on pass j of an 8-pass argsort
        start = S.EPOCH_LAST - j
        plan = S.advance_plan(0, start)
        assert sum(S.argsort_passes(b) for b in plan) == start
        assert S.epoch_after(start, j) == S.EPOCH_LAST           # pass j - 1 takes the last tag
        assert S.epoch_after(start, j + 1) == 1                  # pass j clears the states
        assert S.epoch_after(start, 8) == 8 - j
    assert S.advance_plan(5, 5) == []
    with pytest.raises(ValueError):
        S.advance_plan(10, 9)
