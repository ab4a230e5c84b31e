"""The second bucket pass (sa_split.h k_split_seg, k_bucket_starts,
k_bucket_starts_xq, k_xq_dh) at 8-, 9- and 10-bit digits, against the oracle,
at sizes the oracle sorts in a second or two.

The size alone gives 16 bucket bits (an 8-bit second digit) below 2^29
suffixes; debug flags bb17 / bb18 (SA_DEBUG_BB17 / _BB18) widen the buckets so
that the 9- and 10-bit instantiations -- production's from 2^29 and 2^30
suffixes, the benchmark's among them -- and the 2^17 + 1 and 2^18 + 1 entry
bucket tables the window kernels and the later rounds read run here.  The
texts (tests/local_sort_texts.py sp_text) reach the pass's own edges: empty
segments and digits with the chain of published bases hopping over them,
segments of one unit, of one unit and a few items and of two units, last
units under one wavefront, queues that own no unit of a segment.
tests/test_second_pass_texts.py asserts that coverage, and that the per-XCD
regions fit, on the CPU.  Here every build must

  * take the bucketed round with the digit width asked for (round1_hb),
  * take the layout the host's plan predicts, and
  * equal the oracle's suffix array.

Not covered: padded first-pass segments (k_bucket_sample, striped cursors,
dense_lo / seg_cnt in the second pass) need 2^26 suffixes and stay with
test_gpu_parity.py test_round1_padded_segments and the slow tests, at the
digit width their size gives.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_sort_texts as L   # noqa: E402

pytestmark = pytest.mark.gpu

BB_FLAG = {16: (), 17: ("bb17",), 18: ("bb18",)}
_wants = {}


def _want(oracle, name):
    """The oracle's SA of a text, computed once."""
    if name not in _wants:
        _wants[name] = oracle.sa_c(L.sp_text(name))
    return _wants[name]


def _build(oracle, name, bb, debug=(), **kw):
    from hpc_suffix_array_amd import build_suffix_array
    got, st = build_suffix_array(L.sp_text(name), return_stats=True, round1="bucketed",
                                 debug=BB_FLAG[bb] + tuple(debug), **kw)
    tag = (name, bb, debug)
    print(tag, "hb", st["round1_hb"], st["round1_layout"], "K", st["init_chars"], flush=True)
    assert st["round1"] == "bucketed", (tag, st["round1"], st["largest_window"])
    assert st["round1_hb"] == bb - 8, (tag, st["round1_hb"])
    assert (got == _want(oracle, name)).all(), tag
    return st


def test_flags_never_lower_the_width(gpu, oracle):
    """bb18 wins over bb17; neither flag set: the size's 16 bits."""
    from hpc_suffix_array_amd import build_suffix_array
    t = L.sp_text("dna_no_tt_small")
    for dbg, hb in (((), 8), (("bb17",), 9), (("bb18",), 10), (("bb17", "bb18"), 10)):
        got, st = build_suffix_array(t, return_stats=True, round1="bucketed", debug=dbg)
        assert st["round1"] == "bucketed" and st["round1_hb"] == hb, (dbg, st["round1_hb"])
        assert (got == _want(oracle, "dna_no_tt_small")).all(), dbg


@pytest.mark.parametrize("src", ["pk8", "no_pk8"])
@pytest.mark.parametrize("bb", L.SP_BBS)
@pytest.mark.parametrize("name", L.SP_TEXTS)
def test_digit_width_and_source(gpu, oracle, name, bb, src):
    """k_split_seg<SrcPk8 | SrcBucketKeys, 8 | 9 | 10> with k_bucket_starts<256 |
    512 | 1024>: packed 8-byte items (units of 12288) and 12-byte items
    (units of 10240) on every text."""
    st = _build(oracle, name, bb, () if src == "pk8" else ("no_pk8",))
    p = L.sp_plan(name, bb)
    lay = st["round1_layout"]
    assert st["init_chars"] == p["K"], (name, bb, st["init_chars"], p["K"])
    assert (lay["compact"], lay["eonly"]) == (p["cmp"] != 0, p["cmp"] == 2), (name, bb, lay)
    if src == "no_pk8":
        assert not lay["pk8"], (name, bb, lay)
    elif p["pk8"]:   # (tests/test_second_pass_texts.py: every text, every width)
        assert lay["pk8"], (name, bb, lay)


@pytest.mark.parametrize("bb", [17, 18])
@pytest.mark.parametrize("name", L.SP_TEXTS)
def test_original_layout_at_wide_buckets(gpu, oracle, name, bb):
    """no_cmp: the original key1 low under 9- and 10-bit digits."""
    st = _build(oracle, name, bb, ("no_cmp",))
    p = L.sp_plan(name, bb, no_cmp=True)
    lay = st["round1_layout"]
    assert not lay["compact"] and not lay["eonly"] and p["cmp"] == 0, (name, bb, lay)
    assert st["init_chars"] == p["K"], (name, bb, st["init_chars"], p["K"])


@pytest.mark.parametrize("bb", [17, 18])
@pytest.mark.parametrize("name", ["alnum", "ascii127", "dna_uniform", "dna_no_tt"])
def test_eonly_layout_at_wide_buckets(gpu, oracle, name, bb):
    """eonly: the key1 low without its end bit (round 2 orders the short
    suffixes) under 9- and 10-bit digits."""
    st = _build(oracle, name, bb, ("eonly",))
    p = L.sp_plan(name, bb, eonly=True)
    lay = st["round1_layout"]
    assert p["cmp"] == 2 and lay["eonly"] and lay["compact"], (name, bb, lay)
    assert st["init_chars"] == p["K"], (name, bb, st["init_chars"], p["K"])


@pytest.fixture(scope="module")
def xq_builder(gpu):
    """One context whose keys_u has the per-XCD regions' slack: a context gets
    it with unsorted-set buffers for 2^26 suffixes, so one generated text of
    that size is built first (the recipe of test_gpu_local_sort.py
    test_xq_loads; unchecked: test_gpu_parity.py covers that size)."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder
    n0 = 1 << 26
    b = DeviceBuilder(n0)
    try:
        big = torch.empty(n0, dtype=torch.uint8, device="cuda")
        sa = torch.empty(n0, dtype=torch.int32, device="cuda")
        b.generate_text(big, n0, b"ACGT", seed=1)
        st = b.build(big, n0, sa)
        assert st["round1"] == "bucketed" and st["round1_hb"] == 8, st["round1_hb"]
        del big
        yield b, sa
    finally:
        b.close()


def _xq_leg(xq_builder, oracle, name, bb, debug):
    import torch
    b, sa_buf = xq_builder
    t = L.sp_text(name)
    n = len(t)
    want = torch.from_numpy(_want(oracle, name).view(np.int32)).cuda()
    d = torch.from_numpy(t).cuda()
    sa = sa_buf[:n]
    sa.fill_(-1)
    st = b.build(d, n, sa, round1="bucketed", init_chars=L.SP_XQ_CHARS.get(name, 0),
                 debug=BB_FLAG[bb] + ("fast32_small",) + tuple(debug))
    tag = (name, bb, debug)
    print(tag, "hb", st["round1_hb"], st["round1_layout"], st["round1_windows"], flush=True)
    assert st["round1"] == "bucketed", (tag, st["round1"], st["largest_window"])
    assert st["round1_hb"] == bb - 8, (tag, st["round1_hb"])
    assert bool((sa == want).all().item()), tag
    return st


@pytest.mark.parametrize("mode", ["xq", "xq_overflow", "no_xq"])
@pytest.mark.parametrize("bb", L.SP_BBS)
@pytest.mark.parametrize("name", L.SP_XQ_DNA)
def test_per_xcd_queues(xq_builder, oracle, name, bb, mode):
    """k_split_seg<.., XQ>, k_xq_dh and k_bucket_starts_xq over 256, 512 and
    1024 digits: the queues keep their regions (the CPU test proved every
    share fits); sub-regions without slack overflow and the round runs again
    with one region; no_xq takes one region at once."""
    dbg = {"xq": (), "xq_overflow": ("xq_overflow",), "no_xq": ("no_xq",)}[mode]
    st = _xq_leg(xq_builder, oracle, name, bb, dbg)
    assert st["round1_layout"]["xq"] == (mode == "xq"), (name, bb, mode, st["round1_layout"])
    assert st["round1_layout"]["pk8"], st["round1_layout"]


@pytest.mark.parametrize("bb", [17, 18])
@pytest.mark.parametrize("name", L.SP_XQ_OTHER)
def test_per_xcd_queues_other_alphabets(xq_builder, oracle, name, bb):
    """Non-power-of-two buckets (alnum) and sigma = 256 through the queues at
    9- and 10-bit digits."""
    st = _xq_leg(xq_builder, oracle, name, bb, ())
    if L.sp_plan(name, bb)["fast32"]:
        assert st["round1_layout"]["xq"], (name, bb, st["round1_layout"])


@pytest.mark.parametrize("bb", [17, 18])
def test_later_rounds_inside_wide_buckets(gpu, oracle, bb):
    """Planted repeats keep members after round 2: the later rounds' rank
    search, bounded by the 2^bb + 1 entry bucket table (no_key1_round: from
    round 2 on), against key1 rebuilt from the text."""
    st = _build(oracle, "dna_rounds", bb)
    alt = _build(oracle, "dna_rounds", bb, ("no_key1_round",))
    for s in (st, alt):
        assert s["sparse_ranks"] and s["rounds"] > 2, (bb, s["sparse_ranks"], s["rounds"])
    assert st["distinct"] == alt["distinct"], (bb, st["distinct"], alt["distinct"])
