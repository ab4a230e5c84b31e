"""The window-to-window hand-over of the fixed-span local sort (sa_bucket.h
k_bucket_sort) at sizes the oracle sorts in a second.

The kernel runs 2 x CUs persistent workgroups that take windows by ticket.
The texts of tests/local_sort_texts.py list a few hundred to a few thousand
windows, so in tests/test_gpu_local_sort.py no workgroup takes a second one
and what one window leaves for the next -- zeroed counters, the prefetched
items, the next header, a retried window followed by a sorted one -- is only
exercised by builds of 2^28 suffixes and more.  Debug flag ls_one_wg launches
that kernel with ONE workgroup: every listed window passes through it in
ticket order, each kind after each other kind.  The flag changes nothing
else, so every build here must

  * equal the oracle's suffix array (XQ case: the LSD build's, which
    tests/test_gpu_local_sort.py ties to the oracle),
  * take the bucketed round, and
  * report the windows, the groups of every round and the sparse / dense
    second launch of the same build without the flag;

and the text must hold, by the model, a window the kernel retries (a
sub-bucket above kMaxSub) and, by the build's statistics, at least 100
one-bucket windows, so a retried window is followed by sorted ones.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_sort_texts as L   # noqa: E402

pytestmark = pytest.mark.gpu

_wants = {}


def _want(oracle, name):
    """The oracle's SA of a text, computed once (shared with
    test_gpu_local_sort.py when both run in one session)."""
    try:
        import test_gpu_local_sort as G
        return G._want(oracle, name)
    except ImportError:
        if name not in _wants:
            _wants[name] = oracle.sa_c(L.text(name))
        return _wants[name]


def _leg(oracle, name, debug=(), tune=0):
    from hpc_suffix_array_amd import build_suffix_array
    tag = (name, debug, tune)
    m = L.model(name)
    assert m.clustered >= 1, (tag, m.clustered)     # a window the kernel hands to the retry
    base = ("fast32_small",) + tuple(debug)
    _, ref = build_suffix_array(L.text(name), return_stats=True, round1="bucketed", debug=base, tune=tune)
    got, st = build_suffix_array(L.text(name), return_stats=True, round1="bucketed", debug=base + ("ls_one_wg",),
                                 tune=tune)
    print(tag, "windows", st["round1_windows"], "clustered", m.clustered, flush=True)
    assert st["round1"] == "bucketed" and ref["round1"] == "bucketed", (tag, st["round1"], ref["round1"])
    assert st["round1_windows"][1] >= 100, (tag, st["round1_windows"])
    assert st["round1_windows"] == ref["round1_windows"], (tag, st["round1_windows"], ref["round1_windows"])
    assert st["distinct"] == ref["distinct"], (tag, st["distinct"], ref["distinct"])
    assert st["sparse_ranks"] == ref["sparse_ranks"], (tag, st["sparse_ranks"], ref["sparse_ranks"])
    assert (got == _want(oracle, name)).all(), tag


@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_one_workgroup(gpu, oracle, name):
    """Every window class, the size edges, tie groups and retried windows
    through one workgroup; the sparse and the dense second launch."""
    _leg(oracle, name)


@pytest.mark.parametrize("v", [1, 2, 3, 4])
@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_variants_one_workgroup(gpu, oracle, name, v):
    """The LSV variants (sa_opts.tune bits 16-19)."""
    _leg(oracle, name, tune=v << 16)


@pytest.mark.parametrize("name", L.DNA_TEXTS)
def test_dna_key1_samples_one_workgroup(gpu, oracle, name):
    """no_key1_round: the key samples written from the sorted words."""
    _leg(oracle, name, debug=("no_key1_round",))


@pytest.mark.parametrize("name", ["byte256", "alnum"])
def test_other_alphabets_one_workgroup(gpu, oracle, name):
    _leg(oracle, name)


def test_xq_one_workgroup(gpu):
    """k_bucket_sort<.., XQ = true>, both row forms (sa_opts.tune bit 29), by
    the recipe of test_gpu_local_sort.py test_xq_loads: the dense DNA text at
    2^23 suffixes in a context sized for 2^26.  The one-workgroup build's SA
    is compared on the device with the LSD build's."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder
    n, n0 = 1 << 23, 1 << 26
    t = L.xq_text(n)
    b = DeviceBuilder(n0)
    try:
        big = torch.empty(n0, dtype=torch.uint8, device="cuda")
        sa0 = torch.empty(n0, dtype=torch.int32, device="cuda")
        b.generate_text(big, n0, b"ACGT", seed=1)
        b.build(big, n0, sa0)
        del big
        d = torch.from_numpy(t).cuda()
        want = sa0[:n]
        b.build(d, n, want, round1="lsd", init_chars=L.min_chars(4, n))
        sa = torch.empty(n, dtype=torch.int32, device="cuda")
        for tune in (0, 1 << 29):
            ref = b.build(d, n, sa, round1="bucketed", debug=("fast32_small",), tune=tune)
            sa.fill_(-1)
            st = b.build(d, n, sa, round1="bucketed", debug=("fast32_small", "ls_one_wg"), tune=tune)
            print("xq", tune >> 29, st["round1_layout"], st["round1_windows"], flush=True)
            assert st["round1"] == "bucketed" and st["round1_layout"]["xq"], (tune, st["round1"], st["round1_layout"])
            assert st["round1_windows"][1] >= 100, st["round1_windows"]
            # (which one-bucket windows k_window_split admits depends on how
            # the second pass's queues shared each bucket out, which differs
            # from build to build: a few windows move between the fixed-span
            # kernel and the retry list, so only the listed count is fixed;
            # the recipe's 65- and 90-key sub-buckets make clustered windows)
            assert st["round1_windows"][0] == ref["round1_windows"][0], (tune, st["round1_windows"], ref["round1_windows"])
            assert st["distinct"] == ref["distinct"], (tune, st["distinct"], ref["distinct"])
            assert st["sparse_ranks"] == ref["sparse_ranks"], tune
            assert bool((sa == want).all().item()), tune
    finally:
        b.close()
