"""Round 2 finished from the local sort's staging (k_round2_windows).

After a sparse bucketed round 1 on one GPU, one kernel orders every round-1
group by key1(x + K) straight from the staging the local sort left, and its
verdict rides the read-back the build makes anyway.  It gives up -- and the
build takes the general path: compacted set, keys, per-group sort, segments
-- on a window of more than 64 members, a group of more than 8, or two
members still tied after 2K symbols.

Every case compares the SA with the oracle, and SA and D_j with the same
build under debug "no_round2_fused".  Which path ran shows in the statistics:
the fused round launches no seg_count kernel and its device build makes 3
host waits.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

N1 = 1_000_003
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def builder(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder(1 << 22)   # one context: later builds see the earlier ones' staging
    yield b
    b.close()


_refs = {}


def _ref(oracle, name, t):
    if name not in _refs:
        r = oracle.sa_c(t)
        r.setflags(write=False)
        _refs[name] = r
    return _refs[name]


def _build(gpu, builder, t, debug=()):
    import torch
    n = int(t.size)
    d_text = torch.from_numpy(t).cuda()
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    before = gpu.lib().sa_host_syncs()
    st = builder.build(d_text, n, d_sa, profile=True, round1="bucketed", debug=debug)
    syncs = gpu.lib().sa_host_syncs() - before
    torch.cuda.synchronize()
    return d_sa.cpu().numpy().view(np.uint32), st, syncs


def _leg(gpu, builder, oracle, name, t, fused, debug=()):
    ref = _ref(oracle, name, t)
    got, st, syncs = _build(gpu, builder, t, debug)
    alt, st_alt, syncs_alt = _build(gpu, builder, t, tuple(debug) + ("no_round2_fused",))
    launches = st["kernels"]["seg_count"]["launches"]
    print(name, debug, "rounds", st["rounds"], "seg_count launches", launches, "host waits", syncs, "/", syncs_alt,
          "unsorted", st["sorted_n"][1:2])
    assert st["round1"] == "bucketed" and st["sparse_ranks"], st
    assert (got == ref).all() and (alt == ref).all()
    assert st["distinct"] == st_alt["distinct"]
    assert st_alt["kernels"]["seg_count"]["launches"] > 0 and syncs_alt > 3
    if fused:
        assert launches == 0 and syncs == 3, (launches, syncs)
        assert st["rounds"] == 2 and st["distinct"][1] == t.size
        for k in ("rounds", "distinct", "sorted_n", "passes", "prefix_len"):
            assert st[k] == st_alt[k], (k, st[k], st_alt[k])
        assert st["passes"] == [2, 1] and st["prefix_len"] == [st["init_chars"], 2 * st["init_chars"]]
    elif fused is not None:
        assert launches > 0
    return st


def _K(gpu, builder, t):
    return _build(gpu, builder, t)[1]["init_chars"]


@pytest.mark.parametrize("kind", ["dna", "alnum", "byte256"])
def test_random_text(gpu, builder, oracle, kind):
    t = oracle.gen_text(kind, N1, seed=41)
    _leg(gpu, builder, oracle, "random-" + kind, t, True)


@pytest.mark.parametrize("debug", [("fast32_small",), ("fast32_small", "no_xq")])
def test_fast32_small(gpu, builder, oracle, debug):
    """Random DNA at 2^22 under fast32_small (its windows hold several buckets
    each, so the measured-span kernel still sorts them)."""
    t = oracle.gen_text("dna", 1 << 22, seed=43)
    _leg(gpu, builder, oracle, "dna-4m", t, True, debug)


def test_fixed_span_local_sort_fills_the_staging(gpu, builder, oracle):
    """One-bucket windows, which k_bucket_sort itself sorts (the text of
    test_gpu_local_sort.py: tie groups of every size, so either path may run)."""
    import local_sort_texts as L
    t = L.text("dna_sparse").copy()
    st = _leg(gpu, builder, oracle, "dna_sparse", t, None, ("fast32_small",))
    assert st["round1_windows"][1] > 0, st["round1_windows"]


@pytest.mark.parametrize("extra", [0, 3])
def test_keys_past_the_end(gpu, builder, oracle, extra):
    """x + K == n: key 0; x + K a 3-symbol suffix: a key1 of a short suffix."""
    t = oracle.gen_text("dna", N1, seed=47)
    K = _K(gpu, builder, t)
    t[-(K + extra):] = t[100:100 + K + extra]
    _leg(gpu, builder, oracle, "tail-%d" % extra, t, True)


def test_tie_beyond_2k(gpu, builder, oracle):
    t = oracle.gen_text("dna", N1, seed=53)
    K = _K(gpu, builder, t)
    t[-(2 * K + 5):] = t[500:500 + 2 * K + 5]
    st = _leg(gpu, builder, oracle, "tie-2k", t, False)
    assert st["rounds"] > 2, st


def _starts_with(t, p):
    """positions whose suffix begins with the byte string p"""
    m = np.ones(t.size - len(p) + 1, dtype=bool)
    for i, c in enumerate(p):
        m &= t[i:i + m.size] == c
    return np.flatnonzero(m)


def test_group_of_nine(gpu, builder, oracle):
    t = oracle.gen_text("dna", N1, seed=59)
    K = _K(gpu, builder, t)
    assert K >= 4
    rng = np.random.default_rng(61)
    s = DNA[rng.integers(0, 4, K + 2)]
    places = [50_000 + 1000 * i for i in range(9)]
    for i, p in enumerate(places):
        t[p:p + K + 2] = s
        t[p + K + 2] = DNA[i // 4]   # a different pair of symbols after each copy
        t[p + K + 3] = DNA[i % 4]
    members = _starts_with(t, s[:K])
    assert list(members) == places
    assert len({bytes(t[p:p + 2 * K]) for p in members}) == 9
    _leg(gpu, builder, oracle, "group-9", t, False)


def test_window_of_eighty(gpu, builder, oracle):
    t = oracle.gen_text("dna", N1, seed=67)
    K = _K(gpu, builder, t)
    assert K - 12 >= 3   # three base-4 digits tell 40 pairs apart inside the K-symbol key
    rng = np.random.default_rng(71)
    head = DNA[rng.integers(0, 4, 12)]
    for i in range(40):
        s = np.concatenate([head, DNA[[i // 16, (i // 4) % 4, i % 4]], DNA[rng.integers(0, 4, K + 2 - 15)]])
        a, b = 10_000 + 2000 * i, 11_000 + 2000 * i
        t[a:a + K + 2] = s
        t[b:b + K + 2] = s
        t[a + K + 2] = DNA[0]
        t[b + K + 2] = DNA[1]
    members = _starts_with(t, head)
    assert members.size == 80
    groups = {}
    for p in members:
        groups.setdefault(bytes(t[p:p + K]), []).append(p)
    assert len(groups) == 40 and all(len(g) == 2 for g in groups.values())
    assert all(bytes(t[a:a + 2 * K]) != bytes(t[b:b + 2 * K]) for a, b in groups.values())
    _leg(gpu, builder, oracle, "window-80", t, False)


def test_planted_repeats(gpu, builder, oracle):
    """The second text of test_key1_round_two: 300 repeats of 40-160 symbols."""
    rng = np.random.default_rng(29)
    u = oracle.gen_text("dna", N1, seed=31)
    src = rng.integers(0, N1 - 200, 300)
    dst = rng.integers(0, N1 - 200, 300)
    for a, b, ln in zip(src, dst, rng.integers(40, 160, 300)):
        u[b:b + ln] = u[a:a + ln].copy()
    st = _leg(gpu, builder, oracle, "repeats", u, False)
    assert st["rounds"] > 2, st


def test_not_launched_without_the_key1_round(gpu, builder, oracle):
    t = oracle.gen_text("dna", N1, seed=41)
    st = _leg(gpu, builder, oracle, "random-dna", t, False, ("no_key1_round",))
    alt = _build(gpu, builder, t, ("no_key1_round", "no_round2_fused"))[1]
    assert st["kernels"]["sort_u"]["launches"] == alt["kernels"]["sort_u"]["launches"]
    assert st["kernels"]["seg_write"]["launches"] == alt["kernels"]["seg_write"]["launches"]
