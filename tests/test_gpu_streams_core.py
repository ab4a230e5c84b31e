"""The core entry points on a non-blocking side stream.

torch's side streams do not synchronise with the legacy null stream, so a
step the library enqueues on another stream than the one it was given, or a
blocking copy that reads what the caller's stream has not produced yet, shows
only when the caller's stream is really behind.  Every leg here is shaped by
``leg``:

  * every input and output tensor is poisoned (all ones) and the device waits;
  * in the shape "null_busy" a delay of twice the length is enqueued on the
    null stream: a memset or kernel that lands there by mistake runs after
    the call's own kernels, not before them.  In the shape "null_idle" the
    null stream is left empty: a blocking ``hipMemcpy`` issued before the
    wait for the caller's stream runs at once and reads poison (behind a busy
    null stream it would be ordered late and read good data).  Every test
    runs in both shapes, so each class of mistake meets poison in one;
  * under ``torch.cuda.stream(side)`` a delay is enqueued, then the producer of
    the call's inputs (``generate_text`` or a copy from pinned memory), then,
    with no synchronisation in between, the library call with
    ``stream=side.cuda_stream``;
  * ``side.query()`` is asserted False right before the library call: the
    stream is still busy with the delay when the library starts enqueuing;
  * the side stream is synchronised and the results are compared.

The delay is ``torch.cuda._sleep(CYCLES)``; the ``delay`` fixture measures it
once per module with a pair of events and asserts at least 50 ms (and at most
250 ms: every leg pays it).  Calibration on the MI355X: the kernel spins on
the shader clock, about 2.4 cycles per ns; 100 000 000 cycles measured 41.7 ms,
200 000 000 measured 84.3 ms, and CYCLES = 140 000 000 measured 59.1 ms.

Texts come from the oracle's generator (``generate_text`` on the device is
the same splitmix64 sequence), so every expected value is the CPU's:
oracle.sa_c, oracle.lcp_c, numpy for ISA and BWT, torch's stable sort and
tests/dist_cpu_ops.py for the building blocks of the distributed driver.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from context_helpers import numpy_inverse, periodic, sort_reference   # noqa: E402

pytestmark = pytest.mark.gpu

# torch.cuda._sleep spins for this many cycles of the shader clock (59.1 ms on
# the MI355X; the module docstring has the calibration)
CYCLES = 140_000_000
MIN_DELAY_MS = 50.0
MAX_DELAY_MS = 250.0


@pytest.fixture(scope="module")
def side(gpu):
    import torch
    return torch.cuda.Stream()


@pytest.fixture(scope="module")
def delay(gpu, side):
    """The delay of one leg in ms, measured once with a pair of events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e0.record()
        torch.cuda._sleep(CYCLES)
        e1.record()
    side.synchronize()
    ms = e0.elapsed_time(e1)
    print(f"torch.cuda._sleep({CYCLES}): {ms:.1f} ms")
    assert ms >= MIN_DELAY_MS, f"the delay is {ms:.1f} ms: raise CYCLES"
    assert ms <= MAX_DELAY_MS, f"the delay is {ms:.1f} ms: lower CYCLES (every leg pays it)"
    return ms


@pytest.fixture(scope="module")
def builder(gpu):
    """One context for the module, sized below most legs (the capacities grow
    under the side stream too)."""
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder(1 << 16)
    yield b
    b.close()


def poison(*tensors):
    import torch
    for t in tensors:
        if t.dtype == torch.bool:
            t.fill_(True)
        else:
            t.fill_(255 if t.dtype == torch.uint8 else -1)


def pinned(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).pin_memory()


_shape = {"null_busy": True}


@pytest.fixture(autouse=True, params=["null_idle", "null_busy"])
def null_stream(request):
    """Every test runs in both shapes of the null stream (module docstring)."""
    _shape["null_busy"] = request.param == "null_busy"
    yield request.param
    _shape["null_busy"] = True


def leg(side, delay, tensors, produce, call):
    """One leg: see the module docstring.  ``tensors``: every device tensor
    the call reads or writes; ``produce()`` enqueues the inputs' producer on
    the current (side) stream; ``call(stream_handle)`` is the library call.
    Returns what ``call`` returned, after the side stream has drained."""
    import torch
    assert delay >= MIN_DELAY_MS
    poison(*tensors)
    torch.cuda.synchronize()
    null_busy()                                  # shape "null_busy": busy as well, and for longer
    with torch.cuda.stream(side):
        torch.cuda._sleep(CYCLES)
        produce()
        assert side.query() is False, "the side stream drained before the library call: the leg proves nothing"
        out = call(side.cuda_stream)
    side.synchronize()
    torch.cuda.synchronize()
    return out


def null_busy():
    """Shape "null_busy": another delay on the null stream, whatever the
    current stream is, so a step that lands there by mistake runs after the
    call's own kernels.  Shape "null_idle": nothing, so a blocking copy on the
    null stream runs at once, before the side stream has produced its input."""
    import torch
    if not _shape["null_busy"]:
        return
    with torch.cuda.stream(torch.cuda.default_stream()):
        torch.cuda._sleep(2 * CYCLES)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


_cache = {}


def text_and_sa(oracle, kind, n, seed):
    """(text, oracle SA) of a generator text: computed once, never changed."""
    key = (kind, n, seed)
    if key not in _cache:
        t = oracle.gen_text(kind, n, seed=seed)
        sa = oracle.sa_c(t)
        t.setflags(write=False)
        sa.setflags(write=False)
        _cache[key] = (t, sa)
    return _cache[key]


def sa_of(oracle, t):
    key = ("text", t.tobytes())
    if key not in _cache:
        sa = oracle.sa_c(t)
        sa.setflags(write=False)
        _cache[key] = sa
    return _cache[key]


# ---- builds ----------------------------------------------------------------
# (variant, alphabet kind, build options, what stats must say).  stats["round1"]
# is the first-round sort: the packed schedule's choice, and "lsd" for the
# reference schedule, whose every round is the LSD sort.
GENERATED = [
    ("default", "dna", {}, {"schedule": "packed", "round1": "lsd", "alphabet": "exact"}),
    ("reference", "alnum", {"schedule": "reference"}, {"schedule": "reference", "round1": "lsd"}),
    ("lsd", "byte256", {"round1": "lsd"}, {"schedule": "packed", "round1": "lsd"}),
    ("bucketed", "dna", {"round1": "bucketed"}, {"schedule": "packed", "round1": "bucketed", "alphabet": "exact"}),
    ("reduce_scan", "binary", {"radix": "reduce_scan"}, {"schedule": "packed", "round1": "lsd"}),
    ("perm_always", "ascii127", {"schedule": "reference", "debug": ("perm_always",)},
     {"schedule": "reference", "round1": "lsd"}),
]


def check_stats(st, want, n):
    for k, v in want.items():
        assert st[k] == v, (k, st[k], v)
    assert st["distinct"][-1] == n


@pytest.mark.parametrize("n", [65_537, 300_017])
@pytest.mark.parametrize("variant,kind,opts,want", GENERATED, ids=[g[0] for g in GENERATED])
def test_build_generated_text(builder, oracle, side, delay, variant, kind, opts, want, n):
    """generate_text -> build on the side stream, nothing in between."""
    import torch
    seed = n + len(variant)
    t, sa = text_and_sa(oracle, kind, n, seed)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    alphabet = oracle.ALPHABETS[kind]

    def produce():
        builder.generate_text(d_text, n, alphabet, seed=seed, stream=side.cuda_stream)

    st = leg(side, delay, [d_text, d_sa], produce, lambda s: builder.build(d_text, n, d_sa, stream=s, **opts))
    assert (d_text.cpu().numpy() == t).all()
    assert (u32(d_sa) == sa).all(), variant
    check_stats(st, want, n)


T = 6144          # the first bucket pass's tile of the power-of-two alphabets (tests/test_gpu_alphabet_sample.py)


def copied_texts(oracle):
    """(variant, text, build options, what stats must say) of the builds whose
    text is not the generator's: they arrive by a copy from pinned memory."""
    good = oracle.gen_text("dna", 11 * T + 65, seed=5)
    good[-1] = good.max()                       # no tail run of the smallest symbol
    assert set(good[:4096].tolist()) == set(good.tolist())
    bad = oracle.gen_text("dna", 11 * T + 37, seed=6)
    bad[-1] = bad.max()
    bad[3 * T + 1000] = ord("N")                # outside the sample: the first pass refutes it
    small = {"round1": "bucketed", "debug": ("alpha_sample_small",)}
    return [
        ("alpha_sample_small", good, small, {"round1": "bucketed", "alphabet": "sampled", "sigma": 4}),
        ("alpha_sample_small_refuted", bad, small, {"round1": "bucketed", "alphabet": "refuted", "sigma": 5}),
        ("degenerate", np.full(70_001, ord("a"), np.uint8), {}, {"round1": "pivot", "sigma": 1}),
        ("degenerate_reference", np.full(70_001, ord("a"), np.uint8), {"schedule": "reference"},
         {"schedule": "reference", "round1": "lsd"}),
        # eight distinct first keys of about n / 8 suffixes each: none is shared by half of them, so no pivot
        ("periodic", periodic(65_537), {}, {"schedule": "packed", "round1": "lsd"}),
        ("periodic_300017", periodic(300_017), {}, {"schedule": "packed", "round1": "lsd"}),
    ]


COPIED = ["alpha_sample_small", "alpha_sample_small_refuted", "degenerate", "degenerate_reference", "periodic",
          "periodic_300017"]


@pytest.mark.parametrize("variant", COPIED)
def test_build_copied_text(builder, oracle, side, delay, variant):
    """copy from pinned memory -> build on the side stream."""
    import torch
    _, t, opts, want = next(c for c in copied_texts(oracle) if c[0] == variant)
    n = int(t.size)
    sa = sa_of(oracle, t)
    h_text = pinned(t)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    st = leg(side, delay, [d_text, d_sa], lambda: d_text.copy_(h_text, non_blocking=True),
             lambda s: builder.build(d_text, n, d_sa, stream=s, **opts))
    assert (u32(d_sa) == sa).all(), variant
    check_stats(st, want, n)
    if variant.startswith("degenerate"):
        assert (sa == np.arange(n - 1, -1, -1, dtype=np.uint32)).all()
    if variant.startswith("periodic"):
        assert st["rounds"] >= 4, st["rounds"]           # several unsorted-set rounds
    if variant == "degenerate":
        assert st["rounds"] >= 4, st["rounds"]           # the pivot rounds


# ---- the pipeline ----------------------------------------------------------
def _patterns(t, seed):
    from test_gpu_find import draw_patterns
    tb = bytes(t)
    return draw_patterns(t, 120, seed=seed, lens=[1, 2, 3, 7, 8, 9, 15, 16, 17, 31]) + [b"", tb[-5:], tb[:40], b"\xff" * 3]


@pytest.mark.parametrize("n", [65_537, 300_017])
def test_pipeline(gpu, oracle, side, delay, n):
    """generate_text -> build -> check -> lcp -> bwt -> inverse -> fm_build ->
    fm_count -> fm_locate on the side stream: each later call's input is the
    earlier call's output on that stream, and no host code touches the device
    in between; the null stream is made busy again before every call that
    follows a host wait.  The context first serves a periodic text of the
    same size (long repeats: the LCP's cooperative pair lists and a long LRS
    stay behind in its workspace) and then, with no build in between, the LCP
    of the random text from an SA copied in on the stream."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    from hpc_suffix_array_amd.builder import _pack_patterns
    from test_gpu_find import ref_intervals
    from test_gpu_locate import expected
    seed = 7 * n
    t, sa = text_and_sa(oracle, "dna", n, seed)
    lcp = oracle.lcp_c(t, sa)
    primary = int(np.flatnonzero(sa == 0)[0])
    bwt = t[(sa.astype(np.int64) - 1) % n]
    pats = _patterns(t, n)
    buf, off = _pack_patterns(pats)
    nq = len(pats)
    lo_w, hi_w = ref_intervals(bytes(t), sa, pats)
    occ = hi_w > lo_w
    lo_fm, hi_fm = np.where(occ, lo_w, 0), np.where(occ, hi_w, 0)
    off_w, pos_w = expected(sa, lo_fm, hi_fm)
    h_pat, h_off = pinned(buf), pinned(off)

    b = DeviceBuilder(1 << 14)
    dev = dict(device="cuda")
    d_text = torch.empty(n, dtype=torch.uint8, **dev)
    d_sa = torch.empty(n, dtype=torch.int32, **dev)
    d_lcp = torch.empty(n, dtype=torch.int32, **dev)
    d_bwt = torch.empty(n, dtype=torch.uint8, **dev)
    d_isa = torch.empty(n, dtype=torch.int32, **dev)
    d_stats = torch.empty(N.BWT_STATS, dtype=torch.int64, **dev)
    cap = b.fm_index_bytes(n, 32)
    d_index = torch.empty(cap, dtype=torch.uint8, **dev)
    d_pat = torch.empty(max(int(buf.size), 1), dtype=torch.uint8, **dev)
    d_off = torch.empty(nq + 1, dtype=torch.int64, **dev)
    d_lo = torch.empty(nq, dtype=torch.int32, **dev)
    d_hi = torch.empty(nq, dtype=torch.int32, **dev)
    d_o = torch.empty(nq + 1, dtype=torch.int64, **dev)
    total_w = int(off_w[-1])
    d_pos = torch.empty(total_w + 2, dtype=torch.int32, **dev)
    every = [d_text, d_sa, d_lcp, d_bwt, d_isa, d_stats, d_index, d_pat, d_off, d_lo, d_hi, d_o, d_pos]
    res = {}

    # the context's earlier life: a periodic text, built and its LCP taken
    p = periodic(n)
    p_sa = sa_of(oracle, p)
    p_lcp = oracle.lcp_c(p, p_sa)
    h_p = pinned(p)

    def earlier(s):
        b.build(d_text, n, d_sa, stream=s)
        return b.lcp(d_text, n, d_sa, d_lcp, stream=s)

    ln, pos = leg(side, delay, every, lambda: d_text.copy_(h_p, non_blocking=True), earlier)
    assert (u32(d_sa) == p_sa).all() and (u32(d_lcp) == p_lcp).all()
    assert bytes(p[pos:pos + ln]) == oracle.lrs_c(p, p_sa, p_lcp) and ln > 4096

    # lcp straight after lcp, the SA copied from pinned memory: the earlier call's pair counts and
    # its LRS word (longer than this text's) are what the context holds when this one starts
    h_t, h_sa = pinned(t), pinned(sa)

    def text_and_sa_in():
        d_text.copy_(h_t, non_blocking=True)
        d_sa.copy_(h_sa, non_blocking=True)

    ln, pos = leg(side, delay, every, text_and_sa_in, lambda s: b.lcp(d_text, n, d_sa, d_lcp, stream=s))
    assert (u32(d_lcp) == lcp).all()
    assert bytes(t[pos:pos + ln]) == oracle.lrs_c(t, sa, lcp)

    def produce():
        d_pat[:buf.size].copy_(h_pat, non_blocking=True)
        d_off.copy_(h_off, non_blocking=True)

    def pipeline(s):
        b.generate_text(d_text, n, b"ACGT", seed=seed, stream=s)
        res["stats"] = b.build(d_text, n, d_sa, stream=s)
        null_busy()                                  # before every later call: the build waited for the first
        res["valid"] = b.check(d_text, n, d_sa, stream=s)
        null_busy()
        res["lrs"] = b.lcp(d_text, n, d_sa, d_lcp, stream=s)
        null_busy()
        b.bwt(d_text, n, d_sa, d_bwt, d_stats, stream=s)
        b.inverse(n, d_sa, d_isa, stream=s)
        null_busy()
        res["fm"] = b.fm_build(d_bwt, n, primary, d_index, cap, d_sa, 32, stream=s)
        null_busy()
        b.fm_count(d_index, res["fm"]["bytes"], d_pat, int(buf.size), d_off, nq, d_lo, d_hi, stream=s)
        res["total"] = b.fm_locate(d_index, res["fm"]["bytes"], d_lo, d_hi, nq, d_o, None, 0, stream=s)
        null_busy()
        res["total2"] = b.fm_locate(d_index, res["fm"]["bytes"], d_lo, d_hi, nq, d_o, d_pos[1:], total_w, stream=s)

    try:
        leg(side, delay, every, produce, pipeline)
    finally:
        b.close()
    assert (d_text.cpu().numpy() == t).all()
    assert (u32(d_sa) == sa).all()
    assert res["valid"] is True
    assert (u32(d_lcp) == lcp).all()
    ln, pos = res["lrs"]
    assert bytes(t[pos:pos + ln]) == oracle.lrs_c(t, sa, lcp)
    assert (d_bwt.cpu().numpy() == bwt).all()
    st = d_stats.cpu().numpy()
    assert int(st[0]) == primary and (st[2:] == np.bincount(t, minlength=256)).all()
    assert int(st[1]) == 1 + int((bwt[1:] != bwt[:-1]).sum())
    assert (u32(d_isa) == numpy_inverse(sa)).all()
    assert res["fm"]["sigma"] == 4 and res["fm"]["samples"] == (n + 31) // 32
    lo, hi = u32(d_lo).astype(np.int64), u32(d_hi).astype(np.int64)
    assert (lo == lo_fm).all() and (hi == hi_fm).all()
    assert res["total"] == total_w and res["total2"] == total_w
    assert (d_o.cpu().numpy() == off_w).all()
    got = d_pos.cpu().numpy()
    assert got[0] == -1 and got[-1] == -1 and (got[1:-1] == pos_w).all()


# ---- the building blocks of the distributed driver -------------------------
@pytest.fixture(scope="module")
def hops(builder):
    from hpc_suffix_array_amd.distributed import HipOps
    return HipOps(0, 0, builder=builder)


ARGSORT_BITS = [1, 7, 8, 9, 33, 63, 64]


@pytest.mark.parametrize("m", [1, 63, 4095, 4096, 4097, 12_293, 300_001])
def test_argsort(hops, side, delay, m):
    """sa_sort_pairs_device against torch.sort(stable=True) on the CPU: random
    keys and keys of at most 3 distinct values (stability), every key with
    random bits above `bits`, which must not affect the order."""
    import torch
    g = torch.Generator().manual_seed(m)
    lim = torch.iinfo(torch.int64)
    for bits in ARGSORT_BITS:
        noise = torch.randint(lim.min, lim.max, (m,), generator=g, dtype=torch.int64)
        low = (1 << bits) - 1 if bits < 64 else -1
        few = torch.randint(lim.min, lim.max, (3,), generator=g, dtype=torch.int64)
        for kind in ("random", "few"):
            keys = noise.clone()
            if kind == "few":      # at most 3 distinct values below `bits`, the noise above
                pick = few[torch.randint(0, 3, (m,), generator=g)]
                keys = (noise & ~low) | (pick & low)
            perm = sort_reference(keys, bits)
            h_keys = keys.pin_memory()
            d_keys = torch.empty(m, dtype=torch.int64, device="cuda")
            ko, vo = leg(side, delay, [d_keys], lambda: d_keys.copy_(h_keys, non_blocking=True),
                         lambda s: hops.argsort(d_keys, bits))
            assert torch.equal(vo.cpu(), perm), (m, bits, kind)
            assert torch.equal(ko.cpu(), keys[perm]), (m, bits, kind)


def largest_k(base):
    k = 0
    while base ** (k + 1) <= 1 << 63:
        k += 1
    return k


@pytest.mark.parametrize("sigma", [2, 4, 62, 255])
def test_pack_keys(hops, side, delay, sigma):
    """sa_pack_keys_device against tests/dist_cpu_ops.py: ranges at 0, in the
    middle, ending at n and at n - K + 1 (the zero padding past the end of the
    text is read), K = 1, 2, 7 and the largest with base^K <= 2^63."""
    import torch
    from dist_cpu_ops import CpuOps
    n = 65_537
    rng = np.random.default_rng(sigma)
    symbols = np.sort(rng.choice(256, sigma, replace=False)).astype(np.uint8)
    t = symbols[rng.integers(0, sigma, n)]
    assert np.unique(t).size == sigma
    codes = [0] * 256
    for i, b in enumerate(symbols.tolist()):
        codes[b] = i + 1
    base = sigma + 1
    text_cpu = torch.from_numpy(t)
    h_text = pinned(t)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    for K in sorted({1, 2, min(7, largest_k(base)), largest_k(base)}):
        for lo, hi in ((0, 4097), (n // 2 - 5, n // 2 + 12_293), (n - 8193, n), (n - 5000, n - K + 1)):
            want = CpuOps().pack_keys(text_cpu, n, lo, hi, codes, base, K)
            got = leg(side, delay, [d_text], lambda: d_text.copy_(h_text, non_blocking=True),
                      lambda s: hops.pack_keys(d_text, n, lo, hi, codes, base, K))
            assert torch.equal(got.cpu(), want), (sigma, K, lo, hi)


def test_gather_scatter_scans_search_select(hops, side, delay):
    """The other building blocks under the side stream, each against torch on
    the CPU; gather and scatter with base != 0."""
    import torch
    from dist_cpu_ops import CpuOps
    cpu = CpuOps()
    g = torch.Generator().manual_seed(11)
    m, base = 12_293, 1_000_003
    src = torch.randint(0, 1 << 50, (m,), generator=g, dtype=torch.int64)
    idx = torch.randperm(m, generator=g) + base
    x = torch.randint(0, 1 << 20, (m,), generator=g, dtype=torch.int64)
    v = torch.where(torch.rand(m, generator=g) < 0.7, torch.full((m,), -1, dtype=torch.int64), x << 20)
    xs = torch.sort(x).values
    q = torch.randint(0, (1 << 20) + 5, (5000,), generator=g, dtype=torch.int64)
    mask = torch.rand(m, generator=g) < 0.3
    h = {k: t.pin_memory() for k, t in dict(src=src, idx=idx, x=x, v=v, xs=xs, q=q, mask=mask).items()}
    d = {k: torch.empty(t.shape, dtype=t.dtype, device="cuda") for k, t in h.items()}
    d_dst = torch.empty(m, dtype=torch.int64, device="cuda")
    every = list(d.values()) + [d_dst]

    def produce():
        for k in h:
            d[k].copy_(h[k], non_blocking=True)

    def run(call):
        return leg(side, delay, every, produce, call)

    assert torch.equal(run(lambda s: hops.gather(d["src"], d["idx"], base)).cpu(), cpu.gather(src, idx, base))
    run(lambda s: hops.scatter(d_dst, d["idx"], base, d["src"]))
    want = torch.full((m,), -1, dtype=torch.int64)
    cpu.scatter(want, idx, base, src)
    assert torch.equal(d_dst.cpu(), want)
    assert torch.equal(run(lambda s: hops.running_max(d["v"])).cpu(), cpu.running_max(v))
    assert torch.equal(run(lambda s: hops.cumsum(d["x"])).cpu(), cpu.cumsum(x))
    assert torch.equal(run(lambda s: hops.cumsum(d["mask"])).cpu(), cpu.cumsum(mask))
    for right in (False, True):
        got = run(lambda s: hops.count_below(d["xs"], d["q"], right=right))
        assert torch.equal(got.cpu(), cpu.count_below(xs, q, right=right)), right
    assert torch.equal(run(lambda s: hops.select(d["mask"])).cpu(), cpu.select(mask))
    assert run(lambda s: hops.count_true(d["mask"])) == cpu.count_true(mask)
    t = torch.randint(0, 256, (m,), generator=g, dtype=torch.int64).to(torch.uint8)
    t[t == 7] = 8
    h_t = t.pin_memory()
    d_t = torch.empty(m, dtype=torch.uint8, device="cuda")
    got = leg(side, delay, [d_t], lambda: d_t.copy_(h_t, non_blocking=True), lambda s: hops.alphabet(d_t))
    assert got == cpu.alphabet(t)


# ---- the distributed drivers at world size 1 -------------------------------
def test_distributed_drivers(gpu, oracle, side, delay):
    """One DistributedSA range build and one SampleSortSA build under the side
    stream (the drivers take torch's current stream)."""
    import torch
    import torch.distributed as dist
    from hpc_suffix_array_amd.distributed import DistributedSA, HipOps, HipRangeOps, SampleSortSA, gather_sa
    from test_gpu_parity import _single_rank_group
    _single_rank_group()
    ops = hops = None
    try:
        n = 300_017
        t, sa = text_and_sa(oracle, "dna", n, 8)
        h_text = pinned(t)
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        ops = HipRangeOps(1 << 19, 0)
        d = DistributedSA(ops)
        sa_local, sa_off = leg(side, delay, [d_text], lambda: d_text.copy_(h_text, non_blocking=True),
                               lambda s: d.build(d_text, n))
        assert d.stats["path"] == "range", d.stats
        with torch.cuda.stream(side):
            got = gather_sa(sa_local, sa_off, n).cpu().numpy()
        assert (got == sa.astype(np.int64)).all()

        n = 65_537
        t, sa = text_and_sa(oracle, "alnum", n, 9)
        h_text = pinned(t)
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        hops = HipOps(1 << 16, 0)
        out = leg(side, delay, [d_text], lambda: d_text.copy_(h_text, non_blocking=True),
                  lambda s: SampleSortSA(hops).build(d_text, n))
        with torch.cuda.stream(side):
            got = gather_sa(out, 0, n).cpu().numpy()
        assert (got == sa.astype(np.int64)).all()
    finally:
        for o in (ops, hops):                # the contexts of both drivers
            if o is not None:
                o.b.close()
        dist.destroy_process_group()
