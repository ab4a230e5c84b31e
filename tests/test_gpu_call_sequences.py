"""One long-lived context: the order of calls, and the epoch wrap.

A DeviceBuilder carries state from call to call (tests/call_sequences.py
lists it).  ``test_every_ordered_pair`` runs the model's closed walk -- every
ordered pair of operations, a call followed by itself included -- on ONE
context: every step poisons its outputs and compares with a reference of the
operation itself, computed once per operation (the oracle's SA and LCP, numpy
for ISA / BWT / LF, and the reference helpers of each operation's own test
module: ref_intervals, expected, brute_mems, lpf_two_stacks, by_stack).  The
tests after it run the orders that carry the most state, one context each,
every SA against oracle.sa_c.  The last test drives a context across the wrap
of the radix tile states' epoch in a fresh process and reads from the library's
trace that the wrap happened where the test put it.

Matrix text: N = 16 385 bytes of the oracle's DNA generator, the smallest size
with four full 4096-pair tiles, two full 8192-pair tiles and a ragged last
tile of either (the bound n >= 16 385 of more than one tile of each).  The
references, measured on the CPU at that size: brute_mems 229 ms (the slowest),
CpuOps.pack_keys 62 ms, lpf_two_stacks 17 ms, by_stack 14 ms, the stable
sort 9 ms, each oracle SA under 3 ms, everything else under 1 ms: all under
a second, so the smallest admissible size is the one taken (the ``refs``
fixture prints the times and asserts the bound).

The device form of lcp has a valid SA as its precondition and does not check
it (a duplicate there would be an invalid launch), so the SAError of the step
"lcp of an SA with a duplicate" comes from the host form: lcp_array runs the
checker first, on the library's process-wide context, not on the one under
test.  What the context under test sees in that step is the failing call a
careful caller makes first, ``check`` of the duplicate answering False; the
host form's refusal itself leaves it untouched.
"""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_sequences as S   # noqa: E402
from context_helpers import build_ok, numpy_inverse, periodic, sort_reference   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16_385
SEED = 41


def references(oracle, n=N, times=None):
    """Inputs and expected values of every operation of the walk: computed
    once, never changed.  ``times``: a dict that receives the seconds each
    reference took."""
    import torch
    from dist_cpu_ops import CpuOps
    from test_gpu_find import draw_patterns, ref_intervals
    from test_gpu_ibwt import lf_of
    from test_gpu_locate import expected, intervals
    from test_gpu_lz import lpf_two_stacks, serial_parse
    from test_gpu_mem import brute_mems
    from test_gpu_repeats import by_stack
    from hpc_suffix_array_amd.builder import _pack_patterns

    def timed(name, fn):
        t0 = time.perf_counter()
        out = fn()
        if times is not None:
            times[name] = time.perf_counter() - t0
        return out

    r = {"n": n}
    t = oracle.gen_text("dna", n, seed=SEED)
    r["t"] = t
    r["sa"] = sa = timed("sa", lambda: oracle.sa_c(t))
    r["lcp"] = lcp = timed("lcp", lambda: oracle.lcp_c(t, sa))
    r["lrs"] = oracle.lrs_c(t, sa, lcp)
    r["isa"] = numpy_inverse(sa)
    # texts of the build variants that are not the matrix text
    small = t.copy()
    small[-1] = small.max()
    assert set(small[:4096].tolist()) == set(small.tolist())
    texts = {"build_alpha_sample_small": small, "build_degenerate": np.full(n, ord("a"), np.uint8),
             "build_periodic": periodic(n)}
    r["texts"] = {k: (v, timed("sa " + k, lambda v=v: oracle.sa_c(v))) for k, v in texts.items()}
    # corrupted SAs
    swapped = sa.copy()
    swapped[[n // 2, n // 2 + 1]] = sa[[n // 2 + 1, n // 2]]
    dup = sa.copy()
    dup[n // 3] = sa[2 * n // 3]
    r["swapped"], r["dup"] = swapped, dup
    assert oracle.check_c(t, sa) and not oracle.check_c(t, swapped)
    # locate
    counts = [0, 1, 2, 33, 257, 4097, 0, 5]
    lo, hi = intervals(counts, n, seed=3)
    r["locate"] = (lo, hi) + timed("locate", lambda: expected(sa, lo, hi))
    # mems
    q = np.concatenate([t[1000:1100], t[9000:9120]]).copy()
    q[17::37] = ord("A")
    r["mems"] = (q, 12, timed("mems", lambda: brute_mems(t, q, 12)))
    # lpf + lz77
    lpf, src = timed("lpf", lambda: lpf_two_stacks(sa, lcp))
    r["lz"] = dict(t=t, sa=sa, lcp=lcp, lpf=lpf, src=src, phrases=serial_parse(lpf, src))
    # repeats
    r["repeats"] = dict(t=t, sa=sa, lcp=lcp, want=timed("repeats", lambda: by_stack(t, sa, lcp)))
    # lf + ibwt
    bwt = t[(sa.astype(np.int64) - 1) % n]
    primary = int(np.flatnonzero(sa == 0)[0])
    r["bwt"], r["primary"] = bwt, primary
    r["lf"] = timed("lf", lambda: lf_of(bwt, primary))
    # fm: count and locate
    pats = draw_patterns(t, 60, seed=n, lens=[1, 2, 3, 7, 8, 9, 15, 16, 17]) + [b"", bytes(t[-5:]), b"\xff"]
    buf, off = _pack_patterns(pats)
    plo, phi = timed("find", lambda: ref_intervals(bytes(t), sa, pats))
    occ = phi > plo
    plo, phi = np.where(occ, plo, 0), np.where(occ, phi, 0)
    r["fm"] = dict(buf=buf, off=off, nq=len(pats), lo=plo, hi=phi, loc=expected(sa, plo, phi))
    # argsort
    g = torch.Generator().manual_seed(5)
    lim = torch.iinfo(torch.int64)
    keys = torch.randint(lim.min, lim.max, (12_293,), generator=g, dtype=torch.int64)
    keys[::3] = keys[0]                              # ties: stability
    r["argsort"] = (keys, timed("argsort", lambda: sort_reference(keys, 64)))
    # pack_keys
    codes = [0] * 256
    for i, b in enumerate(b"ACGT"):
        codes[b] = i + 1
    r["pack"] = (codes, 5, 7, n - 9000, n - 3,
                 timed("pack_keys", lambda: CpuOps().pack_keys(torch.from_numpy(t), n, n - 9000, n - 3, codes, 5, 7)))
    for v in (t, sa, lcp, swapped, dup, bwt):
        v.setflags(write=False)
    return r


@pytest.fixture(scope="module")
def refs(gpu, oracle):
    times = {}
    r = references(oracle, N, times)
    print("reference times at n = %d: %s" % (N, ", ".join(f"{k} {v * 1e3:.0f} ms" for k, v in times.items())))
    assert max(times.values()) < 1.0, times
    return r


class Walker:
    """The operations of the walk on one context, each against ``refs``."""

    def __init__(self, refs):
        import torch
        from hpc_suffix_array_amd import DeviceBuilder
        from hpc_suffix_array_amd.distributed import HipOps
        self.r = refs
        self.n = n = refs["n"]
        self.b = DeviceBuilder(1 << 12)              # grows at the first step
        self.hops = HipOps(0, 0, builder=self.b)

        def up(a):
            a = np.ascontiguousarray(a)
            a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
            return torch.from_numpy(a.copy()).cuda()

        self.d_text = up(refs["t"])
        self.d_sa = up(refs["sa"])
        self.d_swapped = up(refs["swapped"])
        self.d_dup = up(refs["dup"])
        self.d_bwt = up(refs["bwt"])
        self.d_texts = {k: up(v[0]) for k, v in refs["texts"].items()}
        self.d_out = torch.empty(n, dtype=torch.int32, device="cuda")
        self.d_out8 = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.d_keys = refs["argsort"][0].cuda()
        f = refs["fm"]
        self.d_pat = up(f["buf"])
        self.d_off = up(f["off"])
        self.cap = self.b.fm_index_bytes(n, 32)
        self.d_index = torch.empty(self.cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def close(self):
        self.b.close()

    def step(self, op):
        if op in S.BUILD_VARIANTS:
            return self.build(op)
        return getattr(self, op)()

    def got32(self):
        import torch
        torch.cuda.synchronize()
        return self.d_out.cpu().numpy().view(np.uint32)

    def build(self, op):
        import torch
        d_text, want = self.d_text, self.r["sa"]
        if op in self.r["texts"]:
            d_text, want = self.d_texts[op], self.r["texts"][op][1]
        self.d_out.fill_(-1)
        torch.cuda.synchronize()
        st = self.b.build(d_text, self.n, self.d_out, **S.BUILD_VARIANTS[op])
        assert (self.got32() == want).all()
        assert st["distinct"][-1] == self.n
        assert st["schedule"] == S.BUILD_VARIANTS[op].get("schedule", "packed")

    def check_valid(self):
        assert self.b.check(self.d_text, self.n, self.d_sa) is True

    def check_swapped(self):
        assert self.b.check(self.d_text, self.n, self.d_swapped) is False

    def lcp_valid(self):
        import torch
        self.d_out.fill_(-1)
        torch.cuda.synchronize()
        ln, pos = self.b.lcp(self.d_text, self.n, self.d_sa, self.d_out)
        assert (self.got32() == self.r["lcp"]).all()
        assert bytes(self.r["t"][pos:pos + ln]) == self.r["lrs"]

    def lcp_duplicate(self):
        from hpc_suffix_array_amd import SAError, lcp_array
        assert self.b.check(self.d_text, self.n, self.d_dup) is False      # what this context sees
        with pytest.raises(SAError):                                       # the host form's own context
            lcp_array(self.r["t"], self.r["dup"])

    def inverse_valid(self):
        import torch
        self.d_out.fill_(-1)
        torch.cuda.synchronize()
        self.b.inverse(self.n, self.d_sa, self.d_out)
        assert (self.got32() == self.r["isa"]).all()

    def inverse_duplicate(self):
        import torch
        from hpc_suffix_array_amd import SAError
        self.d_out.fill_(-1)
        torch.cuda.synchronize()
        with pytest.raises(SAError, match="not a permutation"):
            self.b.inverse(self.n, self.d_dup, self.d_out)

    def locate(self):
        from test_gpu_locate import dev_locate
        lo, hi, woff, wpos = self.r["locate"]
        off, pos = dev_locate(self.b, self.d_sa, self.n, lo, hi, want_total=int(woff[-1]))
        assert np.array_equal(off, woff) and np.array_equal(pos, wpos)

    def mems(self):
        from test_gpu_mem import dev_mems
        q, L, ((wq, wt, wl), woff, winfo) = self.r["mems"]
        off, tp, ln, info = dev_mems(self.b, self.r["t"], self.r["sa"], q, L)
        assert info == winfo and np.array_equal(off, woff) and np.array_equal(tp, wt) and np.array_equal(ln, wl)

    def lpf_lz77(self):
        from test_gpu_lz import dev_check, dev_lz
        dev_check(dev_lz(self.b, self.r["lz"]), self.r["lz"])

    def repeats(self):
        from test_gpu_repeats import REP_KINDS, dev_check, dev_repeats
        c = self.r["repeats"]
        for k in REP_KINDS:
            dev_check(dev_repeats(self.b, c, k), c["want"][k])

    def lf_ibwt(self):
        import torch
        n, p = self.n, self.r["primary"]
        d_sa2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.d_out.fill_(-1)
        self.d_out8.fill_(255)
        torch.cuda.synchronize()
        self.b.lf(self.d_bwt, n, p, self.d_out)
        info = self.b.ibwt(self.d_bwt, n, p, self.d_out8, d_sa2)
        assert (self.got32() == self.r["lf"]).all()
        assert info["steps"] == n - 1
        assert (self.d_out8.cpu().numpy() == self.r["t"]).all()
        assert (d_sa2.cpu().numpy().view(np.uint32) == self.r["sa"]).all()

    def fm_build_locate(self):
        import torch
        f, n = self.r["fm"], self.n
        nq = f["nq"]
        woff, wpos = f["loc"]
        self.d_index.fill_(255)
        d_lo = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
        d_hi = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
        d_o = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
        d_pos = torch.full((int(woff[-1]) + 2,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        info = self.b.fm_build(self.d_bwt, n, self.r["primary"], self.d_index, self.cap, self.d_sa, 32)
        assert info["sigma"] == 4 and info["samples"] == (n + 31) // 32
        self.b.fm_count(self.d_index, info["bytes"], self.d_pat, int(f["buf"].size), self.d_off, nq, d_lo, d_hi)
        total = self.b.fm_locate(self.d_index, info["bytes"], d_lo, d_hi, nq, d_o, None, 0)
        assert total == int(woff[-1])
        assert self.b.fm_locate(self.d_index, info["bytes"], d_lo, d_hi, nq, d_o, d_pos[1:], total) == total
        torch.cuda.synchronize()
        assert (d_lo.cpu().numpy().view(np.uint32) == f["lo"]).all() and (d_hi.cpu().numpy().view(np.uint32) == f["hi"]).all()
        got = d_pos.cpu().numpy()
        assert got[0] == -1 and got[-1] == -1 and (got[1:-1] == wpos).all() and (d_o.cpu().numpy() == woff).all()

    def argsort(self):
        import torch
        keys, perm = self.r["argsort"]
        ko, vo = self.hops.argsort(self.d_keys, 64)
        assert torch.equal(vo.cpu(), perm) and torch.equal(ko.cpu(), keys[perm])

    def pack_keys(self):
        import torch
        codes, base, K, lo, hi, want = self.r["pack"]
        got = self.hops.pack_keys(self.d_text, self.n, lo, hi, codes, base, K)
        assert torch.equal(got.cpu(), want)

    def generate_text(self):
        import torch
        self.d_out8.fill_(255)
        torch.cuda.synchronize()
        self.b.generate_text(self.d_out8, self.n, b"ACGT", seed=SEED)
        torch.cuda.synchronize()
        assert (self.d_out8.cpu().numpy() == self.r["t"]).all()


def test_every_ordered_pair(refs):
    """The closed walk of tests/call_sequences.py on one context: K * K steps,
    every ordered pair of operations once.  No step is skipped; the first
    failing step is reported with the operation before it."""
    w = Walker(refs)
    try:
        walk = S.walk()
        assert len(walk) == len(S.OPERATIONS) ** 2 + 1
        t0 = time.perf_counter()
        prev = None
        for i, op in enumerate(walk):
            try:
                w.step(op)
            except Exception as e:
                pytest.fail(f"step {i}: ({prev} -> {op}) failed: {e!r}")
            prev = op
        print(f"{len(walk)} steps in {time.perf_counter() - t0:.2f} s")
    finally:
        w.close()


# ---- the orders that carry the most state ----------------------------------
@pytest.fixture
def ctx(gpu):
    from hpc_suffix_array_amd import DeviceBuilder
    b = DeviceBuilder(1 << 16)
    yield b
    b.close()


def test_grow_and_shrink(ctx, oracle):
    """The capacities reallocate at the first build; the small builds after it
    run in the large workspace; then the large size again, another alphabet."""
    build_ok(ctx, oracle, oracle.gen_text("dna", 1_000_003, seed=2))
    build_ok(ctx, oracle, oracle.gen_text("alnum", 4_097, seed=3))
    for n in (1, 2, 3):
        build_ok(ctx, oracle, oracle.gen_text("binary", n, seed=n))
    build_ok(ctx, oracle, oracle.gen_text("byte256", 1_000_003, seed=4))


def test_after_failures(ctx, oracle, refs):
    """Each rejected call is followed at once by the same call with good
    inputs and by a build."""
    import torch
    from hpc_suffix_array_amd import SAError, lcp_array
    from hpc_suffix_array_amd.distributed import HipOps
    n, t, sa = refs["n"], refs["t"], refs["sa"]
    d_text = torch.from_numpy(t.copy()).cuda()
    d_sa = torch.from_numpy(sa.view(np.int32).copy()).cuda()
    d_dup = torch.from_numpy(refs["dup"].view(np.int32).copy()).cuda()
    d_swapped = torch.from_numpy(refs["swapped"].view(np.int32).copy()).cuda()
    d_out = torch.full((n + 4,), -1, dtype=torch.int32, device="cuda")
    other = oracle.gen_text("alnum", 20_011, seed=1)

    def lcp_good():
        d_out.fill_(-1)
        torch.cuda.synchronize()
        ln, pos = ctx.lcp(d_text, n, d_sa, d_out[:n])
        torch.cuda.synchronize()
        assert (d_out[:n].cpu().numpy().view(np.uint32) == refs["lcp"]).all()
        assert bytes(t[pos:pos + ln]) == refs["lrs"]

    ctx.build(d_text, n, torch.empty(n, dtype=torch.int32, device="cuda"))     # the context has a past
    # lcp on a duplicate: the context answers check with False, the host form (its own context) refuses
    assert ctx.check(d_text, n, d_dup) is False
    with pytest.raises(SAError):
        lcp_array(t, refs["dup"])
    assert (lcp_array(t, sa)[0] == refs["lcp"]).all()
    lcp_good()
    build_ok(ctx, oracle, other)
    # inverse on a duplicate
    with pytest.raises(SAError, match="not a permutation"):
        ctx.inverse(n, d_dup, d_out[:n])
    d_out.fill_(-1)
    torch.cuda.synchronize()
    ctx.inverse(n, d_sa, d_out[:n])
    torch.cuda.synchronize()
    assert (d_out[:n].cpu().numpy().view(np.uint32) == refs["isa"]).all()
    build_ok(ctx, oracle, other, schedule="reference")
    # check returning False
    assert ctx.check(d_text, n, d_swapped) is False
    assert ctx.check(d_text, n, d_dup) is False
    assert ctx.check(d_text, n, d_sa) is True
    build_ok(ctx, oracle, other)
    # scatter with an index out of range
    hops = HipOps(0, 0, builder=ctx)
    dst = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    idx = torch.tensor([9, 18], dtype=torch.int64, device="cuda")
    val = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    with pytest.raises(SAError, match="scatter indices"):
        hops.scatter(dst, idx, 10, val)
    assert dst.tolist() == [-1] * 8
    hops.scatter(dst, torch.tensor([12, 10], dtype=torch.int64, device="cuda"), 10, val)
    assert dst.tolist() == [2, -1, 1, -1, -1, -1, -1, -1]
    build_ok(ctx, oracle, other, round1="bucketed")
    # a misaligned d_lcp
    with pytest.raises(SAError, match="aligned"):
        ctx.lcp(d_text, n, d_sa, d_out[1:n + 1])
    lcp_good()
    build_ok(ctx, oracle, other)


def test_alphabet_flags(ctx, oracle):
    """A DNA build sets the context's DNA flag: an alnum and a binary build
    follow it.  Then a sampled alphabet the first pass refutes, followed by a
    sampled one that holds, both at the same n."""
    from test_gpu_alphabet_sample import N_REF, POSITIONS, SMALL, _dna_with, _text
    n = 65_537
    st = build_ok(ctx, oracle, oracle.gen_text("dna", n, seed=1), round1="bucketed")
    assert st["sigma"] == 4 and st["round1"] == "bucketed"
    st = build_ok(ctx, oracle, oracle.gen_text("alnum", n, seed=1), round1="bucketed")
    assert st["sigma"] == 62 and st["round1"] == "bucketed"
    st = build_ok(ctx, oracle, oracle.gen_text("binary", n, seed=1), round1="bucketed")
    assert st["sigma"] == 2
    acgu = oracle.gen_text("dna", n, seed=2)
    acgu[acgu == ord("T")] = ord("U")                 # four symbols, not DNA's
    st = build_ok(ctx, oracle, acgu, round1="bucketed")
    assert st["sigma"] == 4
    build_ok(ctx, oracle, oracle.gen_text("dna", n, seed=3))
    bad = _dna_with(oracle, N_REF, POSITIONS["mid-tile"], ord("N"))
    good = _text(oracle, "dna", N_REF)
    assert set(good[:4096].tolist()) == set(good.tolist())
    for _ in range(2):
        st = build_ok(ctx, oracle, bad, round1="bucketed", debug=SMALL)
        assert st["alphabet"] == "refuted" and st["sigma"] == 5, st["alphabet"]
        st = build_ok(ctx, oracle, good, round1="bucketed", debug=SMALL)
        assert st["alphabet"] == "sampled" and st["sigma"] == 4, st["alphabet"]
    st = build_ok(ctx, oracle, good)
    assert st["alphabet"] == "exact"


def test_radix_and_schedule(ctx, oracle):
    """reduce_scan build -> argsort (which leaves the context on the one-sweep
    radix) -> reduce_scan build -> default build; then the reference schedule
    and the packed one, alternating three times."""
    import torch
    from hpc_suffix_array_amd.distributed import HipOps
    t = oracle.gen_text("alnum", 65_537, seed=5)
    hops = HipOps(0, 0, builder=ctx)
    g = torch.Generator().manual_seed(9)
    keys = torch.randint(0, 1 << 40, (12_293,), generator=g, dtype=torch.int64)
    build_ok(ctx, oracle, t, radix="reduce_scan")
    ko, vo = hops.argsort(keys.cuda(), 40)
    perm = sort_reference(keys, 40)
    assert torch.equal(vo.cpu(), perm) and torch.equal(ko.cpu(), keys[perm])
    build_ok(ctx, oracle, t, radix="reduce_scan")
    build_ok(ctx, oracle, t)
    for schedule in ("reference", "packed") * 3:
        st = build_ok(ctx, oracle, t, schedule=schedule)
        assert st["schedule"] == schedule
    build_ok(ctx, oracle, t, schedule="reference", radix="reduce_scan")
    build_ok(ctx, oracle, t, schedule="reference")


def test_pivot_state(ctx, oracle):
    """A degenerate text allocates the group-start buffers and takes pivot
    rounds; random DNA of the same n follows, then the degenerate text again."""
    n = 70_001
    a = np.full(n, ord("a"), np.uint8)
    st = build_ok(ctx, oracle, a)
    assert st["round1"] == "pivot", st["round1"]
    st = build_ok(ctx, oracle, oracle.gen_text("dna", n, seed=7))
    assert st["round1"] == "lsd", st["round1"]
    st = build_ok(ctx, oracle, a)
    assert st["round1"] == "pivot", st["round1"]
    build_ok(ctx, oracle, periodic(n))
    build_ok(ctx, oracle, a, schedule="reference")


# ---- the epoch wrap --------------------------------------------------------
CHILD = r"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import call_sequences as S
from context_helpers import build_ok, periodic, sort_reference
from hpc_suffix_array_amd import DeviceBuilder
from hpc_suffix_array_amd.distributed import HipOps
from oracle import oracle as O


def mark(s):
    sys.stderr.flush()
    print("## " + s, file=sys.stderr, flush=True)


def make_keys(m, seed):
    g = torch.Generator().manual_seed(seed)
    lim = torch.iinfo(torch.int64)
    k = torch.randint(lim.min, lim.max, (m,), generator=g, dtype=torch.int64)
    k[::5] = k[1]
    return k


M = 12293                     # three full tiles and a ragged end
MBIG = 300 * 4096 + 7         # hundreds of tiles: most look back before their predecessor has published
KEYS = {"small": make_keys(M, 3), "A": make_keys(MBIG, 4), "B": make_keys(MBIG, 5)}
DEV = {k: v.cuda() for k, v in KEYS.items()}
_perm = {}


def sort_ok(ops, name, bits):
    if (name, bits) not in _perm:
        _perm[(name, bits)] = sort_reference(KEYS[name], bits)
    perm = _perm[(name, bits)]
    ko, vo = ops.argsort(DEV[name], bits)
    assert torch.equal(vo.cpu(), perm) and torch.equal(ko.cpu(), KEYS[name][perm]), (name, bits)


def advance(ops, epoch, target):
    # target - epoch radix passes of small sorts; the last call is compared, the legs check what follows
    plan = S.advance_plan(epoch, target)
    for bits in plan[:-1]:
        ops.argsort(DEV["small"], bits)
    if plan:
        sort_ok(ops, "small", plan[-1])
    return target


N = 3 * 4096 + 5
random_text = O.gen_text("dna", N, seed=2)
periodic_text = periodic(N)
BUILD_LEGS = {"reference": (random_text, {"schedule": "reference"}),
              "packed_lsd": (random_text, {"round1": "lsd"}),
              "periodic": (periodic_text, {})}
dry = DeviceBuilder(1 << 14)
PASSES = {}
for name, (t, kw) in BUILD_LEGS.items():
    st = build_ok(dry, O, t, **kw)
    PASSES[name] = sum(st["passes"])
    print("passes %s %d %s" % (name, PASSES[name], st["passes"]), flush=True)
dry.close()

for j, name in ((0, "reference"), (3, "packed_lsd"), (7, "periodic")):
    b = DeviceBuilder(1 << 21)
    ops = HipOps(0, 0, builder=b)
    t0 = time.perf_counter()
    # a one-pass sort of hundreds of tiles at the tag the same sort of other keys takes after the wrap:
    # its words (tiles >= 4 are touched by nothing in between) are what the wrap has to clear
    epoch = advance(ops, 0, 8 - j)
    sort_ok(ops, "A", 8)
    epoch += 1
    stale_tag = epoch
    # the first wrap, on pass j of an 8-pass sort of a context that has only sorted so far
    epoch = advance(ops, epoch, S.EPOCH_LAST - j)
    torch.cuda.synchronize()
    print("advance to the first wrap (leg %d): %.3f s" % (j, time.perf_counter() - t0), flush=True)
    mark("argsort pass %d" % j)
    sort_ok(ops, "small", 64)
    mark("after argsort pass %d" % j)
    epoch = S.epoch_after(epoch, 8)
    assert epoch == 8 - j and epoch + 1 == stale_tag
    mark("stale tag %d" % j)
    sort_ok(ops, "B", 8)
    mark("after stale tag %d" % j)
    epoch += 1
    for _ in range(5):
        sort_ok(ops, "small", 64)
    epoch += 40
    t, kw = BUILD_LEGS[name]
    st = build_ok(b, O, random_text)
    epoch += sum(st["passes"])
    # the second wrap, inside a build: half of its passes before the wrap
    p = PASSES[name]
    assert p >= 2, (name, p)
    t0 = time.perf_counter()
    advance(ops, epoch, S.EPOCH_LAST - p // 2)
    torch.cuda.synchronize()
    print("advance to the second wrap (leg %d): %.3f s" % (j, time.perf_counter() - t0), flush=True)
    mark("build %s" % name)
    st = build_ok(b, O, t, **kw)
    mark("after build %s" % name)
    assert sum(st["passes"]) == p, (name, st["passes"], p)
    for _ in range(5):
        sort_ok(ops, "small", 64)
    build_ok(b, O, random_text)
    build_ok(b, O, periodic_text, schedule="reference")
    mark("end %d" % j)
    b.close()

# k_lsd's wider slots: a reference-schedule build of many tiles, then small sorts only up to the wrap,
# then another text's build whose first pass takes the tag of the first build's last pass
NL = 600011
text_a, text_b = O.gen_text("dna", NL, seed=1), O.gen_text("dna", NL, seed=2)
b = DeviceBuilder(1 << 20)
ops = HipOps(0, 0, builder=b)
epoch = advance(ops, 0, 1)
st = build_ok(b, O, text_a, schedule="reference")
pa = sum(st["passes"])
print("passes lsd leg %d %s" % (pa, st["passes"]), flush=True)
epoch += pa                                   # exact if the statistics count every tagged pass:
advance(ops, epoch, S.EPOCH_LAST)             # the trace must then show the wrap inside the next sort
torch.cuda.synchronize()
mark("lsd exact")
sort_ok(ops, "small", 8)
mark("after lsd exact")
epoch = advance(ops, 1, pa)                   # the build's first pass takes tag pa + 1, the last of text_a's
mark("stale lsd")
st = build_ok(b, O, text_b, schedule="reference")
mark("after stale lsd")
for _ in range(5):
    sort_ok(ops, "small", 64)
build_ok(b, O, random_text)
b.close()
print("child ok")
"""

WRAP = re.compile(r"^\[sa\] epoch wrap: (\d+) bytes of tile states cleared before radix pass (\d+) of the context$")


def parse_wraps(stderr):
    """{section: [(bytes cleared, pass number)]} of the child's trace."""
    out, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("## "):
            cur = out.setdefault(line[3:], [])
            continue
        m = WRAP.match(line)
        if m:
            assert cur is not None, "a wrap before the first marker"
            cur.append((int(m.group(1)), int(m.group(2))))
    return out


def test_epoch_wrap(gpu, oracle):
    """Four contexts in one fresh process with SA_TRACE=1.

    Three sort until their tile-state epoch stands j passes before the last
    tag (j = 0, 3, 7), so that the wrap -- the states cleared, the tag back at
    1 -- falls on pass j of an 8-pass argsort of 12 293 pairs (three tiles and
    a ragged end); then they sort on to the second wrap, which falls inside a
    build: the reference schedule (k_lsd's states), a packed build with the
    LSD first round, a periodic text's later rounds.

    A pass overwrites the words of its own tiles, so small sorts alone leave
    nothing for the clear to do.  Each of the three contexts therefore first
    runs a one-pass sort of 300 tiles at tag 9 - j and then only 4-tile sorts
    up to the wrap: tiles 4 .. 299 keep that sort's words.  Right after the
    wrap the same sort runs on other keys at the same tag, where a word that
    was not cleared reads as a predecessor's published count.  The fourth
    context does the same for k_lsd's wider slots with two reference-schedule
    builds of 600 011 symbols, the second starting at the tag of the first's
    last pass; the trace proves the pass count that aims it (the wrap must
    fall inside one marked one-pass sort).

    Every result is compared with the CPU's stable sort or the oracle's SA,
    five more sorts and builds follow each wrap, and the trace must show each
    wrap between the markers of the call it was aimed at, and nowhere else."""
    env = dict(os.environ, SA_TRACE="1")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    print(f"child: {time.perf_counter() - t0:.1f} s\n" + "\n".join(x for x in r.stdout.splitlines()))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stderr[-4000:]
    w = parse_wraps(r.stderr)
    legs = [(0, "reference"), (3, "packed_lsd"), (7, "periodic")]
    for j, name in legs:
        first = w[f"argsort pass {j}"]
        assert len(first) == 1 and first[0][1] == S.EPOCH_LAST + 1, (j, first)
        assert first[0][0] > 0
        assert w[f"stale tag {j}"] == []
        second = w[f"build {name}"]
        assert len(second) == 1 and second[0][1] == 2 * (S.EPOCH_LAST + 1) - 1, (name, second)
    exact = w["lsd exact"]
    assert len(exact) == 1 and exact[0][1] == S.EPOCH_LAST + 1, exact
    assert w["stale lsd"] == []
    total = sum(len(v) for v in w.values())
    assert total == 2 * len(legs) + 1, {k: v for k, v in w.items() if v}
