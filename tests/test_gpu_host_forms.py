"""The nine host-pointer forms side by side (hpc_suffix_array_amd/csrc/
sa_host.h and the host forms of sa_find.h, sa_match.h, sa_bwt.h, sa_locate.h):
each at SA width 4 and width 8 on one small text, the staged copies of
sa_host.h at the smallest size that runs the ring round, and two rejected
inputs that fail after the device buffers are allocated.  The kernels have
their own tests; the expected answers here are the ones those tests compute
(the oracle's SA and LCP, bisect over the suffixes, numpy)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SMALL = 4099
# 3 * 2^23 + 2^19 + 5 suffixes: the 32-bit SA is four staging chunks of 32 MiB,
# the fourth ragged and in ring buffer 0 again, so copy_h2d waits for a
# buffer's earlier DMA and copy_d2h issues its look-ahead chunk
N_RING = 3 * (1 << 23) + (1 << 19) + 5

_SMALL = {}


def small(oracle):
    """Text, oracle SA, the queries and every expected answer: computed once."""
    if not _SMALL:
        from test_gpu_find import ref_intervals
        from test_gpu_match import ref_interval, ref_len, ref_matches
        from hpc_suffix_array_amd import _native as N
        t = oracle.gen_text("dna", N_SMALL, seed=41)
        tb, sa = bytes(t), oracle.sa_c(t)
        long_pat = tb[200:200 + N.FIND_LANE_MAX + 13]                # the wave kernel's class
        pats = [b"", b"ACGTN", long_pat, tb[:1], tb[17:25], tb[1000:1033], tb[-5:], tb[-5:] + b"A", b"TTTTTTTTTTTTTTTT"]
        assert len(pats) == 9 and tb.find(pats[1]) < 0 and len(long_pat) > N.FIND_LANE_MAX
        q = bytearray(tb[3000:3050])
        q[13] ^= 6                                                   # A <-> G, C -> E, T -> R: a substitution
        q = bytes(q)
        sal, ms = sa.tolist(), [ref_len(tb, q[i:]) for i in range(len(q))]
        stats = {}
        for cap in (0, 7):
            ln = [min(m, cap) if cap else m for m in ms]
            iv = [ref_interval(tb, sal, q[i:i + l]) for i, l in enumerate(ln)]
            stats[cap] = tuple(np.array(x, np.int64) for x in (ln, [a for a, _ in iv], [b for _, b in iv]))
        lo, hi = ref_intervals(tb, sa, pats)
        isa = np.empty(N_SMALL, np.int64)
        isa[sa] = np.arange(N_SMALL)
        _SMALL.update(text=t, sa=sa, lcp=oracle.lcp_c(t, sa), pats=pats, lo=lo, hi=hi, match=ref_matches(tb, sa, pats),
                      query=q, stats=stats, bwt=t[(sa.astype(np.int64) - 1) % N_SMALL], primary=int(isa[0]), isa=isa,
                      off=np.concatenate([[0], np.cumsum(hi - lo)]),
                      pos=np.concatenate([np.sort(sa[a:b].astype(np.int64)) for a, b in zip(lo, hi)]))
    return _SMALL


@pytest.mark.parametrize("width", [4, 8])
def test_every_host_form(gpu, oracle, width):
    from hpc_suffix_array_amd import (build_suffix_array, bwt, check_suffix_array, find_patterns, inverse_suffix_array,
                                      lcp_array, locate_intervals, match_patterns, matching_statistics)
    c = small(oracle)
    t, dt = c["text"], (np.uint32 if width == 4 else np.int64)
    sa = build_suffix_array(t, width=width)
    assert sa.dtype == dt and (sa == c["sa"]).all()
    assert check_suffix_array(t, sa) is True
    lcp, lrs = lcp_array(t, sa, width=width)
    assert lcp.dtype == dt and (lcp == c["lcp"]).all()
    assert lrs[0] == c["lcp"].max() and lcp[np.flatnonzero(sa == lrs[1])[0]] == lrs[0]
    lo, hi = find_patterns(t, sa, c["pats"])
    assert (lo == c["lo"]).all() and (hi == c["hi"]).all()
    assert hi[1] == lo[1] and (lo[0], hi[0]) == (0, N_SMALL) and hi[2] - lo[2] >= 1
    for got, want in zip(match_patterns(t, sa, c["pats"]), c["match"]):
        assert (got == want).all()
    for cap in (0, 7):
        for got, want in zip(matching_statistics(t, sa, c["query"], max_len=cap), c["stats"][cap]):
            assert (got == want).all(), cap
    out, primary = bwt(t, sa)
    assert (out == c["bwt"]).all() and primary == c["primary"]
    out, primary, runs, counts = bwt(t, sa, stats=True)
    assert (out == c["bwt"]).all() and primary == c["primary"]
    assert runs == 1 + np.count_nonzero(np.diff(c["bwt"])) and (counts == np.bincount(t, minlength=256)).all()
    isa = inverse_suffix_array(sa, width=width)
    assert isa.dtype == dt and (isa == c["isa"]).all()
    off, pos = locate_intervals(sa, lo, hi)
    assert (off == c["off"]).all() and (pos == c["pos"]).all()


def test_staging_ring(gpu):
    """Four staging chunks each way (N_RING): the width-4 and the width-8
    host build equal each other and the SA the device-resident build leaves
    in HBM (pinned to the oracle by test_gpu_parity.py), and the checker takes
    the width-8 array back through the staged upload of its narrowed copy."""
    import torch
    from hpc_suffix_array_amd import DeviceBuilder, build_suffix_array, check_suffix_array
    n = N_RING
    b = DeviceBuilder(n)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    b.generate_text(d_text, n, b"ACGT", seed=9)
    b.build(d_text, n, d_sa)
    torch.cuda.synchronize()
    t, want = d_text.cpu().numpy(), d_sa.cpu().numpy().view(np.uint32)
    b.close()
    del d_text, d_sa
    sa4, st4 = build_suffix_array(t, width=4, return_stats=True)
    sa8, st8 = build_suffix_array(t, width=8, return_stats=True)
    print(f"n={n} width 4: h2d_ms={st4['h2d_ms']:.2f} d2h_ms={st4['d2h_ms']:.2f}; "
          f"width 8: h2d_ms={st8['h2d_ms']:.2f} d2h_ms={st8['d2h_ms']:.2f}")
    assert sa4.dtype == np.uint32 and sa8.dtype == np.int64
    assert np.array_equal(sa4, want)
    assert np.array_equal(sa8, sa4)
    assert check_suffix_array(t, sa8) is True


def test_errors_after_allocation_leave_the_library_usable(gpu, oracle):
    from hpc_suffix_array_amd import SAError, inverse_suffix_array, lcp_array
    c = small(oracle)
    t, sa = c["text"], c["sa"]
    dup = sa.copy()
    dup[5] = dup[6]
    with pytest.raises(SAError, match="not a permutation"):
        inverse_suffix_array(dup)
    assert (inverse_suffix_array(sa) == c["isa"]).all()
    swapped = sa.copy()
    swapped[[100, 2000]] = swapped[[2000, 100]]
    with pytest.raises(SAError, match="not a valid suffix array"):
        lcp_array(t, swapped)
    assert (lcp_array(t, sa)[0] == c["lcp"]).all()
