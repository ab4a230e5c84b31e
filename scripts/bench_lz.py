#!/usr/bin/env python3
"""Time of the longest previous factor array and the LZ77 parse of a built SA
(sa_lpf_device, sa_lz77_device) on one MI355X, next to sa_lcp_device and
sa_inverse_device of the same library in the same process as the yardstick.

For each case (random DNA at the large sizes; a^(n-1)b and one symbol at 2^24,
whose summed LPF is of order n^2 / 2) it puts the text on the device, builds
its suffix array and its LCP array with DeviceBuilder and times

    lpf_lcp_given     sa_lpf_device with d_lcp (enqueue only; the window ends
                      in a device event)
    lpf_lcp_computed  sa_lpf_device with d_lcp = NULL
    lz77_write        sa_lz77_device, the writing call (out_cap = z)
    lcp               sa_lcp_device
    inverse           sa_inverse_device

Timing: every call is warmed up, then timed alone between two device events,
--runs times, the calls alternating run by run; reported per call: the median,
the minimum and the maximum in ms.  The outputs are checked first, on the
device: LPF and SRC with the LCP given and computed are equal; src < i, the
first and last byte of every match agree and the byte after it does not (all
positions); LPF[i + 1] >= LPF[i] - 1; the phrases tile the text with len =
max(1, LPF[pos]) and src = SRC[pos].  The candidates of the parse are counted
by a torch expression of their definition (the distinct tile exits below n,
and position 0).  Prints one JSON line.  There is no CPU path: with no GPU the
script fails.

    python scripts/bench_lz.py [--n 268435456] [--adversarial-n 16777216] [--runs 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[1 << 28])
    ap.add_argument("--adversarial-n", type=int, nargs="*", default=[1 << 24])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    return ap.parse_args()


def timed(torch, fns, runs, warmup):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: {"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v), "runs": runs}
            for name, v in ms.items()}


def u32(x):
    """An int32 tensor's values as the uint32 they are, in int64."""
    import torch
    return x.to(torch.int64) & 0xFFFFFFFF


def check_outputs(torch, n, d_text, lpf, src, pos, ln, fsrc, tile):
    """The properties, on the device; returns the candidates of the parse."""
    none = 0xFFFFFFFF
    i = torch.arange(n, device=lpf.device)
    L, S = u32(lpf), u32(src)
    has = L > 0
    assert int(L[0]) == 0 and bool(((S == none) == ~has).all()), "src is none exactly where LPF is 0"
    assert bool((S[has] < i[has]).all()) and bool((i + L <= n).all()), "src < i, the match inside the text"
    assert bool((L[1:] >= L[:-1] - 1).all()), "LPF[i + 1] >= LPF[i] - 1"
    ih, sh, lh = i[has], S[has], L[has]
    assert bool((d_text[sh] == d_text[ih]).all()) and bool((d_text[sh + lh - 1] == d_text[ih + lh - 1]).all()), "match"
    end = ih + lh < n
    assert bool((d_text[(sh + lh)[end]] != d_text[(ih + lh)[end]]).all()), "maximal at src"
    del ih, sh, lh, end
    P, K, F = u32(pos), u32(ln), u32(fsrc)
    assert int(P[0]) == 0 and bool((P[1:] == P[:-1] + K[:-1]).all()) and int(P[-1] + K[-1]) == n, "phrases tile"
    assert bool((K == torch.clamp(L[P], min=1)).all()) and bool((F == S[P]).all()), "phrase = (max(1, LPF), SRC)"
    # candidates: position 0 and the distinct exits below n
    e = torch.clamp(i + torch.clamp(L, min=1), max=n)
    tile_end = torch.clamp((i // tile + 1) * tile, max=n)
    del P, K, F, S, has
    for _ in range(12):
        inside = e < tile_end
        e = torch.where(inside, e[torch.where(inside, e, 0)], e)
    mask = torch.zeros(n, dtype=torch.bool, device=lpf.device)
    mask[e[e < n]] = True
    mask[0] = True
    return int(mask.sum())


def one(torch, a, kind, n):
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(n)
    if kind == "dna":
        d_text = torch.empty(n, dtype=torch.uint8, device=dev)
        b.generate_text(d_text, n, b"ACGT", seed=a.seed)
    else:
        d_text = torch.full((n,), ord("a"), dtype=torch.uint8, device=dev)
        if kind == "a_b":
            d_text[-1] = ord("b")
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    st = b.build(d_text, n, d_sa)
    d_lcp, d_lcp2, d_isa = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    d_lpf, d_src, d_lpf2, d_src2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    torch.cuda.synchronize()
    sptr = torch.cuda.current_stream(dev).cuda_stream
    b.lcp(d_text, n, d_sa, d_lcp, stream=sptr)

    # the outputs are checked before anything is timed
    b.lpf(None, n, d_sa, d_lcp, d_lpf, d_src, stream=sptr)
    b.lpf(d_text, n, d_sa, None, d_lpf2, d_src2, stream=sptr)
    torch.cuda.synchronize()
    assert torch.equal(d_lpf, d_lpf2) and torch.equal(d_src, d_src2), "LCP given and computed differ"
    z = b.lz77(n, d_lpf, d_src, None, None, None, 0, stream=sptr)
    d_pos, d_len, d_fsrc = (torch.empty(z, dtype=torch.int32, device=dev) for _ in range(3))
    assert b.lz77(n, d_lpf, d_src, d_pos, d_len, d_fsrc, z, stream=sptr) == z
    cands = check_outputs(torch, n, d_text, d_lpf, d_src, d_pos, d_len, d_fsrc, N.LZ_TILE)
    lpf_sum = int(u32(d_lpf).sum())
    torch.cuda.empty_cache()

    fns = {"lpf_lcp_given": lambda: b.lpf(None, n, d_sa, d_lcp, d_lpf, d_src, stream=sptr),
           "lpf_lcp_computed": lambda: b.lpf(d_text, n, d_sa, None, d_lpf2, d_src2, stream=sptr),
           "lz77_write": lambda: b.lz77(n, d_lpf, d_src, d_pos, d_len, d_fsrc, z, stream=sptr),
           "lcp": lambda: b.lcp(d_text, n, d_sa, d_lcp2, stream=sptr),
           "inverse": lambda: b.inverse(n, d_sa, d_isa, stream=sptr)}
    rec = timed(torch, fns, a.runs, a.warmup)
    tiles = (n + N.LZ_TILE - 1) // N.LZ_TILE
    rec.update(kind=kind, n=n, build_ms=st["total_ms"], z=z, lpf_sum=lpf_sum, candidates=cands,
               candidates_per_tile=cands / tiles,
               lpf_ns_per_position_median=rec["lpf_lcp_given"]["ms_median"] * 1e6 / n,
               lz77_ns_per_position_median=rec["lz77_write"]["ms_median"] * 1e6 / n,
               lpf_over_lcp_median=rec["lpf_lcp_given"]["ms_median"] / rec["lcp"]["ms_median"],
               lpf_over_inverse_median=rec["lpf_lcp_given"]["ms_median"] / rec["inverse"]["ms_median"])
    b.close()
    del d_text, d_sa, d_lcp, d_lcp2, d_isa, d_lpf, d_src, d_lpf2, d_src2, d_pos, d_len, d_fsrc
    torch.cuda.empty_cache()
    return rec


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lz.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import _native as N
    out = {"bench": "lz", "seed": a.seed, "tile": N.LZ_TILE, "src_hash": N.source_hash(),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "results": []}
    for n in a.n:
        out["results"].append(one(torch, a, "dna", n))
    for n in a.adversarial_n:
        for kind in ("dna", "a_b", "one"):
            out["results"].append(one(torch, a, kind, n))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
