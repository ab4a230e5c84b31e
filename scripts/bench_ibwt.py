#!/usr/bin/env python3
"""Time of the LF-mapping and the inverse Burrows-Wheeler transform
(sa_lf_device, sa_ibwt_device) on one MI355X, next to the plain torch
composition on the same GPU: LF from ``torch.sort(stable=True)`` of the
reordered rows, the chain ranked by pointer doubling.

For each text kind and each n it makes the text on the device (random DNA and
random bytes by the library's generator, the structured texts -- one symbol,
(ab)^k, a^(n-1)b, Fibonacci, Thue-Morse, (1..64)^k -- from numpy), builds its
suffix array and its BWT with DeviceBuilder and times

    lf            sa_lf_device
    ibwt          sa_ibwt_device, text only
    ibwt_sa       sa_ibwt_device, text and suffix array
    torch_lf      LF by torch.sort(stable=True)           (n <= --torch-max-n)
    torch_ibwt    that LF, pointer doubling, a scatter    (n <= --torch-max-n)

Timing: every call is warmed up, then timed alone between two device events,
--runs times, the calls alternating run by run; reported per call: the median
and the minimum in ms.  The outputs are checked first: the text and the SA that
come back equal the ones the BWT was made from, LF equals the torch LF where
that is computed.  Prints one JSON line.  There is no CPU path: with no GPU the
script fails.

    python scripts/bench_ibwt.py [--n 16777216 67108864] [--kinds dna byte256 thue-morse] [--runs 10]
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

ALPHABETS = {"dna": b"ACGT", "byte256": bytes(range(256))}
STRUCTURED = ("one-symbol", "ab", "a-b", "fibonacci", "thue-morse", "period64")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 24, 1 << 26, 1 << 28, 1 << 30])
    ap.add_argument("--kinds", nargs="+", default=["dna", "byte256"], choices=sorted(ALPHABETS) + list(STRUCTURED))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-max-n", type=int, default=1 << 26)
    return ap.parse_args()


def structured(kind, n):
    if kind == "one-symbol":
        return np.full(n, ord("a"), np.uint8)
    if kind == "ab":
        return np.resize(np.frombuffer(b"ab", np.uint8), n)
    if kind == "a-b":
        t = np.full(n, ord("a"), np.uint8)
        t[-1] = ord("b")
        return t
    if kind == "fibonacci":
        a, b = b"b", b"a"
        while len(b) < n:
            a, b = b, b + a
        return np.frombuffer(b[:n], np.uint8).copy()
    if kind == "thue-morse":
        i = np.arange(n, dtype=np.uint64)
        pop = np.zeros(n, np.uint8)
        for k in range(max(1, int(n - 1).bit_length())):
            pop ^= ((i >> np.uint64(k)) & np.uint64(1)).astype(np.uint8)
        return (pop + ord("a")).astype(np.uint8)
    return (1 + np.arange(n) % 64).astype(np.uint8)


def timed(torch, fns, runs, warmup):
    """{name: {ms_median, ms_min, runs}}: one call per window, the calls
    alternating run by run."""
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
    return {name: {"ms_median": float(np.median(v)), "ms_min": min(v), "runs": runs} for name, v in ms.items()}


def torch_lf(torch, d_bwt, p, n):
    """(LF as int64, the sorted column): the definition, in torch."""
    dev = d_bwt.device
    rows = torch.cat([torch.tensor([p], device=dev), torch.arange(0, p, device=dev), torch.arange(p + 1, n, device=dev)])
    first, order = torch.sort(d_bwt[rows], stable=True)
    lf = torch.empty(n, dtype=torch.int64, device=dev)
    lf[rows[order]] = torch.arange(n, device=dev)
    return lf, first


def torch_ibwt(torch, d_bwt, p, n):
    """Text and SA by pointer doubling over LF: the steps from a rank to the
    primary row are its suffix, and the sorted column holds its first byte."""
    lf, first = torch_lf(torch, d_bwt, p, n)
    nxt = lf
    nxt[p] = p
    d = torch.ones(n, dtype=torch.int64, device=d_bwt.device)
    d[p] = 0
    for _ in range(max(1, int(n - 1).bit_length())):
        d = d + d[nxt]
        nxt = nxt[nxt]
    text = torch.empty(n, dtype=torch.uint8, device=d_bwt.device)
    text[d] = first
    return text, d


def one(torch, a, kind, n):
    from hpc_suffix_array_amd import DeviceBuilder, _native as N
    dev = torch.device("cuda", 0)
    b = DeviceBuilder(n)
    if kind in ALPHABETS:
        d_text = torch.empty(n, dtype=torch.uint8, device=dev)
        b.generate_text(d_text, n, ALPHABETS[kind], seed=a.seed)
    else:
        d_text = torch.from_numpy(structured(kind, n)).to(dev)
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    st = b.build(d_text, n, d_sa)
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    d_stats = torch.empty(N.BWT_STATS, dtype=torch.int64, device=dev)
    sptr = torch.cuda.current_stream(dev).cuda_stream
    b.bwt(d_text, n, d_sa, d_bwt, d_stats, stream=sptr)
    stats = d_stats.cpu().numpy()
    p = int(stats[0])
    d_lf = torch.empty(n, dtype=torch.int32, device=dev)
    d_out = torch.empty(n, dtype=torch.uint8, device=dev)
    d_sa2 = torch.empty(n, dtype=torch.int32, device=dev)

    # the outputs agree before anything is timed
    info = b.ibwt(d_bwt, n, p, d_out, d_sa2, stream=sptr)
    assert torch.equal(d_out, d_text) and torch.equal(d_sa2, d_sa), "the round trip differs"
    d_out.zero_()
    assert b.ibwt(d_bwt, n, p, d_out, None, stream=sptr) == info and torch.equal(d_out, d_text), "text-only call"
    b.lf(d_bwt, n, p, d_lf, stream=sptr)
    with_torch = n <= a.torch_max_n
    if with_torch:
        lf, _ = torch_lf(torch, d_bwt, p, n)
        assert torch.equal(d_lf.to(torch.int64) & 0xFFFFFFFF, lf), "LF differs from the torch sort"
        t2, s2 = torch_ibwt(torch, d_bwt, p, n)
        assert torch.equal(t2, d_text) and torch.equal(s2, d_sa.to(torch.int64) & 0xFFFFFFFF), "torch composition"
        del lf, t2, s2

    fns = {"lf": lambda: b.lf(d_bwt, n, p, d_lf, stream=sptr),
           "ibwt": lambda: b.ibwt(d_bwt, n, p, d_out, None, stream=sptr),
           "ibwt_sa": lambda: b.ibwt(d_bwt, n, p, d_out, d_sa2, stream=sptr)}
    if with_torch:
        fns["torch_lf"] = lambda: torch_lf(torch, d_bwt, p, n)
        fns["torch_ibwt"] = lambda: torch_ibwt(torch, d_bwt, p, n)
    rec = timed(torch, fns, a.runs, a.warmup)
    rec.update(kind=kind, n=n, build_ms=st["total_ms"], primary=p, runs_in_bwt=int(stats[1]), **info,
               ibwt_ns_per_byte_median=rec["ibwt"]["ms_median"] * 1e6 / n)
    if with_torch:
        rec.update(lf_over_torch_median=rec["lf"]["ms_median"] / rec["torch_lf"]["ms_median"],
                   ibwt_sa_over_torch_median=rec["ibwt_sa"]["ms_median"] / rec["torch_ibwt"]["ms_median"])
    b.close()
    del d_text, d_sa, d_bwt, d_lf, d_out, d_sa2
    torch.cuda.empty_cache()
    return rec


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ibwt.py needs an MI355X: no HIP device is visible")
    from hpc_suffix_array_amd import _native as N
    out = {"bench": "ibwt", "seed": a.seed, "lf_tile": N.LF_TILE, "s": N.IBWT_S, "src_hash": N.source_hash(),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "results": []}
    for kind in a.kinds:
        for n in a.n:
            out["results"].append(one(torch, a, kind, n))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
